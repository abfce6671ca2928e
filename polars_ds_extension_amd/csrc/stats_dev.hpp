// stats_dev.hpp -- device restatement of stats.cpp's Student-t survival function, for the grouped report's epilogue
// (grouped_report_pass.hip), where one p-value per coefficient and group is computed on the device.
//
// Same algorithm, same operation order, FMA contraction off in every function body (the host file is compiled with -ffp-contract=off), so the only
// differences to the host value come from the device's exp / log.  The ln-gamma part of the incomplete beta prefactor,
// lnG(a + b) - lnG(a) - lnG(b) with a = dof / 2, b = 1 / 2, depends on dof alone and is the term whose cancellation amplifies a
// last-bit difference of log() by ~dof (stats.cpp header): it is NOT recomputed here but taken from the host
// (pds::student_t_lng_term, once per distinct dof), bit-identical to what the host's beta_reg uses.
#pragma once
#include <cfloat>

namespace pds {

// beta_reg(a, b, x) of stats.cpp with its ln-gamma term given (`lng` = lnG(a + b) - lnG(a) - lnG(b) of the un-swapped a, b)
__device__ inline double beta_reg_dev(double a, double b, double x, double lng, bool* err) {
#pragma clang fp contract(off)
    if (a <= 0.0 || b <= 0.0 || !(x >= 0.0 && x <= 1.0)) {
        *err = true;
        return __builtin_nan("");
    }
    const double bt = (x == 0.0 || x == 1.0) ? 0.0 : exp(lng + a * log(x) + b * log(1.0 - x));
    const bool symm = x >= (a + 1.0) / (a + b + 2.0);
    const double eps = 0.0000000000000011102230246251565;
    const double fpmin = DBL_MIN / eps;
    if (symm) {
        const double t = a;
        a = b;
        b = t;
        x = 1.0 - x;
    }
    const double qab = a + b, qap = a + 1.0, qam = a - 1.0;
    double c = 1.0;
    double d = 1.0 - qab * x / qap;
    if (fabs(d) < fpmin) d = fpmin;
    d = 1.0 / d;
    double h = d;
    for (int mi = 1; mi < 141; ++mi) {
        const double m = (double)mi;
        const double m2 = m * 2.0;
        double aa = m * (b - m) * x / ((qam + m2) * (a + m2));
        d = 1.0 + aa * d;
        if (fabs(d) < fpmin) d = fpmin;
        c = 1.0 + aa / c;
        if (fabs(c) < fpmin) c = fpmin;
        d = 1.0 / d;
        h = h * d * c;
        aa = -(a + m) * (qab + m) * x / ((a + m2) * (qap + m2));
        d = 1.0 + aa * d;
        if (fabs(d) < fpmin) d = fpmin;
        c = 1.0 + aa / c;
        if (fabs(c) < fpmin) c = fpmin;
        d = 1.0 / d;
        const double del = d * c;
        h *= del;
        if (fabs(del - 1.0) <= eps) break;
    }
    return symm ? 1.0 - bt * h / a : bt * h / a;
}

// pds::student_t_sf of stats.cpp; NaN where the host sets its error flag (pds_student_t_sf)
__device__ inline double student_t_sf_dev(double x, double df, double lng) {
#pragma clang fp contract(off)
    if (__builtin_isinf(df)) return 0.5 * erfc(x / 1.41421356237309504880168872420969808);
    const double h = df / (df + x * x);
    bool err = false;
    const double ib = 0.5 * beta_reg_dev(df / 2.0, 0.5, h, lng, &err);
    if (err) return __builtin_nan("");
    return x <= 0.0 ? 1.0 - ib : ib;
}

}  // namespace pds
