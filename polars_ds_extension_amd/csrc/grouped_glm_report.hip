// grouped_glm_report.hip -- the report of a GLM per group: standard errors, z, p, confidence intervals, deviances and the dispersion
// of every group of a frame in one kernel, at the coefficients the grouped fit (grouped_irls.hip) left in device memory.  The GLM
// twin of grouped_report_pass.hip; the definitions are the unscaled convention of statsmodels' GLM:
//
//   group of n rows, row i = x_i (the constant 1 last with a bias), beta = the group's coefficients AS STORED (an f32 frame: the f32
//   values -- the report describes the numbers the caller receives), families / canonical links of glm_dev.hpp:
//     eta_i = x_i . beta, mu_i = g^-1(eta_i), w_i = 1 / (g'(mu_i)^2 V(mu_i)), I = sum w_i x_i x_i'
//     pearson_chi2 = sum (y_i - mu_i)^2 / V(mu_i);  df_resid = n - p'
//     dispersion phi = 1 (poisson, binomial), pearson_chi2 / df_resid (gaussian, gamma; NaN when df_resid = 0, and se / z / p / CI
//     / cov with it)
//     cov = phi I^-1, se_j = sqrt(cov_jj), z_j = beta_j / se_j, p_j = erfc(|z_j| / sqrt 2), CI = beta_j -+ 1.959963984540054 se_j
//     (the normal distribution for every family: statsmodels' use_t = False)
//     deviance = sum d_i: gaussian (y - mu)^2; poisson 2 [y ln(y / mu) - (y - mu)]; binomial 2 [y ln(y / mu) + (1 - y) ln((1 - y) /
//     (1 - mu))]; gamma 2 [-ln(y / mu) + (y - mu) / mu]; 0 ln 0 = 0
//     null_deviance = the same sum at a constant mean mu0: mean_g(y) with a bias; g^-1(0) without (gaussian 0, poisson 1, binomial
//     0.5, gamma: NaN).  A closed form in (n, sum y, one family sum): gaussian sum (y - y0)^2 (y0 = the group's first y with a
//     bias -- the shift of grouped_report_pass.hip -- and 0 without), poisson sum y ln y, binomial sum [y ln y + (1 - y) ln(1 - y)],
//     gamma sum ln y -- no second pass, and the sums of the pieces of a group add up.
//     report_null = 1 when the fit is null or the factorisation of I meets a pivot that is not a positive finite number: every
//     report field of the group is then NaN (df_resid = n - p' all the same); the coefficients stay what the fit returned.
//
// One wave per group, lane = row, 64 rows per step through a wave-private LDS tile (single pass: no residency), I by
// v_mfma_f64_16x16x4 with operands (w x, x) and the bias row X'w in the side accumulator (wave_tile_dev.hpp); the scalar sums are
// per-lane registers folded by wave_sum.  I is staged like the IRLS kernel's gm (index 16 = bias) and inverted in place by a
// Gauss-Jordan sweep without pivoting (I is symmetric positive definite: every pivot is a Schur complement's diagonal), the 64
// lanes over the p' x p' entries.  No atomics in any sum: repeated calls are bit-identical.  Arithmetic is f64 for f32 frames too.
//
// Groups above `split_rows` are not walked by one wave: the kernel appends them to a list (the one atomic, and the host sorts the
// list), the host cuts their rows into pieces, grouped_glm_report_piece_kernel streams every piece on a wave of its own into a
// record (I, X'w and the five sums) and grouped_glm_report_fold_kernel -- one wave per long group -- adds the records in piece order
// and runs the same epilogue: deterministic whatever the schedule.
//
// The three kernels are templates on <T, P, WO>.  WO is the weighted / offset form: a prior weight pw_i and an offset o_i per row,
// entries P + 1 and P + 2 of the column table, each nullable (the WO = false kernels never read those two entries: their table
// ends at y).  This file is compiled twice so that the two sets of 96 kernels build side by side: as it stands it holds the
// WO = false kernels and the launchers of common.hpp, which pick the set from GlmGroupsDev::wo; grouped_glm_report_wo.hip compiles
// it with PDS_GLM_REPORT_WO and holds the WO = true kernels.  The macro selects nothing but which value of WO is instantiated.
// WO: eta_i = x_i . beta + o_i; I = sum pw_i w~_i x_i x_i' with w~ = 1 / (g'^2 V); pearson_chi2 =
// sum pw_i (y_i - mu_i)^2 / V; deviance = sum pw_i d_i; df_resid = n+ - p' with n+ the rows of positive weight; null_deviance: the
// closed form above with weighted sums (n -> sum pw, sum y -> sum pw y, the family sum weighted; the gaussian shift is the group's
// first y of positive weight), NaN when an offset is given.  A piece's record gains sum pw (277) and n+ (278).
#include "glm_dev.hpp"
#include "wave_tile_dev.hpp"

#include <algorithm>
#include <type_traits>

#ifndef PDS_GLM_REPORT_WO
#define PDS_GLM_REPORT_WO 0
#endif

namespace pds {

namespace {

constexpr int kGrStride = wave_tile_stride(64);  // doubles per feature row of the tile
constexpr int kGrG = 18;                         // row stride of the staged matrix (17 x 17: 16 features + bias)
constexpr int kGrLds = 16 * kGrStride + 64 + 18 + 17 * kGrG + 8;
constexpr double kGrZ975 = 1.959963984540054;

// The scalar sums of a group or a piece, in the order a piece's record holds them (from kGrRecSums on): sum w, sum (y - y0), pearson,
// deviance, the family sum of the null deviance; WO: then sum pw and the rows of positive weight (sy, pe, dv, fs weighted by pw)
enum GrSum { kGrSw, kGrSy, kGrPe, kGrDv, kGrFs, kGrSpw, kGrNpos, kGrSumMax };
template <bool WO>
constexpr int kGrSumCount = WO ? kGrSumMax : kGrSpw;
struct GrSums {
    double v[kGrSumMax];
    __device__ __forceinline__ double& operator[](int i) { return v[i]; }
    __device__ __forceinline__ double operator[](int i) const { return v[i]; }
};
// f(i) for i = 0 .. kGrSumCount<WO> - 1, i a constant in every call: the loop over a record's sums.  (Under a run-time loop the fold
// kernel's copy of the sums stays in memory until the optimiser has unrolled it, and its listing is no longer the spelt-out loads'.)
template <bool WO, int N = kGrSumCount<WO>, typename F>
__device__ __forceinline__ void gr_each_sum(F&& f) {
    if constexpr (N > 0) {
        gr_each_sum<WO, N - 1>(f);
        f(std::integral_constant<int, N - 1>{});
    }
}
constexpr int kGrRecSide = 256;              // a record: I [i * 16 + j], then X'w from here,
constexpr int kGrRecSums = kGrRecSide + 16;  // then the sums
static_assert(kGrRecSums + kGrSumMax <= kGlmReportRec, "a piece's record holds I, X'w and every sum");

// the wave-private carving of a block's LDS
struct GrLds {
    double *xt, *wt, *bs, *gm, *sm;
    __device__ explicit GrLds(double* base) : xt(base), wt(xt + 16 * kGrStride), bs(wt + 64), gm(bs + 18), sm(gm + 17 * kGrG) {}
};

// a term of a sum: weighted by pw in the WO form, as it is otherwise (no product by 1: the unweighted sums keep their operations)
template <bool WO>
__device__ __forceinline__ double gr_wt(double pw, double t) {
    if constexpr (WO) {
        return pw * t;
    } else {
        return t;
    }
}

// rows [r0, r1) of one group at the coefficients in l.bs: I into acc, X'w into column 0 of acc2, the sums (folded) into s
template <typename T, int P, bool WO>
__device__ __forceinline__ void gr_accumulate(const gptr<T> (&cx)[P], gptr<T> cy, int64_t r0, int64_t r1, double y0, int bias, int link,
                                              int variance, const GrLds& l, int lane, d4& acc, d4& acc2, GrSums& s,
                                              const T* pwp, const T* ofp) {
    double sw = 0.0, sy = 0.0, pe = 0.0, dv = 0.0, fs = 0.0;
    [[maybe_unused]] double spw = 0.0, npos = 0.0;
    for (int64_t base = r0; base < r1; base += 64) {
        const int64_t r = base + lane;
        const bool live = r < r1;
        PDS_WAVE_LDS_SYNC();  // (the previous step's operand reads are done)
        double eta = bias ? l.bs[P] : 0.0;
#pragma unroll
        for (int c = 0; c < P; ++c) {
            const double xv = live ? (double)cx[c][r] : 0.0;
            l.xt[c * kGrStride + lane] = xv;
            eta = fma(xv, l.bs[c], eta);
        }
        double w = 0.0;
        [[maybe_unused]] double pwv = 1.0;
        bool on = live;
        if constexpr (WO) {
            pwv = live ? (pwp ? (double)as_global(pwp)[r] : 1.0) : 0.0;
            if (live && ofp) eta += (double)as_global(ofp)[r];
            on = pwv > 0.0;  // (a row of weight 0 contributes nothing whatever its y holds)
        }
        if (on) {
            const double yv = (double)cy[r];
            const double mu = glm_inv<double>(link, eta);
            const double d = glm_deriv<double>(link, mu);
            const double v = glm_var<double>(variance, mu);
            w = (WO ? pwv : 1.0) / (d * d * v);
            const double e = yv - mu;
            pe += gr_wt<WO>(pwv, e * e / v);
            const double dy = yv - y0;
            sy += gr_wt<WO>(pwv, dy);
            if constexpr (WO) {
                spw += pwv;
                npos += 1.0;
            }
            switch (variance) {  // the deviance term (glm_unit_deviance) and the family sum's
                case 1:
                    dv += gr_wt<WO>(pwv, 2.0 * (glm_xlogy(yv, yv / mu) - e));
                    fs += gr_wt<WO>(pwv, glm_xlogy(yv, yv));
                    break;
                case 2:
                    dv += gr_wt<WO>(pwv, 2.0 * (glm_xlogy(yv, yv / mu) + glm_xlogy(1.0 - yv, (1.0 - yv) / (1.0 - mu))));
                    fs += gr_wt<WO>(pwv, glm_xlogy(yv, yv) + glm_xlogy(1.0 - yv, 1.0 - yv));
                    break;
                case 3:
                    dv += gr_wt<WO>(pwv, 2.0 * (e / mu - log(yv / mu)));
                    fs += gr_wt<WO>(pwv, log(yv));
                    break;
                default:
                    dv += gr_wt<WO>(pwv, e * e);
                    fs += gr_wt<WO>(pwv, dy * dy);
                    break;
            }
        }
        sw += w;
        l.wt[lane] = w;
        PDS_WAVE_LDS_SYNC();
        wave_tile_gram<P>(
            l.xt, kGrStride, (int)std::min<int64_t>(64, r1 - base), lane, [&](int row) { return l.wt[row]; },
            [&](int c, int row, double wv) { return c == 0 ? wv : 0.0; },  // B column 0 = w: the bias row X'w
            acc, acc2);
    }
    s[kGrSw] = wave_sum(sw);
    s[kGrSy] = wave_sum(sy);
    s[kGrPe] = wave_sum(pe);
    s[kGrDv] = wave_sum(dv);
    s[kGrFs] = wave_sum(fs);
    if constexpr (WO) {
        s[kGrSpw] = wave_sum(spw);
        s[kGrNpos] = wave_sum(npos);
    }
}

// every report field of group g NaN, report_null = 1
template <typename T>
__device__ __forceinline__ void gr_write_null(const GlmReportDev<T>& o, int64_t g, int64_t n, int pp, int lane) {
    const T nanv = (T)__builtin_nan("");
    if (lane < pp) {
        const int64_t at = g * pp + lane;
        if (o.se) o.se[at] = nanv;
        if (o.z) o.z[at] = nanv;
        if (o.p) o.p[at] = nanv;
        if (o.lo) o.lo[at] = nanv;
        if (o.hi) o.hi[at] = nanv;
    }
    if (o.cov)
        for (int e = lane; e < pp * pp; e += 64) o.cov[g * pp * pp + e] = nanv;
    if (lane == 0) {
        if (o.deviance) o.deviance[g] = nanv;
        if (o.null_deviance) o.null_deviance[g] = nanv;
        if (o.pearson) o.pearson[g] = nanv;
        if (o.dispersion) o.dispersion[g] = nanv;
        if (o.df_resid) o.df_resid[g] = n - pp;
        if (o.report_null) o.report_null[g] = 1;
    }
}

// l.gm holds I (index 16 = bias), l.bs the coefficients, s the group's sums: invert, derive, write
template <typename T, int P, bool WO>
__device__ __forceinline__ void gr_epilogue(const GlmReportDev<T>& o, int64_t g, int64_t n, int bias, int variance, double y0, const GrLds& l,
                                            const GrSums& s, int lane, bool has_offset) {
    const int pp = P + bias, ne = pp * pp;
    auto m = [](int j) { return j < P ? j : 16; };
    bool bad = false;
    for (int k = 0; k < pp; ++k) {
        const int mk = m(k);
        const double d = l.gm[mk * kGrG + mk];
        if (!(d > 0.0) || !(d <= 1.79769313486231570e308)) bad = true;  // (wave-uniform: every lane reads the same pivot)
        const double pv = 1.0 / d;
        double nv[5];
#pragma unroll
        for (int t = 0; t < 5; ++t) {
            const int e = lane + 64 * t;
            nv[t] = 0.0;
            if (e < ne) {
                const int i = e / pp, j = e - i * pp;
                const double aik = l.gm[m(i) * kGrG + mk], akj = l.gm[mk * kGrG + m(j)], aij = l.gm[m(i) * kGrG + m(j)];
                nv[t] = i == k ? (j == k ? pv : akj * pv) : (j == k ? -(aik * pv) : fma(-aik, akj * pv, aij));
            }
        }
        PDS_WAVE_LDS_SYNC();
#pragma unroll
        for (int t = 0; t < 5; ++t) {
            const int e = lane + 64 * t;
            if (e < ne) {
                const int i = e / pp, j = e - i * pp;
                l.gm[m(i) * kGrG + m(j)] = nv[t];
            }
        }
        PDS_WAVE_LDS_SYNC();
    }
    if (bad) {
        gr_write_null<T>(o, g, n, pp, lane);
        return;
    }
    const double nanv = __builtin_nan("");
    const double nn = WO ? s[kGrSpw] : (double)n;  // (WO: sum pw stands where the row count stood; sy, fs are weighted)
    const int64_t df = (WO ? (int64_t)s[kGrNpos] : n) - pp;
    const double phi = (variance == 1 || variance == 2) ? 1.0 : (df > 0 ? s[kGrPe] / (double)df : nanv);
    const double sy = s[kGrSy] + nn * y0;  // sum y
    double nd;
    if (bias) {
        const double ym = sy / nn;
        switch (variance) {
            case 1: nd = 2.0 * (s[kGrFs] - glm_xlogy(sy, ym)); break;
            case 2: nd = 2.0 * (s[kGrFs] - glm_xlogy(sy, ym) - glm_xlogy(nn - sy, 1.0 - ym)); break;
            case 3: nd = 2.0 * (nn * log(ym) - s[kGrFs]); break;
            default: nd = s[kGrFs] - s[kGrSy] * s[kGrSy] / nn; break;
        }
    } else {
        switch (variance) {
            case 1: nd = 2.0 * (s[kGrFs] - sy + nn); break;
            case 2: nd = 2.0 * (s[kGrFs] + nn * 0.693147180559945309417); break;
            case 3: nd = nanv; break;
            default: nd = s[kGrFs]; break;  // (y0 = 0 without a bias: sum y^2)
        }
    }
    if (WO && has_offset) nd = nanv;  // (the intercept-only model under an offset needs an iteration of its own)
    if (lane < pp) {
        const int mj = m(lane);
        const double b = l.bs[lane];  // (the bias sits at bs[P] = bs[lane])
        const double se = sqrt(phi * l.gm[mj * kGrG + mj]);
        const double z = b / se;
        const int64_t at = g * pp + lane;
        if (o.se) o.se[at] = (T)se;
        if (o.z) o.z[at] = (T)z;
        if (o.p) o.p[at] = (T)erfc(fabs(z) * 0.707106781186547524401);
        if (o.lo) o.lo[at] = (T)(b - kGrZ975 * se);
        if (o.hi) o.hi[at] = (T)(b + kGrZ975 * se);
    }
    if (o.cov)
        for (int e = lane; e < ne; e += 64) {
            const int i = e / pp, j = e - i * pp;
            o.cov[g * ne + e] = (T)(phi * l.gm[m(i) * kGrG + m(j)]);
        }
    if (lane == 0) {
        if (o.deviance) o.deviance[g] = (T)s[kGrDv];
        if (o.null_deviance) o.null_deviance[g] = (T)nd;
        if (o.pearson) o.pearson[g] = (T)s[kGrPe];
        if (o.dispersion) o.dispersion[g] = (T)phi;
        if (o.df_resid) o.df_resid[g] = df;
        if (o.report_null) o.report_null[g] = 0;
    }
}

template <typename T, int P>
__device__ __forceinline__ void gr_load_beta(const T* __restrict__ coeffs, int64_t g, int bias, const GrLds& l, int lane) {
    const int pp = P + bias;
    PDS_WAVE_LDS_SYNC();  // (the previous group's reads are done)
    if (lane < pp) l.bs[lane] = (double)coeffs[g * pp + lane];  // (the bias, last, lands at bs[P], where eta reads it)
    PDS_WAVE_LDS_SYNC();
}

// a group for the piece route: appended to the list (the order does not matter: the host sorts it)
__device__ __forceinline__ void gr_append_long(int64_t* long_list, unsigned* long_count, int64_t long_cap, int64_t g, int lane) {
    if (lane == 0) {
        const unsigned k = atomicAdd(long_count, 1u);
        if ((int64_t)k < long_cap) long_list[k] = g;
    }
}

// the shift of the gaussian sums: the group's first y with a bias (the mean is the null model), nothing otherwise
template <typename T>
__device__ __forceinline__ double gr_shift(gptr<T> cy, int64_t first_row, int bias, int variance) {
    return (variance == 0 && bias) ? (double)cy[first_row] : 0.0;
}

// WO: ... the group's first y of positive weight (the same row for every piece of a group: the scan starts at the group's first row)
template <typename T>
__device__ __forceinline__ double gr_shift_wo(gptr<T> cy, const T* pwp, int64_t r0, int64_t r1, int bias, int variance, int lane) {
    if (!(variance == 0 && bias)) return 0.0;
    if (!pwp) return (double)cy[r0];
    for (int64_t base = r0; base < r1; base += 64) {
        const int64_t r = base + lane;
        const unsigned long long m = __ballot(r < r1 && (double)as_global(pwp)[r] > 0.0);
        if (m) return (double)cy[base + (__ffsll((long long)m) - 1)];
    }
    return 0.0;
}

// WO: cols[P + 1] = pw, cols[P + 2] = o (each nullable); the unweighted table ends at y and is not read beyond it
template <typename T, int P, bool WO>
struct GrWoCols {
    const T *pw = nullptr, *of = nullptr;
    __device__ explicit GrWoCols(const T* const* __restrict__ cols) {
        if constexpr (WO) {
            pw = cols[P + 1];
            of = cols[P + 2];
        }
    }
    // the shift of the group of rows [r0, r1)
    __device__ __forceinline__ double shift(gptr<T> cy, int64_t r0, int64_t r1, int bias, int variance, int lane) const {
        if constexpr (WO) {
            return gr_shift_wo<T>(cy, pw, r0, r1, bias, variance, lane);
        } else {
            return gr_shift<T>(cy, r0, bias, variance);
        }
    }
};

template <typename T, int P, bool WO>
__global__ __launch_bounds__(64) void grouped_glm_report_kernel(const T* const* __restrict__ cols, int bias, int64_t n_rows,
                                                                const int64_t* __restrict__ off, int64_t n_groups, int link,
                                                                int variance, int64_t split_rows, const T* __restrict__ coeffs,
                                                                const uint8_t* __restrict__ is_null, GlmReportDev<T> o,
                                                                int64_t* __restrict__ long_list, unsigned* __restrict__ long_count,
                                                                int64_t long_cap) {
    __shared__ double lds[kGrLds];
    const GrLds l(lds);
    const int lane = threadIdx.x;
    const int pp = P + bias;
    gptr<T> cx[P];
#pragma unroll
    for (int c = 0; c < P; ++c) cx[c] = as_global(cols[c]);
    const gptr<T> cy = as_global(cols[P]);
    const GrWoCols<T, P, WO> wc(cols);
    for (int64_t g = blockIdx.x; g < n_groups; g += gridDim.x) {
        const int64_t r0 = off[g], n = off[g + 1] - r0;
        const bool bad = r0 < 0 || n < 0 || r0 + n > n_rows;  // (offsets that leave the frame: nothing is read)
        if (bad || n < pp || is_null[g]) {  // (WO: a group that fails the weight rule is a null fit)
            gr_write_null<T>(o, g, bad ? 0 : n, pp, lane);
            continue;
        }
        if (n > split_rows) {  // the piece route (the order of the list does not matter: the host sorts it)
            gr_append_long(long_list, long_count, long_cap, g, lane);
            continue;
        }
        gr_load_beta<T, P>(coeffs, g, bias, l, lane);
        const double y0 = wc.shift(cy, r0, r0 + n, bias, variance, lane);
        d4 acc = {0.0, 0.0, 0.0, 0.0}, acc2 = {0.0, 0.0, 0.0, 0.0};
        GrSums s;
        gr_accumulate<T, P, WO>(cx, cy, r0, r0 + n, y0, bias, link, variance, l, lane, acc, acc2, s, wc.pw, wc.of);
        PDS_WAVE_LDS_SYNC();
        wave_tile_for_d(
            lane,
            [&](int i, int c, double v, double side) {
                l.gm[i * kGrG + c] = v;
                if (c == 0) {
                    l.gm[i * kGrG + 16] = side;
                    l.gm[16 * kGrG + i] = side;
                }
            },
            acc, acc2);
        if (lane == 0) l.gm[16 * kGrG + 16] = s[kGrSw];
        PDS_WAVE_LDS_SYNC();
        gr_epilogue<T, P, WO>(o, g, n, bias, variance, y0, l, s, lane, wc.of != nullptr);
    }
}

// piece k = rows [pieces[3 k + 1], pieces[3 k + 2]) of group pieces[3 k]: its record rec[k * kGlmReportRec ..]
template <typename T, int P, bool WO>
__global__ __launch_bounds__(64) void grouped_glm_report_piece_kernel(const T* const* __restrict__ cols, int bias,
                                                                      const int64_t* __restrict__ off, int link, int variance,
                                                                      const T* __restrict__ coeffs, const int64_t* __restrict__ pieces,
                                                                      int64_t n_pieces, double* __restrict__ rec) {
    __shared__ double lds[kGrLds];
    const GrLds l(lds);
    const int lane = threadIdx.x;
    gptr<T> cx[P];
#pragma unroll
    for (int c = 0; c < P; ++c) cx[c] = as_global(cols[c]);
    const gptr<T> cy = as_global(cols[P]);
    const GrWoCols<T, P, WO> wc(cols);
    for (int64_t k = blockIdx.x; k < n_pieces; k += gridDim.x) {
        const int64_t g = pieces[3 * k], r0 = pieces[3 * k + 1], r1 = pieces[3 * k + 2];
        gr_load_beta<T, P>(coeffs, g, bias, l, lane);
        const double y0 = wc.shift(cy, off[g], off[g + 1], bias, variance, lane);  // (the group's, not the piece's)
        d4 acc = {0.0, 0.0, 0.0, 0.0}, acc2 = {0.0, 0.0, 0.0, 0.0};
        GrSums s;
        gr_accumulate<T, P, WO>(cx, cy, r0, r1, y0, bias, link, variance, l, lane, acc, acc2, s, wc.pw, wc.of);
        double* out = rec + k * kGlmReportRec;
        wave_tile_for_d(
            lane,
            [&](int i, int c, double v, double side) {
                out[i * 16 + c] = v;
                if (c == 0) out[kGrRecSide + i] = side;
            },
            acc, acc2);
        if (lane == 0) {
            gr_each_sum<WO>([&](auto i) { out[kGrRecSums + i] = s[i]; });
        }
    }
}

// long group j = fin[3 j]: its records fin[3 j + 1] .. + fin[3 j + 2], added in piece order, then the epilogue of the one-wave route
template <typename T, int P, bool WO>
__global__ __launch_bounds__(64) void grouped_glm_report_fold_kernel(const T* const* __restrict__ cols, int bias,
                                                                     const int64_t* __restrict__ off, int variance,
                                                                     const T* __restrict__ coeffs, const int64_t* __restrict__ fin,
                                                                     int64_t n_fin, const double* __restrict__ rec, GlmReportDev<T> o) {
    __shared__ double lds[kGrLds];
    const GrLds l(lds);
    const int lane = threadIdx.x;
    const gptr<T> cy = as_global(cols[P]);
    const GrWoCols<T, P, WO> wc(cols);
    for (int64_t j = blockIdx.x; j < n_fin; j += gridDim.x) {
        const int64_t g = fin[3 * j], first = fin[3 * j + 1], cnt = fin[3 * j + 2];
        gr_load_beta<T, P>(coeffs, g, bias, l, lane);
        for (int e = lane; e < kGrRecSums + kGrSumCount<WO>; e += 64) {
            double v = 0.0;
            for (int64_t k = 0; k < cnt; ++k) v += rec[(first + k) * kGlmReportRec + e];
            if (e < kGrRecSide) {
                l.gm[(e >> 4) * kGrG + (e & 15)] = v;
            } else if (e < kGrRecSums) {
                l.gm[(e - kGrRecSide) * kGrG + 16] = v;
                l.gm[16 * kGrG + (e - kGrRecSide)] = v;
            } else {
                if (e == kGrRecSums + kGrSw) l.gm[16 * kGrG + 16] = v;
                l.sm[e - kGrRecSums] = v;
            }
        }
        PDS_WAVE_LDS_SYNC();
        GrSums s;
        gr_each_sum<WO>([&](auto i) { s[i] = l.sm[i]; });
        const int64_t r0 = off[g], r1 = off[g + 1];
        gr_epilogue<T, P, WO>(o, g, r1 - r0, bias, variance, wc.shift(cy, r0, r1, bias, variance, lane), l, s, lane,
                              wc.of != nullptr);
    }
}

}  // namespace

// What each of the two objects exports: the launches of its own kernels, WO = PDS_GLM_REPORT_WO
template <typename T, bool WO>
struct GroupedGlmReportSet {
    static int launch(pds_ctx* ctx, const GlmGroupsDev<T>& gr, const T* d_coeffs, const uint8_t* d_null, const GlmReportDev<T>& out,
                      const GlmLongList& ll);
    static int launch_pieces(pds_ctx* ctx, const GlmGroupsDev<T>& gr, const T* d_coeffs, const GlmReportDev<T>& out, const int64_t* d_pieces,
                             int64_t n_pieces, const int64_t* d_fin, int64_t n_fin, double* d_rec);
};

template <typename T, bool WO>
int GroupedGlmReportSet<T, WO>::launch(pds_ctx* ctx, const GlmGroupsDev<T>& gr, const T* d_coeffs, const uint8_t* d_null,
                                       const GlmReportDev<T>& out, const GlmLongList& ll) {
    KernelTimer timer(ctx, kKindPass2);
    const int nb = (int)std::min<int64_t>(gr.n_groups, (int64_t)ctx->num_cus * 32);
    dispatch_width<1, kMaxFeatSmall>(gr.n_feat, [&](auto pc) {
        hipLaunchKernelGGL((grouped_glm_report_kernel<T, decltype(pc)::value, WO>), dim3(nb), dim3(64), 0, ctx->stream, gr.d_cols, gr.bias,
                           gr.n_rows, gr.d_off, gr.n_groups, gr.link, gr.variance, gr.split_rows, d_coeffs, d_null, out, ll.d_list,
                           ll.d_count, ll.cap);
    });
    PDS_HIP_CHECK(hipGetLastError());
    return PDS_OK;
}

template <typename T, bool WO>
int GroupedGlmReportSet<T, WO>::launch_pieces(pds_ctx* ctx, const GlmGroupsDev<T>& gr, const T* d_coeffs, const GlmReportDev<T>& out,
                                              const int64_t* d_pieces, int64_t n_pieces, const int64_t* d_fin, int64_t n_fin,
                                              double* d_rec) {
    KernelTimer timer(ctx, kKindPass2);
    const int nbp = (int)std::min<int64_t>(n_pieces, (int64_t)ctx->num_cus * 32);
    const int nbf = (int)std::min<int64_t>(n_fin, (int64_t)ctx->num_cus * 32);
    dispatch_width<1, kMaxFeatSmall>(gr.n_feat, [&](auto pc) {
        constexpr int P = decltype(pc)::value;
        hipLaunchKernelGGL((grouped_glm_report_piece_kernel<T, P, WO>), dim3(nbp), dim3(64), 0, ctx->stream, gr.d_cols, gr.bias, gr.d_off,
                           gr.link, gr.variance, d_coeffs, d_pieces, n_pieces, d_rec);
        hipLaunchKernelGGL((grouped_glm_report_fold_kernel<T, P, WO>), dim3(nbf), dim3(64), 0, ctx->stream, gr.d_cols, gr.bias, gr.d_off,
                           gr.variance, d_coeffs, d_fin, n_fin, d_rec, out);
    });
    PDS_HIP_CHECK(hipGetLastError());
    return PDS_OK;
}
template struct GroupedGlmReportSet<double, PDS_GLM_REPORT_WO != 0>;
template struct GroupedGlmReportSet<float, PDS_GLM_REPORT_WO != 0>;

#if !PDS_GLM_REPORT_WO
extern template struct GroupedGlmReportSet<double, true>;  // (grouped_glm_report_wo.hip)
extern template struct GroupedGlmReportSet<float, true>;

template <typename T>
int launch_grouped_glm_report(pds_ctx* ctx, const GlmGroupsDev<T>& groups, const T* d_coeffs, const uint8_t* d_null,
                              const GlmReportDev<T>& out, const GlmLongList& long_list) {
    if (groups.n_groups <= 0) return PDS_OK;
    if (groups.n_feat < 1 || groups.n_feat > kMaxFeatSmall) return fail(PDS_ERR_UNSUPPORTED, "grouped GLM report: up to 16 feature columns");
    return groups.wo ? GroupedGlmReportSet<T, true>::launch(ctx, groups, d_coeffs, d_null, out, long_list)
                     : GroupedGlmReportSet<T, false>::launch(ctx, groups, d_coeffs, d_null, out, long_list);
}

template <typename T>
int launch_grouped_glm_report_pieces(pds_ctx* ctx, const GlmGroupsDev<T>& groups, const T* d_coeffs, const GlmReportDev<T>& out,
                                     const int64_t* d_pieces, int64_t n_pieces, const int64_t* d_fin, int64_t n_fin, double* d_rec) {
    if (n_pieces <= 0 || n_fin <= 0) return PDS_OK;
    if (groups.n_feat < 1 || groups.n_feat > kMaxFeatSmall) return fail(PDS_ERR_UNSUPPORTED, "grouped GLM report: up to 16 feature columns");
    return groups.wo ? GroupedGlmReportSet<T, true>::launch_pieces(ctx, groups, d_coeffs, out, d_pieces, n_pieces, d_fin, n_fin, d_rec)
                     : GroupedGlmReportSet<T, false>::launch_pieces(ctx, groups, d_coeffs, out, d_pieces, n_pieces, d_fin, n_fin, d_rec);
}

template int launch_grouped_glm_report<double>(pds_ctx*, const GlmGroupsDev<double>&, const double*, const uint8_t*, const GlmReportDev<double>&,
                                               const GlmLongList&);
template int launch_grouped_glm_report<float>(pds_ctx*, const GlmGroupsDev<float>&, const float*, const uint8_t*, const GlmReportDev<float>&,
                                              const GlmLongList&);
template int launch_grouped_glm_report_pieces<double>(pds_ctx*, const GlmGroupsDev<double>&, const double*, const GlmReportDev<double>&,
                                                      const int64_t*, int64_t, const int64_t*, int64_t, double*);
template int launch_grouped_glm_report_pieces<float>(pds_ctx*, const GlmGroupsDev<float>&, const float*, const GlmReportDev<float>&,
                                                     const int64_t*, int64_t, const int64_t*, int64_t, double*);
#endif

}  // namespace pds
