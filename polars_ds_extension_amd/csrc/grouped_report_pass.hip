// grouped_report_pass.hip -- the second half of lin_reg_report for every group of a frame at once (the grouped report,
// capi_report_grouped.hpp): what `df.group_by(key).agg(pds.lin_reg_report(...))` makes the reference do one group at a time
// (linear_regression.rs:848-939 per group).
//
// Pass 1 (grouped Gram records + pivoted-QR solve with (X'X)^-1) is the grouped fit's own machinery.  This file adds
//   grouped_report_pass_kernel       <= 16 features: residuals, y sums and the HC meat of every group in one stream
//   grouped_report_pass_wide_kernel  17 .. 64 features: the same at run-time width
//   grouped_report_epilogue_kernel   report_epilogue's formulas per coefficient (se, t, p, CI) and group (r2, adj_r2)
//
// Layout of the <= 16-feature pass: one wave per work item (a group, or a piece of a group longer than piece_rows -- see
// report_item and grouped_report_finish_kernel), 64 rows per step, lane = row.  A lane loads its row (column-major frame:
// 512 contiguous bytes per column and wave), forms e = y - x.beta_g (beta_g staged in wave-private LDS), the leverage
// h = z' inv_g z for HC2 / HC3 (inv_g in LDS, broadcast reads) and the row weight s.  The meat's 16 x 16 feature block goes to the
// matrix cores by the wave-tile idiom of wave_tile_dev.hpp (A = s x, B = x, no side columns); the bias row of the meat (sum s x,
// sum s) stays in per-lane registers.  Every sum is a per-lane register folded by a fixed butterfly at the end of the group: no
// atomics, repeated calls are bit-identical.
//
// WEIGHTED (the grouped wls_report, plain standard error only -- pl_wls_report knows no HC estimator, linear_regression.rs:982-1117):
// cols[p + 1] is the weight column, loaded like one more column of the frame, and the fourth value of an item's sums slot carries
// sum w e^2 (the mse's numerator); sum e^2 and the y sums stay unweighted, as the reference's r2 has them.
#include "grouped_report.hpp"
#include "stats_dev.hpp"
#include "wave_tile_dev.hpp"

#include <algorithm>
#include <type_traits>

namespace pds {

namespace {

constexpr int kRpThreads = 256;
constexpr int kRpStride = 65;  // doubles per feature row of the transposed tile (64 rows + 1: conflict-free column writes)
constexpr int kRpWaveDoubles = 16 * kRpStride + 64 + 17 + 17 * 17;  // tile, row weights, beta_g, inv_g

// Work item `it` of the pass: items 0 .. n_groups - 1 are the groups themselves (at most `piece_rows` of their rows -- a group's
// first piece), items n_groups + k the k-th extra piece of a larger group (pieces[3 k ..]: group, first row, end row).  Every item
// writes its own sums / meat slot; grouped_report_finish_kernel adds a split group's extra slots to its first one in piece order.
__device__ __forceinline__ bool report_item(int64_t it, const int64_t* __restrict__ off, int64_t n_groups, int pp,
                                            const int64_t* __restrict__ pieces, int64_t piece_rows, int64_t* g, int64_t* r0,
                                            int64_t* r1) {
    if (it < n_groups) {
        *g = it;
        *r0 = off[it];
        const int64_t e = off[it + 1];
        if (e - *r0 < pp) return false;  // null group: the epilogue reads nothing of it
        *r1 = e - *r0 > piece_rows ? *r0 + piece_rows : e;
        return true;
    }
    const int64_t* pc = pieces + 3 * (it - n_groups);
    *g = pc[0];
    *r0 = pc[1];
    *r1 = pc[2];
    return true;
}

template <typename T, int P, bool WEIGHTED = false>
__global__ __launch_bounds__(kRpThreads) void grouped_report_pass_kernel(const T* const* __restrict__ cols, int bias,
                                                                         const int64_t* __restrict__ off, int64_t n_groups,
                                                                         const T* __restrict__ beta, const T* __restrict__ inv,
                                                                         int hc, double* __restrict__ sums, double* __restrict__ meat,
                                                                         const int64_t* __restrict__ pieces, int64_t n_items,
                                                                         int64_t piece_rows) {
    __shared__ double lds[kRpThreads / 64][kRpWaveDoubles];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int pp = P + bias;
    double* xt = lds[wv];
    double* st = xt + 16 * kRpStride;
    double* bs = st + 64;
    double* is = bs + 17;
    for (int i = P * kRpStride + lane; i < 16 * kRpStride; i += 64) xt[i] = 0.0;  // feature rows P .. 15 stay zero
    gptr<T> cx[P];
#pragma unroll
    for (int c = 0; c < P; ++c) cx[c] = as_global(cols[c]);
    const gptr<T> cy = as_global(cols[P]);
    const gptr<T> cw = as_global(cols[WEIGHTED ? P + 1 : P]);
    const int64_t nwaves = (int64_t)gridDim.x * (kRpThreads / 64);
    for (int64_t it = (int64_t)blockIdx.x * (kRpThreads / 64) + wv; it < n_items; it += nwaves) {
        int64_t g, r0, r1;
        if (!report_item(it, off, n_groups, pp, pieces, piece_rows, &g, &r0, &r1)) continue;
        PDS_WAVE_LDS_SYNC();  // (the previous group's reads are done)
        for (int i = lane; i < pp; i += 64) bs[i] = (double)beta[g * pp + i];
        if (hc >= 2)
            for (int i = lane; i < pp * pp; i += 64) is[i] = (double)inv[g * pp * pp + i];
        PDS_WAVE_LDS_SYNC();
        const double y0 = (double)cy[off[g]];  // (the group's first row: the pieces' shifted sums add up)
        double sse = 0.0, sy = 0.0, syy = 0.0, ss = 0.0, swe = 0.0;
        double sb[P];
#pragma unroll
        for (int c = 0; c < P; ++c) sb[c] = 0.0;
        d4 acc = {0.0, 0.0, 0.0, 0.0};
        for (int64_t base = r0; base < r1; base += 64) {
            const int64_t r = base + lane;
            const bool live = r < r1;
            double x[P];
#pragma unroll
            for (int c = 0; c < P; ++c) x[c] = live ? (double)cx[c][r] : 0.0;
            const double yv = live ? (double)cy[r] : 0.0;
            double wr = 0.0;
            if constexpr (WEIGHTED) wr = live ? (double)cw[r] : 0.0;
            double pr = bias ? bs[P] : 0.0;
#pragma unroll
            for (int c = 0; c < P; ++c) pr = fma(x[c], bs[c], pr);
            const double e = live ? yv - pr : 0.0;
            const double e2 = e * e;
            sse += e2;
            if constexpr (WEIGHTED) swe += live ? wr * e2 : 0.0;
            const double dy = live ? yv - y0 : 0.0;
            sy += dy;
            syy += dy * dy;
            if (hc) {
                double s = e2;
                if (hc >= 2) {
                    double h = 0.0;
#pragma unroll
                    for (int b = 0; b < P + 1; ++b) {
                        if (b == P && !bias) break;
                        const double zb = b < P ? x[b] : 1.0;
                        double t = bias ? is[P + b * pp] : 0.0;
#pragma unroll
                        for (int a = 0; a < P; ++a) t = fma(is[a + b * pp], x[a], t);
                        h = fma(zb, t, h);
                    }
                    const double omh = 1.0 - h;
                    s = live ? (hc == 2 ? e2 / omh : e2 / (omh * omh)) : 0.0;
                }
#pragma unroll
                for (int c = 0; c < P; ++c) sb[c] = fma(s, x[c], sb[c]);
                ss += s;
                PDS_WAVE_LDS_SYNC();  // (the previous step's operand reads are done)
#pragma unroll
                for (int c = 0; c < P; ++c) xt[c * kRpStride + lane] = x[c];
                st[lane] = s;
                PDS_WAVE_LDS_SYNC();
                // (all 16 feature rows are read: rows P .. 15 are zero)
                wave_tile_gram<16>(xt, kRpStride, (int)std::min<int64_t>(64, r1 - base), lane, [&](int row) { return st[row]; }, acc);
            }
        }
        sse = wave_sum(sse);
        sy = wave_sum(sy);
        syy = wave_sum(syy);
        if constexpr (WEIGHTED) swe = wave_sum(swe);
        if (lane == 0) {
            sums[it * 4 + 0] = sse;
            sums[it * 4 + 1] = sy;
            sums[it * 4 + 2] = syy;
            sums[it * 4 + 3] = swe;
        }
        if (hc) {
            double* mo = meat + it * pp * pp;
            wave_tile_for_d(
                lane,
                [&](int i, int c, double v) {
                    if (i < P && c < P) mo[i + c * pp] = v;
                },
                acc);
            ss = wave_sum(ss);
#pragma unroll
            for (int c = 0; c < P; ++c) {
                const double v = wave_sum(sb[c]);
                if (bias && lane == 0) {
                    mo[c + P * pp] = v;
                    mo[P + c * pp] = v;
                }
            }
            if (bias && lane == 0) mo[P + P * pp] = ss;
        }
    }
}

// 17 .. 64 features: one wave per group, the 64-row step staged row-major in LDS, the meat's upper triangle owned lane by lane
// (entry t = lane + 64 j) and accumulated in LDS over the rows of each step
constexpr int kRwStride = 65;
constexpr int kRwTri = 65 * 66 / 2;

template <typename T, bool WEIGHTED = false>
__global__ __launch_bounds__(64) void grouped_report_pass_wide_kernel(const T* const* __restrict__ cols, int p, int bias,
                                                                      const int64_t* __restrict__ off, int64_t n_groups,
                                                                      const T* __restrict__ beta, const T* __restrict__ inv, int hc,
                                                                      double* __restrict__ sums, double* __restrict__ meat,
                                                                      const int64_t* __restrict__ pieces, int64_t n_items,
                                                                      int64_t piece_rows) {
    __shared__ double bs[65];
    __shared__ double xt[64 * kRwStride];
    __shared__ double st[64];
    __shared__ double macc[kRwTri];
    const int lane = threadIdx.x;
    const int pp = p + bias, ntri = pp * (pp + 1) / 2;
    const gptr<T> cy = as_global(cols[p]);
    for (int64_t it = blockIdx.x; it < n_items; it += gridDim.x) {
        int64_t g, r0, r1;
        if (!report_item(it, off, n_groups, pp, pieces, piece_rows, &g, &r0, &r1)) continue;
        PDS_WAVE_LDS_SYNC();
        for (int i = lane; i < pp; i += 64) bs[i] = (double)beta[g * pp + i];
        for (int t = lane; t < ntri; t += 64) macc[t] = 0.0;
        PDS_WAVE_LDS_SYNC();
        const T* ig = inv + g * pp * pp;
        const double y0 = (double)cy[off[g]];  // (the group's first row: the pieces' shifted sums add up)
        double sse = 0.0, sy = 0.0, syy = 0.0, swe = 0.0;
        double* xr = xt + lane * kRwStride;
        for (int64_t base = r0; base < r1; base += 64) {
            const int64_t r = base + lane;
            const bool live = r < r1;
            double pr = bias ? bs[p] : 0.0;
            PDS_WAVE_LDS_SYNC();  // (the previous step's reads of the tile are done)
            for (int c = 0; c < p; ++c) {
                const double xv = live ? (double)as_global(cols[c])[r] : 0.0;
                xr[c] = xv;
                pr = fma(xv, bs[c], pr);
            }
            if (bias) xr[p] = live ? 1.0 : 0.0;
            const double yv = live ? (double)cy[r] : 0.0;
            const double e = live ? yv - pr : 0.0;
            const double e2 = e * e;
            sse += e2;
            if constexpr (WEIGHTED) swe += live ? (double)as_global(cols[p + 1])[r] * e2 : 0.0;
            const double dy = live ? yv - y0 : 0.0;
            sy += dy;
            syy += dy * dy;
            if (!hc) continue;
            double s = e2;
            if (hc >= 2) {
                double h = 0.0;
                for (int b = 0; b < pp; ++b) {
                    double t = 0.0;
                    for (int a = 0; a < pp; ++a) t = fma((double)ig[a + b * pp], xr[a], t);
                    h = fma(xr[b], t, h);
                }
                const double omh = 1.0 - h;
                s = live ? (hc == 2 ? e2 / omh : e2 / (omh * omh)) : 0.0;
            }
            st[lane] = s;
            PDS_WAVE_LDS_SYNC();
            const int nv = (int)std::min<int64_t>(64, r1 - base);
            for (int t = lane; t < ntri; t += 64) {
                int b = (int)((sqrt(8.0 * t + 1.0) - 1.0) * 0.5);
                while (b * (b + 1) / 2 > t) --b;
                while ((b + 1) * (b + 2) / 2 <= t) ++b;
                const int a = t - b * (b + 1) / 2;
                double v = macc[t];
                for (int row = 0; row < nv; ++row) v = fma(st[row] * xt[row * kRwStride + a], xt[row * kRwStride + b], v);
                macc[t] = v;
            }
        }
        sse = wave_sum(sse);
        sy = wave_sum(sy);
        syy = wave_sum(syy);
        if constexpr (WEIGHTED) swe = wave_sum(swe);
        if (lane == 0) {
            sums[it * 4 + 0] = sse;
            sums[it * 4 + 1] = sy;
            sums[it * 4 + 2] = syy;
            sums[it * 4 + 3] = swe;
        }
        if (hc) {
            PDS_WAVE_LDS_SYNC();
            double* mo = meat + it * pp * pp;
            for (int t = lane; t < ntri; t += 64) {
                int b = (int)((sqrt(8.0 * t + 1.0) - 1.0) * 0.5);
                while (b * (b + 1) / 2 > t) --b;
                while ((b + 1) * (b + 2) / 2 <= t) ++b;
                const int a = t - b * (b + 1) / 2;
                mo[a + b * pp] = macc[t];
                mo[b + a * pp] = macc[t];
            }
        }
    }
}

// split groups: slot of the group += its extra pieces' slots, in piece order (fin[3 j ..]: group, first extra item, count) -- a fixed
// order, so the result does not depend on which wave finished first
// (nsum: 3 sums per slot, 4 when the slot's fourth value carries sum w e^2)
__global__ __launch_bounds__(256) void grouped_report_finish_kernel(const int64_t* __restrict__ fin, int64_t n_fin, int pp, int hc,
                                                                    int nsum, double* __restrict__ sums, double* __restrict__ meat) {
    const int per = nsum + (hc ? pp * pp : 0);
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_fin * per) return;
    const int64_t j = i / per;
    const int e = (int)(i - j * per);
    const int64_t g = fin[3 * j], first = fin[3 * j + 1], cnt = fin[3 * j + 2];
    if (e < nsum) {
        double v = sums[g * 4 + e];
        for (int64_t k = 0; k < cnt; ++k) v += sums[(first + k) * 4 + e];
        sums[g * 4 + e] = v;
    } else {
        const int64_t m = e - nsum, sz = (int64_t)pp * pp;
        double v = meat[g * sz + m];
        for (int64_t k = 0; k < cnt; ++k) v += meat[(first + k) * sz + m];
        meat[g * sz + m] = v;
    }
}

__device__ __forceinline__ void dof_lookup(const ReportDofTable& tab, int64_t k, double* ta, double* lng) {
    if (k >= 0 && k < tab.dense_len) {
        *ta = tab.dense[2 * k];
        *lng = tab.dense[2 * k + 1];
        return;
    }
    int64_t lo = 0, hi = tab.n_large;  // first key >= k
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (tab.large_keys[mid] < k) lo = mid + 1;
        else hi = mid;
    }
    if (lo < tab.n_large && tab.large_keys[lo] == k) {
        *ta = tab.large[2 * lo];
        *lng = tab.large[2 * lo + 1];
    } else {
        *ta = __builtin_nan("");
        *lng = __builtin_nan("");
    }
}

// one thread per (group, coefficient) -- the p-value's continued fraction is the epilogue's cost, so every lane takes one
// coefficient: report_epilogue (capi_report.hpp) in its own operation order and types
template <typename T>
__global__ __launch_bounds__(256) void grouped_report_epilogue_kernel(const int64_t* __restrict__ off, int64_t n_groups, int p, int bias,
                                                                      int se_type, int weighted, const T* __restrict__ yvar,
                                                                      T* __restrict__ beta,
                                                                      const T* __restrict__ inv, const double* __restrict__ sums,
                                                                      const double* __restrict__ meat, ReportDofTable tab,
                                                                      T* __restrict__ o_se, T* __restrict__ o_t, T* __restrict__ o_p,
                                                                      T* __restrict__ o_lo, T* __restrict__ o_hi, T* __restrict__ o_r2,
                                                                      T* __restrict__ o_adj, uint8_t* __restrict__ o_null) {
#pragma clang fp contract(off)
    const int pp = p + bias;
    const T nanv = (T)__builtin_nan("");
    const int64_t total = n_groups * pp;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int64_t g = idx / pp;
        const int i = (int)(idx - g * pp);
        const int64_t n = off[g + 1] - off[g];
        const size_t o = (size_t)g * pp + i;
        if (n < pp) {  // too small or empty: null (the reference's per-group call raises "#Data < #features")
            beta[o] = nanv;
            o_se[o] = nanv;
            o_t[o] = nanv;
            o_p[o] = nanv;
            o_lo[o] = nanv;
            o_hi[o] = nanv;
            if (i == 0) {
                o_r2[g] = nanv;
                o_adj[g] = nanv;
                o_null[g] = 1;
            }
            continue;
        }
        const T dof = (T)n - (T)pp;
        const T nf = (T)n;
        const T ssr = (T)sums[g * 4];
        if (i == 0) {
            T y_var;
            if (yvar) {
                y_var = yvar[g];
            } else {
                const double nn = (double)n, sy = sums[g * 4 + 1], syy = sums[g * 4 + 2];
                y_var = (T)((syy - sy * sy / nn) / (nn - 1.0));
            }
            const T ratio = ssr / (y_var * nf);
            o_r2[g] = (T)1 - ratio;
            o_adj[g] = (T)1 - ratio * (((T)(n - 1)) / (dof - (T)1));
            o_null[g] = 0;
        }
        double t_alpha, lng;
        dof_lookup(tab, n - pp, &t_alpha, &lng);
        const T* ig = inv + g * (int64_t)pp * pp;
        T se;
        if (se_type == PDS_SE) {
            const T mse = (weighted ? (T)sums[g * 4 + 3] : ssr) / dof;  // (report_epilogue: sum w e^2 / dof when weighted)
            se = (T)sqrt((double)(mse * ig[i + i * pp]));
        } else {
            const double* mg = meat + g * (int64_t)pp * pp;
            const T factor = (se_type == PDS_HC1) ? nf / (T)(n - pp) : (T)1;
            double acc = 0.0;
            // (the meat is symmetric: its column a is read as row a, so both operands of the inner loop are contiguous per thread)
            const T* ic = ig + i * pp;
            for (int a = 0; a < pp; ++a) {
                const double* ma = mg + a * pp;
                double t = 0.0;
                for (int b = 0; b < pp; ++b) t += ma[b] * (double)ic[b];
                acc += (double)ic[a] * t;
            }
            se = (T)sqrt((double)((T)acc * factor));
        }
        const T b = beta[o];
        o_se[o] = se;
        const T tv = b / se;
        o_t[o] = tv;
        const double sf = student_t_sf_dev(fabs((double)tv), (double)dof, lng);
        o_p[o] = (T)(2.0 * sf);
        o_lo[o] = (T)((double)b - t_alpha * (double)se);
        o_hi[o] = (T)((double)b + t_alpha * (double)se);
    }
}

// pass 1 of split groups: the Gram record of group g = the sum of its pieces' records vrec[vfirst[g] ..] in piece order (f64)
template <typename T>
__global__ __launch_bounds__(256) void grouped_report_sum_records_kernel(const T* __restrict__ vrec, const int64_t* __restrict__ vfirst,
                                                                         int64_t n_groups, int qq, T* __restrict__ rec) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_groups * qq) return;
    const int64_t g = i / qq;
    const int e = (int)(i - g * qq);
    double v = 0.0;
    for (int64_t k = vfirst[g]; k < vfirst[g + 1]; ++k) v += (double)vrec[k * qq + e];
    rec[i] = (T)v;
}

__global__ __launch_bounds__(256) void student_t_sf_grid_kernel(const double* __restrict__ x, const double* __restrict__ df,
                                                                const double* __restrict__ lng, int64_t n, double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = student_t_sf_dev(x[i], df[i], lng[i]);
}

}  // namespace

template <typename T>
int launch_grouped_report_pass(pds_ctx* ctx, const T* const* d_cols, int n_feat, int bias, const int64_t* d_off, int64_t n_groups,
                               const T* d_beta, const T* d_inv, int hc, double* d_sums, double* d_meat, const int64_t* d_pieces,
                               int64_t n_pieces, int64_t piece_rows, const int64_t* d_fin, int64_t n_fin, bool weighted) {
    if (n_groups <= 0) return PDS_OK;
    if (weighted && hc) return fail(PDS_ERR_INVALID, "internal: the weighted grouped report has the plain standard error only");
    if (n_feat < 1 || n_feat > kMaxFeatWide) return fail(PDS_ERR_UNSUPPORTED, "grouped report: 1..64 features supported");
    KernelTimer timer(ctx, kKindPass2);
    const int64_t n_items = n_groups + n_pieces;
    auto launch = [&](auto w_c) {
        constexpr bool W = decltype(w_c)::value;
        if (n_feat > kMaxFeatSmall) {
            const int nb = (int)std::min<int64_t>(n_items, (int64_t)ctx->num_cus * 4);
            hipLaunchKernelGGL((grouped_report_pass_wide_kernel<T, W>), dim3(nb), dim3(64), 0, ctx->stream, d_cols, n_feat, bias, d_off,
                               n_groups, d_beta, d_inv, hc, d_sums, d_meat, d_pieces, n_items, piece_rows);
            return;
        }
        const int nb = (int)std::min<int64_t>((n_items + 3) / 4, (int64_t)ctx->num_cus * 8);
        auto pass = [&](auto pc) {
            hipLaunchKernelGGL((grouped_report_pass_kernel<T, decltype(pc)::value, W>), dim3(nb), dim3(kRpThreads), 0, ctx->stream, d_cols,
                               bias, d_off, n_groups, d_beta, d_inv, hc, d_sums, d_meat, d_pieces, n_items, piece_rows);
        };
        if (!dispatch_width<1, 15>(n_feat, pass)) pass(std::integral_constant<int, 16>{});
    };
    if (weighted) launch(std::true_type{});
    else launch(std::false_type{});
    PDS_HIP_CHECK(hipGetLastError());
    if (n_fin > 0) {
        const int nsum = weighted ? 4 : 3;
        const int per = nsum + (hc ? (n_feat + bias) * (n_feat + bias) : 0);
        hipLaunchKernelGGL(grouped_report_finish_kernel, dim3((unsigned)((n_fin * per + 255) / 256)), dim3(256), 0, ctx->stream, d_fin,
                           n_fin, n_feat + bias, hc, nsum, d_sums, d_meat);
        PDS_HIP_CHECK(hipGetLastError());
    }
    return PDS_OK;
}

template <typename T>
int launch_grouped_report_epilogue(pds_ctx* ctx, const int64_t* d_off, int64_t n_groups, int n_feat, int bias, int se_type,
                                   const T* d_yvar, T* d_beta, const T* d_inv, const double* d_sums, const double* d_meat,
                                   const ReportDofTable& tab, T* se, T* t, T* p, T* lo, T* hi, T* r2, T* adj_r2, uint8_t* is_null,
                                   bool weighted) {
    if (n_groups <= 0) return PDS_OK;
    KernelTimer timer(ctx, kKindSolve);
    const int nb = (int)std::min<int64_t>((n_groups * (n_feat + bias) + 255) / 256, (int64_t)ctx->num_cus * 16);
    hipLaunchKernelGGL((grouped_report_epilogue_kernel<T>), dim3(nb), dim3(256), 0, ctx->stream, d_off, n_groups, n_feat, bias, se_type,
                       weighted ? 1 : 0, d_yvar, d_beta, d_inv, d_sums, d_meat, tab, se, t, p, lo, hi, r2, adj_r2, is_null);
    PDS_HIP_CHECK(hipGetLastError());
    return PDS_OK;
}

template <typename T>
int launch_grouped_report_sum_records(pds_ctx* ctx, const T* d_vrec, const int64_t* d_vfirst, int64_t n_groups, int qq, T* d_rec) {
    if (n_groups <= 0) return PDS_OK;
    KernelTimer timer(ctx, kKindGroupedMoments);
    hipLaunchKernelGGL((grouped_report_sum_records_kernel<T>), dim3((unsigned)((n_groups * qq + 255) / 256)), dim3(256), 0, ctx->stream,
                       d_vrec, d_vfirst, n_groups, qq, d_rec);
    PDS_HIP_CHECK(hipGetLastError());
    return PDS_OK;
}
template int launch_grouped_report_sum_records<double>(pds_ctx*, const double*, const int64_t*, int64_t, int, double*);
template int launch_grouped_report_sum_records<float>(pds_ctx*, const float*, const int64_t*, int64_t, int, float*);

int launch_student_t_sf_grid(pds_ctx* ctx, const double* d_x, const double* d_df, const double* d_lng, int64_t n, double* d_out) {
    if (n <= 0) return PDS_OK;
    hipLaunchKernelGGL(student_t_sf_grid_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, d_x, d_df, d_lng, n, d_out);
    PDS_HIP_CHECK(hipGetLastError());
    return PDS_OK;
}

template int launch_grouped_report_pass<double>(pds_ctx*, const double* const*, int, int, const int64_t*, int64_t, const double*,
                                                const double*, int, double*, double*, const int64_t*, int64_t, int64_t, const int64_t*,
                                                int64_t, bool);
template int launch_grouped_report_pass<float>(pds_ctx*, const float* const*, int, int, const int64_t*, int64_t, const float*,
                                               const float*, int, double*, double*, const int64_t*, int64_t, int64_t, const int64_t*,
                                               int64_t, bool);
template int launch_grouped_report_epilogue<double>(pds_ctx*, const int64_t*, int64_t, int, int, int, const double*, double*,
                                                    const double*, const double*, const double*, const ReportDofTable&, double*, double*,
                                                    double*, double*, double*, double*, double*, uint8_t*, bool);
template int launch_grouped_report_epilogue<float>(pds_ctx*, const int64_t*, int64_t, int, int, int, const float*, float*,
                                                   const float*, const double*, const double*, const ReportDofTable&, float*, float*,
                                                   float*, float*, float*, float*, float*, uint8_t*, bool);

}  // namespace pds
