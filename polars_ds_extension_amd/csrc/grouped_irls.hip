// grouped_irls.hip -- a GLM per group by iteratively re-weighted least squares, every iteration of a group on chip: what
// `df.group_by(key).agg(...)` over a per-group GLM fit asks for (faer_irls, glm_solvers.rs:249-359, once per group).
//
// The one-model route (capi_models.hpp, glm_irls_impl) pays per iteration a launch of the full-frame Gram pass, a solve and a
// blocking copy of the coefficients; for a million groups of 100 rows that is millions of launches.  Here ONE wave owns a group
// from its first row to its last iteration:
//   * lane = row, 64 rows per step: the wave-tile idiom of wave_tile_dev.hpp.  A group of up to kGiCap = 128 rows is RESIDENT: its
//     feature columns and y are written once into the wave-private LDS tile (feature-major, row stride kGiStride), and every
//     iteration reads them from there -- the frame is read from HBM once,
//     not once per iteration.  A longer group re-reads its rows from global memory in every iteration (L2 / Infinity Cache
//     traffic) through the first 64 row slots of the same tile; the arithmetic and its order are the same, so are the results.
//   * per iteration (moments.hip WM = 3, orc_glm_irls): eta = x . beta (first iteration: eta0 = g(mu0), mu0 = (y + 0.5) / 2 for the
//     binomial family, (y + mean_g(y)) / 2 otherwise), mu = g^-1(eta), w = 1 / (g'(mu)^2 V(mu)), z = eta + g'(mu) (y - mu);
//     X'WX by v_mfma_f64_16x16x4 with operands (w x, x); X'Wz and the bias row X'w by a second matrix instruction with operands
//     (x, [w z | w | 0 ..]); sum w and sum w z are per-lane registers folded by a fixed butterfly.  No atomics in any sum:
//     repeated calls are bit-identical.
//   * the p' x p' system goes through the register-resident pivoted QR of solve_reg_dev.hpp (no gate, no penalty: what
//     faer_weighted_lr does with LRSolverMethods::QR), lane j = column j, on each of the wave's four 16-lane rows alike.
//     16 features + bias (p' = 17) is one column more than that solver holds: the bias is eliminated first (the weighted
//     centring G_ij - s_i s_j / sum w, as solve_wave.hip centres its systems) and recovered as (sum w z - s . beta) / sum w.
//   * stop: max_j |beta_j - beta_new_j| < tol (a NaN difference never converges; a NaN coefficient cannot recover, so the wave
//     leaves the loop and reports max_iter) or max_iter iterations.
// Arithmetic is f64 for f64 and f32 frames alike (an f32 frame is converted on load).  Groups above `split_rows` are not
// walked here: the wave appends them to a list and the host side fits them with the full-device iteration
// (capi_glm_grouped.hpp).  Per-row means are written at the end of a group's fit from the rows the wave still holds.
#include "glm_dev.hpp"
#include "solve_reg_dev.hpp"
#include "wave_tile_dev.hpp"

#include <algorithm>

namespace pds {

namespace {

constexpr int kGiCap = 128;                           // resident rows of a group (two 64-row steps)
constexpr int kGiStride = wave_tile_stride(kGiCap);  // doubles per feature row of the tile
constexpr int kGiG = 18;                              // row stride of the staged Gram matrix (17 x 17: 16 features + bias)

template <typename T>
__device__ __forceinline__ bool gi_finite(T v) {
    return fabs((double)v) <= 1.79769313486231570e308;  // (false for NaN)
}

// (two waves per SIMD: 250 registers, nothing in scratch; a bound of three spilled 111 registers at 8 features)
template <typename T, int P>
__global__ __launch_bounds__(64, 2) void grouped_irls_kernel(const T* const* __restrict__ cols, int bias, int64_t n_rows,
                                                          const int64_t* __restrict__ off, int64_t n_groups, int link, int variance,
                                                          double tol, int max_iter, int64_t split_rows, T* __restrict__ coeffs,
                                                          int32_t* __restrict__ n_iter, uint8_t* __restrict__ is_null,
                                                          T* __restrict__ pred, uint8_t* __restrict__ row_null,
                                                          const uint32_t* __restrict__ perm, int64_t* __restrict__ long_list,
                                                          unsigned* __restrict__ long_count, int64_t long_cap) {
    __shared__ double lds[(P + 1) * kGiStride + 64 + 64 + 18 + 17 * kGiG + 18];
    double* xt = lds;                      // features 0 .. P - 1, then y: [c * kGiStride + row]
    double* wt = xt + (P + 1) * kGiStride;  // w of the step's rows
    double* zt = wt + 64;                  // w z of the step's rows
    double* bs = zt + 64;                  // coefficients: features, bias at bs[P]
    double* gm = bs + 18;                  // X'WX staged for the solve: index 16 is the bias row / column
    double* rh = gm + 17 * kGiG;           // X'Wz, rh[16] = sum w z
    const int lane = threadIdx.x;
    const int pp = P + bias;
    const double nanv = __builtin_nan("");
    gptr<T> cx[P];
#pragma unroll
    for (int c = 0; c < P; ++c) cx[c] = as_global(cols[c]);
    const gptr<T> cy = as_global(cols[P]);
    SolveRegDev sp;
    sp.p = P;
    sp.bias = bias;
    sp.pp = pp > 16 ? 16 : pp;
    sp.lambda_on_bias = 0;
    sp.gate_on = 0;
    sp.lambda = 0.0;
    sp.ln_tol = 0.0;
    sp.inv_tol = 0.0;
    for (int64_t g = blockIdx.x; g < n_groups; g += gridDim.x) {
        const int64_t r0 = off[g], n = off[g + 1] - r0;
        const bool bad = r0 < 0 || n < 0 || r0 + n > n_rows;  // (offsets that leave the frame: nothing is read)
        if (!bad && n > split_rows) {  // the host side fits it (the order of the list does not matter: the host sorts it)
            if (lane == 0) {
                const unsigned k = atomicAdd(long_count, 1u);
                if ((int64_t)k < long_cap) long_list[k] = g;
            }
            continue;
        }
        if (bad || n < pp) {  // fewer rows than coefficients: null, nothing computed
            if (lane < pp) coeffs[g * pp + lane] = (T)nanv;
            if (lane == 0) {
                n_iter[g] = 0;
                is_null[g] = 1;
            }
            if (!bad && lane < n) {  // (n < p' <= 17 rows)
                const int64_t o = perm ? (int64_t)perm[r0 + lane] : r0 + lane;
                if (pred) pred[o] = (T)nanv;
                if (row_null) row_null[o] = 1;
            }
            continue;
        }
        const bool resident = n <= kGiCap;
        PDS_WAVE_LDS_SYNC();  // (the previous group's reads are done)
        double sy = 0.0;
        for (int64_t base = 0; base < n; base += 64) {
            const int64_t r = base + lane;
            const bool live = r < n;
            const double yv = live ? (double)cy[r0 + r] : 0.0;
            sy += yv;
            if (resident) {
#pragma unroll
                for (int c = 0; c < P; ++c) xt[c * kGiStride + r] = live ? (double)cx[c][r0 + r] : 0.0;
                xt[P * kGiStride + r] = yv;
            }
        }
        const double ymean = wave_sum(sy) / (double)n;
        double bcur = 0.0;  // lane j < p': coefficient j (the bias last)
        int it = 0;
        while (it < max_iter) {
            ++it;
            d4 acc = {0.0, 0.0, 0.0, 0.0}, acc2 = {0.0, 0.0, 0.0, 0.0};
            double sw = 0.0, swz = 0.0;
            for (int64_t base = 0; base < n; base += 64) {
                const int slot = resident ? (int)base : 0;
                const int64_t r = base + lane;
                const bool live = r < n;
                PDS_WAVE_LDS_SYNC();  // (the previous step's operand reads are done)
                double x[P], yv;
                if (resident) {
#pragma unroll
                    for (int c = 0; c < P; ++c) x[c] = xt[c * kGiStride + slot + lane];
                    yv = xt[P * kGiStride + slot + lane];
                } else {
#pragma unroll
                    for (int c = 0; c < P; ++c) {
                        x[c] = live ? (double)cx[c][r0 + r] : 0.0;
                        xt[c * kGiStride + lane] = x[c];
                    }
                    yv = live ? (double)cy[r0 + r] : 0.0;
                }
                double eta, mu;
                if (it == 1) {
                    mu = (variance == 2) ? (yv + 0.5) * 0.5 : (yv + ymean) * 0.5;
                    eta = glm_link<double>(link, mu);
                } else {
                    eta = bias ? bs[P] : 0.0;
#pragma unroll
                    for (int c = 0; c < P; ++c) eta = fma(x[c], bs[c], eta);
                    mu = glm_inv<double>(link, eta);
                }
                const double d = glm_deriv<double>(link, mu);
                const double w = live ? 1.0 / (d * d * glm_var<double>(variance, mu)) : 0.0;
                const double wz = live ? w * (eta + d * (yv - mu)) : 0.0;
                sw += w;
                swz += wz;
                wt[lane] = w;
                zt[lane] = wz;
                PDS_WAVE_LDS_SYNC();
                wave_tile_gram<P>(
                    xt + slot, kGiStride, (int)std::min<int64_t>(64, n - base), lane, [&](int row) { return wt[row]; },
                    [&](int c, int row, double wv) { return c == 0 ? zt[row] : (c == 1 ? wv : 0.0); },  // B columns: 0 = w z, 1 = w
                    acc, acc2);
            }
            sw = wave_sum(sw);
            swz = wave_sum(swz);
            PDS_WAVE_LDS_SYNC();  // (bs / gm / rh: the previous iteration's reads are done)
            wave_tile_for_d(
                lane,
                [&](int i, int c, double g, double side) {
                    gm[i * kGiG + c] = g;
                    if (c == 0) rh[i] = side;
                    if (c == 1) {
                        gm[i * kGiG + 16] = side;
                        gm[16 * kGiG + i] = side;
                    }
                },
                acc, acc2);
            if (lane == 0) {
                gm[16 * kGiG + 16] = sw;
                rh[16] = swz;
            }
            PDS_WAVE_LDS_SYNC();
            // ---- the solve: lane j of every 16-lane row = column j
            const int j = lane & 15;
            const bool centred = pp > 16;  // 16 features + bias: the bias is eliminated, 16 columns remain
            const int ppq = sp.pp;
            const bool colv = j < ppq;
            const int jm = (j < P) ? j : 16;
            const double sj = centred ? gm[jm * kGiG + 16] : 0.0;
            const double mj = centred ? sj / sw : 0.0, mz = centred ? swz / sw : 0.0;
            double a[16], b[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int im = (i < P) ? i : 16;
                const double si = centred ? gm[im * kGiG + 16] : 0.0;
                a[i] = (colv && i < ppq) ? fma(-si, mj, gm[im * kGiG + jm]) : 0.0;
                b[i] = (i < ppq) ? fma(-si, mz, rh[im]) : 0.0;
            }
            const double dj = colv ? gm[jm * kGiG + jm] : 1.0;
            bool snull = false;
            int pj = j;
            double zj = 0.0;
            solve_core<16>(a, b, dj, j, lane, sp, snull, pj, zj);
            if (lane < 16 && colv) bs[pj] = zj;
            if (centred) {
                const double sb = Grp<16>::sum(colv ? gm[pj * kGiG + 16] * zj : 0.0);
                if (lane == 0) bs[16] = (swz - sb) / sw;
            }
            PDS_WAVE_LDS_SYNC();
            const double bnew = lane < pp ? bs[lane] : 0.0;
            const bool open = lane < pp && !(fabs(bcur - bnew) < tol);
            const bool isnan_b = lane < pp && bnew != bnew;
            bcur = bnew;
            if (__any(isnan_b)) {
                it = max_iter;
                break;
            }
            if (!__any(open)) break;
        }
        const T bout = (T)bcur;
        const bool gnull = __any(lane < pp && !gi_finite<T>(bout));
        if (lane < pp) coeffs[g * pp + lane] = bout;
        if (lane == 0) {
            n_iter[g] = it;
            is_null[g] = gnull ? 1 : 0;
        }
        if (pred || row_null) {
            for (int64_t base = 0; base < n; base += 64) {
                const int64_t r = base + lane;
                if (r >= n) break;
                double eta = bias ? bs[P] : 0.0;
                if (resident) {
#pragma unroll
                    for (int c = 0; c < P; ++c) eta = fma(xt[c * kGiStride + r], bs[c], eta);
                } else {
#pragma unroll
                    for (int c = 0; c < P; ++c) eta = fma((double)cx[c][r0 + r], bs[c], eta);
                }
                const int64_t o = perm ? (int64_t)perm[r0 + r] : r0 + r;
                if (pred) pred[o] = gnull ? (T)nanv : (T)glm_inv<double>(link, eta);
                if (row_null) row_null[o] = gnull ? 1 : 0;
            }
        }
    }
}

// per-row means of ONE group's row range from coefficients in memory (the groups the host side fitted)
template <typename T>
__global__ __launch_bounds__(256) void glm_pred_range_kernel(const T* const* __restrict__ cols, int p, int bias, int64_t r0, int64_t r1,
                                                             const T* __restrict__ beta, const uint8_t* __restrict__ null_flag, int link,
                                                             T* __restrict__ pred, uint8_t* __restrict__ row_null,
                                                             const uint32_t* __restrict__ perm) {
    const bool gnull = null_flag[0] != 0;
    for (int64_t r = r0 + (int64_t)blockIdx.x * 256 + threadIdx.x; r < r1; r += (int64_t)gridDim.x * 256) {
        double eta = bias ? (double)beta[p] : 0.0;
        for (int c = 0; c < p; ++c) eta = fma((double)as_global(cols[c])[r], (double)beta[c], eta);
        const int64_t o = perm ? (int64_t)perm[r] : r;
        if (pred) pred[o] = gnull ? (T)__builtin_nan("") : (T)glm_inv<double>(link, eta);
        if (row_null) row_null[o] = gnull ? 1 : 0;
    }
}

}  // namespace

template <typename T>
int launch_grouped_irls(pds_ctx* ctx, const T* const* d_cols, int n_feat, int bias, int64_t n_rows, const int64_t* d_off,
                        int64_t n_groups, int link, int variance, double tol, int max_iter, int64_t split_rows, T* d_coeffs,
                        int32_t* d_n_iter, uint8_t* d_null, T* d_pred, uint8_t* d_row_null, const uint32_t* d_perm,
                        int64_t* d_long_list, unsigned* d_long_count, int64_t long_cap) {
    if (n_groups <= 0) return PDS_OK;
    if (n_feat < 1 || n_feat > kMaxFeatSmall) return fail(PDS_ERR_UNSUPPORTED, "grouped GLM (IRLS): up to 16 feature columns");
    KernelTimer timer(ctx, kKindIter);
    const int nb = (int)std::min<int64_t>(n_groups, (int64_t)ctx->num_cus * 32);
    dispatch_width<1, kMaxFeatSmall>(n_feat, [&](auto pc) {
        hipLaunchKernelGGL((grouped_irls_kernel<T, decltype(pc)::value>), dim3(nb), dim3(64), 0, ctx->stream, d_cols, bias, n_rows, d_off,
                           n_groups, link, variance, tol, max_iter, split_rows, d_coeffs, d_n_iter, d_null, d_pred, d_row_null, d_perm,
                           d_long_list, d_long_count, long_cap);
    });
    PDS_HIP_CHECK(hipGetLastError());
    return PDS_OK;
}

template <typename T>
int launch_glm_pred_range(pds_ctx* ctx, const T* const* d_cols, int n_feat, int bias, int64_t r0, int64_t r1, const T* d_beta,
                          const uint8_t* d_null_flag, int link, T* d_pred, uint8_t* d_row_null, const uint32_t* d_perm) {
    if (r1 <= r0 || (!d_pred && !d_row_null)) return PDS_OK;
    KernelTimer timer(ctx, kKindPass2);
    const int nb = (int)std::min<int64_t>((r1 - r0 + 255) / 256, (int64_t)ctx->num_cus * 16);
    hipLaunchKernelGGL((glm_pred_range_kernel<T>), dim3(nb), dim3(256), 0, ctx->stream, d_cols, n_feat, bias, r0, r1, d_beta, d_null_flag,
                       link, d_pred, d_row_null, d_perm);
    PDS_HIP_CHECK(hipGetLastError());
    return PDS_OK;
}

template int launch_grouped_irls<double>(pds_ctx*, const double* const*, int, int, int64_t, const int64_t*, int64_t, int, int, double, int,
                                         int64_t, double*, int32_t*, uint8_t*, double*, uint8_t*, const uint32_t*, int64_t*, unsigned*,
                                         int64_t);
template int launch_grouped_irls<float>(pds_ctx*, const float* const*, int, int, int64_t, const int64_t*, int64_t, int, int, double, int,
                                        int64_t, float*, int32_t*, uint8_t*, float*, uint8_t*, const uint32_t*, int64_t*, unsigned*, int64_t);
template int launch_glm_pred_range<double>(pds_ctx*, const double* const*, int, int, int64_t, int64_t, const double*, const uint8_t*, int,
                                           double*, uint8_t*, const uint32_t*);
template int launch_glm_pred_range<float>(pds_ctx*, const float* const*, int, int, int64_t, int64_t, const float*, const uint8_t*, int,
                                          float*, uint8_t*, const uint32_t*);

}  // namespace pds
