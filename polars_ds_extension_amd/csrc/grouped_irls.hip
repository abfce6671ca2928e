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
//
// This file is compiled four times: as it stands it holds the unpenalised kernels (PEN = 0) and the launchers;
// grouped_irls_ridge.hip and grouped_irls_cd.hip include it with PDS_GROUPED_IRLS_PEN = 1 / 2 and hold the kernels of one penalised
// mode each; grouped_irls_wo.hip includes it with PDS_GROUPED_IRLS_PEN = 3 and holds the weighted / offset form (kGiWo, below) --
// 32 kernels every time, which one translation unit would compile one after the other.
#include "glm_dev.hpp"
#include "solve_reg_dev.hpp"
#include "wave_tile_dev.hpp"

#include <algorithm>

#ifndef PDS_GROUPED_IRLS_PEN
#define PDS_GROUPED_IRLS_PEN 0
#endif

namespace pds {

namespace {

constexpr int kGiCap = 128;                           // resident rows of a group (two 64-row steps)
constexpr int kGiStride = wave_tile_stride(kGiCap);  // doubles per feature row of the tile
constexpr int kGiG = 18;                              // row stride of the staged Gram matrix (17 x 17: 16 features + bias)

template <typename T>
__device__ __forceinline__ bool gi_finite(T v) {
    return fabs((double)v) <= 1.79769313486231570e308;  // (false for NaN)
}

// The penalised step (PEN = 1 / 2).  The links are canonical, so the IRLS step is the Newton step of sum_i l(y_i, eta_i), and the step
// of  F = (1/n) sum l + (l2/2) |beta_f|^2 + l1 |beta_f|_1  (features only, never the bias) is the minimiser of
//   1/2 beta' G beta - c' beta + (n l2 / 2) |beta_f|^2 + n l1 |beta_f|_1     with G = X'WX, c = X'Wz as staged in gm / rh.
// The scale is the group's row count n, not sum w.
//   * l1 <= 0: n l2 goes on the feature diagonal of the staged system and solve_core runs as it does without a penalty (in the
//     16 + bias form the bias is eliminated first, which is exact because it is unpenalised: the penalty ends up on the centred
//     16 x 16 diagonal).
//   * l1 > 0: coordinate descent in the wave (gi_cd_step below) in place of the solve.
// The two are kernels of their own (PEN = 1 ridge, PEN = 2 coordinate descent): the solve leaves no register to spare at two waves
// per SIMD, and with both steps in one kernel several widths spilled to scratch.
// (kGiCdInner, kGiCdSweeps: common.hpp)

// Covariance-update coordinate descent on the staged system, warm-started from the previous outer iteration's coefficients (0 in
// the first).  Lane k < p' holds beta_k (`bk`) and the running gradient r_k = c_k - sum_j G_kj beta_j; coordinate j's candidate is
// soft(r_j + G_jj beta_j, n l1) / (G_jj + n l2) for a feature and (r_j + G_jj beta_j) / G_jj for the bias (last, index 16 of gm).
// Every lane computes the same candidate from broadcasts, so the decision to move is wave-uniform; a coordinate that does not move
// costs no update.  Lane k reads G_kj as gm[j][k] (the matrix is symmetric up to the rounding of the two matrix-core products):
// consecutive lanes read consecutive doubles of one row, 17 distinct banks, where column j (row stride kGiG = 18 doubles = 36
// banks) would put lanes k and k + 16 on one bank.
template <int P>
__device__ __forceinline__ double gi_cd_step(const double* gm, const double* rh, int pp, int lane, double bk, double nl1, double nl2,
                                             double eps) {
    const int gk = lane < P ? lane : 16;
    const bool mine = lane < pp;
    double r = mine ? rh[gk] : 0.0;
    for (int j = 0; j < pp; ++j) {
        const double bj = __shfl(bk, j);
        if (bj != 0.0) r = fma(-bj, mine ? gm[(j < P ? j : 16) * kGiG + gk] : 0.0, r);
    }
    for (int sweep = 0; sweep < kGiCdSweeps; ++sweep) {
        double moved = 0.0;
        for (int j = 0; j < pp; ++j) {
            const int gj = j < P ? j : 16;
            const double gjj = gm[gj * kGiG + gj];
            const double bj = __shfl(bk, j);
            const double u = fma(gjj, bj, __shfl(r, j));
            double nb;
            if (j < P) {
                const double mag = fabs(u) - nl1;
                nb = mag > 0.0 ? copysign(mag, u) / (gjj + nl2) : 0.0;  // (an exact zero inside the threshold)
            } else {
                nb = u / gjj;
            }
            const double delta = nb - bj;
            if (delta != 0.0) {  // (wave-uniform; true for a NaN)
                r = fma(-delta, mine ? gm[gj * kGiG + gk] : 0.0, r);
                if (lane == j) bk = nb;
                const double d = fabs(delta);
                moved = d > moved ? d : moved;
                if (d != d) moved = d;
            }
        }
        if (!(moved >= eps)) break;  // (converged, or a NaN: the outer loop's NaN rule ends the fit)
    }
    return bk;
}

// The weighted / offset form (PEN = kGiWo = 3: unpenalised, a prior weight pw_i and an offset o_i per row; R's glm(weights=, offset=)).
// The two columns are entries P + 1 and P + 2 of the column table, either may be null (pw = 1, o = 0):
//   eta = x . beta + o,  w = pw / (g'(mu)^2 V(mu)),  z = (eta - o) + g'(mu) (y - mu): x . beta itself from the second iteration on, so
//   the offset is read where eta is formed and nowhere else and does not live across the solve;
//   the start is mu0 = (y + ybar) / 2 with ybar = sum pw y / sum pw (binomial: (y + 0.5) / 2 as ever), eta0 = g(mu0), z's linear
//   part eta0 - o;
//   a row with pw = 0 contributes nothing and is not counted: the group is null with fewer than p' rows of positive weight, or with
//   any weight that is negative or not finite (counted / flagged in the load loop by ballots: wave-uniform, no register per lane).
// A resident group keeps pw and o as two more rows of the tile ((P + 3) x kGiStride doubles: 23 520 bytes per wave at 16 features
// where the other forms take 21 440, six workgroups per CU where they have seven); a streamed group re-reads them with its rows.
// With pw = 1 and o = 0 every operation below is the unweighted one or an exact one (x 1, + 0): the same bits.
constexpr int kGiWo = 3;

// (two waves per SIMD: 250 registers, nothing in scratch; a bound of three spilled 111 registers at 8 features)
// PEN = 0 is the unpenalised fit, the code it was before the penalties existed; PEN = 1 / 2 take the penalised step above.
template <typename T, int P, int PEN>
__global__ __launch_bounds__(64, 2) void grouped_irls_kernel(const T* const* __restrict__ cols, int bias, int64_t n_rows,
                                                          const int64_t* __restrict__ off, int64_t n_groups, int link, int variance,
                                                          double tol, int max_iter, int64_t split_rows, T* __restrict__ coeffs,
                                                          int32_t* __restrict__ n_iter, uint8_t* __restrict__ is_null,
                                                          T* __restrict__ pred, uint8_t* __restrict__ row_null,
                                                          const uint32_t* __restrict__ perm, int64_t* __restrict__ long_list,
                                                          unsigned* __restrict__ long_count, int64_t long_cap, double l1_reg,
                                                          double l2_reg) {
    constexpr bool WO = PEN == kGiWo;
    constexpr bool kPen = PEN == 1 || PEN == 2;
    constexpr int kTileRows = P + 1 + (WO ? 2 : 0);
    __shared__ double lds[kTileRows * kGiStride + 64 + 64 + 18 + 17 * kGiG + 18 + (kPen ? 2 : 0)];
    double* xt = lds;                      // features 0 .. P - 1, then y (WO: then pw, then o): [c * kGiStride + row]
    double* wt = xt + kTileRows * kGiStride;  // w of the step's rows
    double* zt = wt + 64;                  // w z of the step's rows
    double* bs = zt + 64;                  // coefficients: features, bias at bs[P]
    double* gm = bs + 18;                  // X'WX staged for the solve: index 16 is the bias row / column
    double* rh = gm + 17 * kGiG;           // X'Wz, rh[16] = sum w z
    // PEN: l1_reg, l2_reg, read back where an iteration uses them -- as kernel arguments they would stay in registers across the
    // solve, which has none to spare
    [[maybe_unused]] double* pn = rh + (kPen ? 18 : 0);
    if constexpr (kPen) {
        if (threadIdx.x == 0) {
            pn[0] = l1_reg;
            pn[1] = l2_reg;
        }
        PDS_WAVE_LDS_SYNC();
    }
    const int lane = threadIdx.x;
    const int pp = P + bias;
    const double nanv = __builtin_nan("");
    gptr<T> cx[P];
#pragma unroll
    for (int c = 0; c < P; ++c) cx[c] = as_global(cols[c]);
    const gptr<T> cy = as_global(cols[P]);
    [[maybe_unused]] const T* const pwp = WO ? cols[P + 1] : nullptr;  // (null: every weight 1)
    [[maybe_unused]] const T* const ofp = WO ? cols[P + 2] : nullptr;  // (null: every offset 0)
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
        if constexpr (PEN == 1) {
            if (lane == 0) pn[0] = (double)n * pn[1];  // (read at the staging of every iteration, many hand-offs from here)
        }
        double sy = 0.0;
        [[maybe_unused]] double spw = 0.0;
        [[maybe_unused]] int64_t n_pos = 0;   // rows of positive weight
        [[maybe_unused]] bool bad_w = false;  // a weight that is negative or not finite
        for (int64_t base = 0; base < n; base += 64) {
            const int64_t r = base + lane;
            const bool live = r < n;
            const double yv = live ? (double)cy[r0 + r] : 0.0;
            if constexpr (WO) {
                const double pwv = live ? (pwp ? (double)as_global(pwp)[r0 + r] : 1.0) : 0.0;
                n_pos += __popcll(__ballot(pwv > 0.0));
                bad_w = bad_w || __any(!(pwv >= 0.0 && gi_finite<double>(pwv)));
                // (a weight of 0 takes its y out of the mean whatever y holds)
                if (pwv > 0.0) {
                    sy += pwv * yv;
                    spw += pwv;
                }
                if (resident) {
                    xt[(P + 1) * kGiStride + r] = pwv;
                    xt[(P + 2) * kGiStride + r] = (live && ofp) ? (double)as_global(ofp)[r0 + r] : 0.0;
                }
            } else {
                sy += yv;
            }
            if (resident) {
#pragma unroll
                for (int c = 0; c < P; ++c) xt[c * kGiStride + r] = live ? (double)cx[c][r0 + r] : 0.0;
                xt[P * kGiStride + r] = yv;
            }
        }
        if constexpr (WO) {
            if (bad_w || n_pos < pp) {  // null by the weight rule: nothing computed
                if (lane < pp) coeffs[g * pp + lane] = (T)nanv;
                if (lane == 0) {
                    n_iter[g] = 0;
                    is_null[g] = 1;
                }
                if (pred || row_null) {
                    for (int64_t r = lane; r < n; r += 64) {
                        const int64_t o = perm ? (int64_t)perm[r0 + r] : r0 + r;
                        if (pred) pred[o] = (T)nanv;
                        if (row_null) row_null[o] = 1;
                    }
                }
                continue;
            }
        }
        double ymean;
        if constexpr (WO) {
            ymean = wave_sum(sy) / wave_sum(spw);
        } else {
            ymean = wave_sum(sy) / (double)n;
        }
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
                [[maybe_unused]] double pwv = 1.0, ov = 0.0;
                if constexpr (WO) {
                    if (resident) {
                        pwv = xt[(P + 1) * kGiStride + slot + lane];
                        ov = xt[(P + 2) * kGiStride + slot + lane];
                    } else {
                        pwv = live ? (pwp ? (double)as_global(pwp)[r0 + r] : 1.0) : 0.0;
                        ov = (live && ofp) ? (double)as_global(ofp)[r0 + r] : 0.0;
                    }
                }
                double eta, mu;  // eta: the linear part of z, x . beta (the first iteration: g(mu0) - o)
                if (it == 1) {
                    mu = (variance == 2) ? (yv + 0.5) * 0.5 : (yv + ymean) * 0.5;
                    eta = glm_link<double>(link, mu);
                    if constexpr (WO) eta -= ov;
                } else {
                    eta = bias ? bs[P] : 0.0;
#pragma unroll
                    for (int c = 0; c < P; ++c) eta = fma(x[c], bs[c], eta);
                    if constexpr (WO) {
                        mu = glm_inv<double>(link, eta + ov);
                    } else {
                        mu = glm_inv<double>(link, eta);
                    }
                }
                const double d = glm_deriv<double>(link, mu);
                double w, wz;
                if constexpr (WO) {
                    // (a row of weight 0 contributes nothing whatever its y holds; its features stay in the tile for pred and meet
                    // w = 0 in the matrix instructions, so they have to be finite)
                    const bool on = live && pwv > 0.0;
                    w = on ? pwv / (d * d * glm_var<double>(variance, mu)) : 0.0;
                    wz = on ? w * (eta + d * (yv - mu)) : 0.0;
                } else {
                    w = live ? 1.0 / (d * d * glm_var<double>(variance, mu)) : 0.0;
                    wz = live ? w * (eta + d * (yv - mu)) : 0.0;
                }
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
            // ridge (PEN = 1): n l2 on the feature diagonal of the staged system, never on index 16 (the bias); the solve below is
            // the unpenalised one.  In the 16 + bias form the centring then runs on the penalised diagonal: the same matrix.
            double nl2 = 0.0;
            if constexpr (PEN == 1) nl2 = pn[0];
            wave_tile_for_d(
                lane,
                [&](int i, int c, double g, double side) {
                    gm[i * kGiG + c] = (PEN == 1 && i == c) ? g + nl2 : g;
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
            if constexpr (PEN == 2) {
                const double bk = gi_cd_step<P>(gm, rh, pp, lane, bcur, (double)n * pn[0], (double)n * pn[1], kGiCdInner * tol);
                if (lane < pp) bs[lane] = bk;
            } else {
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
            }
            PDS_WAVE_LDS_SYNC();
            const double bnew = lane < pp ? bs[lane] : 0.0;
            // (penalised: the first system is built at the starting mu, not at beta = 0, so an all-zero first step -- every feature
            // inside the l1 threshold -- says nothing about the point beta = 0 itself: the second iteration decides)
            const bool open = lane < pp && (!(fabs(bcur - bnew) < tol) || (kPen && it == 1));
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
                if constexpr (WO) {
                    if (resident) {
                        eta += xt[(P + 2) * kGiStride + r];
                    } else if (ofp) {
                        eta += (double)as_global(ofp)[r0 + r];
                    }
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
                                                             const uint32_t* __restrict__ perm, const T* __restrict__ offset) {
    const bool gnull = null_flag[0] != 0;
    for (int64_t r = r0 + (int64_t)blockIdx.x * 256 + threadIdx.x; r < r1; r += (int64_t)gridDim.x * 256) {
        double eta = bias ? (double)beta[p] : 0.0;
        for (int c = 0; c < p; ++c) eta = fma((double)as_global(cols[c])[r], (double)beta[c], eta);
        if (offset) eta += (double)as_global(offset)[r];
        const int64_t o = perm ? (int64_t)perm[r] : r;
        if (pred) pred[o] = gnull ? (T)__builtin_nan("") : (T)glm_inv<double>(link, eta);
        if (row_null) row_null[o] = gnull ? 1 : 0;
    }
}

}  // namespace

// What each of the four objects exports: the launch of its own kernel set, PEN = PDS_GROUPED_IRLS_PEN.  The kernel keeps its flat
// parameter list (its registers are counted, above), so the description is unpacked here.
template <typename T, int PEN>
struct GroupedIrlsSet {
    static int launch(pds_ctx* ctx, const GlmGroupsDev<T>& gr, const GlmFitDev<T>& fit, const GlmLongList& ll);
};

template <typename T, int PEN>
int GroupedIrlsSet<T, PEN>::launch(pds_ctx* ctx, const GlmGroupsDev<T>& gr, const GlmFitDev<T>& fit, const GlmLongList& ll) {
    KernelTimer timer(ctx, kKindIter);
    const int nb = (int)std::min<int64_t>(gr.n_groups, (int64_t)ctx->num_cus * 32);
    dispatch_width<1, kMaxFeatSmall>(gr.n_feat, [&](auto pc) {
        hipLaunchKernelGGL((grouped_irls_kernel<T, decltype(pc)::value, PEN>), dim3(nb), dim3(64), 0, ctx->stream, gr.d_cols, gr.bias,
                           gr.n_rows, gr.d_off, gr.n_groups, gr.link, gr.variance, fit.tol, fit.max_iter, gr.split_rows, fit.d_coeffs,
                           fit.d_n_iter, fit.d_null, fit.d_pred, fit.d_row_null, fit.d_perm, ll.d_list, ll.d_count, ll.cap, fit.l1_reg,
                           fit.l2_reg);
    });
    PDS_HIP_CHECK(hipGetLastError());
    return PDS_OK;
}
template struct GroupedIrlsSet<double, PDS_GROUPED_IRLS_PEN>;
template struct GroupedIrlsSet<float, PDS_GROUPED_IRLS_PEN>;

#if PDS_GROUPED_IRLS_PEN == 0
// (the other three sets: grouped_irls_ridge.hip, grouped_irls_cd.hip, grouped_irls_wo.hip)
extern template struct GroupedIrlsSet<double, 1>;
extern template struct GroupedIrlsSet<float, 1>;
extern template struct GroupedIrlsSet<double, 2>;
extern template struct GroupedIrlsSet<float, 2>;
extern template struct GroupedIrlsSet<double, kGiWo>;
extern template struct GroupedIrlsSet<float, kGiWo>;

template <typename T>
int launch_grouped_irls(pds_ctx* ctx, const GlmGroupsDev<T>& groups, const GlmFitDev<T>& fit, const GlmLongList& long_list) {
    if (groups.n_groups <= 0) return PDS_OK;
    if (groups.n_feat < 1 || groups.n_feat > kMaxFeatSmall) return fail(PDS_ERR_UNSUPPORTED, "grouped GLM (IRLS): up to 16 feature columns");
    GlmFitDev<T> f = fit;  // (a penalty <= 0 means none; the weighted / offset kernels are unpenalised)
    f.l1_reg = !groups.wo && fit.l1_reg > 0.0 ? fit.l1_reg : 0.0;
    f.l2_reg = !groups.wo && fit.l2_reg > 0.0 ? fit.l2_reg : 0.0;
    if (groups.wo) return GroupedIrlsSet<T, kGiWo>::launch(ctx, groups, f, long_list);
    if (f.l1_reg > 0.0) return GroupedIrlsSet<T, 2>::launch(ctx, groups, f, long_list);
    if (f.l2_reg > 0.0) return GroupedIrlsSet<T, 1>::launch(ctx, groups, f, long_list);
    return GroupedIrlsSet<T, 0>::launch(ctx, groups, f, long_list);
}

template <typename T>
int launch_glm_pred_range(pds_ctx* ctx, const T* const* d_cols, int n_feat, int bias, int64_t r0, int64_t r1, const T* d_beta,
                          const uint8_t* d_null_flag, int link, T* d_pred, uint8_t* d_row_null, const uint32_t* d_perm, const T* d_offset) {
    if (r1 <= r0 || (!d_pred && !d_row_null)) return PDS_OK;
    KernelTimer timer(ctx, kKindPass2);
    const int nb = (int)std::min<int64_t>((r1 - r0 + 255) / 256, (int64_t)ctx->num_cus * 16);
    hipLaunchKernelGGL((glm_pred_range_kernel<T>), dim3(nb), dim3(256), 0, ctx->stream, d_cols, n_feat, bias, r0, r1, d_beta, d_null_flag,
                       link, d_pred, d_row_null, d_perm, d_offset);
    PDS_HIP_CHECK(hipGetLastError());
    return PDS_OK;
}

template int launch_grouped_irls<double>(pds_ctx*, const GlmGroupsDev<double>&, const GlmFitDev<double>&, const GlmLongList&);
template int launch_grouped_irls<float>(pds_ctx*, const GlmGroupsDev<float>&, const GlmFitDev<float>&, const GlmLongList&);
template int launch_glm_pred_range<double>(pds_ctx*, const double* const*, int, int, int64_t, int64_t, const double*, const uint8_t*, int,
                                           double*, uint8_t*, const uint32_t*, const double*);
template int launch_glm_pred_range<float>(pds_ctx*, const float* const*, int, int, int64_t, int64_t, const float*, const uint8_t*, int,
                                          float*, uint8_t*, const uint32_t*, const float*);
#endif

}  // namespace pds
