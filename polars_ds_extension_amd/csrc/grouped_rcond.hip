// grouped_rcond.hip -- lin_reg_w_rcond per group: the minimum-norm least-squares coefficients and the singular values of every
// group's X'X (+ lambda) in one launch (faer_solve_lr_rcond, lr_solvers.rs:225-254, once per group).
//
// The one-system route (capi_lr.hpp, lr_rcond_impl) pays per call a launch of the full-frame Gram pass, a blocking copy and a host
// Jacobi; for a million groups of 100 rows that is a million launches.  Here ONE wave owns a group from its first row to its
// coefficients:
//   * lane = row, 64 rows per step through the wave-private LDS tile of wave_tile_dev.hpp (feature-major, row stride kGrStride):
//     X'X by v_mfma_f64_16x16x4 with operands (x, x); X'y and the column sums by a second matrix instruction with operands
//     (x, [y | 1 | 0 ..]); sum y is a per-lane register folded by a fixed butterfly.  The fit needs one pass over a group's rows, so
//     no row stays resident.  No atomics in any sum: repeated calls are bit-identical, and a group's bits do not depend on where it
//     sits in the frame or on the grid.
//   * G = X'X (+ l2_reg on the feature diagonals, the bias row / column last) is p' x p', p' = P + bias <= 17.  It is decomposed by
//     the one-sided (Hestenes) Jacobi iteration of the host jacobi_svd (capi_lr.hpp): rotation formulas, skip test
//     (gamma == 0 or |gamma| <= eps sqrt(alpha) sqrt(beta)) and the 60-sweep cap are the host's.  Lane j < 32 holds column j of U
//     (starting as G) in registers, lane 32 + j column j of V (starting as I).  A sweep is a round-robin tournament: the columns are
//     padded to an even count with a zero column (it never rotates: gamma == 0), and the disjoint pairs of a round rotate at the
//     same time.  Partners exchange their columns by cross-lane shuffles, alpha / beta / gamma / c / s are computed in-lane (both
//     lanes of a pair run the same operations on the same values, so they agree to the bit), and the V lanes take c and s from
//     their U lane by one more shuffle.  The column arrays are indexed with compile-time indices only (unrolled over P + 1).
//   * finish: eigenvalue s_j = |u_j|, singular_values = sqrt(s) descending (ties: the lower column first), rcond_g =
//     max(rcond, eps_T max(n_g, p')), thr = rcond_g sqrt(s_max), sinv_j = s_j >= thr ? 1 / s_j : 0 (the eigenvalue against
//     rcond * the largest singular value: the reference's rule, kept as written), z_j = sinv_j (u_j . c) / s_j, beta = V z.
// Null groups (is_null = 1, NaN coefficients and singular values): offsets that leave the frame (nothing is read), n_g < p', a
// non-finite entry in X'X / X'y / the column sums, final coefficients that are not all finite (the all-zero system divides by
// zero, as in the reference).  Arithmetic is f64 for f64 and f32 frames alike (an f32 frame is converted on load).
#include "wave_tile_dev.hpp"

#include <algorithm>

namespace pds {

namespace {

constexpr int kGrStride = wave_tile_stride(64);  // doubles per feature row of the tile
constexpr int kGrG = 18;                          // row stride of the staged matrices (17 x 17: 16 features + bias)
constexpr int kGrSolveDoubles = 2 * 17 * kGrG + 3 * 18;  // G, V, right-hand side, eigenvalues, z
constexpr int kGrSweeps = 60;

template <typename T>
__device__ __forceinline__ bool gr_finite(T v) {
    return fabs((double)v) <= 1.79769313486231570e308;  // (false for NaN)
}

constexpr int gr_lds_doubles(int P) { return std::max((P + 1) * kGrStride, kGrSolveDoubles); }

// (four waves per SIMD up to 12 features; beyond, the two column arrays of the rotation -- 2 (P + 1) doubles -- and the shuffle
// temporaries do not fit 128 registers: 13 .. 16 features spilled 12 .. 100 bytes per lane there, three waves per SIMD spill nothing)
template <typename T, int P>
__global__ __launch_bounds__(64, P > 12 ? 3 : 4) void grouped_rcond_kernel(const T* const* __restrict__ cols, int bias, int64_t n_rows,
                                                           const int64_t* __restrict__ off, int64_t n_groups, double l2_reg,
                                                           double rcond, T* __restrict__ coeffs, T* __restrict__ svals,
                                                           uint8_t* __restrict__ is_null) {
    constexpr int M = P + 1;  // length of a column in registers: the features, then the bias row (zero without a bias)
    // the tile of the Gram pass and the staging of the solve share the block: a group's solve starts after its last operand read
    __shared__ double lds[gr_lds_doubles(P)];
    double* xt = lds;                 // features 0 .. P - 1, then y: [c * kGrStride + row]
    double* gm = lds;                 // G, compact: feature i at index i, the bias at index P
    double* vm = gm + 17 * kGrG;      // V at the end of the iteration
    double* rh = vm + 17 * kGrG;      // X'y, rh[P] = sum y
    double* ev = rh + 18;             // eigenvalues, by column
    double* zs = ev + 18;             // z, by column
    const int lane = threadIdx.x;
    const int pp = P + bias;
    const int nc = (pp + 1) & ~1;     // columns of the tournament (even)
    const int j = lane & 31;          // the lane's column
    const bool ulane = lane < 32;
    const bool col_live = j < pp;
    const double nanv = __builtin_nan("");
    const double eps = 2.220446049250313e-16;
    const double eps_t = std::is_same_v<T, float> ? 1.1920928955078125e-07 : eps;
    gptr<T> cx[P];
#pragma unroll
    for (int c = 0; c < P; ++c) cx[c] = as_global(cols[c]);
    const gptr<T> cy = as_global(cols[P]);
    for (int64_t g = blockIdx.x; g < n_groups; g += gridDim.x) {
        const int64_t r0 = off[g], n = off[g + 1] - r0;
        const bool bad = r0 < 0 || n < 0 || r0 + n > n_rows || r0 + n < r0;  // (offsets that leave the frame: nothing is read)
        bool gnull = bad || n < pp;  // fewer rows than coefficients: null, nothing computed
        double beta = nanv, sval = nanv;
        int rank = lane;
        if (!gnull) {
            // ---- X'X, X'y, the column sums, sum y
            d4 acc = {0.0, 0.0, 0.0, 0.0}, acc2 = {0.0, 0.0, 0.0, 0.0};
            double sy = 0.0;
            for (int64_t base = 0; base < n; base += 64) {
                const int64_t r = base + lane;
                const bool live = r < n;
                double x[P];
#pragma unroll
                for (int c = 0; c < P; ++c) x[c] = live ? (double)cx[c][r0 + r] : 0.0;
                const double yv = live ? (double)cy[r0 + r] : 0.0;
                sy += yv;
                PDS_WAVE_LDS_SYNC();  // (the previous step's operand reads, the previous group's solve reads are done)
#pragma unroll
                for (int c = 0; c < P; ++c) xt[c * kGrStride + lane] = x[c];
                xt[P * kGrStride + lane] = yv;
                PDS_WAVE_LDS_SYNC();
                wave_tile_gram<P>(
                    xt, kGrStride, (int)std::min<int64_t>(64, n - base), lane, TileNoScale{},
                    [&](int c, int row) { return c == 0 ? xt[P * kGrStride + row] : (c == 1 ? 1.0 : 0.0); },  // B columns: 0 = y, 1 = 1
                    acc, acc2);
            }
            sy = wave_sum(sy);
            bool fin = gr_finite(sy);
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) fin = fin && gr_finite(acc[reg]) && gr_finite(acc2[reg]);
            gnull = __any(!fin);  // ("SVD failed." of the single-system call)
            if (!gnull) {
                PDS_WAVE_LDS_SYNC();  // (the last step's operand reads are done: the tile becomes the staging block)
                wave_tile_for_d(
                    lane,
                    [&](int i, int c, double gv, double side) {
                        if (i < P) {
                            if (c < P) gm[i * kGrG + c] = (i == c) ? gv + l2_reg : gv;
                            if (c == 0) rh[i] = side;
                            if (c == 1) {
                                gm[i * kGrG + P] = side;
                                gm[P * kGrG + i] = side;
                            }
                        }
                    },
                    acc, acc2);
                if (lane == 0) {
                    gm[P * kGrG + P] = (double)n;
                    rh[P] = sy;
                }
                PDS_WAVE_LDS_SYNC();
                // ---- one-sided Jacobi: lanes 0 .. 31 column j of U (= G), lanes 32 .. 63 column j of V (= I)
                double a[M], b[M];
#pragma unroll
                for (int r = 0; r < M; ++r) {
                    const double gv = (col_live && r < pp) ? gm[r * kGrG + j] : 0.0;
                    a[r] = ulane ? gv : ((col_live && r == j) ? 1.0 : 0.0);
                }
                for (int sweep = 0; sweep < kGrSweeps; ++sweep) {
                    bool rotated = false;
                    for (int k = 0; k < nc - 1; ++k) {
                        // round k of the tournament: column nc - 1 meets k, every other i meets 2 k - i (mod nc - 1)
                        int partner = j;
                        if (j < nc) {
                            if (j == nc - 1) partner = k;
                            else if (j == k) partner = nc - 1;
                            else {
                                partner = 2 * k - j;
                                if (partner < 0) partner += nc - 1;
                                if (partner >= nc - 1) partner -= nc - 1;
                            }
                        }
                        const int src = (lane & 32) | partner;
#pragma unroll
                        for (int r = 0; r < M; ++r) b[r] = __shfl(a[r], src, 64);
                        const bool first = j < partner;  // the pair (i, j), i < j, of the host loop: this lane holds column i
                        double own = 0.0, oth = 0.0, ga = 0.0;
#pragma unroll
                        for (int r = 0; r < M; ++r) {
                            own = fma(a[r], a[r], own);
                            oth = fma(b[r], b[r], oth);
                            ga = fma(a[r], b[r], ga);
                        }
                        const double al = first ? own : oth, be = first ? oth : own;
                        const bool skip = partner == j || ga == 0.0 || fabs(ga) <= eps * sqrt(al) * sqrt(be);  // (al * be may overflow)
                        const double zeta = (be - al) / (2.0 * ga);
                        const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                        double c = 1.0 / sqrt(1.0 + t * t);
                        double s = c * t;
                        c = skip ? 1.0 : c;
                        s = skip ? 0.0 : s;
                        rotated = rotated || (ulane && !skip);
                        c = __shfl(c, j, 64);  // (the V lanes rotate by their U lane's angle)
                        s = __shfl(s, j, 64);
                        // column i: c x - s y; column j: s x + c y
                        const double so = first ? -s : s;
#pragma unroll
                        for (int r = 0; r < M; ++r) a[r] = fma(so, b[r], c * a[r]);
                    }
                    if (!__any(rotated)) break;
                }
                // ---- finish: eigenvalues = column norms of U, z = sinv (U'c), beta = V z
                double nn = 0.0, dot = 0.0;
#pragma unroll
                for (int r = 0; r < M; ++r) {
                    nn = fma(a[r], a[r], nn);
                    dot = fma(a[r], r < pp ? rh[r] : 0.0, dot);
                }
                const double sj = sqrt(nn);
                PDS_WAVE_LDS_SYNC();  // (the loads of G and the right-hand side are done)
                if (ulane && col_live) ev[j] = sj;
                if (!ulane && col_live) {
#pragma unroll
                    for (int r = 0; r < M; ++r) vm[r * kGrG + j] = a[r];
                }
                PDS_WAVE_LDS_SYNC();
                double smax = 0.0;
                int rk = 0;
                for (int q = 0; q < pp; ++q) {
                    const double sq = ev[q];
                    smax = fmax(smax, sq);
                    rk += (sq > sj || (sq == sj && q < j)) ? 1 : 0;  // descending, ties: the lower column first
                }
                const double rc_g = fmax(rcond, eps_t * (double)std::max<int64_t>(n, (int64_t)pp));
                const double thr = rc_g * sqrt(smax);
                const double sinv = sj >= thr ? 1.0 / sj : 0.0;
                const double dj = sj > 0.0 ? dot / sj : dot;
                if (ulane && col_live) zs[j] = dj * sinv;
                PDS_WAVE_LDS_SYNC();
                double bsum = 0.0;
                if (lane < pp)
                    for (int q = 0; q < pp; ++q) bsum = fma(vm[lane * kGrG + q], zs[q], bsum);
                beta = bsum;
                sval = sqrt(sj);
                rank = rk;
                gnull = __any(lane < pp && !gr_finite<T>((T)beta));
            }
        }
        if (lane < pp) {
            coeffs[g * pp + lane] = gnull ? (T)nanv : (T)beta;
            svals[g * pp + (gnull ? lane : rank)] = gnull ? (T)nanv : (T)sval;
        }
        if (lane == 0) is_null[g] = gnull ? 1 : 0;
    }
}

}  // namespace

template <typename T>
int launch_grouped_rcond(pds_ctx* ctx, const T* const* d_cols, int n_feat, int bias, int64_t n_rows, const int64_t* d_off,
                         int64_t n_groups, double l2_reg, double rcond, T* d_coeffs, T* d_svals, uint8_t* d_null) {
    if (n_groups <= 0) return PDS_OK;
    if (n_feat < 1 || n_feat > kMaxFeatSmall) return fail(PDS_ERR_UNSUPPORTED, "grouped lin_reg_w_rcond: up to 16 feature columns");
    KernelTimer timer(ctx, kKindIter);
    hipError_t err = hipSuccess;
    dispatch_width<1, kMaxFeatSmall>(n_feat, [&](auto pc) {
        auto kernel = grouped_rcond_kernel<T, decltype(pc)::value>;
        // every wave walks its share of the groups: as many workgroups as are resident at once (registers and LDS decide), so that none
        // waits for another to finish its whole share
        int per_cu = 0;
        err = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, 64, 0);
        if (err != hipSuccess) return;
        const int nb = (int)std::min<int64_t>(n_groups, (int64_t)ctx->num_cus * std::max(per_cu, 1));
        hipLaunchKernelGGL(kernel, dim3(nb), dim3(64), 0, ctx->stream, d_cols, bias, n_rows, d_off, n_groups, l2_reg, rcond, d_coeffs, d_svals,
                           d_null);
    });
    PDS_HIP_CHECK(err);
    PDS_HIP_CHECK(hipGetLastError());
    return PDS_OK;
}

template int launch_grouped_rcond<double>(pds_ctx*, const double* const*, int, int, int64_t, const int64_t*, int64_t, double, double, double*,
                                          double*, uint8_t*);
template int launch_grouped_rcond<float>(pds_ctx*, const float* const*, int, int, int64_t, const int64_t*, int64_t, double, double, float*,
                                         float*, uint8_t*);

}  // namespace pds
