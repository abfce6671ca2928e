// grouped_multi.hip -- the multi-target fit per group: lin_reg(target=[t_0 .. t_{k-1}], by=key) in one launch (pl_lr_multi once per
// group: k targets share the group's design matrix, linear_regression.rs:517-649).
//
// ONE wave owns a group from its first row to its k coefficient vectors, in the shape of grouped_rcond.hip:
//   * Gram pass: lane = row, 64 rows per step through the wave-private LDS tile of wave_tile_dev.hpp (feature-major, row stride
//     kGmStride): the P feature rows, then the k target rows.  X'X by v_mfma_f64_16x16x4 with operands (x, x); the side block of the
//     second matrix instruction is [t_0 .. t_{k-1} | 1 | 0 ..], so its accumulator holds X't_c in column c and the column sums in
//     column k, out of the operand reads X'X needs anyway.  sum t_c is a per-lane register folded by a fixed butterfly.  An f32 frame
//     is converted on load; all arithmetic is f64.  No atomics in any sum: a group's bits do not depend on its place in the frame, on
//     the grid or on the other groups.
//   * solve: G = X'X (+ l2_reg on the feature diagonals); with an intercept the system is centred (G_ij - s_i s_j / n, c_j - s_j
//     sum t / n) and b0 = (sum t - s . beta) / n, exactly as wave_ldl_solve / the fused kernel do, so the intercept never takes a
//     lane.  Lane j holds column j in registers (the staging block that transposes the accumulators reuses the tile after the last
//     operand read).  The square-root-free L D L' of solve_wave_dev.hpp runs ONCE per group; lane j keeps its multiplier of every
//     step, and each target's right-hand side then takes the same steps in the same order it would take riding along as an extra
//     row (the same operations on the same values: the same bits), followed by the back substitution.  The loop over the targets
//     runs to the run-time k: no register array is indexed by a target.
//   * gate and nulls: lin_reg_by's, group for group.  Null (flag 1, NaN coefficients): offsets that leave the frame (nothing is
//     read), fewer rows than coefficients, a non-finite entry in X'X / X't / the sums, a non-positive diagonal or pivot, the product
//     of the pivot ratios G_kk / d_k at or past 1 / singular_x_tol.  The gate depends on X alone, and a group is null for every
//     target or for none: a NaN in ONE target therefore nulls the whole group.  A group next to the gate (solve_suspect) is not
//     answered here: flag 2, its index appended to mark_list (one atomic on the list cursor per such group -- the order of the list
//     is arbitrary, the values are not), and the caller puts it through the reference's factorisation (capi_multi_grouped.hpp).
// One wave walks its group whatever its length: correctness is not bounded by a row count.
#include "solve_wave_dev.hpp"
#include "wave_tile_dev.hpp"

#include <algorithm>

namespace pds {

namespace {

constexpr int kGmStride = wave_tile_stride(64);  // doubles per row of the tile
constexpr int kGmMaxT = 15;                        // targets: the side block has 16 columns, one of them the ones column
constexpr int kGmG = 18;                           // row stride of the staged matrices
// staging block: G [16][kGmG], X't [15][kGmG], column sums [kGmG], sum t [16]
constexpr int kGmRh = 16 * kGmG, kGmCs = kGmRh + kGmMaxT * kGmG, kGmSt = kGmCs + kGmG, kGmStageDoubles = kGmSt + 16;

inline size_t gm_lds_bytes(int P, int k) { return sizeof(double) * (size_t)std::max((P + k) * kGmStride, kGmStageDoubles); }

__device__ __forceinline__ bool gm_finite(double v) {
    return fabs(v) <= 1.79769313486231570e308;  // (false for NaN)
}

// (four waves per SIMD asked for up to 8 features; beyond, the feature registers of a step, the 15 target registers and the 15 sums
//  pass 128 registers from 12 features on (three waves per SIMD there).  No instance uses scratch: DESIGN.md 4.2a has the figures.)
template <typename T, int P>
__global__ __launch_bounds__(64, P > 8 ? 3 : 4) void grouped_multi_kernel(const T* const* __restrict__ cols, int k, int bias, int64_t n_rows,
                                                                          const int64_t* __restrict__ off, int64_t n_groups, double lambda,
                                                                          double inv_tol, double sus_tol, T* __restrict__ coeffs,
                                                                          uint8_t* __restrict__ flags, int32_t* __restrict__ mark_list,
                                                                          unsigned* __restrict__ mark_count) {
    // the tile of the Gram pass and the staging of the solve share the block: a group's solve starts after its last operand read
    extern __shared__ __attribute__((aligned(16))) double gm_lds[];
    double* xt = gm_lds;          // features 0 .. P - 1, then targets 0 .. k - 1: [c * kGmStride + row]
    double* gm = gm_lds;          // G [i * kGmG + j]
    double* rh = gm_lds + kGmRh;  // X't_c [c * kGmG + i]
    double* cs = gm_lds + kGmCs;  // column sums
    double* stt = gm_lds + kGmSt; // sum t_c
    const int lane = threadIdx.x;
    const int j = lane;
    const bool colv = j < P;
    const int pp = P + bias;
    const double nanv = __builtin_nan("");
    SolveRegDev sp;
    sp.inv_tol = inv_tol;
    sp.sus_tol = sus_tol;
    gptr<T> cx[P];
#pragma unroll
    for (int c = 0; c < P; ++c) cx[c] = as_global(cols[c]);
    for (int64_t g = blockIdx.x; g < n_groups; g += gridDim.x) {
        const int64_t r0 = off[g], n = off[g + 1] - r0;
        const bool bad = r0 < 0 || n < 0 || r0 + n > n_rows || r0 + n < r0;  // (offsets that leave the frame: nothing is read)
        bool gnull = bad || n < pp;  // fewer rows than coefficients: null, nothing computed
        bool suspect = false;
        T* const cg = coeffs + g * (int64_t)k * pp;
        if (!gnull) {
            // ---- X'X, X't_c, the column sums, sum t_c
            d4 acc = {0.0, 0.0, 0.0, 0.0}, acc2 = {0.0, 0.0, 0.0, 0.0};
            double st[kGmMaxT];
#pragma unroll
            for (int c = 0; c < kGmMaxT; ++c) st[c] = 0.0;
            for (int64_t base = 0; base < n; base += 64) {
                const int64_t r = base + lane;
                const bool live = r < n;
                double x[P], tv[kGmMaxT];
#pragma unroll
                for (int c = 0; c < P; ++c) x[c] = live ? (double)cx[c][r0 + r] : 0.0;
#pragma unroll
                for (int c = 0; c < kGmMaxT; ++c) tv[c] = (c < k && live) ? (double)as_global(cols[P + c])[r0 + r] : 0.0;
                PDS_WAVE_LDS_SYNC();  // (the previous step's operand reads, the previous group's solve reads are done)
#pragma unroll
                for (int c = 0; c < P; ++c) xt[c * kGmStride + lane] = x[c];
#pragma unroll
                for (int c = 0; c < kGmMaxT; ++c) {
                    st[c] += tv[c];
                    if (c < k) xt[(P + c) * kGmStride + lane] = tv[c];
                }
                PDS_WAVE_LDS_SYNC();
                wave_tile_gram<P>(
                    xt, kGmStride, (int)std::min<int64_t>(64, n - base), lane, TileNoScale{},
                    [&](int c, int row) { return c < k ? xt[(P + c) * kGmStride + row] : (c == k ? 1.0 : 0.0); },  // B columns: t_c, then 1
                    acc, acc2);
            }
            bool fin = true;
#pragma unroll
            for (int c = 0; c < kGmMaxT; ++c) {
                if (c < k) {
                    st[c] = wave_sum(st[c]);
                    fin = fin && gm_finite(st[c]);
                }
            }
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) fin = fin && gm_finite(acc[reg]) && gm_finite(acc2[reg]);
            gnull = __any(!fin);
            if (!gnull) {
                PDS_WAVE_LDS_SYNC();  // (the last step's operand reads are done: the tile becomes the staging block)
                wave_tile_for_d(
                    lane,
                    [&](int i, int c, double gv, double side) {
                        if (i < P) {
                            if (c < P) gm[i * kGmG + c] = gv;
                            if (c < k) rh[c * kGmG + i] = side;
                            if (c == k) cs[i] = side;
                        }
                    },
                    acc, acc2);
                if (lane == 0) {
#pragma unroll
                    for (int c = 0; c < kGmMaxT; ++c)
                        if (c < k) stt[c] = st[c];
                }
                PDS_WAVE_LDS_SYNC();
                // ---- lane j: column j of the (centred) system, the uncentred diagonal (+ lambda) for the gate
                const double nn = (double)n;
                const double sj = colv ? cs[j] : 0.0;
                const double mj = bias ? sj / nn : 0.0;  // mean of the lane's feature
                double a[P], nt[P];
                double dj = 1.0;
#pragma unroll
                for (int i = 0; i < P; ++i) {
                    double gv = colv ? gm[i * kGmG + j] : 0.0;
                    if (i == j) {
                        gv += lambda;  // (never on the intercept: lr_solvers.rs:199-208)
                        dj = gv;
                    }
                    a[i] = bias ? fma(-cs[i], mj, gv) : gv;
                }
                bool is_null = __any(colv && dj <= 0.0);  // a non-positive diagonal entry gates (lr_solvers.rs:341-347)
                // ---- L D L', once: step K broadcasts lane K's entries, lane j > K updates its rows i > K and keeps its multiplier
                double invd = 1.0;
                bool ok = true;
#pragma unroll
                for (int K = 0; K < P; ++K) {
                    const double d = wave_lane_bcast(a[K], K);
                    ok = ok && (d > 0.0);
                    double xr = __builtin_amdgcn_rcp(d);
#pragma unroll
                    for (int it = 0; it < PDS_RCP_NEWTON; ++it) xr = fma(fma(-d, xr, 1.0), xr, xr);
                    nt[K] = (colv && j > K) ? -(a[K] * xr) : 0.0;
#pragma unroll
                    for (int i = K + 1; i < P; ++i) a[i] = fma(wave_lane_bcast(a[i], K), nt[K], a[i]);
                    if (j == K) invd = xr;
                }
                if (!ok) is_null = true;  // "Not positive-definite -> rank-deficient" (lr_solvers.rs:370-371)
                const double ratio = colv ? dj * invd : 1.0;
                const double grow = wave_prod64(ratio);  // prod G_kk / L_kk^2
                if (grow >= sp.inv_tol) is_null = true;
                suspect = solve_suspect(sp, ok, grow, 0.0);
                gnull = is_null || suspect;
                if (!gnull) {
                    // ---- per target: the elimination steps on its right-hand side, back substitution, the intercept
                    double cb[P];
#pragma unroll
                    for (int m = 1; m < P; ++m) cb[m] = (colv && j < m) ? -(a[m] * invd) : 0.0;
                    for (int c = 0; c < k; ++c) {
                        const double stc = stt[c];
                        double b = colv ? rh[c * kGmG + j] : 0.0;
                        if (bias) b = fma(-stc, mj, b);
#pragma unroll
                        for (int K = 0; K < P - 1; ++K) b = fma(wave_lane_bcast(b, K), nt[K], b);
                        double w = b * invd;
#pragma unroll
                        for (int m = P - 1; m >= 1; --m) w = fma(wave_lane_bcast(w, m), cb[m], w);
                        if (colv) cg[c * pp + j] = (T)w;
                        if (bias) {
                            const double sb = wave_sum(colv ? sj * w : 0.0);
                            if (lane == 0) cg[c * pp + P] = (T)((stc - sb) / nn);
                        }
                    }
                }
            }
        }
        if (gnull) {
            for (int e = lane; e < k * pp; e += 64) cg[e] = (T)nanv;
        }
        if (lane == 0) {
            flags[g] = suspect ? 2 : (gnull ? 1 : 0);
            if (suspect) mark_list[atomicAdd(mark_count, 1u)] = (int32_t)g;
        }
    }
}

// one target's coefficient block [n][pp] and flags -> rows list[i] (or i) of the [n_groups][k][pp] block; a group is null when any
// of its targets is (`first`: this target sets the flag, the later ones add to it)
template <typename T>
__global__ void multi_scatter_kernel(const T* __restrict__ co, const uint8_t* __restrict__ fl, const int32_t* __restrict__ list, int64_t n, int t,
                                     int k, int pp, int first, T* __restrict__ coeffs, uint8_t* __restrict__ flags) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * pp) return;
    const int64_t s = i / pp;
    const int c = (int)(i - s * pp);
    const int64_t g = list ? (int64_t)list[s] : s;
    coeffs[(g * k + t) * pp + c] = co[i];
    if (c == 0) flags[g] = ((fl[s] ? 1 : 0) | (first ? 0 : (flags[g] ? 1 : 0)));
}

// NaN coefficients for every target of a null group.  check_finite: a group with a coefficient that is not finite is null as well
// (the per-target kernels pass a system whose X'X is regular whatever its right-hand side holds: a NaN in one target's rows ends as NaN
// coefficients of that target under a clear flag)
template <typename T>
__global__ void multi_null_fill_kernel(uint8_t* __restrict__ flags, const int32_t* __restrict__ list, int64_t n, int kpp, int check_finite,
                                       T* __restrict__ coeffs) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n) return;
    const int64_t g = list ? (int64_t)list[s] : s;
    bool null = flags[g] != 0;
    if (check_finite && !null) {  // (the marked groups of a list: few)
        for (int e = 0; e < kpp; ++e) null = null || !gm_finite((double)coeffs[g * kpp + e]);
        if (null) flags[g] = 1;
    }
    if (!null) return;
    for (int e = 0; e < kpp; ++e) coeffs[g * kpp + e] = (T)__builtin_nan("");
}

// the finite check of a whole block, one coefficient per thread (a thread per group walks its k p' values 8 k p' bytes apart from
// its neighbour's: 0.27 ms for 1e6 groups x 2 x 9, against 0.04 ms read this way); every writer of a flag stores the same value
template <typename T>
__global__ void multi_finite_flags_kernel(const T* __restrict__ coeffs, int64_t n_groups, int kpp, uint8_t* __restrict__ flags) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_groups * kpp) return;
    if (!gm_finite((double)coeffs[i])) flags[i / kpp] = 1;
}

// target t's coefficients out of the [n_groups][k][pp] block: the [n_groups][pp] block the per-row prediction pass reads
template <typename T>
__global__ void multi_extract_kernel(const T* __restrict__ coeffs, int64_t n_groups, int t, int k, int pp, T* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_groups * pp) return;
    const int64_t g = i / pp;
    out[i] = coeffs[(g * k + t) * pp + (i - g * pp)];
}

// *bad = 1 when the offsets decrease or leave the frame
__global__ void multi_offsets_check_kernel(const int64_t* __restrict__ off, int64_t n_groups, int64_t n_rows, unsigned* __restrict__ bad) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n_groups) return;
    const int64_t a = off[g], b = off[g + 1];
    if (a < 0 || b < a || b > n_rows) *bad = 1u;  // (every writer stores the same value)
}

}  // namespace

template <typename T>
int launch_grouped_multi(pds_ctx* ctx, const T* const* d_cols, int n_feat, int n_targets, int bias, int64_t n_rows, const int64_t* d_off,
                         int64_t n_groups, double l2_reg, double gate_tol, bool mark_suspects, T* d_coeffs, uint8_t* d_flags,
                         int32_t* d_mark_list, unsigned* d_mark_count) {
    if (n_groups <= 0) return PDS_OK;
    if (n_feat < 1 || n_feat > kMaxFeatSmall || n_targets < 1 || n_targets > kGmMaxT)
        return fail(PDS_ERR_UNSUPPORTED, "grouped multi-target lin_reg: up to 16 feature columns and 15 targets");
    if (!(gate_tol > 0.0)) return fail(PDS_ERR_INVALID, "internal: the grouped multi-target kernel is the gated factorisation");
    if (n_groups >= (1ll << 31)) return fail(PDS_ERR_UNSUPPORTED, "grouped multi-target lin_reg: fewer than 2^31 groups per call");
    const double inv_tol = 1.0 / gate_tol;
    const double sus_tol = mark_suspects ? std::sqrt(inv_tol) : 0.0;  // the fused kernel's rule (launch_grouped_fused)
    KernelTimer timer(ctx, kKindGroupedMoments);
    hipError_t err = hipSuccess;
    const size_t lds = gm_lds_bytes(n_feat, n_targets);
    dispatch_width<1, kMaxFeatSmall>(n_feat, [&](auto pc) {
        auto kernel = grouped_multi_kernel<T, decltype(pc)::value>;
        // every wave walks its share of the groups: as many workgroups as are resident at once (registers and LDS decide)
        int per_cu = 0;
        err = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, 64, lds);
        if (err != hipSuccess) return;
        int64_t nb = std::min<int64_t>(n_groups, (int64_t)ctx->num_cus * std::max(per_cu, 1));
        if (ctx->opt_multi_waves > 0) nb = std::min<int64_t>(nb, ctx->opt_multi_waves);  // "grouped_multi_waves": a cap (tests)
        hipLaunchKernelGGL(kernel, dim3((unsigned)nb), dim3(64), lds, ctx->stream, d_cols, n_targets, bias, n_rows, d_off, n_groups, l2_reg,
                           inv_tol, sus_tol, d_coeffs, d_flags, d_mark_list, d_mark_count);
    });
    PDS_HIP_CHECK(err);
    PDS_HIP_CHECK(hipGetLastError());
    return PDS_OK;
}

template <typename T>
int launch_multi_scatter(pds_ctx* ctx, const T* d_co, const uint8_t* d_fl, const int32_t* d_list, int64_t n, int t, int k, int pp, bool first,
                         T* d_coeffs, uint8_t* d_flags) {
    if (n <= 0) return PDS_OK;
    hipLaunchKernelGGL((multi_scatter_kernel<T>), dim3((unsigned)((n * pp + 255) / 256)), dim3(256), 0, ctx->stream, d_co, d_fl, d_list, n, t, k, pp,
                       first ? 1 : 0, d_coeffs, d_flags);
    PDS_HIP_CHECK(hipGetLastError());
    return PDS_OK;
}

template <typename T>
int launch_multi_null_fill(pds_ctx* ctx, uint8_t* d_flags, const int32_t* d_list, int64_t n, int kpp, bool check_finite, T* d_coeffs) {
    if (n <= 0) return PDS_OK;
    if (check_finite && !d_list) {  // every group: the flags first, one coefficient per thread
        hipLaunchKernelGGL((multi_finite_flags_kernel<T>), dim3((unsigned)((n * kpp + 255) / 256)), dim3(256), 0, ctx->stream, d_coeffs, n, kpp,
                           d_flags);
        check_finite = false;
    }
    hipLaunchKernelGGL((multi_null_fill_kernel<T>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, d_flags, d_list, n, kpp,
                       check_finite ? 1 : 0, d_coeffs);
    PDS_HIP_CHECK(hipGetLastError());
    return PDS_OK;
}

template <typename T>
int launch_multi_extract(pds_ctx* ctx, const T* d_coeffs, int64_t n_groups, int t, int k, int pp, T* d_out) {
    if (n_groups <= 0) return PDS_OK;
    hipLaunchKernelGGL((multi_extract_kernel<T>), dim3((unsigned)((n_groups * pp + 255) / 256)), dim3(256), 0, ctx->stream, d_coeffs, n_groups, t, k,
                       pp, d_out);
    PDS_HIP_CHECK(hipGetLastError());
    return PDS_OK;
}

int launch_multi_offsets_check(pds_ctx* ctx, const int64_t* d_off, int64_t n_groups, int64_t n_rows, unsigned* d_bad) {
    if (n_groups <= 0) return PDS_OK;
    hipLaunchKernelGGL(multi_offsets_check_kernel, dim3((unsigned)((n_groups + 255) / 256)), dim3(256), 0, ctx->stream, d_off, n_groups, n_rows, d_bad);
    PDS_HIP_CHECK(hipGetLastError());
    return PDS_OK;
}

#define PDS_MULTI_INST(T)                                                                                                                            \
    template int launch_grouped_multi<T>(pds_ctx*, const T* const*, int, int, int, int64_t, const int64_t*, int64_t, double, double, bool, T*,      \
                                         uint8_t*, int32_t*, unsigned*);                                                                             \
    template int launch_multi_scatter<T>(pds_ctx*, const T*, const uint8_t*, const int32_t*, int64_t, int, int, int, bool, T*, uint8_t*);           \
    template int launch_multi_null_fill<T>(pds_ctx*, uint8_t*, const int32_t*, int64_t, int, bool, T*);                                              \
    template int launch_multi_extract<T>(pds_ctx*, const T*, int64_t, int, int, int, T*);
PDS_MULTI_INST(double)
PDS_MULTI_INST(float)
#undef PDS_MULTI_INST

}  // namespace pds
