// within_pass.hip -- the device side of the fixed-effects (within) regression (capi_within.hpp): with the group means m_g of
// [x, y] (mixed.hip's statistics pass) and the coefficients beta of the centred regression known, ONE pass over the frame gives every
// per-row quantity of y_i = alpha_g(i) + x_i' beta + e_i:
//     alpha_g = m_y,g - m_g' beta,   e_i = (y_i - m_y,g) - (x_i - m_g)' beta  (= y_i - alpha_g - x_i' beta),   pred_i = y_i - e_i,
//     sum e^2,   and, for errors clustered on the absorbed key, the meat M = sum_g s_g s_g',  s_g = sum_{i in g} (x_i - m_g) e_i.
// It is cluster_meat.hip's pass with the rows centred on the way in: the score / meat idiom (the compensated sum e^2, the score step,
// the park and its flush, the record, the long-group kernel) is score_meat_dev.hpp's, instantiated here without a bias entry
// (HAS_BIAS = false).
//
//   * within_pass_kernel<T, P, MEAT>: ONE wave walks groups (grid stride) and takes the rows of a group 64 per step.  The step's
//     loads (P features, y, the row's place in the caller's frame when the frame was reordered) are issued back to back on a clamped
//     row index.  x - m_g and e are formed per row in registers; resid / pred go out through the permutation, alpha_g is written once
//     per group by lane 0.  e^2 is summed per lane across ALL the groups of the wave as a compensated sum (value + error term, two-sum
//     at every level: lane, butterfly, records), as in cluster_meat.hip.
//   * MEAT: x - m_g and e go through a wave-private LDS tile (feature-major, the wave-tile idiom of wave_tile_dev.hpp); the score of
//     the group comes from one v_mfma_f64_16x16x4 per four rows with operands (x - m, [e | 0 ..]) in an accumulator that lives for the
//     group.  Finished scores are parked in LDS four at a time; one matrix instruction with operands (s, s) per four groups adds
//     their outer products to the 16 x 16 meat, which the wave keeps across its groups.  There is no bias entry: the centred score of
//     the absorbed intercept is sum_i e_i = 0 and is never formed.  MEAT = false (classical errors, fit only) has no tile, no
//     accumulators and no park.
//   * groups above `split_rows` are the chunks the statistics pass was given (MixedChunks): m_g and beta are known, so chunks are
//     independent work items.  within_chunk_kernel (a wave per chunk: the rows' outputs, the chunk's sum e^2 into the wave's record,
//     its score to memory; the group's first chunk writes alpha_g) and score_long_meat_kernel<false> (a group's chunk scores added in
//     chunk order, lane = entry, then parked and multiplied like any other score).
//   * every wave writes ONE record in the layout of common.hpp (kMixedRecStride): [0,256) the meat, 288 sum e^2 and 290 its error
//     term.  Records are added in index order with a compensated running sum per entry (launch_sum_records, mixed.hip): no
//     floating-point atomics anywhere, so two calls give the same bits.
// Arithmetic is f64 for f64 and f32 frames alike (an f32 frame is converted on load; beta and the means are f64).
#include "score_meat_dev.hpp"

#include <algorithm>

namespace pds {

namespace {

// where the rows' outputs go: each nullable; perm (nullable): row r of the frame the kernels read is row perm[r] of the caller's
template <typename T>
struct WpRowOut {
    const uint32_t* perm;
    T* pred;
    T* resid;
};

// rows [r0, r0 + n) of the frame, 64 per step, centred with m (features, then y): resid / pred out, sum e^2 into ee and, with MEAT,
// the score of these rows into sc (side block, column 0)
template <typename T, int P, bool MEAT>
__device__ __forceinline__ void wp_stream(const gptr<T>* cx, gptr<T> cy, int64_t r0, int64_t n, const double* m, const double* b,
                                          const WpRowOut<T>& ro, double* xt, int lane, d4& sc, CompSq& ee) {
    const int f = lane & 15, kq = lane >> 4;
    const bool rows_out = ro.pred || ro.resid;
    for (int64_t base = 0; base < n; base += 64) {
        const int64_t r = base + lane;
        const bool live = r < n;
        const int64_t ri = r0 + (live ? r : 0);  // (n >= 1: the group's first row is always there)
        T raw[P + 1];
#pragma unroll
        for (int c = 0; c < P; ++c) raw[c] = cx[c][ri];
        raw[P] = cy[ri];
        int64_t ro_i = ri;
        if (rows_out && ro.perm) ro_i = (int64_t)ro.perm[ri];
        if constexpr (MEAT) PDS_WAVE_LDS_SYNC();  // (the previous step's operand reads are done)
        double e = live ? (double)raw[P] - m[P] : 0.0;
#pragma unroll
        for (int c = 0; c < P; ++c) {
            const double x = live ? (double)raw[c] - m[c] : 0.0;
            if constexpr (MEAT) xt[c * kScoreTileStride + lane] = x;
            e = fma(-x, b[c], e);
        }
        if constexpr (MEAT) xt[P * kScoreTileStride + lane] = e;
        ee.add(e);
        if (live) {
            if (ro.resid) ro.resid[ro_i] = (T)e;
            if (ro.pred) ro.pred[ro_i] = (T)((double)raw[P] - e);
        }
        if constexpr (MEAT) {
            PDS_WAVE_LDS_SYNC();
            const int rows = (int)std::min<int64_t>(64, n - base);
            const int steps = (rows + 3) >> 2;  // (the row slots past `rows` hold zeros)
            for (int k = 0; k < steps; ++k) score_rows4<P>(xt, 4 * k + kq, f, sc);
        }
    }
}

// the means of group g (features, then y) and alpha_g = m_y - m . beta
template <int P>
__device__ __forceinline__ double wp_group_means(const double* __restrict__ means, int64_t n_groups, int64_t g, const double* b, double* m) {
#pragma unroll
    for (int c = 0; c <= P; ++c) m[c] = means[(int64_t)c * n_groups + g];
    double a = m[P];
#pragma unroll
    for (int c = 0; c < P; ++c) a = fma(-m[c], b[c], a);
    return a;
}

// alpha (nullable): one value per group, at gmap[g] (nullable: g) -- the group's index among the caller's groups, empty ones included
template <typename T, int P, bool MEAT>
__global__ __launch_bounds__(64) void within_pass_kernel(const T* const* __restrict__ cols, const int64_t* __restrict__ off, int64_t n_groups,
                                                         int64_t split_rows, const double* __restrict__ beta, const double* __restrict__ means,
                                                         const int64_t* __restrict__ gmap, T* __restrict__ alpha, WpRowOut<T> ro,
                                                         double* __restrict__ partials) {
    __shared__ double xt[MEAT ? (P + 1) * kScoreTileStride + kScoreBatch * kScorePark : 1];  // features 0 .. P - 1, then e: [c * kScoreTileStride + row]; the park
    double* park = xt + (P + 1) * kScoreTileStride;
    const int lane = threadIdx.x;
    double b[P];
#pragma unroll
    for (int c = 0; c < P; ++c) b[c] = beta[c];
    gptr<T> cx[P];
#pragma unroll
    for (int c = 0; c < P; ++c) cx[c] = as_global(cols[c]);
    const gptr<T> cy = as_global(cols[P]);
    ScoreMeat<false> mt;
    CompSq ee;
    int64_t g = blockIdx.x;
    int64_t o0 = g < n_groups ? off[g] : 0, o1 = g < n_groups ? off[g + 1] : 0;  // (the host has validated the offsets)
    while (g < n_groups) {
        const int64_t r0 = o0, n = o1 - o0, gi = g;
        g += gridDim.x;  // the next group's offsets: asked for now, needed a group later
        o0 = g < n_groups ? off[g] : 0;
        o1 = g < n_groups ? off[g + 1] : 0;
        if (n <= 0 || n > split_rows) continue;  // empty: nothing; cut into chunks: the chunk kernels
        double m[P + 1];
        const double a = wp_group_means<P>(means, n_groups, gi, b, m);
        if (alpha && lane == 0) alpha[gmap ? gmap[gi] : gi] = (T)a;
        d4 sc = {0.0, 0.0, 0.0, 0.0};
        wp_stream<T, P, MEAT>(cx, cy, r0, n, m, b, ro, xt, lane, sc, ee);
        if constexpr (MEAT) mt.park_d(park, lane, sc);
    }
    if constexpr (MEAT) mt.flush(park, lane);
    mt.write_record(partials + (int64_t)blockIdx.x * kMixedRecStride, lane, ee);
}

// a wave per chunk (grid stride): the rows' outputs, with MEAT the chunk's score -> scores[k * kScorePark + entry]; the wave's record
// carries its sum e^2 alone.  The first chunk of a group (chunk_r0 == chunk_first) writes the group's alpha.
template <typename T, int P, bool MEAT>
__global__ __launch_bounds__(64) void within_chunk_kernel(const T* const* __restrict__ cols, const int64_t* __restrict__ chunk_r0,
                                                          const int64_t* __restrict__ chunk_n, const int64_t* __restrict__ chunk_g,
                                                          const int64_t* __restrict__ chunk_first, int64_t n_chunks, int64_t n_groups,
                                                          const double* __restrict__ beta, const double* __restrict__ means,
                                                          const int64_t* __restrict__ gmap, T* __restrict__ alpha, WpRowOut<T> ro,
                                                          double* __restrict__ scores, double* __restrict__ partials) {
    __shared__ double xt[MEAT ? (P + 1) * kScoreTileStride : 1];
    const int lane = threadIdx.x;
    double b[P];
#pragma unroll
    for (int c = 0; c < P; ++c) b[c] = beta[c];
    gptr<T> cx[P];
#pragma unroll
    for (int c = 0; c < P; ++c) cx[c] = as_global(cols[c]);
    const gptr<T> cy = as_global(cols[P]);
    CompSq ee;
    for (int64_t k = blockIdx.x; k < n_chunks; k += gridDim.x) {
        const int64_t gi = chunk_g[k], r0 = chunk_r0[k];
        double m[P + 1];
        const double a = wp_group_means<P>(means, n_groups, gi, b, m);
        if (alpha && lane == 0 && r0 == chunk_first[k]) alpha[gmap ? gmap[gi] : gi] = (T)a;
        d4 sc = {0.0, 0.0, 0.0, 0.0};
        wp_stream<T, P, MEAT>(cx, cy, r0, chunk_n[k], m, b, ro, xt, lane, sc, ee);
        if constexpr (MEAT) score_store_d(scores + k * kScorePark, lane, sc, 0.0);
    }
    ScoreMeat<false>{}.write_record(partials + (int64_t)blockIdx.x * kMixedRecStride, lane, ee);
}

}  // namespace

// one wave per block, 12 per compute unit, as the cluster pass (DESIGN 4.4b measured that grid on this stream)
int within_pass_blocks(const pds_ctx* ctx, int64_t n_work) {
    return (int)std::max<int64_t>(1, std::min<int64_t>(n_work, (int64_t)ctx->num_cus * 12));
}

template <typename T>
int launch_within_pass(pds_ctx* ctx, const T* const* d_cols, int n_feat, const int64_t* d_off, int64_t n_groups, int64_t split_rows,
                       const MixedChunks& ch, double* d_scores, const double* d_beta, const double* d_means, bool meat, const int64_t* d_gmap,
                       const uint32_t* d_perm, T* d_alpha, T* d_pred, T* d_resid, double* d_partials, double* d_stage, double* d_rec) {
    if (n_feat < 1 || n_feat > kMaxFeatSmall) return fail(PDS_ERR_UNSUPPORTED, "fixed-effects regression: up to 16 feature columns");
    if (meat && ch.n_chunks > 0 && !d_scores) return fail(PDS_ERR_INVALID, "null argument");
    KernelTimer timer(ctx, kKindPass2);
    const int nb = within_pass_blocks(ctx, n_groups);
    const int nbc = ch.n_chunks > 0 ? within_pass_blocks(ctx, ch.n_chunks) : 0;
    const int nbl = ch.n_chunks > 0 && meat ? within_pass_blocks(ctx, ch.n_long) : 0;
    const WpRowOut<T> ro{d_perm, d_pred, d_resid};
    dispatch_width<1, kMaxFeatSmall>(n_feat, [&](auto pc) {
        constexpr int P = decltype(pc)::value;
        auto go = [&](auto mc) {
            constexpr bool MEAT = decltype(mc)::value;
            hipLaunchKernelGGL((within_pass_kernel<T, P, MEAT>), dim3(nb), dim3(64), 0, ctx->stream, d_cols, d_off, n_groups, split_rows, d_beta,
                               d_means, d_gmap, d_alpha, ro, d_partials);
            if (nbc > 0)
                hipLaunchKernelGGL((within_chunk_kernel<T, P, MEAT>), dim3(nbc), dim3(64), 0, ctx->stream, d_cols, ch.d_chunk_r0, ch.d_chunk_n,
                                   ch.d_chunk_g, ch.d_chunk_first, ch.n_chunks, n_groups, d_beta, d_means, d_gmap, d_alpha, ro, d_scores,
                                   d_partials + (int64_t)nb * kMixedRecStride);
        };
        if (meat) go(std::true_type{});
        else go(std::false_type{});
    });
    if (nbl > 0)
        hipLaunchKernelGGL(score_long_meat_kernel<false>, dim3(nbl), dim3(64), 0, ctx->stream, ch.d_long_c0, ch.d_long_nc, ch.n_long,
                           (const double*)d_scores, d_partials + (int64_t)(nb + nbc) * kMixedRecStride);
    PDS_HIP_CHECK(hipGetLastError());
    return launch_sum_records(ctx, d_partials, nb + nbc + nbl, d_stage, d_rec, /*compensated=*/true);
}

template int launch_within_pass<double>(pds_ctx*, const double* const*, int, const int64_t*, int64_t, int64_t, const MixedChunks&, double*,
                                        const double*, const double*, bool, const int64_t*, const uint32_t*, double*, double*, double*, double*,
                                        double*, double*);
template int launch_within_pass<float>(pds_ctx*, const float* const*, int, const int64_t*, int64_t, int64_t, const MixedChunks&, double*,
                                       const double*, const double*, bool, const int64_t*, const uint32_t*, float*, float*, float*, double*,
                                       double*, double*);

}  // namespace pds
