// cluster_meat.hip -- the device side of the cluster-robust report (capi_report_cluster.hpp): the meat of the sandwich,
//     M = sum_g s_g s_g',   s_g = X_g' e_g   (p' values per cluster; with a bias its last entry is sum e),
// and sum e^2, in ONE pass over the frame.
//
// The score / meat idiom itself (the compensated sum e^2, the score step, the park and its flush, the record, the long-cluster kernel)
// is score_meat_dev.hpp's, shared with within_pass.hip; this file instantiates it with a bias entry (HAS_BIAS = true).
//
//   * cluster_meat_kernel: ONE wave walks clusters (grid stride) and takes the rows of a cluster 64 per step through a wave-private
//     LDS tile (feature-major, row stride kScoreTileStride: the wave-tile idiom of wave_tile_dev.hpp).  e_i = y_i - [x_i, 1] . beta is
//     formed per row in registers and written to the tile behind the features.  The score of the cluster comes from one
//     v_mfma_f64_16x16x4 per four rows with operands (x, [e | 0 ..]) -- the side block of the Gram tile, as W_xy in mixed.hip --
//     accumulated over the cluster's steps; the bias entry sum e is a per-lane register folded by wave_sum().  e^2 is summed per
//     lane across ALL the clusters of the wave and folded once at its end -- as a compensated sum (value + error term, two-sum at
//     every level: lane, butterfly, records): r2 = 1 - sum e^2 / (n var y) magnifies the sum's last bits by (1 - r2) / r2.
//     A step's 17 loads are issued back to back on a clamped row index (a dead lane re-reads the cluster's first row and drops
//     it): behind a per-column `live ?` each load waited for the one before.  The next cluster's offsets are fetched a cluster ahead.
//   * the meat is S'S with the CLUSTER as the K dimension: a finished score is parked in LDS (four slots); every four clusters
//     one v_mfma_f64_16x16x4 with operands (s, s) adds their outer products to the 16 x 16 feature block, a second one with
//     B = [s_bias | 0 ..] gives the bias column, and the bias diagonal is a wave-uniform register.  A short last batch is flushed
//     with zero scores in the unused slots.  The wave keeps the meat across all the clusters it walks and writes ONE partial record.
//   * clusters above `split_rows` are cut by the host into row chunks that are separate work items: cluster_chunk_scores_kernel
//     (a wave per chunk: the chunk's score to memory, its e^2 into the wave's record) and score_long_meat_kernel<true> (a cluster's
//     chunk scores added in chunk order, lane = entry, then the same parking and outer products).
//   * records have the layout of mixed.hip's (common.hpp) and are added in index order in two stages by launch_sum_records
//     (mixed.hip) with a compensated running sum per entry: no floating-point atomics anywhere, so two calls give the same bits.
// Arithmetic is f64 for f64 and f32 frames alike (an f32 frame and its coefficients are converted on load).
#include "score_meat_dev.hpp"

#include <algorithm>

namespace pds {

namespace {

// beta (features, then the bias or 0) as doubles
template <typename T, int P>
__device__ __forceinline__ void cm_load_beta(const T* __restrict__ beta, int bias, double* b) {
#pragma unroll
    for (int c = 0; c < P; ++c) b[c] = (double)beta[c];
    b[P] = bias ? (double)beta[P] : 0.0;
}

// rows [r0, r0 + n) of the frame, 64 per step: their residuals' score into sc (side block, column 0), sum e into es, sum e^2 into ee
template <typename T, int P>
__device__ __forceinline__ void cm_stream_score(const gptr<T>* cx, gptr<T> cy, int64_t r0, int64_t n, const double* b, double* xt, int lane,
                                                d4& sc, double& es, CompSq& ee) {
    const int f = lane & 15, kq = lane >> 4;
    for (int64_t base = 0; base < n; base += 64) {
        const int64_t r = base + lane;
        const bool live = r < n;
        const int64_t ri = r0 + (live ? r : 0);  // (n >= 1: the cluster's first row is always there)
        T raw[P + 1];
#pragma unroll
        for (int c = 0; c < P; ++c) raw[c] = cx[c][ri];
        raw[P] = cy[ri];
        PDS_WAVE_LDS_SYNC();  // (the previous step's operand reads are done)
        double e = live ? (double)raw[P] - b[P] : 0.0;
#pragma unroll
        for (int c = 0; c < P; ++c) {
            const double x = live ? (double)raw[c] : 0.0;
            xt[c * kScoreTileStride + lane] = x;
            e = fma(-x, b[c], e);
        }
        xt[P * kScoreTileStride + lane] = e;
        es += e;
        ee.add(e);
        PDS_WAVE_LDS_SYNC();
        const int rows = (int)std::min<int64_t>(64, n - base);
        const int steps = (rows + 3) >> 2;  // (the row slots past `rows` hold zeros)
        for (int m = 0; m < steps; ++m) score_rows4<P>(xt, 4 * m + kq, f, sc);
    }
}

template <typename T, int P>
__global__ __launch_bounds__(64) void cluster_meat_kernel(const T* const* __restrict__ cols, const int64_t* __restrict__ off, int64_t n_clusters,
                                                          int64_t split_rows, const T* __restrict__ beta, int bias,
                                                          double* __restrict__ partials) {
    __shared__ double xt[(P + 1) * kScoreTileStride + kScoreBatch * kScorePark];  // features 0 .. P - 1, then e: [c * kScoreTileStride + row]; the park
    double* park = xt + (P + 1) * kScoreTileStride;
    const int lane = threadIdx.x;
    double b[P + 1];
    cm_load_beta<T, P>(beta, bias, b);
    gptr<T> cx[P];
#pragma unroll
    for (int c = 0; c < P; ++c) cx[c] = as_global(cols[c]);
    const gptr<T> cy = as_global(cols[P]);
    ScoreMeat<true> mt;
    mt.bias = bias;
    CompSq ee;
    int64_t g = blockIdx.x;
    int64_t o0 = g < n_clusters ? off[g] : 0, o1 = g < n_clusters ? off[g + 1] : 0;  // (the host has validated the offsets)
    while (g < n_clusters) {
        const int64_t r0 = o0, n = o1 - o0;
        g += gridDim.x;  // the next cluster's offsets: asked for now, needed a cluster later
        o0 = g < n_clusters ? off[g] : 0;
        o1 = g < n_clusters ? off[g + 1] : 0;
        if (n <= 0 || n > split_rows) continue;  // empty: nothing; cut into chunks: the chunk kernels
        d4 sc = {0.0, 0.0, 0.0, 0.0};
        double es = 0.0;
        cm_stream_score<T, P>(cx, cy, r0, n, b, xt, lane, sc, es, ee);
        const double sb = bias ? wave_sum(es) : 0.0;
        mt.park_d(park, lane, sc, sb);
    }
    mt.flush(park, lane);
    mt.write_record(partials + (int64_t)blockIdx.x * kMixedRecStride, lane, ee);
}

// a wave per chunk (grid stride): the chunk's score -> scores[k * kScorePark + entry]; the wave's record carries its sum e^2 alone
template <typename T, int P>
__global__ __launch_bounds__(64) void cluster_chunk_scores_kernel(const T* const* __restrict__ cols, const int64_t* __restrict__ chunk_r0,
                                                                  const int64_t* __restrict__ chunk_n, int64_t n_chunks,
                                                                  const T* __restrict__ beta, int bias, double* __restrict__ scores,
                                                                  double* __restrict__ partials) {
    __shared__ double xt[(P + 1) * kScoreTileStride];
    const int lane = threadIdx.x;
    double b[P + 1];
    cm_load_beta<T, P>(beta, bias, b);
    gptr<T> cx[P];
#pragma unroll
    for (int c = 0; c < P; ++c) cx[c] = as_global(cols[c]);
    const gptr<T> cy = as_global(cols[P]);
    CompSq ee;
    for (int64_t k = blockIdx.x; k < n_chunks; k += gridDim.x) {
        d4 sc = {0.0, 0.0, 0.0, 0.0};
        double es = 0.0;
        cm_stream_score<T, P>(cx, cy, chunk_r0[k], chunk_n[k], b, xt, lane, sc, es, ee);
        const double sb = bias ? wave_sum(es) : 0.0;
        score_store_d(scores + k * kScorePark, lane, sc, sb);
    }
    ScoreMeat<true>{}.write_record(partials + (int64_t)blockIdx.x * kMixedRecStride, lane, ee);
}

}  // namespace

// one wave per block, 12 per compute unit (three per SIMD: measured against 4, 8 and 16 on the 1e8 x 16 frame);
// "cluster_waves" caps the grid (which wave walks which clusters: a smaller grid gives other sums, to rounding)
int cluster_meat_blocks(const pds_ctx* ctx, int64_t n_work) {
    const int64_t cap = ctx->opt_cluster_waves > 0 ? ctx->opt_cluster_waves : (int64_t)ctx->num_cus * 12;
    return (int)std::max<int64_t>(1, std::min<int64_t>(n_work, cap));
}

template <typename T>
int launch_cluster_meat(pds_ctx* ctx, const T* const* d_cols, int n_feat, const int64_t* d_off, int64_t n_clusters, int64_t split_rows,
                        const ClusterChunks& ch, const T* d_beta, int bias, double* d_partials, double* d_stage, double* d_rec) {
    if (n_feat < 1 || n_feat > kMaxFeatSmall) return fail(PDS_ERR_UNSUPPORTED, "cluster-robust report: up to 16 feature columns");
    KernelTimer timer(ctx, kKindPass2);
    const int nb = cluster_meat_blocks(ctx, n_clusters);
    const int nbc = ch.n_chunks > 0 ? cluster_meat_blocks(ctx, ch.n_chunks) : 0;
    const int nbl = ch.n_chunks > 0 ? cluster_meat_blocks(ctx, ch.n_long) : 0;
    dispatch_width<1, kMaxFeatSmall>(n_feat, [&](auto pc) {
        constexpr int P = decltype(pc)::value;
        hipLaunchKernelGGL((cluster_meat_kernel<T, P>), dim3(nb), dim3(64), 0, ctx->stream, d_cols, d_off, n_clusters, split_rows, d_beta, bias,
                           d_partials);
        if (nbc > 0) {
            hipLaunchKernelGGL((cluster_chunk_scores_kernel<T, P>), dim3(nbc), dim3(64), 0, ctx->stream, d_cols, ch.d_chunk_r0, ch.d_chunk_n,
                               ch.n_chunks, d_beta, bias, ch.d_scores, d_partials + (int64_t)nb * kMixedRecStride);
            hipLaunchKernelGGL((score_long_meat_kernel<true, int>), dim3(nbl), dim3(64), 0, ctx->stream, ch.d_long_c0, ch.d_long_nc, ch.n_long,
                               (const double*)ch.d_scores, bias, d_partials + (int64_t)(nb + nbc) * kMixedRecStride);
        }
    });
    PDS_HIP_CHECK(hipGetLastError());
    return launch_sum_records(ctx, d_partials, nb + nbc + nbl, d_stage, d_rec, /*compensated=*/true);
}

template int launch_cluster_meat<double>(pds_ctx*, const double* const*, int, const int64_t*, int64_t, int64_t, const ClusterChunks&, const double*,
                                         int, double*, double*, double*);
template int launch_cluster_meat<float>(pds_ctx*, const float* const*, int, const int64_t*, int64_t, int64_t, const ClusterChunks&, const float*, int,
                                        double*, double*, double*);

}  // namespace pds
