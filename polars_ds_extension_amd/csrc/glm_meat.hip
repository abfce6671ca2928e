// glm_meat.hip -- the device side of the robust / cluster-robust one-model GLM report (capi_glm_sandwich.hpp): the meat of the sandwich
// V = I^-1 M I^-1 at the coefficients as stored, in ONE pass over the frame.  Per row
//     eta_i = x_i . beta + o_i,   mu_i = g^-1(eta_i),   r_i = pw_i (y_i - mu_i) / (V(mu_i) g'(mu_i))
// is the score residual (general in (link, variance): glm_dev.hpp); a row with pw_i <= 0 has r_i = 0 by a select, so that whatever
// its mu is cannot reach a sum; its features enter the tiles as zeros for the same reason (the FIT asks that they be finite: they give
// the row's linear predictor there).  With a bias the score carries the constant 1 last: its entry is sum r.
//
// The score / meat idiom (the tile, the score step, the park and its flush, the record, the long-cluster kernel) is
// score_meat_dev.hpp's, shared with cluster_meat.hip and within_pass.hip; this file instantiates it with a bias entry.
//
//   * glm_cluster_meat_kernel (cluster forms): M = sum_g s_g s_g', s_g = sum_{i in g} r_i x_i.  ONE wave walks clusters (grid stride),
//     64 rows per step through the wave-private LDS tile.  A step issues its loads back to back on a clamped row index (P features,
//     y, and pw / o when present), forms r_i per row in registers and writes it behind the features; the score comes from
//     score_rows4<P>, sum r from a per-lane register folded by wave_sum(); the finished score is parked (ScoreMeat<true>::park_d)
//     and multiplied four clusters at a time.  The wave counts the clusters that hold a row of positive weight, and those rows,
//     into its record (kGlmRecClusters, kGlmRecRows: integer-valued doubles, exact under the record sum).
//   * clusters above `split_rows` are cut by the host into row chunks: glm_chunk_scores_kernel (a wave per chunk: the chunk's score
//     to memory, and in the score's padding entry whether the chunk holds a row of positive weight), score_long_meat_kernel<true, int>
//     (the chunk scores added in chunk order, parked and multiplied) and glm_long_count_kernel (the long clusters with a positive
//     chunk, one record).
//   * glm_hc_meat_kernel (hc0 / hc1): M = sum_i r_i^2 x_i x_i', the same tile with ROWS as the K dimension.  Work items are row
//     ranges of kGlmHcSteps 64-row steps (grid stride).  A step writes x_c r_i into feature row c and r_i into row P; per four
//     rows one v_mfma_f64_16x16x4 with operands (x r, x r) adds to the feature block and one more with B = [r | 0 ..] gives the bias
//     column; sum r^2 is a compensated sum and is the bias diagonal (record slots kScoreRecEE + kScoreRecEC).  There is no park.
//   * records have the layout of common.hpp and are added in index order by launch_sum_records(compensated): no floating-point
//     atomic anywhere, two calls give the same bits, and the host drops empty clusters before the launch.
// Arithmetic is f64 for f64 and f32 frames alike (an f32 frame, its weights, offsets and coefficients are converted on load).
#include "glm_dev.hpp"
#include "score_meat_dev.hpp"

#include <algorithm>

namespace pds {

namespace {

constexpr int kGlmHcSteps = 8;  // 64-row steps of a work item of the HC pass

// what a wave needs of the model: beta (features, then the bias or 0) as doubles, the frame's columns and the family
template <typename T, int P>
struct GlmRows {
    double b[P + 1];
    gptr<T> cx[P], cy, cpw, co;
    bool has_pw, has_o;
    int link, variance;

    // cols: x_0 .. x_{P-1}, y, weights (nullable), offset (nullable)
    __device__ __forceinline__ void open(const T* const* __restrict__ cols, const T* __restrict__ beta, int bias, int link_, int variance_) {
#pragma unroll
        for (int c = 0; c < P; ++c) b[c] = (double)beta[c];
        b[P] = bias ? (double)beta[P] : 0.0;
#pragma unroll
        for (int c = 0; c < P; ++c) cx[c] = as_global(cols[c]);
        cy = as_global(cols[P]);
        has_pw = cols[P + 1] != nullptr;
        has_o = cols[P + 2] != nullptr;
        cpw = as_global(cols[P + 1]);
        co = as_global(cols[P + 2]);
        link = link_;
        variance = variance_;
    }

    // row ri of the frame: its features into x (zeros for a dead lane) and its score residual; pos: the row counts (live, pw > 0)
    __device__ __forceinline__ double residual(int64_t ri, bool live, double* x, bool& pos) const {
        T raw[P + 1];
#pragma unroll
        for (int c = 0; c < P; ++c) raw[c] = cx[c][ri];
        raw[P] = cy[ri];
        const T rpw = has_pw ? cpw[ri] : T(1);
        const T ro = has_o ? co[ri] : T(0);
        double eta = b[P] + (double)ro;
#pragma unroll
        for (int c = 0; c < P; ++c) {
            x[c] = live ? (double)raw[c] : 0.0;
            eta = fma(x[c], b[c], eta);
        }
        const double pw = (double)rpw;
        const double mu = glm_inv<double>(link, eta);
        const double r = pw * ((double)raw[P] - mu) / (glm_var<double>(variance, mu) * glm_deriv<double>(link, mu));
        pos = live && pw > 0.0;
        return pos ? r : 0.0;  // (a select: a dead lane's or a zero-weight row's r, whatever it is, reaches no sum)
    }
};

// rows [r0, r0 + n) of the frame, 64 per step: their score into sc (side block, column 0), sum r into es; any: a row counted;
// npos: the lane's rows of positive weight (an integer)
template <typename T, int P>
__device__ __forceinline__ void gm_stream_score(const GlmRows<T, P>& gr, int64_t r0, int64_t n, double* xt, int lane, d4& sc, double& es,
                                                bool& any, double& npos) {
    const int f = lane & 15, kq = lane >> 4;
    for (int64_t base = 0; base < n; base += 64) {
        const int64_t r = base + lane;
        const bool live = r < n;
        const int64_t ri = r0 + (live ? r : 0);  // (n >= 1: the cluster's first row is always there)
        double x[P];
        bool pos;
        const double e = gr.residual(ri, live, x, pos);
        PDS_WAVE_LDS_SYNC();  // (the previous step's operand reads are done)
#pragma unroll
        for (int c = 0; c < P; ++c) xt[c * kScoreTileStride + lane] = pos ? x[c] : 0.0;  // (r = 0 there: 0 x, not 0 * x, reaches the score)
        xt[P * kScoreTileStride + lane] = e;
        es += e;
        any |= pos;
        npos += pos ? 1.0 : 0.0;
        PDS_WAVE_LDS_SYNC();
        const int rows = (int)std::min<int64_t>(64, n - base);
        const int steps = (rows + 3) >> 2;  // (the row slots past `rows` hold zeros)
        for (int m = 0; m < steps; ++m) score_rows4<P>(xt, 4 * m + kq, f, sc);
    }
}

// the record slots of the two counts, integer-valued doubles (exact under the record sum): the clusters that hold a row of positive
// weight (the log-determinant slot of mixed.hip's layout) and the rows of positive weight (the first slot of its cross-moment row);
// no score / meat pass uses either
constexpr int kGlmRecClusters = kMixedRecLD, kGlmRecRows = kMixedRecCM;

// after ScoreMeat::write_record: the counts into their slots, each by the lane that zeroed it (one lane, program order); npos is the
// lane's own count and is folded here
__device__ __forceinline__ void gm_write_counts(double* rec, int lane, double clusters, double npos) {
    const double rows = wave_sum(npos);  // (integers: exact)
    if (lane == kGlmRecClusters - kMixedRecCM) rec[kGlmRecClusters] = clusters;
    if (lane == kGlmRecRows - kMixedRecCM) rec[kGlmRecRows] = rows;
}

template <typename T, int P>
__global__ __launch_bounds__(64) void glm_cluster_meat_kernel(const T* const* __restrict__ cols, const int64_t* __restrict__ off, int64_t n_clusters,
                                                              int64_t split_rows, const T* __restrict__ beta, int bias, int link, int variance,
                                                              double* __restrict__ partials) {
    __shared__ double xt[(P + 1) * kScoreTileStride + kScoreBatch * kScorePark];  // features 0 .. P - 1, then r: [c * kScoreTileStride + row]; the park
    double* park = xt + (P + 1) * kScoreTileStride;
    const int lane = threadIdx.x;
    GlmRows<T, P> gr;
    gr.open(cols, beta, bias, link, variance);
    ScoreMeat<true> mt;
    mt.bias = bias;
    double count = 0.0, npos = 0.0;
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
        bool any = false;
        gm_stream_score<T, P>(gr, r0, n, xt, lane, sc, es, any, npos);
        if (__ballot(any) != 0) count += 1.0;
        const double sb = bias ? wave_sum(es) : 0.0;
        mt.park_d(park, lane, sc, sb);
    }
    mt.flush(park, lane);
    double* rec = partials + (int64_t)blockIdx.x * kMixedRecStride;
    mt.write_record(rec, lane, CompSq{});
    gm_write_counts(rec, lane, count, npos);
}

// a wave per chunk (grid stride): the chunk's score -> scores[k * kScorePark + entry], entry 17 (the padding, which nothing
// multiplies): 1 when the chunk holds a row of positive weight.  The wave's record carries its rows of positive weight alone.
template <typename T, int P>
__global__ __launch_bounds__(64) void glm_chunk_scores_kernel(const T* const* __restrict__ cols, const int64_t* __restrict__ chunk_r0,
                                                              const int64_t* __restrict__ chunk_n, int64_t n_chunks, const T* __restrict__ beta,
                                                              int bias, int link, int variance, double* __restrict__ scores,
                                                              double* __restrict__ partials) {
    __shared__ double xt[(P + 1) * kScoreTileStride];
    const int lane = threadIdx.x;
    GlmRows<T, P> gr;
    gr.open(cols, beta, bias, link, variance);
    double npos = 0.0;
    for (int64_t k = blockIdx.x; k < n_chunks; k += gridDim.x) {
        d4 sc = {0.0, 0.0, 0.0, 0.0};
        double es = 0.0;
        bool any = false;
        gm_stream_score<T, P>(gr, chunk_r0[k], chunk_n[k], xt, lane, sc, es, any, npos);
        const double sb = bias ? wave_sum(es) : 0.0;
        const double flag = __ballot(any) != 0 ? 1.0 : 0.0;
        score_store_d(scores + k * kScorePark, lane, sc, sb);
        if (lane == 0) scores[k * kScorePark + 17] = flag;  // (the lane that zeroed it)
    }
    double* rec = partials + (int64_t)blockIdx.x * kMixedRecStride;
    ScoreMeat<true>{}.write_record(rec, lane, CompSq{});
    gm_write_counts(rec, lane, 0.0, npos);
}

// ONE wave: the long clusters with a chunk that holds a row of positive weight -> one record with nothing else in it
__global__ __launch_bounds__(64) void glm_long_count_kernel(const int64_t* __restrict__ long_c0, const int64_t* __restrict__ long_nc, int64_t n_long,
                                                            const double* __restrict__ scores, double* __restrict__ rec) {
    const int lane = threadIdx.x;
    double count = 0.0;
    for (int64_t j = lane; j < n_long; j += 64) {
        const int64_t c0 = long_c0[j], nc = long_nc[j];
        bool any = false;
        for (int64_t k = 0; k < nc; ++k) any |= scores[(c0 + k) * kScorePark + 17] > 0.0;
        count += any ? 1.0 : 0.0;
    }
    count = wave_sum(count);  // (integers: exact)
    for (int slot = lane; slot < kMixedRecStride; slot += 64) rec[slot] = slot == kGlmRecClusters ? count : 0.0;
}

// hc0 / hc1: work item t is the rows [t * 64 kGlmHcSteps, (t + 1) * 64 kGlmHcSteps) of the frame
template <typename T, int P>
__global__ __launch_bounds__(64) void glm_hc_meat_kernel(const T* const* __restrict__ cols, int64_t n_rows, const T* __restrict__ beta, int bias,
                                                         int link, int variance, double* __restrict__ partials) {
    __shared__ double xt[(P + 1) * kScoreTileStride];  // x_c r in feature row c, r in row P
    const int lane = threadIdx.x;
    GlmRows<T, P> gr;
    gr.open(cols, beta, bias, link, variance);
    ScoreMeat<true> mt;  // (the holder of the accumulators and the writer of the record: nothing is parked)
    mt.bias = bias;
    CompSq rr;
    double npos = 0.0;
    constexpr int64_t kItemRows = 64 * kGlmHcSteps;
    const int64_t n_items = (n_rows + kItemRows - 1) / kItemRows;
    for (int64_t t = blockIdx.x; t < n_items; t += gridDim.x) {
        const int64_t end = std::min<int64_t>(n_rows, (t + 1) * kItemRows);
        for (int64_t base = t * kItemRows; base < end; base += 64) {
            const int64_t r = base + lane;
            const bool live = r < end;
            double x[P];
            bool pos;
            const double e = gr.residual(live ? r : base, live, x, pos);  // (base < end <= n_rows: a dead lane re-reads a row of the frame)
            PDS_WAVE_LDS_SYNC();  // (the previous step's operand reads are done)
#pragma unroll
            for (int c = 0; c < P; ++c) xt[c * kScoreTileStride + lane] = pos ? x[c] * e : 0.0;
            xt[P * kScoreTileStride + lane] = e;
            rr.add(e);
            npos += pos ? 1.0 : 0.0;
            PDS_WAVE_LDS_SYNC();
            const int rows = (int)std::min<int64_t>(64, end - base);
            if (bias)
                wave_tile_gram<P>(xt, kScoreTileStride, rows, lane, TileNoScale{},
                                  [&](int f, int row) { return f == 0 ? xt[P * kScoreTileStride + row] : 0.0; }, mt.m, mt.mb);
            else
                wave_tile_gram<P>(xt, kScoreTileStride, rows, lane, TileNoScale{}, mt.m);
        }
    }
    double* rec = partials + (int64_t)blockIdx.x * kMixedRecStride;
    mt.write_record(rec, lane, rr);
    gm_write_counts(rec, lane, 0.0, npos);
}

}  // namespace

int64_t glm_hc_items(int64_t n_rows) { return (n_rows + 64 * kGlmHcSteps - 1) / (64 * kGlmHcSteps); }

int glm_meat_records(const pds_ctx* ctx, int64_t n_rows, int64_t n_clusters, const ClusterChunks& ch) {
    if (n_clusters <= 0) return cluster_meat_blocks(ctx, glm_hc_items(n_rows));
    return cluster_meat_blocks(ctx, n_clusters) +
           (ch.n_chunks > 0 ? cluster_meat_blocks(ctx, ch.n_chunks) + cluster_meat_blocks(ctx, ch.n_long) + 1 : 0);
}

template <typename T>
int launch_glm_meat(pds_ctx* ctx, const T* const* d_cols, int n_feat, int64_t n_rows, const int64_t* d_off, int64_t n_clusters,
                    int64_t split_rows, const ClusterChunks& ch, const T* d_beta, int bias, int link, int variance, double* d_partials,
                    double* d_stage, double* d_rec) {
    if (n_feat < 1 || n_feat > kMaxFeatSmall) return fail(PDS_ERR_UNSUPPORTED, "robust GLM report: up to 16 feature columns");
    KernelTimer timer(ctx, kKindPass2);
    int n_rec = 0;
    if (n_clusters <= 0) {
        const int nb = cluster_meat_blocks(ctx, glm_hc_items(n_rows));
        dispatch_width<1, kMaxFeatSmall>(n_feat, [&](auto pc) {
            constexpr int P = decltype(pc)::value;
            hipLaunchKernelGGL((glm_hc_meat_kernel<T, P>), dim3(nb), dim3(64), 0, ctx->stream, d_cols, n_rows, d_beta, bias, link, variance,
                               d_partials);
        });
        n_rec = nb;
    } else {
        const int nb = cluster_meat_blocks(ctx, n_clusters);
        const int nbc = ch.n_chunks > 0 ? cluster_meat_blocks(ctx, ch.n_chunks) : 0;
        const int nbl = ch.n_chunks > 0 ? cluster_meat_blocks(ctx, ch.n_long) : 0;
        dispatch_width<1, kMaxFeatSmall>(n_feat, [&](auto pc) {
            constexpr int P = decltype(pc)::value;
            hipLaunchKernelGGL((glm_cluster_meat_kernel<T, P>), dim3(nb), dim3(64), 0, ctx->stream, d_cols, d_off, n_clusters, split_rows, d_beta,
                               bias, link, variance, d_partials);
            if (nbc > 0) {
                hipLaunchKernelGGL((glm_chunk_scores_kernel<T, P>), dim3(nbc), dim3(64), 0, ctx->stream, d_cols, ch.d_chunk_r0, ch.d_chunk_n,
                                   ch.n_chunks, d_beta, bias, link, variance, ch.d_scores, d_partials + (int64_t)nb * kMixedRecStride);
                hipLaunchKernelGGL((score_long_meat_kernel<true, int>), dim3(nbl), dim3(64), 0, ctx->stream, ch.d_long_c0, ch.d_long_nc, ch.n_long,
                                   (const double*)ch.d_scores, bias, d_partials + (int64_t)(nb + nbc) * kMixedRecStride);
                hipLaunchKernelGGL(glm_long_count_kernel, dim3(1), dim3(64), 0, ctx->stream, ch.d_long_c0, ch.d_long_nc, ch.n_long,
                                   (const double*)ch.d_scores, d_partials + (int64_t)(nb + nbc + nbl) * kMixedRecStride);
            }
        });
        n_rec = nb + nbc + nbl + (nbc > 0 ? 1 : 0);
    }
    PDS_HIP_CHECK(hipGetLastError());
    return launch_sum_records(ctx, d_partials, n_rec, d_stage, d_rec, /*compensated=*/true);
}

template int launch_glm_meat<double>(pds_ctx*, const double* const*, int, int64_t, const int64_t*, int64_t, int64_t, const ClusterChunks&,
                                     const double*, int, int, int, double*, double*, double*);
template int launch_glm_meat<float>(pds_ctx*, const float* const*, int, int64_t, const int64_t*, int64_t, int64_t, const ClusterChunks&,
                                    const float*, int, int, int, double*, double*, double*);

}  // namespace pds
