// within_cluster.hip -- the device side of the fixed-effects regression's standard errors clustered on ANY key (capi_within_cluster.hpp):
// the meat M = sum_c s_c s_c', s_c = sum_{i in c} x~_i e_i, over clusters c that are NOT contiguous in the order the within pass walks.
// x~ and e are the projected features and the residuals of the fit (one absorbed factor: x - m_g; two: the projected columns less
// their factor-1 means); the cluster key arrives as dense int32 codes per row.  That is a gather problem, solved the way the
// two-factor sweeps solve it for factor 2: a stable radix order of (code, row) (launch_within2_order), the level starts from the run
// boundaries (w2g_level_starts_kernel), chunk lists of at most 1 024 rows built on the host.  What is new here:
//
//   * cluster_nested_kernel<Off>: NESTEDNESS, integers only.  One wave per level of an absorbed factor (grid stride) takes the minimum
//     and the maximum cluster code over the level's rows -- factor 1: the rows [off[l], off[l + 1]) of the frame; factor 2: the same
//     walk over the code-2 ordered row index of the two-factor pipeline.  A wave that saw min != max raises the factor's flag with one
//     integer atomicOr; a wave that finds the flag up ends its walk (the answer is known); the host reads the two flags.
//   * within_row_scores_kernel<T, P>: the STAGING pass.  within_pass_kernel's walk over the frame (a wave per group, 64 rows per step,
//     the groups above the split threshold as the same chunks), the step's column loads issued back to back on a clamped row index;
//     x~_i and e_i are formed in f64 from the group means and beta exactly as the within pass forms them, and the row's score x~_i e_i is
//     written row-major (within_cluster_dev.hpp: P doubles per row, padded to an even count).  One contiguous read of the frame, one
//     streamed write of n x P x 8 bytes.  WHY: gathering the column-major frame directly costs P + 1 cache lines per row; one staged
//     row is 1 - 3 lines.
//   * cluster_gather_chunk_kernel<P>: a wave per chunk of the cluster-ordered row index (grid stride), lane = row.  The lane looks up
//     its row (the place is clamped in the tail chunk, the value masked), reads the staged score row and adds it to its P running
//     sums; after the chunk's steps every column is summed over the wave by the fixed-order butterfly of wave_sum().  The wave writes
//     one record of kClusterScoreStride doubles per chunk (entries P .. 17 are zeros).  No LDS, no floating-point atomics.
//   * the meat: score_long_meat_kernel<false> (score_meat_dev.hpp) with (first chunk, chunks) per occupied cluster -- a cluster's chunk
//     scores added in chunk order, four finished scores per v_mfma_f64_16x16x4, one record per wave, the records folded by
//     launch_sum_records (compensated, as the within pass folds its own).
// Every loop is counted; no workgroup waits for another; two calls give the same bits.
#include "score_meat_dev.hpp"
#include "within_cluster_dev.hpp"

#include <algorithm>
#include <climits>

namespace pds {

namespace {

// min / max of the cluster codes over the rows of every level; idx (nullable): place r of the level's list is row idx[r] of the frame
template <typename Off>
__global__ __launch_bounds__(64) void cluster_nested_kernel(const Off* __restrict__ off, int64_t n_levels, const uint32_t* __restrict__ idx,
                                                            const int32_t* __restrict__ codes, int* flag) {
    const int lane = threadIdx.x;
    for (int64_t l = blockIdx.x; l < n_levels; l += gridDim.x) {
        // the flag is up: no further level can change the answer.  (Without this a key that crosses EVERY level sends a million
        // atomics to one address: 11.4 ms at 1e6 levels, against 0.2 ms for the walk itself.)
        if (*(const volatile int*)flag != 0) return;
        const int64_t r0 = (int64_t)off[l], r1 = (int64_t)off[l + 1];
        int32_t lo = INT_MAX, hi = INT_MIN;  // (an empty level leaves lo > hi: no flag)
        for (int64_t r = r0 + lane; r < r1; r += 64) {
            const int32_t c = codes[idx ? (int64_t)idx[r] : r];
            lo = c < lo ? c : lo;
            hi = c > hi ? c : hi;
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            const int32_t lo_o = __shfl_xor(lo, o, 64), hi_o = __shfl_xor(hi, o, 64);
            lo = lo_o < lo ? lo_o : lo;
            hi = hi_o > hi ? hi_o : hi;
        }
        if (lane == 0 && lo < hi) atomicOr(flag, 1);
    }
}

// rows [r0, r0 + n) of the frame, 64 per step, centred with m (features, then y): the score x~ e of every live row -> its staged row
template <typename T, int P>
__device__ __forceinline__ void cl_score_rows(const gptr<T>* cx, gptr<T> cy, int64_t r0, int64_t n, const double* m, const double* b,
                                              double* __restrict__ rows, int lane) {
    for (int64_t base = 0; base < n; base += 64) {
        const int64_t r = base + lane;
        const bool live = r < n;
        const int64_t ri = r0 + (live ? r : 0);  // (n >= 1: the first row is always there)
        T raw[P + 1];
#pragma unroll
        for (int c = 0; c < P; ++c) raw[c] = cx[c][ri];
        raw[P] = cy[ri];
        double x[P], e = (double)raw[P] - m[P];
#pragma unroll
        for (int c = 0; c < P; ++c) {
            x[c] = (double)raw[c] - m[c];
            e = fma(-x[c], b[c], e);
        }
#pragma unroll
        for (int c = 0; c < P; ++c) x[c] *= e;
        if (live) cluster_row_store<P>(rows, ri, x);
    }
}

// chunk_r0 == nullptr: a wave walks the groups (grid stride) and skips those above split_rows, as within_pass_kernel does;
// otherwise the work items are the chunks of those groups, as within_chunk_kernel's
template <typename T, int P>
__global__ __launch_bounds__(64) void within_row_scores_kernel(const T* const* __restrict__ cols, const int64_t* __restrict__ off, int64_t n_groups,
                                                               int64_t split_rows, const int64_t* __restrict__ chunk_r0,
                                                               const int64_t* __restrict__ chunk_n, const int64_t* __restrict__ chunk_g,
                                                               int64_t n_work, const double* __restrict__ beta, const double* __restrict__ means,
                                                               double* __restrict__ rows) {
    const int lane = threadIdx.x;
    double b[P];
#pragma unroll
    for (int c = 0; c < P; ++c) b[c] = beta[c];
    gptr<T> cx[P];
#pragma unroll
    for (int c = 0; c < P; ++c) cx[c] = as_global(cols[c]);
    const gptr<T> cy = as_global(cols[P]);
    for (int64_t k = blockIdx.x; k < n_work; k += gridDim.x) {
        int64_t g = k, r0, n;
        if (chunk_r0) {
            g = chunk_g[k];
            r0 = chunk_r0[k];
            n = chunk_n[k];
        } else {
            r0 = off[k];
            n = off[k + 1] - r0;
            if (n <= 0 || n > split_rows) continue;  // empty: nothing; cut into chunks: the second launch
        }
        double m[P + 1];
#pragma unroll
        for (int c = 0; c <= P; ++c) m[c] = means[(int64_t)c * n_groups + g];
        cl_score_rows<T, P>(cx, cy, r0, n, m, b, rows, lane);
    }
}

// a wave per chunk of idx (rows of ONE cluster, ascending): lane = row
template <int P>
__global__ __launch_bounds__(64) void cluster_gather_chunk_kernel(const double* __restrict__ rows, const uint32_t* __restrict__ idx,
                                                                  const int64_t* __restrict__ chunk_pos, const int64_t* __restrict__ chunk_n,
                                                                  int64_t n_chunks, double* __restrict__ scores) {
    constexpr int PS = cluster_row_stride(P);
    const int lane = threadIdx.x;
    const gptr<double> s = as_global(rows);
    for (int64_t k = blockIdx.x; k < n_chunks; k += gridDim.x) {
        const int64_t pos = chunk_pos[k], n = chunk_n[k];
        double acc[P];
#pragma unroll
        for (int c = 0; c < P; ++c) acc[c] = 0.0;
        for (int64_t base = 0; base < n; base += 64) {
            const int64_t i = base + lane;
            const bool live = i < n;
            const int64_t r = (int64_t)idx[pos + (live ? i : n - 1)];  // (n >= 1; the tail's lanes re-read the chunk's last row)
            double v[PS];
            cluster_row_load<P>(s, r, v);
#pragma unroll
            for (int c = 0; c < P; ++c) acc[c] += live ? v[c] : 0.0;
        }
        double mine = 0.0;
#pragma unroll
        for (int c = 0; c < P; ++c) {
            const double tot = wave_sum(acc[c]);
            if (lane == c) mine = tot;
        }
        if (lane < kClusterScoreStride) scores[k * kClusterScoreStride + lane] = mine;
    }
}

int cl_waves(const pds_ctx* ctx, int64_t n_work) { return (int)std::max<int64_t>(1, std::min<int64_t>(n_work, (int64_t)ctx->num_cus * 32)); }

}  // namespace

int launch_cluster_nested(pds_ctx* ctx, const int64_t* d_off1, int64_t n1, const uint32_t* d_start2, int64_t n_levels2, const uint32_t* d_idx2,
                          const int32_t* d_codes, int* d_flags) {
    KernelTimer timer(ctx, kKindGraph);
    PDS_HIP_CHECK(hipMemsetAsync(d_flags, 0, 2 * sizeof(int), ctx->stream));
    hipLaunchKernelGGL(cluster_nested_kernel<int64_t>, dim3(cl_waves(ctx, n1)), dim3(64), 0, ctx->stream, d_off1, n1, (const uint32_t*)nullptr, d_codes,
                       d_flags);
    if (d_start2)
        hipLaunchKernelGGL(cluster_nested_kernel<uint32_t>, dim3(cl_waves(ctx, n_levels2)), dim3(64), 0, ctx->stream, d_start2, n_levels2, d_idx2,
                           d_codes, d_flags + 1);
    PDS_HIP_CHECK(hipGetLastError());
    return PDS_OK;
}

template <typename T>
int launch_within_row_scores(pds_ctx* ctx, const T* const* d_cols, int n_feat, const int64_t* d_off, int64_t n_groups, int64_t split_rows,
                             const MixedChunks& ch, const double* d_beta, const double* d_means, double* d_rows) {
    if (n_feat < 1 || n_feat > kMaxFeatSmall) return fail(PDS_ERR_UNSUPPORTED, "fixed-effects regression: up to 16 feature columns");
    KernelTimer timer(ctx, kKindIter);
    const int nb = within_pass_blocks(ctx, n_groups);
    const int nbc = ch.n_chunks > 0 ? within_pass_blocks(ctx, ch.n_chunks) : 0;
    dispatch_width<1, kMaxFeatSmall>(n_feat, [&](auto pc) {
        constexpr int P = decltype(pc)::value;
        hipLaunchKernelGGL((within_row_scores_kernel<T, P>), dim3(nb), dim3(64), 0, ctx->stream, d_cols, d_off, n_groups, split_rows,
                           (const int64_t*)nullptr, (const int64_t*)nullptr, (const int64_t*)nullptr, n_groups, d_beta, d_means, d_rows);
        if (nbc > 0)
            hipLaunchKernelGGL((within_row_scores_kernel<T, P>), dim3(nbc), dim3(64), 0, ctx->stream, d_cols, d_off, n_groups, split_rows,
                               ch.d_chunk_r0, ch.d_chunk_n, ch.d_chunk_g, ch.n_chunks, d_beta, d_means, d_rows);
    });
    PDS_HIP_CHECK(hipGetLastError());
    return PDS_OK;
}

int cluster_meat_records(const pds_ctx* ctx, int64_t n_clusters) { return within_pass_blocks(ctx, n_clusters); }

int launch_cluster_gather_meat(pds_ctx* ctx, int n_feat, const double* d_rows, const uint32_t* d_idx, const int64_t* d_chunk_pos,
                               const int64_t* d_chunk_n, int64_t n_chunks, const int64_t* d_cl_c0, const int64_t* d_cl_nc, int64_t n_clusters,
                               double* d_scores, double* d_partials, double* d_stage, double* d_rec) {
    if (n_feat < 1 || n_feat > kMaxFeatSmall) return fail(PDS_ERR_UNSUPPORTED, "fixed-effects regression: up to 16 feature columns");
    if (n_chunks < 1 || n_clusters < 1) return fail(PDS_ERR_INVALID, "fixed-effects regression: no cluster holds a row");
    {
        KernelTimer timer(ctx, kKindRolling);
        dispatch_width<1, kMaxFeatSmall>(n_feat, [&](auto pc) {
            constexpr int P = decltype(pc)::value;
            hipLaunchKernelGGL((cluster_gather_chunk_kernel<P>), dim3(cl_waves(ctx, n_chunks)), dim3(64), 0, ctx->stream, d_rows, d_idx, d_chunk_pos,
                               d_chunk_n, n_chunks, d_scores);
        });
        PDS_HIP_CHECK(hipGetLastError());
    }
    KernelTimer timer(ctx, kKindSolve);
    const int nbl = cluster_meat_records(ctx, n_clusters);
    hipLaunchKernelGGL(score_long_meat_kernel<false>, dim3(nbl), dim3(64), 0, ctx->stream, d_cl_c0, d_cl_nc, n_clusters, (const double*)d_scores,
                       d_partials);
    PDS_HIP_CHECK(hipGetLastError());
    return launch_sum_records(ctx, d_partials, nbl, d_stage, d_rec, /*compensated=*/true);
}

template int launch_within_row_scores<double>(pds_ctx*, const double* const*, int, const int64_t*, int64_t, int64_t, const MixedChunks&,
                                              const double*, const double*, double*);
template int launch_within_row_scores<float>(pds_ctx*, const float* const*, int, const int64_t*, int64_t, int64_t, const MixedChunks&,
                                             const double*, const double*, double*);

}  // namespace pds
