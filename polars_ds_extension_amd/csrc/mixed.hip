// mixed.hip -- the device side of the random-intercept mixed model (REML, capi_mixed.hpp): everything the profiled deviance needs
// from the frame, in a fixed number of passes over it, and the per-gamma reduction over the groups.
//
// With z_i = [x_i, y_i], m_g the mean of z over group g and n_g its row count,
//     [X y]' H^-1 [X y] = W + sum_g c_g(gamma) [1, m_g] [1, m_g]',   c_g = n_g / (1 + gamma n_g),   H = I + gamma Z Z',
// where W = sum_g sum_{i in g} (z_i - m_g)(z_i - m_g)' is the within-group scatter (its intercept row and column are exactly zero
// and never formed).  Every term is positive semi-definite: nothing cancels, whatever the size of the group means.
//
//   * mixed_stats_kernel: ONE wave walks groups (grid stride).  A group of up to kMxCap = 128 rows is loaded once into a
//     wave-private LDS tile (feature-major, row stride kMxStride: the wave-tile idiom of wave_tile_dev.hpp), summed and centred
//     there; a longer group reads its rows twice (sums, then centred products through the first 64 row slots of the tile).  The
//     16 x 16 feature block of W comes from one v_mfma_f64_16x16x4 accumulator with operands (x - m, x - m), W_xy from a second
//     matrix instruction with B = [y - m_y | 0 ..], W_yy from a per-lane register folded by a fixed butterfly.  The wave keeps its
//     accumulators across all the groups it walks and writes ONE partial record at its end.  It also writes the group's means
//     (feature-major, G values per column) and ORs into a word the features that vary inside some group (an exact comparison
//     of every row with the group's first row; integer OR, so the order does not matter).  A column that does not vary inside a
//     group has that group's first value as its mean, exactly.
//   * groups above `split_rows` are cut by the host into row chunks that are separate work items: mixed_chunk_sums_kernel (a wave
//     per chunk), mixed_chunk_means_kernel (a group's chunk sums added in chunk order) and mixed_chunk_scatter_kernel (centred
//     products of a chunk with its group's mean; again one partial record per wave).
//   * sum_records_kernel adds partial records in index order (two stages, launch_sum_records); no floating-point atomics anywhere, so
//     two calls give the same bits.  It is the one record sum of the library: a plain running sum for this file's passes, a
//     compensated one (its template flag) for the passes of cluster_meat.hip and within_pass.hip.
//   * mixed_profile_kernel: for one gamma, 64 groups per step through the same LDS layout: sum_g c_g m m' (matrix instruction,
//     operands (c m, m)), sum_g c_g m m_y and sum_g c_g m (second instruction), and sum c, sum c m_y, sum c m_y^2,
//     sum ln(1 + gamma n_g) from per-lane registers; records summed by sum_records_kernel.  Empty groups contribute nothing.
//   * every frame kernel takes an optional coefficient vector beta0 (intercept first): the target column is then read as
//     y - [1, x] . beta0, formed per row in registers.  The host runs the passes twice (capi_mixed.hpp): on y itself, then on the
//     residual of a first GLS solution, so that r' H^-1 r comes out of sums of its own size instead of a difference of large ones.
// Arithmetic is f64 for f64 and f32 frames alike (an f32 frame is converted on load).
#include "score_meat_dev.hpp"  // (two_sum, for the compensated record sum; it includes wave_tile_dev.hpp)

#include <algorithm>

namespace pds {

namespace {

constexpr int kMxCap = 128;                           // resident rows of a group (two 64-row steps)
constexpr int kMxStride = wave_tile_stride(kMxCap);  // doubles per feature row of the tile
constexpr int kMxPStride = wave_tile_stride(64);     // the profile kernel's tile: 64 groups per step

// the target of a row: y, or y - [1, x] . beta0 (b0: intercept first; x: the row's features)
template <int P>
__device__ __forceinline__ double mx_target(double yv, const double* x, const double* b0, bool has_b0) {
    if (has_b0) {
        yv -= b0[0];
#pragma unroll
        for (int c = 0; c < P; ++c) yv = fma(-x[c], b0[1 + c], yv);
    }
    return yv;
}

template <int P>
__device__ __forceinline__ bool mx_load_beta0(const double* __restrict__ beta0, double* b0) {
#pragma unroll
    for (int c = 0; c <= P; ++c) b0[c] = beta0 ? beta0[c] : 0.0;
    return beta0 != nullptr;
}

// the centred rows of a step (features, then y - m_y at feature row P) -> W block and W_xy
template <int P>
__device__ __forceinline__ void mx_centred_gram(const double* xt, int rows, int lane, d4& acc, d4& acc2) {
    wave_tile_gram<P>(
        xt, kMxStride, rows, lane, TileNoScale{}, [&](int c, int row) { return c == 0 ? xt[P * kMxStride + row] : 0.0; },  // B column 0 = y - m_y
        acc, acc2);
}

// centred products of the rows [r0, r0 + n) with the means `mean` (features, then y), 64 rows per step through the first 64 row
// slots of the tile
template <typename T, int P>
__device__ __forceinline__ void mx_stream_centred(const gptr<T>* cx, gptr<T> cy, int64_t r0, int64_t n, const double* mean, const double* b0,
                                                  bool has_b0, double* xt, int lane, d4& acc, d4& acc2, double& yy) {
    for (int64_t base = 0; base < n; base += 64) {
        const int64_t r = base + lane;
        const bool live = r < n;
        PDS_WAVE_LDS_SYNC();  // (the previous step's operand reads are done)
        double x[P];
#pragma unroll
        for (int c = 0; c < P; ++c) {
            x[c] = live ? (double)cx[c][r0 + r] : 0.0;
            xt[c * kMxStride + lane] = live ? x[c] - mean[c] : 0.0;
        }
        const double yc = live ? mx_target<P>((double)cy[r0 + r], x, b0, has_b0) - mean[P] : 0.0;
        xt[P * kMxStride + lane] = yc;
        yy = fma(yc, yc, yy);
        PDS_WAVE_LDS_SYNC();
        mx_centred_gram<P>(xt, (int)std::min<int64_t>(64, n - base), lane, acc, acc2);
    }
}

// entry (i, c) of the 16 x 16 block and of the side block -> a record (a scatter partial or a profile record)
__device__ __forceinline__ void mx_put_w_xy(double* rec, int i, int c, double w, double side) {
    rec[kMixedRecW + i * 16 + c] = w;
    if (c == 0) rec[kMixedRecXY + i] = side;
}

__device__ __forceinline__ void mx_write_record(double* rec, int lane, const d4& acc, const d4& acc2, double yy) {
    wave_tile_for_d(lane, [&](int i, int c, double w, double side) { mx_put_w_xy(rec, i, c, w, side); }, acc, acc2);
    yy = wave_sum(yy);
    if (lane == 0) rec[kMixedRecYY] = yy;
    // the slots only the profile records use: the record sum reads all of them
    if (lane < 16) rec[kMixedRecCM + lane] = 0.0;
    if (lane > 0 && lane < kMixedRecStride - kMixedRecYY) rec[kMixedRecYY + lane] = 0.0;
}

template <typename T, int P>
__global__ __launch_bounds__(64) void mixed_stats_kernel(const T* const* __restrict__ cols, const int64_t* __restrict__ off, int64_t n_groups,
                                                         int64_t split_rows, const double* __restrict__ beta0, double* __restrict__ means,
                                                         unsigned* __restrict__ flags, double* __restrict__ partials) {
    __shared__ double xt[(P + 1) * kMxStride];  // features 0 .. P - 1, then y: [c * kMxStride + row]
    const int lane = threadIdx.x;
    double b0[P + 1];
    const bool has_b0 = mx_load_beta0<P>(beta0, b0);
    gptr<T> cx[P];
#pragma unroll
    for (int c = 0; c < P; ++c) cx[c] = as_global(cols[c]);
    const gptr<T> cy = as_global(cols[P]);
    d4 acc = {0.0, 0.0, 0.0, 0.0}, acc2 = {0.0, 0.0, 0.0, 0.0};
    double yy = 0.0;
    unsigned vary_all = 0;
    for (int64_t g = blockIdx.x; g < n_groups; g += gridDim.x) {
        const int64_t r0 = off[g], n = off[g + 1] - r0;  // (the host has validated the offsets)
        if (n > split_rows) continue;                    // cut into chunks: the chunk kernels
        if (n <= 0) {
            if (lane <= P) means[(int64_t)lane * n_groups + g] = 0.0;
            continue;
        }
        const bool resident = n <= kMxCap;
        PDS_WAVE_LDS_SYNC();  // (the previous group's operand reads are done)
        double s[P + 1], first[P + 1], mean[P + 1];
        unsigned vary = 0;
#pragma unroll
        for (int c = 0; c <= P; ++c) s[c] = 0.0;
        for (int64_t base = 0; base < n; base += 64) {
            const int64_t r = base + lane;
            const bool live = r < n;
            double x[P];
#pragma unroll
            for (int c = 0; c < P; ++c) x[c] = live ? (double)cx[c][r0 + r] : 0.0;
            const double yv = live ? mx_target<P>((double)cy[r0 + r], x, b0, has_b0) : 0.0;
#pragma unroll
            for (int c = 0; c <= P; ++c) {
                const double v = c < P ? x[c] : yv;
                if (base == 0) first[c] = __shfl(v, 0, 64);
                s[c] += v;
                if (__any(live && v != first[c])) vary |= 1u << c;
                if (resident) xt[c * kMxStride + r] = v;
            }
        }
#pragma unroll
        for (int c = 0; c <= P; ++c) {
            const double sum = wave_sum(s[c]);
            mean[c] = ((vary >> c) & 1u) ? sum / (double)n : first[c];
            if (lane == c) means[(int64_t)c * n_groups + g] = mean[c];
        }
        vary_all |= vary;
        if (resident) {
            for (int64_t base = 0; base < n; base += 64) {  // (a lane centres the slots it wrote)
                const int64_t r = base + lane;
                const bool live = r < n;
#pragma unroll
                for (int c = 0; c < P; ++c) xt[c * kMxStride + r] = live ? xt[c * kMxStride + r] - mean[c] : 0.0;
                const double yc = live ? xt[P * kMxStride + r] - mean[P] : 0.0;
                xt[P * kMxStride + r] = yc;
                yy = fma(yc, yc, yy);
            }
            PDS_WAVE_LDS_SYNC();
            mx_centred_gram<P>(xt, (int)n, lane, acc, acc2);  // (the rows n .. up to the next multiple of 4 hold zeros)
        } else {
            mx_stream_centred<T, P>(cx, cy, r0, n, mean, b0, has_b0, xt, lane, acc, acc2, yy);
        }
    }
    if (lane == 0 && (vary_all & ((1u << P) - 1u))) atomicOr(flags, vary_all & ((1u << P) - 1u));
    mx_write_record(partials + (int64_t)blockIdx.x * kMixedRecStride, lane, acc, acc2, yy);
}

// column sums of one chunk, and which columns differ from the first row of the chunk's GROUP
template <typename T, int P>
__global__ __launch_bounds__(64) void mixed_chunk_sums_kernel(const T* const* __restrict__ cols, const int64_t* __restrict__ chunk_r0,
                                                              const int64_t* __restrict__ chunk_n, const int64_t* __restrict__ chunk_first,
                                                              int64_t n_chunks, const double* __restrict__ beta0, double* __restrict__ sums,
                                                              unsigned* __restrict__ varies) {
    const int lane = threadIdx.x;
    gptr<T> cx[P + 1];
#pragma unroll
    for (int c = 0; c <= P; ++c) cx[c] = as_global(cols[c]);
    double b0[P + 1];
    const bool has_b0 = mx_load_beta0<P>(beta0, b0);
    for (int64_t k = blockIdx.x; k < n_chunks; k += gridDim.x) {
        const int64_t r0 = chunk_r0[k], n = chunk_n[k], rf = chunk_first[k];
        double s[P + 1], first[P + 1];
        unsigned vary = 0;
#pragma unroll
        for (int c = 0; c <= P; ++c) {
            s[c] = 0.0;
            first[c] = (double)cx[c][rf];
        }
        first[P] = mx_target<P>(first[P], first, b0, has_b0);
        for (int64_t base = 0; base < n; base += 64) {
            const int64_t r = base + lane;
            const bool live = r < n;
            double x[P];
#pragma unroll
            for (int c = 0; c < P; ++c) x[c] = live ? (double)cx[c][r0 + r] : 0.0;
            const double yv = live ? mx_target<P>((double)cx[P][r0 + r], x, b0, has_b0) : 0.0;
#pragma unroll
            for (int c = 0; c <= P; ++c) {
                const double v = c < P ? x[c] : yv;
                s[c] += v;
                if (__any(live && v != first[c])) vary |= 1u << c;
            }
        }
#pragma unroll
        for (int c = 0; c <= P; ++c) {
            const double sum = wave_sum(s[c]);
            if (lane == c) sums[k * (P + 1) + c] = sum;
        }
        if (lane == 0) varies[k] = vary;
    }
}

// a long group's chunk sums in chunk order -> its means; lane c = column c
template <typename T>
__global__ __launch_bounds__(64) void mixed_chunk_means_kernel(const T* const* __restrict__ cols, int p, const int64_t* __restrict__ long_g,
                                                               const int64_t* __restrict__ long_c0, const int64_t* __restrict__ long_nc,
                                                               const int64_t* __restrict__ long_first, const int64_t* __restrict__ long_n,
                                                               const double* __restrict__ sums, const unsigned* __restrict__ varies,
                                                               const double* __restrict__ beta0, int64_t n_groups,
                                                               double* __restrict__ means, unsigned* __restrict__ flags) {
    const int lane = threadIdx.x;
    const int64_t j = blockIdx.x;
    const int64_t c0 = long_c0[j], nc = long_nc[j];
    unsigned vary = 0;
    double sum = 0.0;
    for (int64_t k = 0; k < nc; ++k) {
        vary |= varies[c0 + k];
        if (lane <= p) sum += sums[(c0 + k) * (p + 1) + lane];
    }
    if (lane <= p) {
        double first = (double)as_global(cols[lane])[long_first[j]];
        if (lane == p && beta0) {  // (the order of mx_target)
            first -= beta0[0];
            for (int c = 0; c < p; ++c) first = fma(-(double)as_global(cols[c])[long_first[j]], beta0[1 + c], first);
        }
        means[(int64_t)lane * n_groups + long_g[j]] = ((vary >> lane) & 1u) ? sum / (double)long_n[j] : first;
    }
    vary &= (1u << p) - 1u;
    if (lane == 0 && vary) atomicOr(flags, vary);
}

// centred products of the chunks with their groups' means: the wave keeps its accumulators across the chunks it walks
template <typename T, int P>
__global__ __launch_bounds__(64) void mixed_chunk_scatter_kernel(const T* const* __restrict__ cols, const int64_t* __restrict__ chunk_r0,
                                                                 const int64_t* __restrict__ chunk_n, const int64_t* __restrict__ chunk_g,
                                                                 int64_t n_chunks, int64_t n_groups, const double* __restrict__ beta0,
                                                                 const double* __restrict__ means, double* __restrict__ partials) {
    __shared__ double xt[(P + 1) * kMxStride];
    const int lane = threadIdx.x;
    double b0[P + 1];
    const bool has_b0 = mx_load_beta0<P>(beta0, b0);
    gptr<T> cx[P];
#pragma unroll
    for (int c = 0; c < P; ++c) cx[c] = as_global(cols[c]);
    const gptr<T> cy = as_global(cols[P]);
    d4 acc = {0.0, 0.0, 0.0, 0.0}, acc2 = {0.0, 0.0, 0.0, 0.0};
    double yy = 0.0;
    for (int64_t k = blockIdx.x; k < n_chunks; k += gridDim.x) {
        const int64_t g = chunk_g[k];
        double mean[P + 1];
#pragma unroll
        for (int c = 0; c <= P; ++c) mean[c] = means[(int64_t)c * n_groups + g];
        mx_stream_centred<T, P>(cx, cy, chunk_r0[k], chunk_n[k], mean, b0, has_b0, xt, lane, acc, acc2, yy);
    }
    mx_write_record(partials + (int64_t)blockIdx.x * kMixedRecStride, lane, acc, acc2, yy);
}

// block b: out[b] = in[b per] + in[b per + 1] + ... in index order, entry by entry.  COMPENSATED: the running sum's rounding errors
// are collected beside it (two_sum) and added at the end; without it a plain running sum.  The two give different bits: each caller
// keeps the one its results were defined with.
template <bool COMPENSATED>
__global__ __launch_bounds__(320) void sum_records_kernel(const double* __restrict__ in, int n_rec, int per, double* __restrict__ out) {
    const int e = threadIdx.x;
    if (e >= kMixedRecStride) return;
    const int r0 = blockIdx.x * per, r1 = std::min(n_rec, r0 + per);
    double s = 0.0, c = 0.0;
    for (int r = r0; r < r1; ++r) {
        const double v = in[(int64_t)r * kMixedRecStride + e];
        if constexpr (COMPENSATED) two_sum(s, c, v);
        else s += v;
    }
    out[(int64_t)blockIdx.x * kMixedRecStride + e] = COMPENSATED ? s + c : s;
}

template <int P>
__global__ __launch_bounds__(64) void mixed_profile_kernel(const double* __restrict__ means, const int64_t* __restrict__ off, int64_t n_groups,
                                                           double gamma, double* __restrict__ partials) {
    __shared__ double mt[(P + 1) * kMxPStride + 64];
    double* ct = mt + (P + 1) * kMxPStride;  // c_g of the step's groups
    const int lane = threadIdx.x;
    d4 acc = {0.0, 0.0, 0.0, 0.0}, acc2 = {0.0, 0.0, 0.0, 0.0};
    double sc = 0.0, scy = 0.0, scyy = 0.0, sld = 0.0;
    const int64_t n_tiles = (n_groups + 63) / 64;
    for (int64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const int64_t g = t * 64 + lane;
        const int64_t ng = g < n_groups ? off[g + 1] - off[g] : 0;
        const bool live = ng > 0;  // (an empty group contributes nothing)
        const double nd = (double)ng;
        const double cg = live ? nd / (1.0 + gamma * nd) : 0.0;
        PDS_WAVE_LDS_SYNC();  // (the previous step's operand reads are done)
        double my = 0.0;
#pragma unroll
        for (int c = 0; c <= P; ++c) {
            const double mv = live ? means[(int64_t)c * n_groups + g] : 0.0;
            mt[c * kMxPStride + lane] = mv;
            if (c == P) my = mv;
        }
        ct[lane] = cg;
        sc += cg;
        scy = fma(cg, my, scy);
        scyy = fma(cg * my, my, scyy);
        PDS_WAVE_LDS_SYNC();
        wave_tile_gram<P>(
            mt, kMxPStride, (int)std::min<int64_t>(64, n_groups - t * 64), lane, [&](int row) { return ct[row]; },
            [&](int c, int row, double cv) { return c == 0 ? cv * mt[P * kMxPStride + row] : (c == 1 ? cv : 0.0); },  // B columns: 0 = c m_y, 1 = c
            acc, acc2);
        if (live) sld += log(1.0 + gamma * nd);  // (behind the matrix loop: in front of it the compiler keeps an accumulator in 8 more VGPRs)
    }
    double* rec = partials + (int64_t)blockIdx.x * kMixedRecStride;
    wave_tile_for_d(
        lane,
        [&](int i, int c, double w, double side) {
            mx_put_w_xy(rec, i, c, w, side);
            if (c == 1) rec[kMixedRecCM + i] = side;
        },
        acc, acc2);
    sc = wave_sum(sc);
    scy = wave_sum(scy);
    scyy = wave_sum(scyy);
    sld = wave_sum(sld);
    if (lane == 0) {
        rec[kMixedRecYY] = scyy;
        rec[kMixedRecC] = sc;
        rec[kMixedRecCY] = scy;
        rec[kMixedRecLD] = sld;
    }
    if (lane > kMixedRecLD - kMixedRecYY && lane < kMixedRecStride - kMixedRecYY) rec[kMixedRecYY + lane] = 0.0;  // (padding)
}

}  // namespace

// records [0, n_rec) of `d_rec` -> one record at d_out, in index order: blocks of `per` records, then the block sums
int launch_sum_records(pds_ctx* ctx, const double* d_rec, int n_rec, double* d_stage, double* d_out, bool compensated) {
    const int per = 64;
    const int nb = (n_rec + per - 1) / per;
    const auto kernel = compensated ? sum_records_kernel<true> : sum_records_kernel<false>;
    if (nb > 1) {
        hipLaunchKernelGGL(kernel, dim3(nb), dim3(320), 0, ctx->stream, d_rec, n_rec, per, d_stage);
        hipLaunchKernelGGL(kernel, dim3(1), dim3(320), 0, ctx->stream, (const double*)d_stage, nb, nb, d_out);
    } else {
        hipLaunchKernelGGL(kernel, dim3(1), dim3(320), 0, ctx->stream, d_rec, n_rec, n_rec, d_out);
    }
    PDS_HIP_CHECK(hipGetLastError());
    return PDS_OK;
}

int mixed_stats_blocks(const pds_ctx* ctx, int64_t n_work) { return (int)std::max<int64_t>(1, std::min<int64_t>(n_work, (int64_t)ctx->num_cus * 8)); }
int mixed_profile_blocks(const pds_ctx* ctx, int64_t n_groups) {
    return (int)std::max<int64_t>(1, std::min<int64_t>((n_groups + 63) / 64, (int64_t)ctx->num_cus * 4));
}

template <typename T>
int launch_mixed_stats(pds_ctx* ctx, const T* const* d_cols, int n_feat, const int64_t* d_off, int64_t n_groups, int64_t split_rows,
                       const MixedChunks& ch, const double* d_beta0, double* d_means, unsigned* d_flags, double* d_partials,
                       double* d_stage, double* d_w) {
    if (n_feat < 1 || n_feat > kMaxFeatSmall) return fail(PDS_ERR_UNSUPPORTED, "mixed model: up to 16 feature columns");
    KernelTimer timer(ctx, kKindGroupedMoments);
    PDS_HIP_CHECK(hipMemsetAsync(d_flags, 0, sizeof(unsigned), ctx->stream));
    const int nb = mixed_stats_blocks(ctx, n_groups);
    const int nbc = ch.n_chunks > 0 ? mixed_stats_blocks(ctx, ch.n_chunks) : 0;
    dispatch_width<1, kMaxFeatSmall>(n_feat, [&](auto pc) {
        constexpr int P = decltype(pc)::value;
        hipLaunchKernelGGL((mixed_stats_kernel<T, P>), dim3(nb), dim3(64), 0, ctx->stream, d_cols, d_off, n_groups, split_rows, d_beta0,
                           d_means, d_flags, d_partials);
        if (nbc > 0) {
            hipLaunchKernelGGL((mixed_chunk_sums_kernel<T, P>), dim3(nbc), dim3(64), 0, ctx->stream, d_cols, ch.d_chunk_r0, ch.d_chunk_n,
                               ch.d_chunk_first, ch.n_chunks, d_beta0, ch.d_sums, ch.d_varies);
            hipLaunchKernelGGL((mixed_chunk_means_kernel<T>), dim3((unsigned)ch.n_long), dim3(64), 0, ctx->stream, d_cols, P, ch.d_long_g,
                               ch.d_long_c0, ch.d_long_nc, ch.d_long_first, ch.d_long_n, (const double*)ch.d_sums,
                               (const unsigned*)ch.d_varies, d_beta0, n_groups, d_means, d_flags);
            hipLaunchKernelGGL((mixed_chunk_scatter_kernel<T, P>), dim3(nbc), dim3(64), 0, ctx->stream, d_cols, ch.d_chunk_r0, ch.d_chunk_n,
                               ch.d_chunk_g, ch.n_chunks, n_groups, d_beta0, (const double*)d_means,
                               d_partials + (int64_t)nb * kMixedRecStride);
        }
    });
    PDS_HIP_CHECK(hipGetLastError());
    return launch_sum_records(ctx, d_partials, nb + nbc, d_stage, d_w, /*compensated=*/false);
}

int launch_mixed_profile(pds_ctx* ctx, const double* d_means, int n_feat, const int64_t* d_off, int64_t n_groups, double gamma,
                         double* d_partials, double* d_stage, double* d_out) {
    if (n_feat < 1 || n_feat > kMaxFeatSmall) return fail(PDS_ERR_UNSUPPORTED, "mixed model: up to 16 feature columns");
    KernelTimer timer(ctx, kKindIter);
    const int nb = mixed_profile_blocks(ctx, n_groups);
    dispatch_width<1, kMaxFeatSmall>(n_feat, [&](auto pc) {
        hipLaunchKernelGGL((mixed_profile_kernel<decltype(pc)::value>), dim3(nb), dim3(64), 0, ctx->stream, d_means, d_off, n_groups, gamma,
                           d_partials);
    });
    PDS_HIP_CHECK(hipGetLastError());
    return launch_sum_records(ctx, d_partials, nb, d_stage, d_out, /*compensated=*/false);
}

template int launch_mixed_stats<double>(pds_ctx*, const double* const*, int, const int64_t*, int64_t, int64_t, const MixedChunks&, const double*,
                                        double*, unsigned*, double*, double*, double*);
template int launch_mixed_stats<float>(pds_ctx*, const float* const*, int, const int64_t*, int64_t, int64_t, const MixedChunks&, const double*,
                                       double*, unsigned*, double*, double*, double*);

}  // namespace pds
