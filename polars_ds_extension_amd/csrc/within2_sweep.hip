// within2_sweep.hip -- the device side of the fixed-effects regression with TWO absorbed factors (capi_within2.hpp): the projection
// of the p + 1 columns [x, y] off both sets of dummies by alternating sweeps.
//
// The sweeps never rewrite the frame.  The state is the two tables of accumulated level means a1 [G1 x (p + 1)] and
// a2 [codes of factor 2 x (p + 1)]; the working value of row r is
//     z_r = (w_r - a1[g1(r)]) - a2[code2(r)],          w_r the row's original values in f64,
// formed in registers wherever it is needed, always by this expression.  One sweep:
//     factor 1:  m1_g = mean of z over level g;  a1_g += m1_g      (z is thereby less its factor-1 level means)
//     factor 2:  m2_l = mean of z over level l;  a2_l += m2_l      (... and then less its factor-2 level means)
//     delta = max_j max_l |m2_l,j| / s_j
// which is the sweep of the definition (include/pds_lstsq.h) with the subtractions kept as tables: two reads of the frame per sweep
// and no write, and the rounding of one sweep is not carried into the next (every z is formed from the original value).
//
//   * w2_init_kernel<T, P>: the frame (column-major, T) -> w0, a row-major f64 copy ((p + 1) doubles per row: a gathered row is 2 - 3
//     cache lines), and per wave the shifted moments sum (x - x_0), sum (x - x_0)^2 of every column (s_j and sum (y - ybar)^2).
//   * factor 1, rows contiguous: w2_level1_kernel<T, P> -- ONE wave per level (grid stride), rows 64 per step, the step's loads
//     (p + 1 columns, the row's code of factor 2) issued back to back on a clamped row index, the level's p + 1 sums by a butterfly.
//     Levels above `split_rows` are the chunks of plan_group_chunks: w2_chunk1_kernel (a wave per chunk, sums to memory) and
//     w2_long1_kernel (a level's chunk sums added in chunk order, lane = column).
//   * factor 2, rows gathered: idx2 lists the rows in ascending code order (launch_within2_order: a stable radix sort, once per call);
//     every level is cut into chunks of idx2 from the start.  w2_chunk2_kernel<P>: a wave per chunk, lane = row: idx2 -> the row of
//     w0 and the row of a1 (its level of factor 1 from the row map g1).  w2_level2_kernel: a wave per level, lane = column, the
//     chunk sums in chunk order, a2 += mean, and the level's |mean| / s_j into the wave's running maximum; one value per wave goes to
//     d_delta, the host takes the maximum of those.
//   * the accelerated iteration ("within2_accel" = 1; capi_within2.hpp has the scheme): w2_level2_accel_kernel<SECOND> is w2_level2_kernel
//     that also keeps the sweep's means (Delta1 / Delta2) and, on the second sweep of a cycle, one record of sum Delta2 d and sum d d per
//     wave; w2_accel_coef_kernel (one wave) adds the records in index order into c_j; w2_accel_apply_kernel: a2 -= c_j Delta2.
//   * w2_final_kernel<T, P>: z, column-major f64, for the final stage (the statistics pass and the within pass of the one-factor fit).
//   * w2_rows_out_kernel<T>: resid = e and pred = y - e, y the ORIGINAL target, in the caller's row order and type.
// No floating-point atomics, every sum in a fixed order: two calls give the same bits.  Every loop is bounded by a count known at
// launch; no workgroup waits for another.
#include "common.hpp"

#include <algorithm>

#include <hipcub/hipcub.hpp>

namespace pds {

namespace {

constexpr int kW2WavesPerCu = 16;  // one wave per block; the kernels hold the row in registers (about 100 VGPRs at P = 16)

__device__ __forceinline__ double w2_wave_sum(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// the larger of two non-negative values; a NaN, once in, stays
__device__ __forceinline__ double w2_max_nan(double a, double b) { return (b > a || b != b) ? b : a; }

template <typename T, int P>
__global__ __launch_bounds__(64) void w2_init_kernel(const T* const* __restrict__ cols, int64_t n, double* __restrict__ w0,
                                                     double* __restrict__ partials) {
    constexpr int NC = P + 1;
    const int lane = threadIdx.x;
    gptr<T> cx[NC];
    double x0[NC], s[NC], q[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        cx[c] = as_global(cols[c]);
        x0[c] = (double)cx[c][0];
        s[c] = q[c] = 0.0;
    }
    for (int64_t r = (int64_t)blockIdx.x * 64 + lane; r < n; r += (int64_t)gridDim.x * 64) {
        T raw[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) raw[c] = cx[c][r];
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const double v = (double)raw[c];
            w0[r * NC + c] = v;
            const double d = v - x0[c];
            s[c] += d;
            q[c] = fma(d, d, q[c]);
        }
    }
    double* out = partials + (int64_t)blockIdx.x * (2 * NC);
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const double ts = w2_wave_sum(s[c]), tq = w2_wave_sum(q[c]);
        if (lane == 0) {
            out[c] = ts;
            out[NC + c] = tq;
        }
    }
}

// records of `len` doubles, added in index order: lane = entry
__global__ __launch_bounds__(64) void w2_sum_records_kernel(const double* __restrict__ rec, int n_rec, int len, double* __restrict__ out) {
    const int e = threadIdx.x;
    if (e >= len) return;
    double s = 0.0;
    for (int i = 0; i < n_rec; ++i) s += rec[(int64_t)i * len + e];
    out[e] = s;
}

// the level of factor 1 of every row: the last level whose first row is <= r (the offsets are those of non-empty levels)
__global__ __launch_bounds__(256) void w2_row_level_kernel(const int64_t* __restrict__ off, int64_t n_levels, int64_t n, uint32_t* __restrict__ g1) {
    for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < n; r += (int64_t)gridDim.x * 256) {
        int64_t lo = 0, hi = n_levels;
        for (int it = 0; it < 64 && hi - lo > 1; ++it) {
            const int64_t mid = lo + ((hi - lo) >> 1);
            if (off[mid] <= r) lo = mid;
            else hi = mid;
        }
        g1[r] = (uint32_t)lo;
    }
}

__global__ __launch_bounds__(256) void w2_iota_kernel(uint32_t* __restrict__ v, int64_t n) {
    for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < n; r += (int64_t)gridDim.x * 256) v[r] = (uint32_t)r;
}

__global__ __launch_bounds__(256) void w2_gather_codes_kernel(const int32_t* __restrict__ in, const uint32_t* __restrict__ perm, int64_t n,
                                                              int32_t* __restrict__ out) {
    for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < n; r += (int64_t)gridDim.x * 256) out[r] = in[perm[r]];
}

// rows [r0, r0 + n) of the frame, 64 per step: acc[c] += z of the live rows, z = (x - a1g) - a2[code2]
template <typename T, int P>
__device__ __forceinline__ void w2_rows1(const gptr<T>* cx, gptr<int32_t> code2, const double* __restrict__ a2, int64_t r0, int64_t n,
                                         const double* a1g, int lane, double* acc) {
    constexpr int NC = P + 1;
    for (int64_t base = 0; base < n; base += 64) {
        const int64_t r = base + lane;
        const bool live = r < n;
        const int64_t ri = r0 + (live ? r : 0);  // (n >= 1: the first row is always there)
        T raw[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) raw[c] = cx[c][ri];
        const double* a2l = a2 + (int64_t)code2[ri] * NC;
        double t[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) t[c] = a2l[c];
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const double z = ((double)raw[c] - a1g[c]) - t[c];
            acc[c] += live ? z : 0.0;
        }
    }
}

template <typename T, int P>
__global__ __launch_bounds__(64) void w2_level1_kernel(const T* const* __restrict__ cols, const int32_t* __restrict__ code2,
                                                       const int64_t* __restrict__ off, int64_t n_levels, int64_t split_rows,
                                                       double* a1, const double* __restrict__ a2) {
    constexpr int NC = P + 1;
    const int lane = threadIdx.x;
    gptr<T> cx[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) cx[c] = as_global(cols[c]);
    const gptr<int32_t> cd = as_global(code2);
    for (int64_t g = blockIdx.x; g < n_levels; g += gridDim.x) {
        const int64_t r0 = off[g], n = off[g + 1] - r0;
        if (n <= 0 || n > split_rows) continue;  // cut into chunks: the chunk kernels
        double a1g[NC], acc[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            a1g[c] = a1[g * NC + c];
            acc[c] = 0.0;
        }
        w2_rows1<T, P>(cx, cd, a2, r0, n, a1g, lane, acc);
        const double nd = (double)n;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const double tot = w2_wave_sum(acc[c]);
            if (lane == c) a1[g * NC + c] = a1g[c] + tot / nd;
        }
    }
}

template <typename T, int P>
__global__ __launch_bounds__(64) void w2_chunk1_kernel(const T* const* __restrict__ cols, const int32_t* __restrict__ code2,
                                                       const int64_t* __restrict__ chunk_r0, const int64_t* __restrict__ chunk_n,
                                                       const int64_t* __restrict__ chunk_g, int64_t n_chunks, const double* __restrict__ a1,
                                                       const double* __restrict__ a2, double* __restrict__ sums) {
    constexpr int NC = P + 1;
    const int lane = threadIdx.x;
    gptr<T> cx[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) cx[c] = as_global(cols[c]);
    const gptr<int32_t> cd = as_global(code2);
    for (int64_t k = blockIdx.x; k < n_chunks; k += gridDim.x) {
        const int64_t g = chunk_g[k];
        double a1g[NC], acc[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            a1g[c] = a1[g * NC + c];
            acc[c] = 0.0;
        }
        w2_rows1<T, P>(cx, cd, a2, chunk_r0[k], chunk_n[k], a1g, lane, acc);
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const double tot = w2_wave_sum(acc[c]);
            if (lane == c) sums[k * NC + c] = tot;
        }
    }
}

// a wave per long level of factor 1: its chunk sums in chunk order, lane = column
__global__ __launch_bounds__(64) void w2_long1_kernel(const int64_t* __restrict__ long_g, const int64_t* __restrict__ long_c0,
                                                      const int64_t* __restrict__ long_nc, const int64_t* __restrict__ long_n, int64_t n_long,
                                                      int nc, const double* __restrict__ sums, double* __restrict__ a1) {
    const int lane = threadIdx.x;
    if (lane >= nc) return;
    for (int64_t v = blockIdx.x; v < n_long; v += gridDim.x) {
        const int64_t c0 = long_c0[v], k = long_nc[v];
        double s = 0.0;
        for (int64_t i = 0; i < k; ++i) s += sums[(c0 + i) * nc + lane];
        a1[long_g[v] * nc + lane] += s / (double)long_n[v];
    }
}

// a wave per chunk of idx2 (rows of ONE level of factor 2, ascending): lane = row
template <int P>
__global__ __launch_bounds__(64) void w2_chunk2_kernel(const double* __restrict__ w0, const uint32_t* __restrict__ idx2,
                                                       const uint32_t* __restrict__ g1, const double* __restrict__ a1, const double* __restrict__ a2,
                                                       const int64_t* __restrict__ chunk_pos, const int64_t* __restrict__ chunk_n,
                                                       const int32_t* __restrict__ chunk_code, int64_t n_chunks, double* __restrict__ sums) {
    constexpr int NC = P + 1;
    const int lane = threadIdx.x;
    const gptr<double> w = as_global(w0), t1 = as_global(a1);
    for (int64_t k = blockIdx.x; k < n_chunks; k += gridDim.x) {
        const int64_t pos = chunk_pos[k], n = chunk_n[k];
        const double* a2l = a2 + (int64_t)chunk_code[k] * NC;
        double t[NC], acc[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            t[c] = a2l[c];
            acc[c] = 0.0;
        }
        for (int64_t base = 0; base < n; base += 64) {
            const int64_t i = base + lane;
            const bool live = i < n;
            const int64_t r = (int64_t)idx2[pos + (live ? i : 0)];
            const int64_t g = (int64_t)g1[r];
            double x[NC], b[NC];
#pragma unroll
            for (int c = 0; c < NC; ++c) x[c] = w[r * NC + c];
#pragma unroll
            for (int c = 0; c < NC; ++c) b[c] = t1[g * NC + c];
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                const double z = (x[c] - b[c]) - t[c];
                acc[c] += live ? z : 0.0;
            }
        }
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const double tot = w2_wave_sum(acc[c]);
            if (lane == c) sums[k * NC + c] = tot;
        }
    }
}

// a wave per occupied level of factor 2: its chunk sums in chunk order, lane = column; a2 += mean; |mean| / s_j into the wave's maximum
__global__ __launch_bounds__(64) void w2_level2_kernel(const double* __restrict__ sums, const int64_t* __restrict__ lev_c0,
                                                       const int64_t* __restrict__ lev_nc, const int64_t* __restrict__ lev_n,
                                                       const int32_t* __restrict__ lev_code, int64_t n_levels, int nc, double* __restrict__ a2,
                                                       const double* __restrict__ scale, double* __restrict__ delta) {
    const int lane = threadIdx.x;
    double dmax = 0.0;
    if (lane < nc) {
        const double s_j = scale[lane];
        for (int64_t v = blockIdx.x; v < n_levels; v += gridDim.x) {
            const int64_t c0 = lev_c0[v], k = lev_nc[v];
            double s = 0.0;
            for (int64_t i = 0; i < k; ++i) s += sums[(c0 + i) * nc + lane];
            const double m = s / (double)lev_n[v];
            a2[(int64_t)lev_code[v] * nc + lane] += m;
            dmax = w2_max_nan(dmax, fabs(m) / s_j);
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) dmax = w2_max_nan(dmax, __shfl_xor(dmax, m, 64));
    if (lane == 0) delta[blockIdx.x] = dmax;
}

// w2_level2_kernel for the accelerated iteration (Irons-Tuck, "within2_accel" = 1: capi_within2.hpp has the scheme): the same walk, the
// same sums and the same update of a2; besides, the level's mean m goes to dm_out[code] (Delta1 on the first sweep of a cycle, Delta2
// on the second), and on the SECOND sweep the lane adds m d and d d, d = m - dm_prev[code], over the levels the wave walks, in ascending
// level order: one record [num (nc) | den (nc)] per wave.  The grid is within2_delta_blocks(n_levels): rec has that many records.
template <bool SECOND>
__global__ __launch_bounds__(64) void w2_level2_accel_kernel(const double* __restrict__ sums, const int64_t* __restrict__ lev_c0,
                                                             const int64_t* __restrict__ lev_nc, const int64_t* __restrict__ lev_n,
                                                             const int32_t* __restrict__ lev_code, int64_t n_levels, int nc, double* __restrict__ a2,
                                                             const double* __restrict__ scale, double* __restrict__ delta,
                                                             const double* __restrict__ dm_prev, double* __restrict__ dm_out, double* __restrict__ rec) {
    const int lane = threadIdx.x;
    double dmax = 0.0, num = 0.0, den = 0.0;
    if (lane < nc) {
        const double s_j = scale[lane];
        for (int64_t v = blockIdx.x; v < n_levels; v += gridDim.x) {
            const int64_t c0 = lev_c0[v], k = lev_nc[v];
            double s = 0.0;
            for (int64_t i = 0; i < k; ++i) s += sums[(c0 + i) * nc + lane];
            const double m = s / (double)lev_n[v];
            const int64_t at = (int64_t)lev_code[v] * nc + lane;
            a2[at] += m;
            dm_out[at] = m;
            if (SECOND) {
                const double d = m - dm_prev[at];
                num = fma(m, d, num);
                den = fma(d, d, den);
            }
            dmax = w2_max_nan(dmax, fabs(m) / s_j);
        }
        if (SECOND) {
            rec[(int64_t)blockIdx.x * (2 * nc) + lane] = num;
            rec[(int64_t)blockIdx.x * (2 * nc) + nc + lane] = den;
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) dmax = w2_max_nan(dmax, __shfl_xor(dmax, m, 64));
    if (lane == 0) delta[blockIdx.x] = dmax;
}

// one wave, lane = column: the records of a cycle added in index order, eight loads in flight; c_j = sum m d / sum d d, and 0 (the
// column is left alone) when the denominator is 0 or a sum, or the quotient, is not finite
__global__ __launch_bounds__(64) void w2_accel_coef_kernel(const double* __restrict__ rec, int n_rec, int nc, double* __restrict__ coef) {
    const int lane = threadIdx.x;
    if (lane >= nc) return;
    double num = 0.0, den = 0.0;
    for (int i0 = 0; i0 < n_rec; i0 += 8) {
        double a[8], b[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int i = i0 + u < n_rec ? i0 + u : n_rec - 1;
            a[u] = rec[(int64_t)i * (2 * nc) + lane];
            b[u] = rec[(int64_t)i * (2 * nc) + nc + lane];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const bool live = i0 + u < n_rec;
            num += live ? a[u] : 0.0;
            den += live ? b[u] : 0.0;
        }
    }
    const double c = num / den;
    coef[lane] = (den != 0.0 && isfinite(num) && isfinite(den) && isfinite(c)) ? c : 0.0;
}

// a2[code][j] -= c_j Delta2[code][j] over the occupied codes: tables only
__global__ __launch_bounds__(256) void w2_accel_apply_kernel(const int32_t* __restrict__ lev_code, int64_t n_levels, int nc,
                                                             const double* __restrict__ coef, const double* __restrict__ dm2, double* __restrict__ a2) {
    const int64_t total = n_levels * nc;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t v = i / nc;
        const int j = (int)(i - v * nc);
        const int64_t at = (int64_t)lev_code[v] * nc + j;
        a2[at] = fma(-coef[j], dm2[at], a2[at]);
    }
}

template <typename T, int P>
__global__ __launch_bounds__(256) void w2_final_kernel(const T* const* __restrict__ cols, const int32_t* __restrict__ code2,
                                                       const uint32_t* __restrict__ g1, const double* __restrict__ a1, const double* __restrict__ a2,
                                                       int64_t n, double* __restrict__ z) {
    constexpr int NC = P + 1;
    gptr<T> cx[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) cx[c] = as_global(cols[c]);
    for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < n; r += (int64_t)gridDim.x * 256) {
        const double* b = a1 + (int64_t)g1[r] * NC;
        const double* t = a2 + (int64_t)code2[r] * NC;
        T raw[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) raw[c] = cx[c][r];
#pragma unroll
        for (int c = 0; c < NC; ++c) z[(int64_t)c * n + r] = ((double)raw[c] - b[c]) - t[c];
    }
}

template <typename T>
__global__ __launch_bounds__(256) void w2_rows_out_kernel(const T* __restrict__ y, const double* __restrict__ e, const uint32_t* __restrict__ perm,
                                                          int64_t n, T* __restrict__ pred, T* __restrict__ resid) {
    for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < n; r += (int64_t)gridDim.x * 256) {
        const int64_t ro = perm ? (int64_t)perm[r] : r;
        const double ev = e[r];
        if (resid) resid[ro] = (T)ev;
        if (pred) pred[ro] = (T)((double)y[r] - ev);
    }
}

int w2_waves(const pds_ctx* ctx, int64_t n_work) { return (int)std::max<int64_t>(1, std::min<int64_t>(n_work, (int64_t)ctx->num_cus * kW2WavesPerCu)); }
int w2_row_blocks(const pds_ctx* ctx, int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, (int64_t)ctx->num_cus * 8)); }

}  // namespace

int within2_init_records(const pds_ctx* ctx, int64_t n_rows) { return w2_waves(ctx, (n_rows + 63) / 64); }
int within2_delta_blocks(const pds_ctx* ctx, int64_t n_levels2) { return w2_waves(ctx, n_levels2); }

template <typename T>
int launch_within2_init(pds_ctx* ctx, const T* const* d_cols, int n_feat, int64_t n_rows, double* d_w0, double* d_partials, double* d_moments) {
    if (n_feat < 1 || n_feat > kMaxFeatSmall) return fail(PDS_ERR_UNSUPPORTED, "fixed-effects regression: up to 16 feature columns");
    KernelTimer timer(ctx, kKindMoments);
    const int nb = within2_init_records(ctx, n_rows);
    dispatch_width<1, kMaxFeatSmall>(n_feat, [&](auto pc) {
        constexpr int P = decltype(pc)::value;
        hipLaunchKernelGGL((w2_init_kernel<T, P>), dim3(nb), dim3(64), 0, ctx->stream, d_cols, n_rows, d_w0, d_partials);
    });
    hipLaunchKernelGGL(w2_sum_records_kernel, dim3(1), dim3(64), 0, ctx->stream, (const double*)d_partials, nb, 2 * (n_feat + 1), d_moments);
    PDS_HIP_CHECK(hipGetLastError());
    return PDS_OK;
}

int launch_within2_row_levels(pds_ctx* ctx, const int64_t* d_off, int64_t n_levels, int64_t n_rows, uint32_t* d_g1) {
    hipLaunchKernelGGL(w2_row_level_kernel, dim3(w2_row_blocks(ctx, n_rows)), dim3(256), 0, ctx->stream, d_off, n_levels, n_rows, d_g1);
    PDS_HIP_CHECK(hipGetLastError());
    return PDS_OK;
}

int launch_within2_gather_codes(pds_ctx* ctx, const int32_t* d_in, const uint32_t* d_perm, int64_t n_rows, int32_t* d_out) {
    hipLaunchKernelGGL(w2_gather_codes_kernel, dim3(w2_row_blocks(ctx, n_rows)), dim3(256), 0, ctx->stream, d_in, d_perm, n_rows, d_out);
    PDS_HIP_CHECK(hipGetLastError());
    return PDS_OK;
}

size_t within2_order_temp_bytes(int64_t n_rows) {
    size_t b = 0;
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, b, (const uint32_t*)nullptr, (uint32_t*)nullptr, (const uint32_t*)nullptr, (uint32_t*)nullptr,
                                             (int)std::min<int64_t>(n_rows, INT32_MAX));
    return ((b + 255) & ~(size_t)255) + 256;
}

// d_idx2: the rows in ascending order of their code, rows of one code in ascending row order.  d_iota, d_sorted: n_rows values of scratch
int launch_within2_order(pds_ctx* ctx, const int32_t* d_code2, int64_t n_rows, int64_t n_codes, uint32_t* d_iota, uint32_t* d_sorted,
                         uint32_t* d_idx2, void* d_temp, size_t temp_bytes) {
    KernelTimer timer(ctx, kKindGroupedMoments);
    int bits = 1;
    for (; bits < 32 && ((int64_t)1 << bits) < n_codes; ++bits) {}
    hipLaunchKernelGGL(w2_iota_kernel, dim3(w2_row_blocks(ctx, n_rows)), dim3(256), 0, ctx->stream, d_iota, n_rows);
    PDS_HIP_CHECK(hipGetLastError());
    PDS_HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(d_temp, temp_bytes, reinterpret_cast<const uint32_t*>(d_code2), d_sorted, (const uint32_t*)d_iota,
                                                     d_idx2, (int)n_rows, 0, bits, ctx->stream));
    return PDS_OK;
}

template <typename T>
int launch_within2_sweep(pds_ctx* ctx, const T* const* d_cols, int n_feat, const Within2Dev& d, int accel_phase) {
    if (accel_phase < 0 || accel_phase > 2 || (accel_phase && !(d.d_dm1 && d.d_dm2 && d.d_arec)))
        return fail(PDS_ERR_INVALID, "fixed-effects regression: the accelerated sweep needs its tables");
    if (n_feat < 1 || n_feat > kMaxFeatSmall) return fail(PDS_ERR_UNSUPPORTED, "fixed-effects regression: up to 16 feature columns");
    const int nc = n_feat + 1;
    const int nb1 = w2_waves(ctx, d.n1), nbc = d.ch1.n_chunks > 0 ? w2_waves(ctx, d.ch1.n_chunks) : 0;
    const int nb2 = w2_waves(ctx, d.n_chunks2), nbl = within2_delta_blocks(ctx, d.n_lev2);
    dispatch_width<1, kMaxFeatSmall>(n_feat, [&](auto pc) {
        constexpr int P = decltype(pc)::value;
        {
            KernelTimer timer(ctx, kKindSweep1);
            hipLaunchKernelGGL((w2_level1_kernel<T, P>), dim3(nb1), dim3(64), 0, ctx->stream, d_cols, d.d_code2, d.d_off1, d.n1, d.split1, d.d_a1,
                               (const double*)d.d_a2);
            if (nbc > 0) {
                hipLaunchKernelGGL((w2_chunk1_kernel<T, P>), dim3(nbc), dim3(64), 0, ctx->stream, d_cols, d.d_code2, d.ch1.d_chunk_r0,
                                   d.ch1.d_chunk_n, d.ch1.d_chunk_g, d.ch1.n_chunks, (const double*)d.d_a1, (const double*)d.d_a2, d.ch1.d_sums);
                hipLaunchKernelGGL(w2_long1_kernel, dim3(w2_waves(ctx, d.ch1.n_long)), dim3(64), 0, ctx->stream, d.ch1.d_long_g, d.ch1.d_long_c0,
                                   d.ch1.d_long_nc, d.ch1.d_long_n, d.ch1.n_long, nc, (const double*)d.ch1.d_sums, d.d_a1);
            }
        }
        KernelTimer timer(ctx, kKindSweep2);
        hipLaunchKernelGGL((w2_chunk2_kernel<P>), dim3(nb2), dim3(64), 0, ctx->stream, (const double*)d.d_w0, d.d_idx2, d.d_g1, (const double*)d.d_a1,
                           (const double*)d.d_a2, d.d_c2_pos, d.d_c2_n, d.d_c2_code, d.n_chunks2, d.d_csum2);
        if (accel_phase == 0)
            hipLaunchKernelGGL(w2_level2_kernel, dim3(nbl), dim3(64), 0, ctx->stream, (const double*)d.d_csum2, d.d_l2_c0, d.d_l2_nc, d.d_l2_n,
                               d.d_l2_code, d.n_lev2, nc, d.d_a2, (const double*)d.d_scale, d.d_delta);
        else if (accel_phase == 1)
            hipLaunchKernelGGL(w2_level2_accel_kernel<false>, dim3(nbl), dim3(64), 0, ctx->stream, (const double*)d.d_csum2, d.d_l2_c0, d.d_l2_nc,
                               d.d_l2_n, d.d_l2_code, d.n_lev2, nc, d.d_a2, (const double*)d.d_scale, d.d_delta, (const double*)nullptr, d.d_dm1,
                               (double*)nullptr);
        else
            hipLaunchKernelGGL(w2_level2_accel_kernel<true>, dim3(nbl), dim3(64), 0, ctx->stream, (const double*)d.d_csum2, d.d_l2_c0, d.d_l2_nc,
                               d.d_l2_n, d.d_l2_code, d.n_lev2, nc, d.d_a2, (const double*)d.d_scale, d.d_delta, (const double*)d.d_dm1, d.d_dm2,
                               d.d_arec);
    });
    PDS_HIP_CHECK(hipGetLastError());
    return PDS_OK;
}

// after the second sweep of a cycle: c_j from the cycle's records (on the device: the host does not read them), then a2 -= c_j Delta2
int launch_within2_extrapolate(pds_ctx* ctx, int n_feat, const Within2Dev& d) {
    if (n_feat < 1 || n_feat > kMaxFeatSmall || !(d.d_dm2 && d.d_arec && d.d_coef)) return fail(PDS_ERR_INVALID, "fixed-effects regression: the accelerated sweep needs its tables");
    const int nc = n_feat + 1;
    KernelTimer timer(ctx, kKindSweep2);
    hipLaunchKernelGGL(w2_accel_coef_kernel, dim3(1), dim3(64), 0, ctx->stream, (const double*)d.d_arec, within2_delta_blocks(ctx, d.n_lev2), nc, d.d_coef);
    hipLaunchKernelGGL(w2_accel_apply_kernel, dim3(w2_row_blocks(ctx, d.n_lev2 * nc)), dim3(256), 0, ctx->stream, d.d_l2_code, d.n_lev2, nc,
                       (const double*)d.d_coef, (const double*)d.d_dm2, d.d_a2);
    PDS_HIP_CHECK(hipGetLastError());
    return PDS_OK;
}

template <typename T>
int launch_within2_final(pds_ctx* ctx, const T* const* d_cols, int n_feat, const Within2Dev& d, double* d_z) {
    if (n_feat < 1 || n_feat > kMaxFeatSmall) return fail(PDS_ERR_UNSUPPORTED, "fixed-effects regression: up to 16 feature columns");
    KernelTimer timer(ctx, kKindPass2);
    dispatch_width<1, kMaxFeatSmall>(n_feat, [&](auto pc) {
        constexpr int P = decltype(pc)::value;
        hipLaunchKernelGGL((w2_final_kernel<T, P>), dim3(w2_row_blocks(ctx, d.n_rows)), dim3(256), 0, ctx->stream, d_cols, d.d_code2, d.d_g1,
                           (const double*)d.d_a1, (const double*)d.d_a2, d.n_rows, d_z);
    });
    PDS_HIP_CHECK(hipGetLastError());
    return PDS_OK;
}

template <typename T>
int launch_within2_rows_out(pds_ctx* ctx, const T* d_y, const double* d_e, const uint32_t* d_perm, int64_t n_rows, T* d_pred, T* d_resid) {
    hipLaunchKernelGGL((w2_rows_out_kernel<T>), dim3(w2_row_blocks(ctx, n_rows)), dim3(256), 0, ctx->stream, d_y, d_e, d_perm, n_rows, d_pred, d_resid);
    PDS_HIP_CHECK(hipGetLastError());
    return PDS_OK;
}

template int launch_within2_init<double>(pds_ctx*, const double* const*, int, int64_t, double*, double*, double*);
template int launch_within2_init<float>(pds_ctx*, const float* const*, int, int64_t, double*, double*, double*);
template int launch_within2_sweep<double>(pds_ctx*, const double* const*, int, const Within2Dev&, int);
template int launch_within2_sweep<float>(pds_ctx*, const float* const*, int, const Within2Dev&, int);
template int launch_within2_final<double>(pds_ctx*, const double* const*, int, const Within2Dev&, double*);
template int launch_within2_final<float>(pds_ctx*, const float* const*, int, const Within2Dev&, double*);
template int launch_within2_rows_out<double>(pds_ctx*, const double*, const double*, const uint32_t*, int64_t, double*, double*);
template int launch_within2_rows_out<float>(pds_ctx*, const float*, const double*, const uint32_t*, int64_t, float*, float*);

}  // namespace pds
