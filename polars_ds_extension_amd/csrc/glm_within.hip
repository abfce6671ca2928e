// glm_within.hip -- the device side of the fixed-effects GLM (capi_glm_within.hpp): IRLS with one absorbed factor.  Every iteration is
// a WEIGHTED within regression of the working response on the features, with weights that change every iteration:
//     w_i = pw_i / (g'(mu_i)^2 V(mu_i)),   z_i = (eta_i - o_i) + g'(mu_i)(y_i - mu_i),   m_g = the w-weighted mean of [x, z] over group g,
//     W = sum_g sum_{i in g} w_i ([x_i, z_i] - m_g)([x_i, z_i] - m_g)',   beta solves W_xx beta = W_xz (host),   alpha_g = m_z,g - m_x,g . beta.
// The state between two iterations is beta (p doubles) and the group means m_g ((p + 1) x G doubles, feature-major): eta_i = alpha_g +
// x_i . beta + o_i is formed per row in registers, so nothing of the size of the frame is written by an iteration.
//
//   * gw_pre_kernel (once): ONE wave walks groups (grid stride): the counting rows (pw > 0), sum pw, sum pw y, whether a weight is
//     negative or not finite, whether some counting y differs from 0 / from 1 and which features differ from the group's first counting
//     row (exact comparisons, integer OR).  From those the drop flag of the group (no counting row; poisson: every counting y is 0;
//     binomial: every counting y is 0 or every one is 1) and, over the kept groups, the "varies inside some kept group" bits.
//   * gw_iter_kernel (per iteration): ONE wave walks groups (grid stride) and skips dropped ones with a wave-uniform branch.  The loads
//     of a 64-row step (P features, y, pw and o when present) are issued back to back on a clamped row index; mu, w, z are formed in
//     registers.  A group of up to kGwCap = 128 rows is resident in the wave-private LDS tile (feature-major: P features, z, w; the
//     wave-tile idiom of wave_tile_dev.hpp) and read once: weighted sums, means, centring in place, then wave_tile_gram with scale = w
//     and the side column w (z - m_z).  A longer group is read twice (sums, then centred products through the first 64 row slots).
//     The accumulators live across the wave's groups; the wave writes ONE record and each group's means.
//   * groups above `split_rows` are the host's chunks (MixedChunks): gw_chunk_sums_kernel (a wave per chunk), gw_chunk_means_kernel (a
//     group's chunk sums added in chunk order) and gw_chunk_scatter_kernel (centred products of a chunk with its group's means).
//   * gw_final_kernel / gw_final_chunk_kernel: at the returned beta and the last means: alpha through gmap, mu per row through the
//     permutation (NaN on the rows of dropped groups), the deviance and Pearson's chi2 as compensated per-lane sums, and with MEAT the
//     centred scores s_g = sum r_i (x_i - m_x,g) and their outer products through ScoreMeat<false> / score_long_meat_kernel<false>.
//   * records have the layout of common.hpp and are added in index order by launch_sum_records (compensated): no floating-point atomic
//     anywhere, two calls give the same bits; the host drops empty groups before any launch.
// Arithmetic is f64 for f64 and f32 frames alike (an f32 frame, its weights and offsets are converted on load).
#include "glm_dev.hpp"
#include "score_meat_dev.hpp"

#include <algorithm>

namespace pds {

namespace {

constexpr int kGwCap = 128;                          // resident rows of a group (two 64-row steps)
constexpr int kGwStride = wave_tile_stride(kGwCap);  // doubles per feature row of the iteration's tile
// the bits of a group's (or chunk's) pre-pass word: [0, 16) feature c differs from the first counting row; then
constexpr unsigned kGwBitNZ = 1u << 16, kGwBitN1 = 1u << 17, kGwBitBad = 1u << 18;  // a counting y != 0; != 1; a bad weight

// the frame's columns (x_0 .. x_{P-1}, y, weights (nullable), offset (nullable)) and the family
template <typename T, int P>
struct GwFrame {
    gptr<T> cx[P], cy, cpw, co;
    bool has_pw, has_o;
    int link, variance;

    __device__ __forceinline__ void open(const T* const* __restrict__ cols, int link_, int variance_) {
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

    // row ri: every load of the row issued back to back, then the conversions
    __device__ __forceinline__ void load(int64_t ri, double* x, double& y, double& pw, double& o) const {
        T raw[P + 1];
#pragma unroll
        for (int c = 0; c < P; ++c) raw[c] = cx[c][ri];
        raw[P] = cy[ri];
        const T rpw = has_pw ? cpw[ri] : T(1);
        const T ro = has_o ? co[ri] : T(0);
#pragma unroll
        for (int c = 0; c < P; ++c) x[c] = (double)raw[c];
        y = (double)raw[P];
        pw = (double)rpw;
        o = (double)ro;
    }
};

__device__ __forceinline__ bool gw_dropped(int variance, double cnt, unsigned bits) {
    if (!(cnt > 0.0)) return true;
    if (variance == 1) return !(bits & kGwBitNZ);
    if (variance == 2) return !(bits & kGwBitNZ) || !(bits & kGwBitN1);
    return false;
}

// ---- the pre-pass
template <int P>
struct GwPre {
    double cnt, spw, spwy;  // wave-uniform after gw_pre_rows
    unsigned bits;
    double first[P];  // the features of the first counting row (have)
    bool have;
};

template <typename T, int P>
__device__ __forceinline__ void gw_pre_rows(const GwFrame<T, P>& fr, int64_t r0, int64_t n, int lane, GwPre<P>& ps) {
    double cnt = 0.0, spw = 0.0, spwy = 0.0;
    unsigned bits = 0;
    ps.have = false;
#pragma unroll
    for (int c = 0; c < P; ++c) ps.first[c] = 0.0;
    for (int64_t base = 0; base < n; base += 64) {
        const int64_t r = base + lane;
        const bool live = r < n;
        const int64_t ri = r0 + (live ? r : 0);  // (n >= 1: the first row is always there)
        double x[P], y, pw, o;
        fr.load(ri, x, y, pw, o);
        const bool fin = pw >= 0.0 && pw < INFINITY;  // (false for a NaN)
        const bool pos = live && fin && pw > 0.0;
        cnt += pos ? 1.0 : 0.0;
        spw += pos ? pw : 0.0;
        spwy += pos ? pw * y : 0.0;
        if (__any(live && !fin)) bits |= kGwBitBad;
        if (__any(pos && y != 0.0)) bits |= kGwBitNZ;
        if (__any(pos && y != 1.0)) bits |= kGwBitN1;
        const unsigned long long m = __ballot(pos);
        if (!ps.have && m != 0) {
            const int src = __ffsll((long long)m) - 1;
#pragma unroll
            for (int c = 0; c < P; ++c) ps.first[c] = __shfl(x[c], src, 64);
            ps.have = true;
        }
        if (ps.have) {
#pragma unroll
            for (int c = 0; c < P; ++c)
                if (__any(pos && x[c] != ps.first[c])) bits |= 1u << c;
        }
    }
    ps.cnt = wave_sum(cnt);  // (integers: exact)
    ps.spw = wave_sum(spw);
    ps.spwy = wave_sum(spwy);
    ps.bits = bits;
}

// gstat: [3 x n_groups] the counting rows, sum pw, sum pw y; drop [n_groups]; flags[0] |= the varies bits of the kept groups,
// flags[1] |= 1 for a bad weight anywhere
template <typename T, int P>
__global__ __launch_bounds__(64) void gw_pre_kernel(const T* const* __restrict__ cols, const int64_t* __restrict__ off, int64_t n_groups,
                                                    int64_t split_rows, int variance, double* __restrict__ gstat, int32_t* __restrict__ drop,
                                                    unsigned* __restrict__ flags) {
    const int lane = threadIdx.x;
    GwFrame<T, P> fr;
    fr.open(cols, 0, variance);
    unsigned vary_all = 0, bad = 0;
    for (int64_t g = blockIdx.x; g < n_groups; g += gridDim.x) {
        const int64_t r0 = off[g], n = off[g + 1] - r0;  // (the host has validated the offsets and dropped the empty groups)
        if (n <= 0 || n > split_rows) continue;
        GwPre<P> ps;
        gw_pre_rows<T, P>(fr, r0, n, lane, ps);
        const bool dr = gw_dropped(variance, ps.cnt, ps.bits);
        if (lane == 0) {
            gstat[g] = ps.cnt;
            gstat[n_groups + g] = ps.spw;
            gstat[2 * n_groups + g] = ps.spwy;
            drop[g] = dr ? 1 : 0;
        }
        if (!dr) vary_all |= ps.bits & 0xFFFFu;
        bad |= ps.bits & kGwBitBad;
    }
    if (lane == 0 && vary_all) atomicOr(flags, vary_all);
    if (lane == 0 && bad) atomicOr(flags + 1, 1u);
}

// a wave per chunk: cpre[k * (3 + P)] = the counting rows, sum pw, sum pw y, the features of the chunk's first counting row; cbits[k]
template <typename T, int P>
__global__ __launch_bounds__(64) void gw_pre_chunk_kernel(const T* const* __restrict__ cols, const int64_t* __restrict__ chunk_r0,
                                                          const int64_t* __restrict__ chunk_n, int64_t n_chunks, int variance,
                                                          double* __restrict__ cpre, unsigned* __restrict__ cbits) {
    const int lane = threadIdx.x;
    GwFrame<T, P> fr;
    fr.open(cols, 0, variance);
    for (int64_t k = blockIdx.x; k < n_chunks; k += gridDim.x) {
        GwPre<P> ps;
        gw_pre_rows<T, P>(fr, chunk_r0[k], chunk_n[k], lane, ps);
        double* out = cpre + k * (3 + P);
        if (lane == 0) {
            out[0] = ps.cnt;
            out[1] = ps.spw;
            out[2] = ps.spwy;
#pragma unroll
            for (int c = 0; c < P; ++c) out[3 + c] = ps.first[c];
            cbits[k] = ps.bits;
        }
    }
}

// a thread per long group: its chunks in chunk order -> the group's entries; the group's first counting row is the first one of its
// first chunk that has one
__global__ __launch_bounds__(64) void gw_pre_long_kernel(int p, const int64_t* __restrict__ long_g, const int64_t* __restrict__ long_c0,
                                                         const int64_t* __restrict__ long_nc, int64_t n_long, int64_t n_groups, int variance,
                                                         const double* __restrict__ cpre, const unsigned* __restrict__ cbits,
                                                         double* __restrict__ gstat, int32_t* __restrict__ drop, unsigned* __restrict__ flags) {
    const int64_t j = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (j >= n_long) return;
    const int64_t c0 = long_c0[j], nc = long_nc[j], g = long_g[j];
    double cnt = 0.0, spw = 0.0, spwy = 0.0;
    unsigned bits = 0;
    int64_t kf = -1;
    for (int64_t k = c0; k < c0 + nc; ++k) {
        const double* in = cpre + k * (3 + p);
        if (in[0] > 0.0) {
            if (kf < 0) kf = k;
            else
                for (int c = 0; c < p; ++c)
                    if (in[3 + c] != cpre[kf * (3 + p) + 3 + c]) bits |= 1u << c;
        }
        cnt += in[0];
        spw += in[1];
        spwy += in[2];
        bits |= cbits[k];
    }
    const bool dr = gw_dropped(variance, cnt, bits);
    gstat[g] = cnt;
    gstat[n_groups + g] = spw;
    gstat[2 * n_groups + g] = spwy;
    drop[g] = dr ? 1 : 0;
    if (!dr && (bits & 0xFFFFu)) atomicOr(flags, bits & 0xFFFFu);
    if (bits & kGwBitBad) atomicOr(flags + 1, 1u);
}

// ---- the iteration
// what an iteration knows of the model: beta, whether this is the first iteration (the start rule) and its ybar
template <int P>
struct GwModel {
    double b[P];
    double ybar;
    bool first;
};

// the group's effect alpha_g = m_z - m_x . beta from the means of the iteration before
template <int P>
__device__ __forceinline__ double gw_alpha(const double* __restrict__ means, int64_t n_groups, int64_t g, const double* b) {
    double a = means[(int64_t)P * n_groups + g];
#pragma unroll
    for (int c = 0; c < P; ++c) a = fma(-means[(int64_t)c * n_groups + g], b[c], a);
    return a;
}

// row ri: its features (zeros for a row that does not count), working weight and working response.  A dead lane and a row of weight 0
// have w = z = 0 by selects: whatever their mu is reaches no sum
template <typename T, int P>
__device__ __forceinline__ void gw_working(const GwFrame<T, P>& fr, const GwModel<P>& md, double alpha, int64_t ri, bool live, double* x,
                                           double& w, double& z) {
    double y, pw, o;
    fr.load(ri, x, y, pw, o);
    double eta, mu;
    if (md.first) {
        mu = fr.variance == 2 ? (y + 0.5) * 0.5 : (y + md.ybar) * 0.5;
        eta = glm_link<double>(fr.link, mu);
    } else {
        eta = alpha + o;
#pragma unroll
        for (int c = 0; c < P; ++c) eta = fma(x[c], md.b[c], eta);
        mu = glm_inv<double>(fr.link, eta);
    }
    const double d = glm_deriv<double>(fr.link, mu), v = glm_var<double>(fr.variance, mu);
    const bool pos = live && pw > 0.0;
    w = pos ? pw / (d * d * v) : 0.0;
    z = pos ? (eta - o) + d * (y - mu) : 0.0;
#pragma unroll
    for (int c = 0; c < P; ++c) x[c] = pos ? x[c] : 0.0;
}

// the centred rows of a step (P features, z - m_z at feature row P, w at row P + 1) -> W_xx and W_xz
template <int P>
__device__ __forceinline__ void gw_gram(const double* xt, int rows, int lane, d4& acc, d4& acc2) {
    wave_tile_gram<P>(
        xt, kGwStride, rows, lane, [&](int row) { return xt[(P + 1) * kGwStride + row]; },
        [&](int f, int row, double s) { return f == 0 ? s * xt[P * kGwStride + row] : 0.0; },  // B column 0 = w (z - m_z)
        acc, acc2);
}

// weighted sums of the rows [r0, r0 + n): s[0 .. P) sum w x, s[P] sum w z, s[P + 1] sum w (per lane)
template <typename T, int P>
__device__ __forceinline__ void gw_stream_sums(const GwFrame<T, P>& fr, const GwModel<P>& md, double alpha, int64_t r0, int64_t n, int lane,
                                               double* s) {
    for (int64_t base = 0; base < n; base += 64) {
        const int64_t r = base + lane;
        const bool live = r < n;
        double x[P], w, z;
        gw_working<T, P>(fr, md, alpha, r0 + (live ? r : 0), live, x, w, z);
#pragma unroll
        for (int c = 0; c < P; ++c) s[c] = fma(w, x[c], s[c]);
        s[P] = fma(w, z, s[P]);
        s[P + 1] += w;
    }
}

// centred weighted products of the rows [r0, r0 + n) with the means `mean` (features, then z), 64 rows per step through the first 64
// row slots of the tile
template <typename T, int P>
__device__ __forceinline__ void gw_stream_centred(const GwFrame<T, P>& fr, const GwModel<P>& md, double alpha, int64_t r0, int64_t n,
                                                  const double* mean, double* xt, int lane, d4& acc, d4& acc2) {
    for (int64_t base = 0; base < n; base += 64) {
        const int64_t r = base + lane;
        const bool live = r < n;
        double x[P], w, z;
        gw_working<T, P>(fr, md, alpha, r0 + (live ? r : 0), live, x, w, z);
        PDS_WAVE_LDS_SYNC();  // (the previous step's operand reads are done)
#pragma unroll
        for (int c = 0; c < P; ++c) xt[c * kGwStride + lane] = live ? x[c] - mean[c] : 0.0;
        xt[P * kGwStride + lane] = live ? z - mean[P] : 0.0;
        xt[(P + 1) * kGwStride + lane] = w;
        PDS_WAVE_LDS_SYNC();
        gw_gram<P>(xt, (int)std::min<int64_t>(64, n - base), lane, acc, acc2);
    }
}

template <int P>
__device__ __forceinline__ void gw_open_model(GwModel<P>& md, const double* __restrict__ beta, int first, double ybar) {
#pragma unroll
    for (int c = 0; c < P; ++c) md.b[c] = beta[c];
    md.ybar = ybar;
    md.first = first != 0;
}

__device__ __forceinline__ void gw_write_record(double* rec, int lane, const d4& acc, const d4& acc2) {
    wave_tile_for_d(
        lane,
        [&](int i, int c, double w, double side) {
            rec[kMixedRecW + i * 16 + c] = w;
            if (c == 0) rec[kMixedRecXY + i] = side;
        },
        acc, acc2);
    if (lane < kMixedRecStride - kMixedRecCM) rec[kMixedRecCM + lane] = 0.0;  // (the slots the pass does not use: the record sum reads them)
}

template <typename T, int P>
__global__ __launch_bounds__(64) void gw_iter_kernel(const T* const* __restrict__ cols, const int64_t* __restrict__ off, int64_t n_groups,
                                                     int64_t split_rows, const int32_t* __restrict__ drop, int link, int variance, int first,
                                                     double ybar, const double* __restrict__ beta, const double* __restrict__ m_in,
                                                     double* __restrict__ m_out, double* __restrict__ partials) {
    __shared__ double xt[(P + 2) * kGwStride];  // features 0 .. P - 1, then z, then w: [c * kGwStride + row]
    const int lane = threadIdx.x;
    GwFrame<T, P> fr;
    fr.open(cols, link, variance);
    GwModel<P> md;
    gw_open_model<P>(md, beta, first, ybar);
    d4 acc = {0.0, 0.0, 0.0, 0.0}, acc2 = {0.0, 0.0, 0.0, 0.0};
    for (int64_t g = blockIdx.x; g < n_groups; g += gridDim.x) {
        const int64_t r0 = off[g], n = off[g + 1] - r0;  // (the host has validated the offsets)
        if (n <= 0 || n > split_rows) continue;          // cut into chunks: the chunk kernels
        if (drop[g]) continue;                           // (wave-uniform)
        const double alpha = md.first ? 0.0 : gw_alpha<P>(m_in, n_groups, g, md.b);
        const bool resident = n <= kGwCap;
        PDS_WAVE_LDS_SYNC();  // (the previous group's operand reads are done)
        double s[P + 2], mean[P + 1];
#pragma unroll
        for (int c = 0; c < P + 2; ++c) s[c] = 0.0;
        if (resident) {
            for (int64_t base = 0; base < n; base += 64) {
                const int64_t r = base + lane;
                const bool live = r < n;
                double x[P], w, z;
                gw_working<T, P>(fr, md, alpha, r0 + (live ? r : 0), live, x, w, z);
#pragma unroll
                for (int c = 0; c < P; ++c) {
                    s[c] = fma(w, x[c], s[c]);
                    xt[c * kGwStride + r] = x[c];
                }
                s[P] = fma(w, z, s[P]);
                s[P + 1] += w;
                xt[P * kGwStride + r] = z;
                xt[(P + 1) * kGwStride + r] = w;
            }
        } else {
            gw_stream_sums<T, P>(fr, md, alpha, r0, n, lane, s);
        }
        const double sw = wave_sum(s[P + 1]);
#pragma unroll
        for (int c = 0; c <= P; ++c) {
            mean[c] = wave_sum(s[c]) / sw;
            if (lane == c) m_out[(int64_t)c * n_groups + g] = mean[c];
        }
        if (resident) {
            for (int64_t base = 0; base < n; base += 64) {  // (a lane centres the slots it wrote)
                const int64_t r = base + lane;
                const bool live = r < n;
#pragma unroll
                for (int c = 0; c <= P; ++c) xt[c * kGwStride + r] = live ? xt[c * kGwStride + r] - mean[c] : 0.0;
            }
            PDS_WAVE_LDS_SYNC();
            gw_gram<P>(xt, (int)n, lane, acc, acc2);  // (the rows n .. up to the next multiple of 4 hold zeros)
        } else {
            gw_stream_centred<T, P>(fr, md, alpha, r0, n, mean, xt, lane, acc, acc2);
        }
    }
    gw_write_record(partials + (int64_t)blockIdx.x * kMixedRecStride, lane, acc, acc2);
}

// the weighted sums of one chunk -> sums[k * (P + 2)]
template <typename T, int P>
__global__ __launch_bounds__(64) void gw_chunk_sums_kernel(const T* const* __restrict__ cols, const int64_t* __restrict__ chunk_r0,
                                                           const int64_t* __restrict__ chunk_n, const int64_t* __restrict__ chunk_g,
                                                           int64_t n_chunks, int64_t n_groups, const int32_t* __restrict__ drop, int link,
                                                           int variance, int first, double ybar, const double* __restrict__ beta,
                                                           const double* __restrict__ m_in, double* __restrict__ sums) {
    const int lane = threadIdx.x;
    GwFrame<T, P> fr;
    fr.open(cols, link, variance);
    GwModel<P> md;
    gw_open_model<P>(md, beta, first, ybar);
    for (int64_t k = blockIdx.x; k < n_chunks; k += gridDim.x) {
        const int64_t g = chunk_g[k];
        if (drop[g]) continue;
        const double alpha = md.first ? 0.0 : gw_alpha<P>(m_in, n_groups, g, md.b);
        double s[P + 2];
#pragma unroll
        for (int c = 0; c < P + 2; ++c) s[c] = 0.0;
        gw_stream_sums<T, P>(fr, md, alpha, chunk_r0[k], chunk_n[k], lane, s);
#pragma unroll
        for (int c = 0; c < P + 2; ++c) {
            const double sum = wave_sum(s[c]);
            if (lane == c) sums[k * (P + 2) + c] = sum;
        }
    }
}

// a long group's chunk sums in chunk order -> its means; lane c = column c, lane p + 1 = sum w
__global__ __launch_bounds__(64) void gw_chunk_means_kernel(int p, const int64_t* __restrict__ long_g, const int64_t* __restrict__ long_c0,
                                                            const int64_t* __restrict__ long_nc, int64_t n_groups,
                                                            const int32_t* __restrict__ drop, const double* __restrict__ sums,
                                                            double* __restrict__ m_out) {
    const int lane = threadIdx.x;
    const int64_t j = blockIdx.x, g = long_g[j];
    if (drop[g]) return;
    const int64_t c0 = long_c0[j], nc = long_nc[j];
    double sum = 0.0;
    if (lane <= p + 1)
        for (int64_t k = 0; k < nc; ++k) sum += sums[(c0 + k) * (p + 2) + lane];
    const double sw = __shfl(sum, p + 1, 64);
    if (lane <= p) m_out[(int64_t)lane * n_groups + g] = sum / sw;
}

// centred products of the chunks with their groups' means: the wave keeps its accumulators across the chunks it walks
template <typename T, int P>
__global__ __launch_bounds__(64) void gw_chunk_scatter_kernel(const T* const* __restrict__ cols, const int64_t* __restrict__ chunk_r0,
                                                              const int64_t* __restrict__ chunk_n, const int64_t* __restrict__ chunk_g,
                                                              int64_t n_chunks, int64_t n_groups, const int32_t* __restrict__ drop, int link,
                                                              int variance, int first, double ybar, const double* __restrict__ beta,
                                                              const double* __restrict__ m_in, const double* __restrict__ m_out,
                                                              double* __restrict__ partials) {
    __shared__ double xt[(P + 2) * kGwStride];
    const int lane = threadIdx.x;
    GwFrame<T, P> fr;
    fr.open(cols, link, variance);
    GwModel<P> md;
    gw_open_model<P>(md, beta, first, ybar);
    d4 acc = {0.0, 0.0, 0.0, 0.0}, acc2 = {0.0, 0.0, 0.0, 0.0};
    for (int64_t k = blockIdx.x; k < n_chunks; k += gridDim.x) {
        const int64_t g = chunk_g[k];
        if (drop[g]) continue;
        const double alpha = md.first ? 0.0 : gw_alpha<P>(m_in, n_groups, g, md.b);
        double mean[P + 1];
#pragma unroll
        for (int c = 0; c <= P; ++c) mean[c] = m_out[(int64_t)c * n_groups + g];
        gw_stream_centred<T, P>(fr, md, alpha, chunk_r0[k], chunk_n[k], mean, xt, lane, acc, acc2);
    }
    gw_write_record(partials + (int64_t)blockIdx.x * kMixedRecStride, lane, acc, acc2);
}

// ---- the final pass
// where the rows' means go: pred (nullable); perm (nullable): row r of the frame the kernels read is row perm[r] of the caller's
template <typename T>
struct GwRowOut {
    const uint32_t* perm;
    T* pred;
};

// NaN for the rows [r0, r0 + n): a dropped group
template <typename T>
__device__ __forceinline__ void gw_rows_nan(const GwRowOut<T>& ro, int64_t r0, int64_t n, int lane) {
    if (!ro.pred) return;
    for (int64_t r = lane; r < n; r += 64) ro.pred[ro.perm ? (int64_t)ro.perm[r0 + r] : r0 + r] = (T)NAN;
}

// rows [r0, r0 + n), 64 per step, at (alpha, beta): mu out, the deviance and Pearson's chi2 into dv / pe (value + error term) and,
// with MEAT, the score sum r_i (x_i - m_x) of these rows into sc (side block, column 0)
template <typename T, int P, bool MEAT>
__device__ __forceinline__ void gw_final_stream(const GwFrame<T, P>& fr, const double* b, double alpha, const double* m, int64_t r0, int64_t n,
                                                const GwRowOut<T>& ro, double* xt, int lane, d4& sc, CompSq& dv, CompSq& pe) {
    const int f = lane & 15, kq = lane >> 4;
    for (int64_t base = 0; base < n; base += 64) {
        const int64_t r = base + lane;
        const bool live = r < n;
        const int64_t ri = r0 + (live ? r : 0);  // (n >= 1: the group's first row is always there)
        double x[P], y, pw, o;
        fr.load(ri, x, y, pw, o);
        int64_t ro_i = ri;
        if (ro.pred && ro.perm) ro_i = (int64_t)ro.perm[ri];
        if constexpr (MEAT) PDS_WAVE_LDS_SYNC();  // (the previous step's operand reads are done)
        double eta = alpha + o;
#pragma unroll
        for (int c = 0; c < P; ++c) eta = fma(x[c], b[c], eta);
        const double mu = glm_inv<double>(fr.link, eta);
        const double d = glm_deriv<double>(fr.link, mu), v = glm_var<double>(fr.variance, mu);
        const bool pos = live && pw > 0.0;
        const double e = y - mu;
        const double rs = pos ? pw * e / (v * d) : 0.0;  // (a select: a dead lane's or a zero-weight row's r reaches no sum)
        two_sum(dv.s, dv.c, pos ? pw * glm_unit_deviance(fr.variance, y, mu) : 0.0);
        two_sum(pe.s, pe.c, pos ? pw * (e * e / v) : 0.0);
        if (live && ro.pred) ro.pred[ro_i] = (T)mu;
        if constexpr (MEAT) {
#pragma unroll
            for (int c = 0; c < P; ++c) xt[c * kScoreTileStride + lane] = pos ? x[c] - m[c] : 0.0;
            xt[P * kScoreTileStride + lane] = rs;
            PDS_WAVE_LDS_SYNC();
            const int rows = (int)std::min<int64_t>(64, n - base);
            const int steps = (rows + 3) >> 2;  // (the row slots past `rows` hold zeros)
            for (int k = 0; k < steps; ++k) score_rows4<P>(xt, 4 * k + kq, f, sc);
        }
    }
}

// the record of a final-pass wave: the meat, the deviance in the sum-e^2 pair of slots, Pearson's chi2 in kGwRecPe / kGwRecPeC
constexpr int kGwRecPe = kMixedRecC, kGwRecPeC = kMixedRecLD;
__device__ __forceinline__ void gw_final_record(const ScoreMeat<false>& mt, double* rec, int lane, CompSq dv, CompSq pe) {
    mt.write_record(rec, lane, dv);
    pe.wave_fold();
    const double ps = __shfl(pe.s, 0, 64), pc = __shfl(pe.c, 0, 64);
    if (lane == kGwRecPe - kMixedRecXY) rec[kGwRecPe] = ps;  // (each by the lane that zeroed it: one lane, program order)
    if (lane == kGwRecPeC - kMixedRecXY) rec[kGwRecPeC] = pc;
}

template <int P>
__device__ __forceinline__ double gw_group_means(const double* __restrict__ means, int64_t n_groups, int64_t g, const double* b, double* m) {
#pragma unroll
    for (int c = 0; c <= P; ++c) m[c] = means[(int64_t)c * n_groups + g];
    double a = m[P];
#pragma unroll
    for (int c = 0; c < P; ++c) a = fma(-m[c], b[c], a);
    return a;
}

template <typename T, int P, bool MEAT>
__global__ __launch_bounds__(64) void gw_final_kernel(const T* const* __restrict__ cols, const int64_t* __restrict__ off, int64_t n_groups,
                                                      int64_t split_rows, const int32_t* __restrict__ drop, int link, int variance,
                                                      const double* __restrict__ beta, const double* __restrict__ means,
                                                      const int64_t* __restrict__ gmap, T* __restrict__ alpha, GwRowOut<T> ro,
                                                      double* __restrict__ partials) {
    __shared__ double xt[MEAT ? (P + 1) * kScoreTileStride + kScoreBatch * kScorePark : 1];  // features, then r; the park
    double* park = xt + (P + 1) * kScoreTileStride;
    const int lane = threadIdx.x;
    GwFrame<T, P> fr;
    fr.open(cols, link, variance);
    double b[P];
#pragma unroll
    for (int c = 0; c < P; ++c) b[c] = beta[c];
    ScoreMeat<false> mt;
    CompSq dv, pe;
    for (int64_t g = blockIdx.x; g < n_groups; g += gridDim.x) {
        const int64_t r0 = off[g], n = off[g + 1] - r0;  // (the host has validated the offsets)
        if (n <= 0 || n > split_rows) continue;          // empty: nothing; cut into chunks: the chunk kernel
        if (drop[g]) {                                   // (wave-uniform)
            gw_rows_nan<T>(ro, r0, n, lane);
            continue;
        }
        double m[P + 1];
        const double a = gw_group_means<P>(means, n_groups, g, b, m);
        if (alpha && lane == 0) alpha[gmap ? gmap[g] : g] = (T)a;
        d4 sc = {0.0, 0.0, 0.0, 0.0};
        gw_final_stream<T, P, MEAT>(fr, b, a, m, r0, n, ro, xt, lane, sc, dv, pe);
        if constexpr (MEAT) mt.park_d(park, lane, sc);
    }
    if constexpr (MEAT) mt.flush(park, lane);
    gw_final_record(mt, partials + (int64_t)blockIdx.x * kMixedRecStride, lane, dv, pe);
}

// a wave per chunk (grid stride): the rows' means, with MEAT the chunk's score -> scores[k * kScorePark + entry] (zeros for a chunk of a
// dropped group); the wave's record carries its deviance and Pearson sums alone.  The first chunk of a group writes the group's alpha.
template <typename T, int P, bool MEAT>
__global__ __launch_bounds__(64) void gw_final_chunk_kernel(const T* const* __restrict__ cols, const int64_t* __restrict__ chunk_r0,
                                                            const int64_t* __restrict__ chunk_n, const int64_t* __restrict__ chunk_g,
                                                            const int64_t* __restrict__ chunk_first, int64_t n_chunks, int64_t n_groups,
                                                            const int32_t* __restrict__ drop, int link, int variance,
                                                            const double* __restrict__ beta, const double* __restrict__ means,
                                                            const int64_t* __restrict__ gmap, T* __restrict__ alpha, GwRowOut<T> ro,
                                                            double* __restrict__ scores, double* __restrict__ partials) {
    __shared__ double xt[MEAT ? (P + 1) * kScoreTileStride : 1];
    const int lane = threadIdx.x;
    GwFrame<T, P> fr;
    fr.open(cols, link, variance);
    double b[P];
#pragma unroll
    for (int c = 0; c < P; ++c) b[c] = beta[c];
    CompSq dv, pe;
    for (int64_t k = blockIdx.x; k < n_chunks; k += gridDim.x) {
        const int64_t g = chunk_g[k], r0 = chunk_r0[k], n = chunk_n[k];
        d4 sc = {0.0, 0.0, 0.0, 0.0};
        if (drop[g]) {
            gw_rows_nan<T>(ro, r0, n, lane);
        } else {
            double m[P + 1];
            const double a = gw_group_means<P>(means, n_groups, g, b, m);
            if (alpha && lane == 0 && r0 == chunk_first[k]) alpha[gmap ? gmap[g] : g] = (T)a;
            gw_final_stream<T, P, MEAT>(fr, b, a, m, r0, n, ro, xt, lane, sc, dv, pe);
        }
        if constexpr (MEAT) score_store_d(scores + k * kScorePark, lane, sc, 0.0);
    }
    gw_final_record(ScoreMeat<false>{}, partials + (int64_t)blockIdx.x * kMixedRecStride, lane, dv, pe);
}

}  // namespace

int glm_within_iter_blocks(const pds_ctx* ctx, int64_t n_work) { return mixed_stats_blocks(ctx, n_work); }
int glm_within_final_blocks(const pds_ctx* ctx, int64_t n_work) { return within_pass_blocks(ctx, n_work); }

template <typename T>
int launch_glm_within_pre(pds_ctx* ctx, const T* const* d_cols, int n_feat, const int64_t* d_off, int64_t n_groups, int64_t split_rows,
                          const MixedChunks& ch, int variance, double* d_cpre, double* d_gstat, int32_t* d_drop, unsigned* d_flags) {
    if (n_feat < 1 || n_feat > kMaxFeatSmall) return fail(PDS_ERR_UNSUPPORTED, "fixed-effects GLM: up to 16 feature columns");
    KernelTimer timer(ctx, kKindGroupedMoments);
    PDS_HIP_CHECK(hipMemsetAsync(d_flags, 0, 2 * sizeof(unsigned), ctx->stream));
    const int nb = glm_within_iter_blocks(ctx, n_groups);
    const int nbc = ch.n_chunks > 0 ? glm_within_iter_blocks(ctx, ch.n_chunks) : 0;
    dispatch_width<1, kMaxFeatSmall>(n_feat, [&](auto pc) {
        constexpr int P = decltype(pc)::value;
        hipLaunchKernelGGL((gw_pre_kernel<T, P>), dim3(nb), dim3(64), 0, ctx->stream, d_cols, d_off, n_groups, split_rows, variance, d_gstat,
                           d_drop, d_flags);
        if (nbc > 0) {
            hipLaunchKernelGGL((gw_pre_chunk_kernel<T, P>), dim3(nbc), dim3(64), 0, ctx->stream, d_cols, ch.d_chunk_r0, ch.d_chunk_n,
                               ch.n_chunks, variance, d_cpre, ch.d_varies);
            hipLaunchKernelGGL(gw_pre_long_kernel, dim3((unsigned)((ch.n_long + 63) / 64)), dim3(64), 0, ctx->stream, P, ch.d_long_g,
                               ch.d_long_c0, ch.d_long_nc, ch.n_long, n_groups, variance, (const double*)d_cpre,
                               (const unsigned*)ch.d_varies, d_gstat, d_drop, d_flags);
        }
    });
    PDS_HIP_CHECK(hipGetLastError());
    return PDS_OK;
}

template <typename T>
int launch_glm_within_iter(pds_ctx* ctx, const T* const* d_cols, int n_feat, const int64_t* d_off, int64_t n_groups, int64_t split_rows,
                           const MixedChunks& ch, const int32_t* d_drop, int link, int variance, bool first, double ybar, const double* d_beta,
                           const double* d_means_in, double* d_means_out, double* d_partials, double* d_stage, double* d_rec) {
    if (n_feat < 1 || n_feat > kMaxFeatSmall) return fail(PDS_ERR_UNSUPPORTED, "fixed-effects GLM: up to 16 feature columns");
    KernelTimer timer(ctx, kKindIter);
    const int nb = glm_within_iter_blocks(ctx, n_groups);
    const int nbc = ch.n_chunks > 0 ? glm_within_iter_blocks(ctx, ch.n_chunks) : 0;
    const int fi = first ? 1 : 0;
    dispatch_width<1, kMaxFeatSmall>(n_feat, [&](auto pc) {
        constexpr int P = decltype(pc)::value;
        hipLaunchKernelGGL((gw_iter_kernel<T, P>), dim3(nb), dim3(64), 0, ctx->stream, d_cols, d_off, n_groups, split_rows, d_drop, link,
                           variance, fi, ybar, d_beta, d_means_in, d_means_out, d_partials);
        if (nbc > 0) {
            hipLaunchKernelGGL((gw_chunk_sums_kernel<T, P>), dim3(nbc), dim3(64), 0, ctx->stream, d_cols, ch.d_chunk_r0, ch.d_chunk_n,
                               ch.d_chunk_g, ch.n_chunks, n_groups, d_drop, link, variance, fi, ybar, d_beta, d_means_in, ch.d_sums);
            hipLaunchKernelGGL(gw_chunk_means_kernel, dim3((unsigned)ch.n_long), dim3(64), 0, ctx->stream, P, ch.d_long_g, ch.d_long_c0,
                               ch.d_long_nc, n_groups, d_drop, (const double*)ch.d_sums, d_means_out);
            hipLaunchKernelGGL((gw_chunk_scatter_kernel<T, P>), dim3(nbc), dim3(64), 0, ctx->stream, d_cols, ch.d_chunk_r0, ch.d_chunk_n,
                               ch.d_chunk_g, ch.n_chunks, n_groups, d_drop, link, variance, fi, ybar, d_beta, d_means_in,
                               (const double*)d_means_out, d_partials + (int64_t)nb * kMixedRecStride);
        }
    });
    PDS_HIP_CHECK(hipGetLastError());
    return launch_sum_records(ctx, d_partials, nb + nbc, d_stage, d_rec, /*compensated=*/true);
}

template <typename T>
int launch_glm_within_final(pds_ctx* ctx, const T* const* d_cols, int n_feat, const int64_t* d_off, int64_t n_groups, int64_t split_rows,
                            const MixedChunks& ch, double* d_scores, const int32_t* d_drop, int link, int variance, const double* d_beta,
                            const double* d_means, bool meat, const int64_t* d_gmap, const uint32_t* d_perm, T* d_alpha, T* d_pred,
                            double* d_partials, double* d_stage, double* d_rec) {
    if (n_feat < 1 || n_feat > kMaxFeatSmall) return fail(PDS_ERR_UNSUPPORTED, "fixed-effects GLM: up to 16 feature columns");
    if (meat && ch.n_chunks > 0 && !d_scores) return fail(PDS_ERR_INVALID, "null argument");
    KernelTimer timer(ctx, kKindPass2);
    const int nb = glm_within_final_blocks(ctx, n_groups);
    const int nbc = ch.n_chunks > 0 ? glm_within_final_blocks(ctx, ch.n_chunks) : 0;
    const int nbl = ch.n_chunks > 0 && meat ? glm_within_final_blocks(ctx, ch.n_long) : 0;
    const GwRowOut<T> ro{d_perm, d_pred};
    dispatch_width<1, kMaxFeatSmall>(n_feat, [&](auto pc) {
        constexpr int P = decltype(pc)::value;
        auto go = [&](auto mc) {
            constexpr bool MEAT = decltype(mc)::value;
            hipLaunchKernelGGL((gw_final_kernel<T, P, MEAT>), dim3(nb), dim3(64), 0, ctx->stream, d_cols, d_off, n_groups, split_rows, d_drop, link,
                               variance, d_beta, d_means, d_gmap, d_alpha, ro, d_partials);
            if (nbc > 0)
                hipLaunchKernelGGL((gw_final_chunk_kernel<T, P, MEAT>), dim3(nbc), dim3(64), 0, ctx->stream, d_cols, ch.d_chunk_r0, ch.d_chunk_n,
                                   ch.d_chunk_g, ch.d_chunk_first, ch.n_chunks, n_groups, d_drop, link, variance, d_beta, d_means, d_gmap,
                                   d_alpha, ro, d_scores, d_partials + (int64_t)nb * kMixedRecStride);
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

#define PDS_GW_INSTANTIATE(T)                                                                                                                  \
    template int launch_glm_within_pre<T>(pds_ctx*, const T* const*, int, const int64_t*, int64_t, int64_t, const MixedChunks&, int, double*,  \
                                          double*, int32_t*, unsigned*);                                                                       \
    template int launch_glm_within_iter<T>(pds_ctx*, const T* const*, int, const int64_t*, int64_t, int64_t, const MixedChunks&,               \
                                           const int32_t*, int, int, bool, double, const double*, const double*, double*, double*, double*,   \
                                           double*);                                                                                           \
    template int launch_glm_within_final<T>(pds_ctx*, const T* const*, int, const int64_t*, int64_t, int64_t, const MixedChunks&, double*,     \
                                            const int32_t*, int, int, const double*, const double*, bool, const int64_t*, const uint32_t*, T*, \
                                            T*, double*, double*, double*);
PDS_GW_INSTANTIATE(double)
PDS_GW_INSTANTIATE(float)
#undef PDS_GW_INSTANTIATE

}  // namespace pds
