// within2_graph.hip -- the integer side of the fixed-effects regression with TWO absorbed factors (capi_within2.hpp): what the call
// needs to know about the bipartite graph of the occupied cells, and the estimated effects formed from the sweeps' tables.
//
// NODES: the n_a levels of factor 1 (indices 0 .. n_a - 1), then the n_b codes of factor 2 (node n_a + code).  Every row is an edge
// (u(row), n_a + v(row)).  Nothing here is floating point until the effects, and nothing is summed: the labels, the counts and the
// reference levels are integers, so two calls give the same bits whatever the scheduling.
//
//   * w2g_range_kernel: reads the codes and nothing else; one integer atomicOr per wave that saw a code outside [0, n_levels).  The
//     host reads the flag BEFORE any kernel indexes anything by a code.
//   * w2g_level_starts_kernel: the first place of every code in the code-ordered list (a counted binary search per code): the level
//     counts of factor 2 are differences of neighbours, exact.
//   * components by hook and compress.  label[v] = v to start; `root` is the flat labelling a round starts from (every node points at
//     its root).  One round:
//       hook      every edge whose ends have roots ru != rv does atomicMin(&label[max(ru, rv)], min(ru, rv)) -- 32-bit integer
//                 vector atomics, the only atomics of the pass; it reads `root`, which no one writes meanwhile, so label[r] ends as
//                 the smallest neighbouring root of r, in every order of arrival.  (A plain load in front of the atomic skips the
//                 ones that cannot lower the label: labels only fall, so a stale value only costs an atomic.)
//       compress  jump passes label[v] = label[label[v]] in place until every node points at its root: a pass halves every depth, a
//                 value read while another lane writes it is an older ancestor, still an ancestor; at most ceil(log2 nodes) passes.
//     A parent is always smaller than its child, so there are no cycles and the final label of a node is the SMALLEST node index of
//     its component: a level of factor 1.
//     THE ROUND BOUND.  Take the T >= 2 trees of one component at the start of a round.  H: the roots with a smaller neighbouring
//     root -- they hook, each into one target, and are roots no more.  The others are local minima: L1, those hooked into, and L0,
//     the stagnant ones.  |L1| <= |H| (every target received a hooker of its own) and |L1| <= T - |H|.  A stagnant root s has a
//     neighbouring root r > s; r hooked into some m <= s, and m != s because s is stagnant: after the round r's tree has a root below
//     s, so s hooks in the NEXT round.  After two rounds at most |L1| <= min(|H|, T - |H|) <= T / 2 trees are left.  (After ONE round
//     T - |H| may be left: a star whose centre is the largest root keeps every leaf.)  So a component is one tree after at most
//     2 ceil(log2 nodes) rounds and one more round finds nothing to hook: 2 ceil(log2 nodes) + 1 is the cap, proved, not tuned.  The
//     rounds are driven from the host (within2_components), which reads 8 bytes per round ("something hooked", "not yet flat") and 4
//     per further jump pass.
//   * w2g_count_kernel: occupied levels of both factors and roots among the occupied levels of factor 1, per block, no atomics; the
//     host adds the blocks' counts.
//   * effects: w2g_gamma_raw_kernel (gamma_raw per code), w2g_ref_kernel (the lowest occupied code of factor 2 in every component,
//     integer atomicMin into ref[label]), w2g_effects_kernel<T> (lane = level, f64, terms in ascending column order).
// Every device loop is a counted `for`; no workgroup waits for another; no floating-point atomics.
#include "common.hpp"

#include <algorithm>

namespace pds {

namespace {

constexpr int kG2Threads = 256;
constexpr int kG2CountBlocks = 256;  // blocks of w2g_count_kernel: 3 counts each come back to the host
constexpr int kG2Flags = 64;         // [0] something hooked; [1 + k] jump pass k left a node that does not point at its root
constexpr uint32_t kG2NoRef = 0x7fffffffu;

int g2_blocks(const pds_ctx* ctx, int64_t n) {
    return (int)std::max<int64_t>(1, std::min<int64_t>((n + kG2Threads - 1) / kG2Threads, (int64_t)ctx->num_cus * 8));
}

int g2_ceil_log2(int64_t n) {
    int b = 0;
    for (; b < 62 && ((int64_t)1 << b) < n; ++b) {}
    return b;
}

__global__ __launch_bounds__(kG2Threads) void w2g_range_kernel(const int32_t* __restrict__ codes, int64_t n, uint32_t n_levels, int* flag) {
    bool bad = false;
    for (int64_t r = (int64_t)blockIdx.x * kG2Threads + threadIdx.x; r < n; r += (int64_t)gridDim.x * kG2Threads)
        bad |= (uint32_t)codes[r] >= n_levels;  // (a negative code is above 2^31 as an unsigned one)
    if (__ballot(bad) != 0 && (threadIdx.x & 63) == 0) atomicOr(flag, 1);
}

// start[l] = rows whose code is below l, l = 0 .. n_levels: `sorted` is ascending
__global__ __launch_bounds__(kG2Threads) void w2g_level_starts_kernel(const uint32_t* __restrict__ sorted, int64_t n, int64_t n_levels,
                                                                      uint32_t* __restrict__ start) {
    for (int64_t l = (int64_t)blockIdx.x * kG2Threads + threadIdx.x; l <= n_levels; l += (int64_t)gridDim.x * kG2Threads) {
        int64_t lo = 0, hi = n;
        for (int it = 0; it < 33 && lo < hi; ++it) {
            const int64_t mid = lo + ((hi - lo) >> 1);
            if ((int64_t)sorted[mid] < l) lo = mid + 1;
            else hi = mid;
        }
        start[l] = (uint32_t)lo;
    }
}

__global__ __launch_bounds__(kG2Threads) void w2g_init_kernel(uint32_t* __restrict__ label, uint32_t* __restrict__ root, int64_t n_nodes) {
    for (int64_t v = (int64_t)blockIdx.x * kG2Threads + threadIdx.x; v < n_nodes; v += (int64_t)gridDim.x * kG2Threads)
        label[v] = root[v] = (uint32_t)v;
}

// occ[u(row)] = 1 (every writer stores the same word)
__global__ __launch_bounds__(kG2Threads) void w2g_mark_kernel(const uint32_t* __restrict__ u, int64_t n, uint32_t* occ) {
    for (int64_t r = (int64_t)blockIdx.x * kG2Threads + threadIdx.x; r < n; r += (int64_t)gridDim.x * kG2Threads) occ[u[r]] = 1u;
}

__global__ __launch_bounds__(kG2Threads) void w2g_hook_kernel(const uint32_t* __restrict__ u, const uint32_t* __restrict__ v, int64_t n, uint32_t n_a,
                                                              const uint32_t* __restrict__ root, uint32_t* label, int* changed) {
    bool any = false;
    for (int64_t r = (int64_t)blockIdx.x * kG2Threads + threadIdx.x; r < n; r += (int64_t)gridDim.x * kG2Threads) {
        const uint32_t ru = root[u[r]], rv = root[n_a + v[r]];
        if (ru == rv) continue;
        any = true;
        const uint32_t hi = ru > rv ? ru : rv, lo = ru > rv ? rv : ru;
        if (label[hi] > lo) atomicMin(&label[hi], lo);
    }
    if (any) *changed = 1;
}

__global__ __launch_bounds__(kG2Threads) void w2g_jump_kernel(uint32_t* label, int64_t n_nodes, int* not_flat) {
    bool any = false;
    for (int64_t v = (int64_t)blockIdx.x * kG2Threads + threadIdx.x; v < n_nodes; v += (int64_t)gridDim.x * kG2Threads) {
        const uint32_t p = label[v];
        if (p == (uint32_t)v) continue;
        const uint32_t gp = label[p];
        if (gp == p) continue;  // p is a root, and a root stays one through the passes
        label[v] = gp;
        any |= label[gp] != gp;
    }
    if (any) *not_flat = 1;
}

// per block: occupied levels of factor 1, occupied codes of factor 2 (their root is a level of factor 1), components
__global__ __launch_bounds__(kG2Threads) void w2g_count_kernel(const uint32_t* __restrict__ label, const uint32_t* __restrict__ occ, uint32_t n_a,
                                                               int64_t n_nodes, int64_t* __restrict__ counts) {
    __shared__ int64_t part[3][kG2Threads / 64];
    int64_t c[3] = {0, 0, 0};
    for (int64_t v = (int64_t)blockIdx.x * kG2Threads + threadIdx.x; v < n_nodes; v += (int64_t)gridDim.x * kG2Threads) {
        const uint32_t l = label[v];
        if (v < (int64_t)n_a) {
            const bool used = !occ || occ[v] != 0u;
            c[0] += used;
            c[2] += used && l == (uint32_t)v;
        } else {
            c[1] += l < n_a;
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) c[k] += __shfl_xor(c[k], m, 64);
        if (lane == 0) part[k][wave] = c[k];
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        int64_t s = 0;
        for (int w = 0; w < kG2Threads / 64; ++w) s += part[threadIdx.x][w];
        counts[(int64_t)blockIdx.x * 3 + threadIdx.x] = s;
    }
}

// the labels as components per level: -1 for a level no row uses
__global__ __launch_bounds__(kG2Threads) void w2g_components_out_kernel(const uint32_t* __restrict__ label, const uint32_t* __restrict__ occ,
                                                                        uint32_t n_a, int64_t n_nodes, int32_t* __restrict__ comp1,
                                                                        int32_t* __restrict__ comp2) {
    for (int64_t v = (int64_t)blockIdx.x * kG2Threads + threadIdx.x; v < n_nodes; v += (int64_t)gridDim.x * kG2Threads) {
        const uint32_t l = label[v];
        if (v < (int64_t)n_a) {
            if (comp1) comp1[v] = (!occ || occ[v] != 0u) ? (int32_t)l : -1;
        } else if (comp2) {
            comp2[v - n_a] = l < n_a ? (int32_t)l : -1;
        }
    }
}

__global__ __launch_bounds__(kG2Threads) void w2g_gamma_raw_kernel(const double* __restrict__ a2, const double* __restrict__ beta, int p,
                                                                   int64_t n_levels2, double* __restrict__ graw) {
    for (int64_t l = (int64_t)blockIdx.x * kG2Threads + threadIdx.x; l < n_levels2; l += (int64_t)gridDim.x * kG2Threads) {
        const double* t = a2 + l * (p + 1);
        double s = 0.0;
        for (int j = 0; j < p; ++j) s = fma(beta[j], t[j], s);
        graw[l] = t[p] - s;
    }
}

__global__ __launch_bounds__(kG2Threads) void w2g_ref_init_kernel(uint32_t* __restrict__ ref, int64_t n_a) {
    for (int64_t g = (int64_t)blockIdx.x * kG2Threads + threadIdx.x; g < n_a; g += (int64_t)gridDim.x * kG2Threads) ref[g] = kG2NoRef;
}

// ref[root] = the lowest occupied code of factor 2 in the component of that root
__global__ __launch_bounds__(kG2Threads) void w2g_ref_kernel(const uint32_t* __restrict__ label, uint32_t n_a, int64_t n_levels2, uint32_t* ref) {
    for (int64_t l = (int64_t)blockIdx.x * kG2Threads + threadIdx.x; l < n_levels2; l += (int64_t)gridDim.x * kG2Threads) {
        const uint32_t r = label[n_a + l];
        if (r < n_a) atomicMin(&ref[r], (uint32_t)l);
    }
}

// lane = level.  alpha_g = (a1[g][y] - sum_j beta_j a1[g][j] + alpha'_g) + c, gamma_l = gamma_raw[l] - c, c = gamma_raw[ref[label]]
template <typename T>
__global__ __launch_bounds__(kG2Threads) void w2g_effects_kernel(const double* __restrict__ a1, const double* __restrict__ beta,
                                                                 const double* __restrict__ alpha1, const double* __restrict__ graw,
                                                                 const uint32_t* __restrict__ label, const uint32_t* __restrict__ ref,
                                                                 const int64_t* __restrict__ gmap, int p, uint32_t n_a, int64_t n_nodes,
                                                                 T* __restrict__ eff1, T* __restrict__ eff2, int32_t* __restrict__ comp1,
                                                                 int32_t* __restrict__ comp2) {
    for (int64_t v = (int64_t)blockIdx.x * kG2Threads + threadIdx.x; v < n_nodes; v += (int64_t)gridDim.x * kG2Threads) {
        const uint32_t root = label[v];
        const bool used = root < n_a;  // (every level of factor 1 is occupied; a code no row uses is its own root)
        const uint32_t rf = used ? ref[root] : kG2NoRef;  // (a root holds a row, so a code: the comparison below is never false for it)
        const double c = (int64_t)rf < n_nodes - (int64_t)n_a ? graw[rf] : (double)NAN;
        const int32_t comp = used ? (int32_t)(gmap ? gmap[root] : (int64_t)root) : -1;
        if (v < (int64_t)n_a) {
            const double* t = a1 + v * (p + 1);
            double s = 0.0;
            for (int j = 0; j < p; ++j) s = fma(beta[j], t[j], s);
            const int64_t o = gmap ? gmap[v] : v;
            if (eff1) eff1[o] = (T)(((t[p] - s) + alpha1[v]) + c);
            if (comp1) comp1[o] = comp;
        } else {
            const int64_t l = v - n_a;
            if (eff2) eff2[l] = used ? (T)(graw[l] - c) : (T)NAN;
            if (comp2) comp2[l] = comp;
        }
    }
}

}  // namespace

size_t within2_graph_count_bytes() { return (size_t)kG2CountBlocks * 3 * sizeof(int64_t); }
size_t within2_graph_flag_bytes() { return (size_t)kG2Flags * sizeof(int); }

int launch_within2_range_check(pds_ctx* ctx, const int32_t* d_codes, int64_t n_rows, int64_t n_levels, int* d_flag) {
    hipLaunchKernelGGL(w2g_range_kernel, dim3(g2_blocks(ctx, n_rows)), dim3(kG2Threads), 0, ctx->stream, d_codes, n_rows, (uint32_t)n_levels, d_flag);
    PDS_HIP_CHECK(hipGetLastError());
    return PDS_OK;
}

int launch_within2_level_starts(pds_ctx* ctx, const uint32_t* d_sorted, int64_t n_rows, int64_t n_levels, uint32_t* d_start) {
    KernelTimer timer(ctx, kKindGraph);
    hipLaunchKernelGGL(w2g_level_starts_kernel, dim3(g2_blocks(ctx, n_levels + 1)), dim3(kG2Threads), 0, ctx->stream, d_sorted, n_rows, n_levels,
                       d_start);
    PDS_HIP_CHECK(hipGetLastError());
    return PDS_OK;
}

int launch_within2_mark(pds_ctx* ctx, const uint32_t* d_u, int64_t n_rows, uint32_t* d_occ) {
    hipLaunchKernelGGL(w2g_mark_kernel, dim3(g2_blocks(ctx, n_rows)), dim3(kG2Threads), 0, ctx->stream, d_u, n_rows, d_occ);
    PDS_HIP_CHECK(hipGetLastError());
    return PDS_OK;
}

int within2_components(pds_ctx* ctx, const uint32_t* d_u, const uint32_t* d_v, int64_t n_rows, int64_t n_a, int64_t n_b, const uint32_t* d_occ,
                       uint32_t* d_label, uint32_t* d_root, int* d_flags, int64_t* d_counts, int64_t* n1, int64_t* n2, int64_t* n_components,
                       int* n_rounds) {
    const int64_t n_nodes = n_a + n_b;
    if (n_a < 1 || n_b < 1 || n_nodes >= ((int64_t)1 << 32)) return fail(PDS_ERR_INVALID, "component labelling: fewer than 2^32 levels in all");
    const int jump_cap = g2_ceil_log2(n_nodes) + 1;  // jump passes of one round: a pass halves every depth, the last one only confirms
    const int cap = 2 * g2_ceil_log2(n_nodes) + 1;   // rounds: the trees of a component halve in two rounds (the file's head), the last one finds nothing
    if (1 + jump_cap > kG2Flags) return fail(PDS_ERR_INVALID, "component labelling: fewer than 2^32 levels in all");
    const int nb_rows = g2_blocks(ctx, n_rows), nb_nodes = g2_blocks(ctx, n_nodes);
    const dim3 th(kG2Threads);
    {
        KernelTimer timer(ctx, kKindGraph);
        hipLaunchKernelGGL(w2g_init_kernel, dim3(nb_nodes), th, 0, ctx->stream, d_label, d_root, n_nodes);
        PDS_HIP_CHECK(hipGetLastError());
    }
    int h[2] = {0, 0}, rounds = 0;
    for (bool done = false; !done;) {
        if (rounds == cap) return fail(PDS_ERR_NUMERIC, "fixed-effects regression: component labelling did not finish");
        ++rounds;
        PDS_HIP_CHECK(hipMemsetAsync(d_flags, 0, within2_graph_flag_bytes(), ctx->stream));
        {
            KernelTimer timer(ctx, kKindGraph);
            hipLaunchKernelGGL(w2g_hook_kernel, dim3(nb_rows), th, 0, ctx->stream, d_u, d_v, n_rows, (uint32_t)n_a, (const uint32_t*)d_root, d_label,
                               d_flags);
            hipLaunchKernelGGL(w2g_jump_kernel, dim3(nb_nodes), th, 0, ctx->stream, d_label, n_nodes, d_flags + 1);
            PDS_HIP_CHECK(hipGetLastError());
        }
        PDS_HIP_CHECK(hipMemcpyAsync(h, d_flags, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
        PDS_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        if (!h[0]) {  // nothing hooked: the labels are final
            done = true;
            continue;
        }
        for (int k = 1; h[1]; ++k) {
            if (k == jump_cap) return fail(PDS_ERR_NUMERIC, "fixed-effects regression: component labelling did not finish");
            {
                KernelTimer timer(ctx, kKindGraph);
                hipLaunchKernelGGL(w2g_jump_kernel, dim3(nb_nodes), th, 0, ctx->stream, d_label, n_nodes, d_flags + 1 + k);
                PDS_HIP_CHECK(hipGetLastError());
            }
            PDS_HIP_CHECK(hipMemcpyAsync(h + 1, d_flags + 1 + k, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
            PDS_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        }
        PDS_HIP_CHECK(hipMemcpyAsync(d_root, d_label, (size_t)n_nodes * 4, hipMemcpyDeviceToDevice, ctx->stream));
    }
    {
        KernelTimer timer(ctx, kKindGraph);
        hipLaunchKernelGGL(w2g_count_kernel, dim3(kG2CountBlocks), th, 0, ctx->stream, (const uint32_t*)d_label, d_occ, (uint32_t)n_a, n_nodes, d_counts);
        PDS_HIP_CHECK(hipGetLastError());
    }
    int64_t counts[kG2CountBlocks * 3];
    PDS_HIP_CHECK(hipMemcpyAsync(counts, d_counts, sizeof(counts), hipMemcpyDeviceToHost, ctx->stream));
    PDS_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    int64_t tot[3] = {0, 0, 0};
    for (int b = 0; b < kG2CountBlocks; ++b)
        for (int k = 0; k < 3; ++k) tot[k] += counts[b * 3 + k];
    if (n1) *n1 = tot[0];
    if (n2) *n2 = tot[1];
    if (n_components) *n_components = tot[2];
    if (n_rounds) *n_rounds = rounds;
    return PDS_OK;
}

int launch_within2_components_out(pds_ctx* ctx, const uint32_t* d_label, const uint32_t* d_occ, int64_t n_a, int64_t n_b, int32_t* d_comp1,
                                  int32_t* d_comp2) {
    const int64_t n_nodes = n_a + n_b;
    hipLaunchKernelGGL(w2g_components_out_kernel, dim3(g2_blocks(ctx, n_nodes)), dim3(kG2Threads), 0, ctx->stream, d_label, d_occ, (uint32_t)n_a, n_nodes,
                       d_comp1, d_comp2);
    PDS_HIP_CHECK(hipGetLastError());
    return PDS_OK;
}

template <typename T>
int launch_within2_effects(pds_ctx* ctx, const double* d_a1, const double* d_a2, const double* d_beta, const double* d_alpha1, const uint32_t* d_label,
                           const int64_t* d_gmap, int n_feat, int64_t n_a, int64_t n_levels2, double* d_graw, uint32_t* d_ref, T* d_eff1, T* d_eff2,
                           int32_t* d_comp1, int32_t* d_comp2) {
    if (n_feat < 1 || n_feat > kMaxFeatSmall) return fail(PDS_ERR_UNSUPPORTED, "fixed-effects regression: up to 16 feature columns");
    KernelTimer timer(ctx, kKindGraph);
    const int64_t n_nodes = n_a + n_levels2;
    const dim3 th(kG2Threads);
    hipLaunchKernelGGL(w2g_gamma_raw_kernel, dim3(g2_blocks(ctx, n_levels2)), th, 0, ctx->stream, d_a2, d_beta, n_feat, n_levels2, d_graw);
    hipLaunchKernelGGL(w2g_ref_init_kernel, dim3(g2_blocks(ctx, n_a)), th, 0, ctx->stream, d_ref, n_a);
    hipLaunchKernelGGL(w2g_ref_kernel, dim3(g2_blocks(ctx, n_levels2)), th, 0, ctx->stream, d_label, (uint32_t)n_a, n_levels2, d_ref);
    hipLaunchKernelGGL((w2g_effects_kernel<T>), dim3(g2_blocks(ctx, n_nodes)), th, 0, ctx->stream, d_a1, d_beta, d_alpha1, (const double*)d_graw, d_label,
                       (const uint32_t*)d_ref, d_gmap, n_feat, (uint32_t)n_a, n_nodes, d_eff1, d_eff2, d_comp1, d_comp2);
    PDS_HIP_CHECK(hipGetLastError());
    return PDS_OK;
}

template int launch_within2_effects<double>(pds_ctx*, const double*, const double*, const double*, const double*, const uint32_t*, const int64_t*, int,
                                            int64_t, int64_t, double*, uint32_t*, double*, double*, int32_t*, int32_t*);
template int launch_within2_effects<float>(pds_ctx*, const double*, const double*, const double*, const double*, const uint32_t*, const int64_t*, int,
                                           int64_t, int64_t, double*, uint32_t*, float*, float*, int32_t*, int32_t*);

}  // namespace pds
