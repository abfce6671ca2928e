// capi_within_cluster.hpp -- fixed-effects regression with standard errors clustered on ANY key (pds_lin_reg_within_cl_* /
// pds_lin_reg_within2_cl_*): the host side of within_cluster.hip.  It hangs off within_impl (capi_within.hpp), the final stage of the
// one-factor AND the two-factor fit, through the struct WithinCluster, which is absent by default: without it every call launches the
// kernels it launched before and returns the same bits.
// Part of the one translation unit capi.hip (included there, inside namespace pds, in dependency order).
//
// DEFINITIONS (what this file computes; no equivalence with any package's small-sample conventions is claimed).  x~, y~: the columns
// projected off the absorbed dummies; B = (X~'X~)^-1; e = y~ - X~ beta -- all formed by the fit as without a cluster key (beta, r2,
// pred, resid, n_iter: the same bits).  The cluster key: dense int32 codes per row in [0, n_levels), the caller's row order,
// `space`-resident.  A code that no row uses counts nowhere; a code outside the range is PDS_ERR_INVALID, found by a kernel that reads
// nothing else, before anything is indexed by a code.  Gc: the occupied codes.
//     s_c = sum_{i in c} x~_i e_i,   M = sum_c s_c s_c'
//     PDS_CLUSTER0  V = B M B
//     PDS_CLUSTER   V times Gc / (Gc - 1) * (n - 1) / (n - K),  K = p + sum_f (nested_f ? 0 : A_f) + (some factor nested ? 1 : 0),
//                   A_1 = G1, A_2 = G2 - C (= A - G1).  Factor f is NESTED when every occupied level of it has all its rows in one
//                   cluster: its effects, nested in the clusters, are not counted, and the one intercept is counted in their place.
//                   One key clustered on itself: K = p + 1 (capi_within.hpp's definition); two keys clustered on the first:
//                   K = p + 1 + (A - G1) (capi_within2.hpp's); no factor nested: K = p + A.
//     t, p and the 95 % interval: Student t, Gc - 1 degrees of freedom.  Gc < 2: PDS_ERR_INVALID.  PDS_SE with a cluster key:
//     PDS_ERR_INVALID.
//
// Stages (within_cluster_open before the fit's passes, within_cluster_meat after the within pass):
//   1. the codes on the device, their range check, and -- the by-key forms -- their gather through the row permutation
//      (launch_within2_gather_codes): cluster codes in within_impl's row order;
//   2. the row order by cluster: launch_within2_order (stable radix sort of (code, row)) and launch_within2_level_starts; the cluster
//      sizes are exact integers from the run boundaries; the host builds one chunk list per occupied cluster, a chunk at most
//      kWithin2GatherChunkRows rows ("within_split_rows" rows if that is smaller) -- factor 2's rule;
//   3. nestedness (launch_cluster_nested): two integer flags read by the host;
//   4. the row scores, staged row-major (launch_within_row_scores); 5. the chunk scores and 6. the meat (launch_cluster_gather_meat);
//   7. the sandwich on the host from the inverse of the solve, in within_impl's epilogue.
// The staging costs one streamed write of n x p x 8 bytes and that much workspace (ensure_ws: a workspace the device cannot hold
// fails with the allocation's error).  Fewer than 2^31 rows per call (the row index is 32 bits wide).
#pragma once

// rows of a gathered chunk at most: every level of factor 2 (capi_within2.hpp) and every cluster is cut into chunks of this many rows
// of the ordered row index ("within_split_rows", if smaller, takes its place)
constexpr int64_t kWithin2GatherChunkRows = 1024;

struct WithinCluster {
    const int32_t* codes = nullptr;         // [n_rows] the caller's row order, in code_space
    pds_space code_space = PDS_HOST;
    int64_t n_levels = 0;
    const uint32_t* d_code_perm = nullptr;  // nullable: row r of the frame within_impl walks is row d_code_perm[r] of the caller's
    // two absorbed factors (capi_within2.hpp sets these; null: one factor): the rows in ascending code-2 order and the level starts
    const uint32_t* d_idx2 = nullptr;
    const uint32_t* d_start2 = nullptr;
    int64_t n_levels2 = 0;
    // out
    int64_t n_clusters = 0;
    int nested1 = 0, nested2 = 0;
};

// what the open stage leaves on the device for the meat stage
struct WithinClusterDev {
    const int32_t* d_codes = nullptr;  // frame order
    const uint32_t* d_idx = nullptr;   // the rows in cluster order
    const int64_t *d_chunk_pos = nullptr, *d_chunk_n = nullptr, *d_cl_c0 = nullptr, *d_cl_nc = nullptr;
    int64_t n_chunks = 0, n_clusters = 0;
    double *d_rows = nullptr, *d_scores = nullptr;
    int* d_flags = nullptr;
};

static int within_cluster_check(const WithinCluster* cl, int se_type, int64_t n_rows, bool want_se) {
    if (!cl) return PDS_OK;
    if (!cl->codes) return fail(PDS_ERR_INVALID, "null argument");
    if (se_type == PDS_SE) return fail(PDS_ERR_INVALID, "fixed-effects regression: a cluster key goes with PDS_CLUSTER or PDS_CLUSTER0");
    if (!want_se) return fail(PDS_ERR_INVALID, "fixed-effects regression: a cluster key goes with std_err .. ci_upper");
    if (cl->n_levels < 1 || cl->n_levels >= (1ll << 31)) return fail(PDS_ERR_INVALID, "fixed-effects regression: the cluster key's n_levels is in [1, 2^31)");
    if (n_rows >= (1ll << 31)) return fail(PDS_ERR_UNSUPPORTED, "fixed-effects regression with a cluster key: fewer than 2^31 rows per call");
    return PDS_OK;
}

static int64_t within_cluster_chunk_rows(int64_t split) { return std::max<int64_t>(64, std::min<int64_t>(split, kWithin2GatherChunkRows)); }

// device bytes the two stages take out of within_impl's workspace
static size_t within_cluster_bytes(const WithinCluster& cl, int64_t n, int p, int64_t split) {
    const auto up = Bump::up;
    const int64_t lev_cap = std::min<int64_t>(n, cl.n_levels), c_cap = n / within_cluster_chunk_rows(split) + lev_cap + 1;
    return (cl.code_space == PDS_HOST ? up((size_t)n * 4) : 0) + (cl.d_code_perm ? up((size_t)n * 4) : 0) + 3 * up((size_t)n * 4) +
           up(within2_order_temp_bytes(n)) + up((size_t)(cl.n_levels + 1) * 4) + up(256) + up((size_t)n * cluster_row_stride(p) * 8) +
           2 * up((size_t)c_cap * 8) + 2 * up((size_t)lev_cap * 8) + up((size_t)c_cap * kClusterScoreStride * 8) + 4096;
}

// stages 1 and 2.  Blocking: the range flag, then the level starts come back to the host.
static int within_cluster_open(pds_ctx* ctx, Bump& w, WithinCluster& cl, int64_t n, int p, int64_t split, WithinClusterDev& cd) {
    const int32_t* d_in = cl.codes;
    if (cl.code_space == PDS_HOST) {
        int32_t* t = w.take<int32_t>((size_t)n);
        PDS_HIP_CHECK(hipMemcpyAsync(t, cl.codes, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
        d_in = t;
    }
    cd.d_flags = w.take<int>(64);
    {  // the range BEFORE any kernel indexes anything by a code
        int bad = 0;
        PDS_HIP_CHECK(hipMemsetAsync(cd.d_flags, 0, sizeof(int), ctx->stream));
        if (int rc = launch_within2_range_check(ctx, d_in, n, cl.n_levels, cd.d_flags)) return rc;
        PDS_HIP_CHECK(hipMemcpyAsync(&bad, cd.d_flags, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        PDS_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        if (bad) return fail(PDS_ERR_INVALID, "fixed-effects regression: a code of the cluster key is outside [0, n_levels)");
    }
    cd.d_codes = d_in;
    if (cl.d_code_perm) {
        int32_t* t = w.take<int32_t>((size_t)n);
        if (int rc = launch_within2_gather_codes(ctx, d_in, cl.d_code_perm, n, t)) return rc;
        cd.d_codes = t;
    }
    uint32_t *iota = w.take<uint32_t>((size_t)n), *sorted = w.take<uint32_t>((size_t)n), *idx = w.take<uint32_t>((size_t)n);
    const size_t sort_temp = within2_order_temp_bytes(n);
    void* temp = w.take<char>(sort_temp);
    uint32_t* d_start = w.take<uint32_t>((size_t)cl.n_levels + 1);
    if (int rc = launch_within2_order(ctx, cd.d_codes, n, cl.n_levels, iota, sorted, idx, temp, sort_temp)) return rc;
    cd.d_idx = idx;
    if (int rc = launch_within2_level_starts(ctx, sorted, n, cl.n_levels, d_start)) return rc;
    std::vector<uint32_t> start;
    try {
        start.resize((size_t)cl.n_levels + 1);
    } catch (const std::bad_alloc&) {
        return fail(PDS_ERR_INVALID, "fixed-effects regression: no host memory for the level counts of the cluster key");
    }
    PDS_HIP_CHECK(hipMemcpyAsync(start.data(), d_start, start.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
    PDS_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    // one chunk list per occupied cluster, the chunks in row order: the order the meat kernel adds in
    const int64_t chunk = within_cluster_chunk_rows(split);
    std::vector<int64_t> c_pos, c_n, l_c0, l_nc;
    int64_t pos = 0;
    for (int64_t l = 0; l < cl.n_levels; ++l) {
        const int64_t m = (int64_t)start[(size_t)l + 1] - (int64_t)start[(size_t)l];
        if (m == 0) continue;
        const int64_t k = (m + chunk - 1) / chunk;
        l_c0.push_back((int64_t)c_pos.size());
        l_nc.push_back(k);
        for (int64_t i = 0; i < k; ++i) {
            c_pos.push_back(pos + i * chunk);
            c_n.push_back(std::min<int64_t>(chunk, m - i * chunk));
        }
        pos += m;
    }
    cd.n_clusters = cl.n_clusters = (int64_t)l_c0.size();
    cd.n_chunks = (int64_t)c_pos.size();
    if (cd.n_clusters < 2) return fail(PDS_ERR_INVALID, "standard errors clustered on a key need at least two occupied clusters");
    auto put = [&](const std::vector<int64_t>& h, const int64_t*& d) -> int {
        int64_t* t = w.take<int64_t>(h.size());
        PDS_HIP_CHECK(hipMemcpyAsync(t, h.data(), h.size() * 8, hipMemcpyHostToDevice, ctx->stream));
        d = t;
        return PDS_OK;
    };
    if (int rc = put(c_pos, cd.d_chunk_pos)) return rc;
    if (int rc = put(c_n, cd.d_chunk_n)) return rc;
    if (int rc = put(l_c0, cd.d_cl_c0)) return rc;
    if (int rc = put(l_nc, cd.d_cl_nc)) return rc;
    cd.d_scores = w.take<double>((size_t)cd.n_chunks * kClusterScoreStride);
    cd.d_rows = w.take<double>((size_t)n * cluster_row_stride(p));
    PDS_HIP_CHECK(hipStreamSynchronize(ctx->stream));  // (the lists: sources of the copies)
    return PDS_OK;
}

// stages 3 - 6: the nestedness flags into cl, the meat into one record at d_rec (read by the caller after it synchronises)
template <typename T>
static int within_cluster_meat(pds_ctx* ctx, WithinCluster& cl, const WithinClusterDev& cd, const T* const* d_tbl, int p, const int64_t* d_off,
                               int64_t n_groups, int64_t split, const MixedChunks& ch, const double* d_beta, const double* d_means,
                               double* d_partials, double* d_stage, double* d_rec) {
    if (int rc = launch_cluster_nested(ctx, d_off, n_groups, cl.d_idx2 ? cl.d_start2 : nullptr, cl.n_levels2, cl.d_idx2, cd.d_codes, cd.d_flags)) return rc;
    int flags[2] = {0, 0};
    PDS_HIP_CHECK(hipMemcpyAsync(flags, cd.d_flags, sizeof(flags), hipMemcpyDeviceToHost, ctx->stream));
    if (int rc = launch_within_row_scores<T>(ctx, d_tbl, p, d_off, n_groups, split, ch, d_beta, d_means, cd.d_rows)) return rc;
    if (int rc = launch_cluster_gather_meat(ctx, p, cd.d_rows, cd.d_idx, cd.d_chunk_pos, cd.d_chunk_n, cd.n_chunks, cd.d_cl_c0, cd.d_cl_nc, cd.n_clusters,
                                            cd.d_scores, d_partials, d_stage, d_rec))
        return rc;
    PDS_HIP_CHECK(hipStreamSynchronize(ctx->stream));  // (flags: the target of the copy)
    cl.nested1 = flags[0] == 0;
    cl.nested2 = cl.d_idx2 ? flags[1] == 0 : 0;
    return PDS_OK;
}
