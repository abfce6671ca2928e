// capi_group_chunks.hpp -- the host side of "one wave per group, long groups cut into row chunks", once: the offsets of contiguous
// groups are validated, the empty groups are taken out and the groups above the split threshold are listed as chunks; and, for the
// pipelines whose kernels read MixedChunks, the workspace of the shared part is sized, carved and filled.
// Part of the one translation unit capi.hip (included there, inside namespace pds, in dependency order).  Host code only.
//
// Who uses which step:
//   plan_group_chunks (+ upload_cluster_chunks)   the cluster-robust report (capi_report_cluster.hpp) and the robust GLM report
//                                                 (capi_glm_sandwich.hpp): ClusterChunks out of ctx->ws / a caller's Bump
//   plan_group_frame                              the plan step: the offsets on the host + plan_group_chunks, owned by one object.  The
//                                                 two-key fit (capi_within2.hpp) uses this step alone; its workspace is its own
//   plan_group_frame, then open_group_frame       the mixed model (capi_mixed.hpp), the fixed-effects regression (capi_within.hpp) and the
//                                                 fixed-effects GLM (capi_glm_within.hpp).  Two steps, because each caller refuses
//                                                 frames between them (too few rows, too few groups) from what the plan counted
//
// Empty groups are dropped HERE (equal neighbours of the offsets), so that they cannot change which wave sums what: the device works
// on the non-empty groups alone and gives the bits it gives without them.  The chunk order (groups in order, a group's chunks in row
// order) is the order the long-group kernels add in.
#pragma once

struct GroupChunkPlan {
    int64_t n_obs = 0;                   // rows inside the groups
    int64_t n_nonempty = 0;              // groups with rows = the groups the device works on
    const int64_t* h_off = nullptr;      // their n_nonempty + 1 offsets: the caller's array, or `compact`
    bool upload_off = false;             // the device needs a copy of h_off (the caller's offsets are on the host, or groups were dropped)
    std::vector<int64_t> compact, gmap;  // gmap (on request, when groups were dropped): the place of a kept group among the caller's
    std::vector<int64_t> hc[4], hl[5];   // chunk: r0, n, group, first row of the group; long group: g, first chunk, chunks, first row, rows
    bool dropped() const { return !compact.empty(); }
    int64_t n_chunks() const { return (int64_t)hc[0].size(); }
    int64_t n_long() const { return (int64_t)hl[0].size(); }
};

// h_off: n_groups + 1 host offsets into a frame of n_rows rows.  cover: the groups are [0, n_rows) exactly; otherwise they lie
// inside the frame.  Offsets that decrease or break that rule: PDS_ERR_INVALID with the text bad_off.  Groups above `split` rows are
// cut into chunks of `split` rows (the last one shorter).  The plan points into h_off: it lives no longer than that array.
static int plan_group_chunks(const int64_t* h_off, int64_t n_groups, int64_t n_rows, int64_t split, bool cover, bool offsets_on_host,
                             bool want_gmap, const char* bad_off, GroupChunkPlan& pl) {
    if (cover ? (h_off[0] != 0 || h_off[n_groups] != n_rows) : (h_off[0] < 0 || h_off[n_groups] > n_rows)) return fail(PDS_ERR_INVALID, bad_off);
    int64_t n_nonempty = 0;  // (a local: the walks over a million groups stay in registers)
    for (int64_t g = 0; g < n_groups; ++g) {
        const int64_t n = h_off[g + 1] - h_off[g];
        if (n < 0 || h_off[g + 1] > n_rows) return fail(PDS_ERR_INVALID, bad_off);
        n_nonempty += n > 0;
    }
    pl.n_obs = h_off[n_groups] - h_off[0];  // (the sum of the row counts, none of them negative)
    pl.n_nonempty = n_nonempty;
    pl.upload_off = offsets_on_host || n_nonempty != n_groups;
    if (n_nonempty != n_groups) {
        pl.compact.reserve((size_t)n_nonempty + 1);
        if (want_gmap) pl.gmap.reserve((size_t)n_nonempty);
        pl.compact.push_back(h_off[0]);
        for (int64_t g = 0; g < n_groups; ++g)
            if (h_off[g + 1] != pl.compact.back()) {
                pl.compact.push_back(h_off[g + 1]);
                if (want_gmap) pl.gmap.push_back(g);
            }
        h_off = pl.compact.data();
    }
    pl.h_off = h_off;
    for (int64_t g = 0; g < n_nonempty; ++g) {
        const int64_t r0 = h_off[g], n = h_off[g + 1] - r0;
        if (n <= split) continue;
        const int64_t k = (n + split - 1) / split;
        pl.hl[0].push_back(g);
        pl.hl[1].push_back(pl.n_chunks());
        pl.hl[2].push_back(k);
        pl.hl[3].push_back(r0);
        pl.hl[4].push_back(n);
        for (int64_t i = 0; i < k; ++i) {
            pl.hc[0].push_back(r0 + i * split);
            pl.hc[1].push_back(std::min<int64_t>(split, n - i * split));
            pl.hc[2].push_back(g);
            pl.hc[3].push_back(r0);
        }
    }
    return PDS_OK;
}

// the plan's lists -> the device as the ClusterChunks the cluster kernels read (cluster_meat.hip, glm_meat.hip: per chunk r0 and n, per
// long cluster its first chunk and its chunks: no more is sent) and room for the chunk scores; nothing is taken without chunks.
// take(bytes) hands out device memory (ws_take of ctx->ws, or a Bump).  The copies are asynchronous: the plan outlives the caller's
// next stream synchronisation.
template <typename Take>
static int upload_cluster_chunks(pds_ctx* ctx, Take&& take, const GroupChunkPlan& pl, ClusterChunks& ch) {
    ch.n_chunks = pl.n_chunks();
    ch.n_long = pl.n_long();
    if (ch.n_chunks == 0) return PDS_OK;
    const std::vector<int64_t>* lists[4] = {&pl.hc[0], &pl.hc[1], &pl.hl[1], &pl.hl[2]};
    const int64_t* d[4];
    for (int i = 0; i < 4; ++i) {
        const std::vector<int64_t>& h = *lists[i];
        int64_t* t = reinterpret_cast<int64_t*>(take(h.size() * 8));
        PDS_HIP_CHECK(hipMemcpyAsync(t, h.data(), h.size() * 8, hipMemcpyHostToDevice, ctx->stream));
        d[i] = t;
    }
    ch.d_chunk_r0 = d[0], ch.d_chunk_n = d[1], ch.d_long_c0 = d[2], ch.d_long_nc = d[3];
    ch.d_scores = reinterpret_cast<double*>(take((size_t)ch.n_chunks * kClusterScoreStride * 8));
    return PDS_OK;
}

// the plan's lists -> the device, out of w, as the MixedChunks the kernels of mixed.hip and within_pass.hip read (nc = p + 1 columns:
// d_sums); nothing is taken without chunks.  The copies are asynchronous: the plan outlives the caller's next stream synchronisation.
static int upload_mixed_chunks(pds_ctx* ctx, Bump& w, const GroupChunkPlan& pl, int nc, MixedChunks& ch) {
    ch.n_chunks = pl.n_chunks();
    ch.n_long = pl.n_long();
    if (ch.n_chunks == 0) return PDS_OK;
    auto up = [&](const std::vector<int64_t>& h, const int64_t*& d) -> int {
        int64_t* t = w.take<int64_t>(h.size());
        PDS_HIP_CHECK(hipMemcpyAsync(t, h.data(), h.size() * 8, hipMemcpyHostToDevice, ctx->stream));
        d = t;
        return PDS_OK;
    };
    const int64_t** dc[4] = {&ch.d_chunk_r0, &ch.d_chunk_n, &ch.d_chunk_g, &ch.d_chunk_first};
    const int64_t** dl[5] = {&ch.d_long_g, &ch.d_long_c0, &ch.d_long_nc, &ch.d_long_first, &ch.d_long_n};
    for (int i = 0; i < 4; ++i)
        if (int rc = up(pl.hc[i], *dc[i])) return rc;
    for (int i = 0; i < 5; ++i)
        if (int rc = up(pl.hl[i], *dl[i])) return rc;
    ch.d_sums = w.take<double>((size_t)ch.n_chunks * nc);
    ch.d_varies = w.take<unsigned>((size_t)ch.n_chunks);
    return PDS_OK;
}

// ---- the plan step: the offsets where the host can read them (host_offsets) and their plan, in one object.  Not copyable: the plan
// points into `fetched` (or into the caller's host array), which has to stay where it is while the plan is used.
struct GroupFramePlan {
    GroupChunkPlan pl;
    const int64_t* offsets = nullptr;  // the caller's n_groups + 1 offsets, where the caller has them
    std::vector<int64_t> fetched;      // the host copy of device offsets
    GroupFramePlan() = default;
    GroupFramePlan(const GroupFramePlan&) = delete;
    GroupFramePlan& operator=(const GroupFramePlan&) = delete;
};

// offsets: n_groups + 1 offsets in `space`; the other arguments are plan_group_chunks'
static int plan_group_frame(pds_ctx* ctx, const int64_t* offsets, int64_t n_groups, int64_t n_rows, pds_space space, int64_t split, bool cover,
                            bool want_gmap, const char* bad_off, GroupFramePlan& gp) {
    const int64_t* h_off = nullptr;
    if (int rc = host_offsets(ctx, offsets, n_groups, space, gp.fetched, h_off)) return rc;
    gp.offsets = offsets;
    return plan_group_chunks(h_off, n_groups, n_rows, split, cover, space == PDS_HOST, want_gmap, bad_off, gp.pl);
}

// ---- the frame step.  What a caller needs from the shared part of the workspace:
struct GroupFrameNeeds {
    int n_means = 1;          // tables of n_feat + 1 means per group (2: an iteration reads one and writes the other)
    size_t n_rec = 0;         // records of the caller's widest launch (its max over the *_blocks functions)
    int sum_cols = 0;         // columns of the chunk sums (MixedChunks::d_sums)
    bool scores = false;      // a score of kClusterScoreStride doubles per chunk
    bool gmap = false;        // the device needs the places of the kept groups among the caller's (sent when groups were dropped; the plan has them)
    size_t caller_bytes = 0;  // what the caller takes from `w` afterwards (Bump::up per slice)
};

constexpr int kGroupBetaSlot = kMaxFeatSmall + 2;  // doubles: [1, x_0 .. x_15, y] at the most

// The shared part on the device.  tbl and (through gp) the plan's lists are sources of asynchronous copies: both outlive the caller's
// next stream synchronisation.
template <typename T>
struct GroupFrame {
    Bump w{};                    // behind the shared part: the caller's own slices, caller_bytes of them
    std::vector<const T*> tbl;   // the host copy of d_tbl
    const T** d_tbl = nullptr;   // the frame in kernel order (kernel_order_table)
    const int64_t* d_off = nullptr;   // the n_nonempty + 1 offsets of the non-empty groups
    const int64_t* d_gmap = nullptr;  // null unless asked for and groups were dropped
    double* d_means[2] = {nullptr, nullptr};
    double *d_partials = nullptr, *d_stage = nullptr, *d_rec = nullptr;  // n_rec records, their first-stage sums (launch_sum_records), the one record
    unsigned* d_flags = nullptr;  // 64 words
    double* d_beta = nullptr;     // kGroupBetaSlot doubles
    MixedChunks ch;
    double* d_scores = nullptr;   // null without chunks or unless asked for
};

// cols: [y, x1..xp] in `space`; trailing (nullable): the pair {weights, offset}, each nullable, in `space` -- they are staged behind
// the frame and become the two table entries behind y (kernel_order_table).  The block is ctx->wkeyed: a by-key caller's ordered frame
// lives in ctx->keyed, the two-key fit's tables in ctx->ws.
template <typename T>
static int open_group_frame(pds_ctx* ctx, const GroupFramePlan& gp, const T* const* cols, const T* const* trailing, int n_feat, int64_t n_rows,
                            pds_space space, const GroupFrameNeeds& nd, GroupFrame<T>& f) {
    const GroupChunkPlan& pl = gp.pl;
    const auto up = Bump::up;
    const size_t ng = (size_t)pl.n_nonempty, n_chunks = (size_t)pl.n_chunks(), n_long = (size_t)pl.n_long();
    const size_t nc = (size_t)n_feat + 1, n_stage = nd.n_rec / 64 + 1, n_tbl = trailing ? 20 : 18;
    const bool send_gmap = nd.gmap && pl.dropped();
    std::vector<const T*> src = frame_cols<T>(cols, n_feat);  // reference order [y, x1..xp (, weights) (, offset)]
    for (int k = 0; trailing && k < 2; ++k)
        if (trailing[k]) src.push_back(trailing[k]);
    // one term per slice taken below, in the order they are taken
    size_t need = 4096 + (space == PDS_HOST ? src.size() * up((size_t)n_rows * sizeof(T)) : 0) + up(n_tbl * sizeof(T*)) +
                  (pl.upload_off ? up((ng + 1) * 8) : 0) + (send_gmap ? up(ng * 8) : 0) + (size_t)nd.n_means * up(nc * ng * 8) +
                  up(nd.n_rec * kMixedRecStride * 8) + up(n_stage * kMixedRecStride * 8) + up(kMixedRecStride * 8) + up(64 * sizeof(unsigned)) +
                  up(kGroupBetaSlot * 8);
    if (n_chunks > 0)  // (upload_mixed_chunks: four lists per chunk, five per long group, the sums, the varies words)
        need += 4 * up(n_chunks * 8) + 5 * up(n_long * 8) + up(n_chunks * (size_t)nd.sum_cols * 8) + up(n_chunks * sizeof(unsigned)) +
                (nd.scores ? up(n_chunks * kClusterScoreStride * 8) : 0);
    if (int rc = ensure_ws(ctx, ctx->wkeyed, need + nd.caller_bytes)) return rc;
    Bump w{static_cast<char*>(ctx->wkeyed.ptr)};
    if (space == PDS_HOST)
        if (int rc = cols_to_device<T>(ctx, w, src, n_rows)) return rc;
    const T* d_wo[2] = {nullptr, nullptr};  // (the staged columns behind the frame, in the order they were appended)
    for (size_t k = 0, at = nc; trailing && k < 2; ++k)
        if (trailing[k]) d_wo[k] = src[at++];
    src.resize(nc);
    if (int rc = kernel_order_table<T>(ctx, w, src, n_feat, f.tbl, f.d_tbl, trailing ? d_wo : nullptr)) return rc;
    f.d_off = gp.offsets;
    if (pl.upload_off) {
        int64_t* t = w.take<int64_t>(ng + 1);
        PDS_HIP_CHECK(hipMemcpyAsync(t, pl.h_off, (ng + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
        f.d_off = t;
    }
    if (send_gmap) {
        int64_t* t = w.take<int64_t>(ng);
        PDS_HIP_CHECK(hipMemcpyAsync(t, pl.gmap.data(), ng * 8, hipMemcpyHostToDevice, ctx->stream));
        f.d_gmap = t;
    }
    for (int k = 0; k < nd.n_means; ++k) f.d_means[k] = w.take<double>(nc * ng);
    f.d_partials = w.take<double>(nd.n_rec * kMixedRecStride);
    f.d_stage = w.take<double>(n_stage * kMixedRecStride);
    f.d_rec = w.take<double>(kMixedRecStride);
    f.d_flags = w.take<unsigned>(64);
    f.d_beta = w.take<double>(kGroupBetaSlot);
    if (int rc = upload_mixed_chunks(ctx, w, pl, nd.sum_cols, f.ch)) return rc;
    if (nd.scores && n_chunks > 0) f.d_scores = w.take<double>(n_chunks * kClusterScoreStride);
    f.w = w;
    return PDS_OK;
}
