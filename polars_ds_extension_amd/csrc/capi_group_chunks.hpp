// capi_group_chunks.hpp -- the host side of "one wave per group, long groups cut into row chunks", once: the offsets of contiguous
// groups are validated, the empty groups are taken out and the groups above the split threshold are listed as chunks.  Used by the
// mixed model (capi_mixed.hpp), the cluster-robust report (capi_report_cluster.hpp) and the fixed-effects regression (capi_within.hpp).
// Part of the one translation unit capi.hip (included there, inside namespace pds, in dependency order).  Host code only.
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
