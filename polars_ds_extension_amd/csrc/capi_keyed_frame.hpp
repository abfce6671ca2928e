// capi_keyed_frame.hpp -- an int64 key column in any row order + a frame -> contiguous groups in ascending key order: the stage every
// by-key entry point starts with (pds_lr_by_key*, pds_*_report_by_key*, pds_{rolling,recursive}_lr_by_key*, pds_glm_irls_by_key*,
// pds_lr_rcond_by_key*, pds_mixed_reml_by_key*), and the host-side pieces the grouped pipelines share
// Part of the one translation unit capi.hip (included there, inside namespace pds, in dependency order): the entry-point
// pipelines are templates with internal linkage, split by concern, not by compilation unit.
//
// Two steps, because a caller may pick another route between them (lr_by_key_impl's partition route):
//   A  keyed_order_check: keys on the device, one pass for order flag, key range and the run marks of an ordered column
//   B  keyed_frame_bytes + keyed_frame_build: the caller adds its own output staging to the bytes, calls ensure_ws(ctx->keyed) ONCE
//      (it may move the block) and hands the build a Bump over that block, from which it goes on taking its own slices afterwards
// keyed_frame_open is A and B in one call, for every caller that picks no route between them.
//
// Outputs that may live on the host are declared once in a StagedOuts (capi_staged_out.hpp: bytes, device pointers) and come back
// through staged_copy_back; host_offsets and check_cols are the offsets fetch and the column check of the contiguous-group forms.
#pragma once

// every staged output the caller gave a host buffer for: `units` units of it back to the caller (asynchronous, no synchronisation)
static int staged_copy_back(pds_ctx* ctx, const StagedOuts& so, size_t units) {
    for (int i = 0; i < so.n; ++i)
        if (so.outs[i].back)
            PDS_HIP_CHECK(hipMemcpyAsync(so.outs[i].user, so.dev(i), units * so.outs[i].unit_bytes, hipMemcpyDeviceToHost, ctx->stream));
    return PDS_OK;
}

// group offsets where the host can read them: device offsets are fetched into `store` (one copy + a synchronisation), host offsets
// are the caller's own.  Validation is the caller's (the rules and their messages differ).
static int host_offsets(pds_ctx* ctx, const int64_t* offsets, int64_t n_groups, pds_space space, std::vector<int64_t>& store, const int64_t*& h_off) {
    h_off = offsets;
    if (space == PDS_HOST) return PDS_OK;
    store.resize((size_t)n_groups + 1);
    PDS_HIP_CHECK(hipMemcpyAsync(store.data(), offsets, store.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
    PDS_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    h_off = store.data();
    return PDS_OK;
}

// every column [y, x1..xp] of the frame is there
template <typename T>
static int check_cols(const T* const* cols, int n_feat) {
    for (int c = 0; c <= n_feat; ++c)
        if (!cols[c]) return fail(PDS_ERR_INVALID, "null argument");
    return PDS_OK;
}

// reference order [y, x1..xp (, w)]: a weight column rides through the staging, the sort and the gather as one more column
template <typename T>
static std::vector<const T*> frame_cols(const T* const* cols, int n_feat, const T* weights = nullptr) {
    std::vector<const T*> src(cols, cols + n_feat + 1);
    if (weights) src.push_back(weights);
    return src;
}

// host columns -> slices of `w` (asynchronous); src then holds the device pointers
template <typename T>
static int cols_to_device(pds_ctx* ctx, Bump& w, std::vector<const T*>& src, int64_t n_rows) {
    for (const T*& col : src) {
        T* d = w.take<T>((size_t)n_rows);
        PDS_HIP_CHECK(hipMemcpyAsync(d, col, (size_t)n_rows * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
        col = d;
    }
    return PDS_OK;
}

// device pointer table of a frame in the kernels' order x_0 .. x_{p-1}, y, padded to 18 entries.  `tbl` is the source of an
// asynchronous copy: the caller keeps it alive until it has synchronised the stream.  `trailing` (nullable): two more entries behind
// y, each of which may be null -- the prior weights and the offsets of the weighted / offset GLM kernels; the table then has 20.
template <typename T>
static int kernel_order_table(pds_ctx* ctx, Bump& w, const std::vector<const T*>& src, int n_feat, std::vector<const T*>& tbl,
                              const T**& d_tbl, const T* const* trailing = nullptr) {
    tbl.assign(trailing ? 20 : std::max<size_t>(src.size(), 18), src[0]);
    for (int c = 0; c < n_feat; ++c) tbl[c] = src[c + 1];
    tbl[n_feat] = src[0];
    if (trailing) {
        tbl[n_feat + 1] = trailing[0];
        tbl[n_feat + 2] = trailing[1];
    }
    d_tbl = w.take<const T*>(tbl.size());
    PDS_HIP_CHECK(hipMemcpyAsync(d_tbl, tbl.data(), sizeof(T*) * tbl.size(), hipMemcpyHostToDevice, ctx->stream));
    return PDS_OK;
}

// ---- step A
struct KeyOrder {
    bool sorted = false;
    int64_t mm[2] = {0, 0};   // smallest / largest key
    int64_t n_runs = 0;       // keys that differ from their successor: n_groups - 1 of an ordered column
    bool hist_taken = false;  // d_slots holds the bucket histogram of (key >> hist_shift)
    const int64_t* d_keys = nullptr;
    int64_t *d_state = nullptr, *d_minmax = nullptr;  // the order check's 8 slots; {min, max} on the device
    uint32_t *d_run_counts = nullptr, *d_run_prefix = nullptr;
    unsigned long long* d_run_masks = nullptr;
    unsigned* d_slots = nullptr;  // kKeySlots x 8 counters (null without the slot block)
};

// slot_block: room for the order check's bucket histogram; hist_shift >= 0: take it along (keys_order_minmax decides, ko.hist_taken)
static int keyed_order_check(pds_ctx* ctx, const int64_t* keys, int64_t n_rows, pds_space space, bool slot_block, int hist_shift,
                             KeyOrder& ko) {
    ko.d_keys = keys;
    if (space == PDS_HOST) {
        if (int rc = ensure_ws(ctx, ctx->stage, Bump::up((size_t)n_rows * 8) + 256)) return rc;
        PDS_HIP_CHECK(hipMemcpyAsync(ctx->stage.ptr, keys, (size_t)n_rows * 8, hipMemcpyHostToDevice, ctx->stream));
        ko.d_keys = static_cast<const int64_t*>(ctx->stage.ptr);
    }
    // order flag + key range + the run counts of the order check (keyed.hip) live in ctx->solve_ws: they outlive the sizing of ctx->keyed
    const size_t runs = Bump::up((key_run_slots(n_rows) + 1) * sizeof(uint32_t));
    const size_t slots = slot_block ? Bump::up((size_t)kKeySlots * 8 * sizeof(unsigned)) : 0;
    if (int rc = ensure_ws(ctx, ctx->solve_ws, 8192 + 2 * runs + slots + key_run_mask_bytes(n_rows))) return rc;
    char* sw = static_cast<char*>(ctx->solve_ws.ptr);
    ko.d_state = reinterpret_cast<int64_t*>(sw + 256);
    ko.d_minmax = ko.d_state + 2;
    ko.d_run_counts = reinterpret_cast<uint32_t*>(sw + 4096);
    ko.d_run_prefix = reinterpret_cast<uint32_t*>(sw + 4096 + runs);
    ko.d_slots = slot_block ? reinterpret_cast<unsigned*>(sw + 4096 + 2 * runs) : nullptr;
    ko.d_run_masks = reinterpret_cast<unsigned long long*>(sw + 4096 + 2 * runs + slots);
    if (int rc = keys_order_minmax(ctx, ko.d_keys, n_rows, ko.d_state, &ko.sorted, ko.mm, ko.d_run_counts, ko.d_run_masks, &ko.n_runs,
                                   hist_shift, ko.d_slots, &ko.hist_taken))
        return rc;
    // ORDERED keys have no row bound of their own (the order check, the run marks and the fits index rows with 64 bits; 2^31 + rows x 8
    // f64 features fit this device's HBM, and the reference's series_to_mat_for_lr has no bound either, linear_regression.rs:151-267);
    // the routes for keys in ANY order carry 32-bit row ranks through the sort / the partition
    if (!ko.sorted && n_rows >= (1ll << 31)) return fail(PDS_ERR_UNSUPPORTED, "keyed grouping of unordered keys: fewer than 2^31 rows per call");
    return PDS_OK;
}

// ---- step B
template <typename T>
struct KeyedFrame {
    std::vector<const T*> src;         // in: the caller's columns (frame_cols); out: the ordered frame, device resident
    const uint32_t* d_perm = nullptr;  // row r of the ordered frame is row d_perm[r] of the caller's; null when nothing moved
    const int64_t* d_keys = nullptr;   // the ordered key column
    int64_t *d_unique = nullptr, *d_offsets = nullptr;
    int64_t ng = 0;
};

// bytes of ctx->keyed the build takes: [runs, temp] [raw columns (host frames)] [sorted keys, index in/out, gathered columns, records
// (unordered keys)].  run_cap: capacity of unique keys / offsets -- ordered keys: the order check has counted them (n_runs + 1, or
// the caller's bound if smaller); unordered: one per row.
template <typename T>
static size_t keyed_frame_bytes(bool sorted, int64_t n_rows, int nc, pds_space space, int64_t run_cap) {
    const size_t key_bytes = Bump::up((size_t)n_rows * 8), col_bytes = Bump::up((size_t)n_rows * sizeof(T)), idx_bytes = Bump::up((size_t)n_rows * 4);
    size_t need = (sorted ? keyed_ordered_temp_bytes(n_rows) : keyed_temp_bytes(n_rows)) + 3 * Bump::up((size_t)(run_cap + 1) * 8) + 8192;
    if (space == PDS_HOST) need += col_bytes * nc;
    if (!sorted) need += 2 * key_bytes + 2 * idx_bytes + col_bytes * nc + Bump::up((size_t)n_rows * nc * sizeof(T)) + Bump::up(2 * (size_t)nc * sizeof(T*)) + 1024;
    return need;
}

// Ordered keys: the order check's run marks give the offsets and nothing moves.  Otherwise the stable radix sort of (key, row) pairs
// (rows keep their order inside a group) and the frame gather.  *n_groups (nullable) is written before the max_groups failure: callers
// grow their outputs from it and call again.
template <typename T>
static int keyed_frame_build(pds_ctx* ctx, const KeyOrder& ko, Bump& w, int64_t n_rows, pds_space space, int64_t run_cap, int64_t max_groups,
                             int64_t* n_groups, KeyedFrame<T>& kf, StageTrace* tr = nullptr) {
    const int nc = (int)kf.src.size();
    const size_t temp_bytes = ko.sorted ? keyed_ordered_temp_bytes(n_rows) : keyed_temp_bytes(n_rows);
    void* d_temp = w.take<char>(temp_bytes);
    kf.d_unique = w.take<int64_t>((size_t)run_cap + 1);
    int64_t* d_counts = w.take<int64_t>((size_t)run_cap + 1);
    kf.d_offsets = w.take<int64_t>((size_t)run_cap + 1);
    int64_t* d_nruns = w.take<int64_t>(32);
    if (space == PDS_HOST)
        if (int rc = cols_to_device<T>(ctx, w, kf.src, n_rows)) return rc;
    if (tr) tr->mark("columns H2D");
    kf.d_keys = ko.d_keys;
    if (!ko.sorted) {
        int64_t* sk = w.take<int64_t>((size_t)n_rows);
        uint32_t* idx_in = w.take<uint32_t>((size_t)n_rows);
        uint32_t* perm = w.take<uint32_t>((size_t)n_rows);
        int64_t* sk2 = w.take<int64_t>((size_t)n_rows);
        if (int rc = keyed_sort(ctx, ko.d_keys, n_rows, idx_in, sk, perm, d_temp, temp_bytes, sk2, ko.d_minmax, ko.mm)) return rc;
        kf.d_keys = sk;
        kf.d_perm = perm;
        static const bool by_column = [] { const char* e = dev_env("PDS_KEYED_GATHER_BY_COLUMN"); return e && e[0] == '1'; }();
        // frames too wide for the 256-row transposition tile (32 f64 / 64 f32 columns and beyond) gather column by column
        if (by_column || !gather_frame_fits<T>(nc)) {  // (one random 8-byte read per element; the env switch is the A/B)
            for (const T*& col : kf.src) {
                T* d = w.take<T>((size_t)n_rows);
                if (int rc = launch_gather_rows<T>(ctx, col, perm, n_rows, d)) return rc;
                col = d;
            }
        } else {
            // transpose to row-major records, then one random access per ROW (keyed.hip)
            std::vector<const T*> tbl(kf.src);
            for (const T*& col : kf.src) tbl.push_back(col = w.take<T>((size_t)n_rows));
            T* records = w.take<T>((size_t)n_rows * nc);
            const T** d_tbl = w.take<const T*>(tbl.size());
            PDS_HIP_CHECK(hipMemcpyAsync(d_tbl, tbl.data(), tbl.size() * sizeof(T*), hipMemcpyHostToDevice, ctx->stream));
            if (int rc = launch_gather_frame<T>(ctx, d_tbl, perm, nc, n_rows, records, (T* const*)(d_tbl + nc))) return rc;
            PDS_HIP_CHECK(hipStreamSynchronize(ctx->stream));  // (tbl: source of the table copy)
        }
    }
    if (tr) tr->mark("sort + gather");
    if (ko.sorted) {  // keys in order: the order check has counted and marked the run starts already -- a scan and one pass over the marks,
        kf.ng = ko.n_runs + 1;  // left on the stream in front of the fit (the number of groups came back with the order flag)
        if (kf.ng <= max_groups)
            if (int rc = keyed_runs_ordered(ctx, ko.d_keys, n_rows, ko.d_run_counts, ko.d_run_prefix, ko.d_run_masks, run_cap, kf.d_unique,
                                            kf.d_offsets, d_temp, temp_bytes))
                return rc;
    } else if (int rc = keyed_runs(ctx, kf.d_keys, n_rows, kf.d_unique, d_counts, kf.d_offsets, d_nruns, d_temp, temp_bytes, &kf.ng)) {
        return rc;
    }
    if (tr) tr->mark("run lengths + offsets");
    if (n_groups) *n_groups = kf.ng;
    if (kf.ng > max_groups) return fail(PDS_ERR_INVALID, "more distinct keys than max_groups");
    return PDS_OK;
}

// Steps A and B in one call.  kf.src holds the caller's columns (frame_cols).  max_groups: the caller's bound, n_rows for none.
// extra_bytes(sorted): what the caller's own slices need behind the frame (its staged outputs), asked once the order of the keys is
// known.  `w` is left behind the frame for those slices.  *n_groups (nullable) is written before the max_groups failure, as in
// keyed_frame_build.
template <typename T, typename ExtraBytes>
static int keyed_frame_open(pds_ctx* ctx, const int64_t* keys, int64_t n_rows, pds_space space, int64_t max_groups, ExtraBytes extra_bytes,
                            int64_t* n_groups, KeyedFrame<T>& kf, Bump& w) {
    KeyOrder ko;
    if (int rc = keyed_order_check(ctx, keys, n_rows, space, false, -1, ko)) return rc;
    const int64_t cap = std::min<int64_t>(max_groups, n_rows);
    const int64_t run_cap = ko.sorted ? std::min<int64_t>(ko.n_runs + 1, cap) : n_rows;
    const size_t need = keyed_frame_bytes<T>(ko.sorted, n_rows, (int)kf.src.size(), space, run_cap) + extra_bytes(ko.sorted);
    if (int rc = ensure_ws(ctx, ctx->keyed, need)) return rc;
    w = Bump{static_cast<char*>(ctx->keyed.ptr)};
    return keyed_frame_build<T>(ctx, ko, w, n_rows, space, run_cap, max_groups, n_groups, kf);
}
