// capi_rolling.hpp -- rolling / recursive regressions
// Part of the one translation unit capi.hip (included there, inside namespace pds, in dependency order): the entry-point
// pipelines are templates with internal linkage, split by concern, not by compilation unit.
#pragma once

template <typename T>
static int rolling_impl(pds_ctx* ctx, const T* const* cols, int n_feat, int64_t n_rows, pds_space space, int add_bias,
                        int64_t window, int64_t min_size, double lambda, bool expanding, T* coeffs, T* pred,
                        uint8_t* valid, const T* seed_moments = nullptr) {
    if (!ctx || !cols || !coeffs || !pred || !valid) return fail(PDS_ERR_INVALID, "null argument");
    if (int rc = check_shape(n_feat, n_rows, add_bias)) return rc;
    const int pp = n_feat + (add_bias ? 1 : 0);
    std::vector<double> seed;
    if (seed_moments) {  // rows in front of this frame: they count towards start_with
        const int q = n_feat + 2;
        seed.assign(seed_moments, seed_moments + (size_t)q * q);
        for (double v : seed)
            if (!std::isfinite(v)) return fail(PDS_ERR_INVALID, "seed moments must be finite");
        const double seen = seed[n_feat + (size_t)n_feat * q];
        if (window < 1 || seen < 0.0) return fail(PDS_ERR_INVALID, "start_with must be >= 1 and the seed row count >= 0");
        const double left = (double)window - seen;
        window = left <= 1.0 ? 1 : (left > (double)n_rows ? n_rows + 1 : (int64_t)left);
    } else if (window < 1 || window > n_rows) {
        return fail(PDS_ERR_INVALID, "window / start_with must be in [1, n_rows]");
    }
    PDS_HIP_CHECK(hipSetDevice(ctx->device));
    size_t need = 131072 + ((size_t)(n_rows / 4096) + 2) * 96 * sizeof(double)  // + per-tile totals (expanding)
                  + ((size_t)(n_rows / 4096 / 32) + 2) * 128 * sizeof(double);   // + their chunk sums (tile prefix)
    T *d_co, *d_pr;
    uint8_t* d_va;
    StagedOuts outs(space == PDS_HOST, (size_t)n_rows);
    outs.add(&d_co, coeffs, pp);
    outs.add(&d_pr, pred, 1);
    outs.add(&d_va, valid, 1);
    if (space == PDS_HOST) need += outs.bytes() + 4096;
    if (pp > 12) need += rolling_wide_workspace(n_feat, n_rows, sizeof(T));
    if (int rc = ws_reserve(ctx, need)) return rc;
    DeviceCols<T> dc;
    if (int rc = make_device_cols<T>(ctx, cols, (const T*)nullptr, n_feat, n_rows, space, dc)) return rc;
    outs.place([&](size_t b) { return ws_take(ctx, b); });
    if (int rc = launch_rolling<T>(ctx, dc, n_feat, n_rows, add_bias, window, min_size, lambda, expanding,
                                   seed.empty() ? nullptr : seed.data(), d_co, d_pr, d_va))
        return rc;
    if (int rc = staged_copy_back(ctx, outs, (size_t)n_rows)) return rc;
    PDS_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return PDS_OK;
}

// ---- grouped rolling / expanding fits: for every group g = rows [off[g], off[g+1]) what the plain call gives on g's rows alone
// (segmented sums: launch_rolling_grouped).  Columns [y, x1..xp] as in rolling_impl.
static int check_grouped_window(int n_feat, int add_bias, int64_t n_rows, int64_t window, int64_t min_size) {
    if (n_feat < 1) return fail(PDS_ERR_INVALID, "need at least one feature column");
    if (n_feat + (add_bias ? 1 : 0) > 64)
        return fail(PDS_ERR_UNSUPPORTED, "grouped rolling / recursive: at most 64 coefficients");
    if (n_rows <= 0) return fail(PDS_ERR_EMPTY, "Empty data");
    if (window < 1) return fail(PDS_ERR_INVALID, "window / start_with must be >= 1");
    if (min_size < 0) return fail(PDS_ERR_INVALID, "min_size must be >= 0");
    return PDS_OK;
}
// workspace of one grouped launch over n_rows rows (launch_rolling_grouped: tile totals, flags and chunk sums of the expanding
// form, the record chunk of the wide form)
static size_t rolling_grouped_need(int n_feat, int add_bias, int64_t n_rows, size_t elem) {
    const int pp = n_feat + (add_bias ? 1 : 0);
    size_t need = 131072 + ((size_t)(n_rows / 4096) + 2) * (96 * sizeof(double) + 1) + ((size_t)(n_rows / 4096 / 32) + 2) * (128 * sizeof(double) + 1);
    if (pp > 8) need += rolling_wide_workspace(n_feat, n_rows, elem) + (size_t)(n_rows / 256) + 256;
    return need;
}

// device-resident columns and offsets (validated), device outputs: the ws arena is reserved here
template <typename T>
static int rolling_grouped_device(pds_ctx* ctx, const T* const* d_cols, int n_feat, int64_t n_rows, const int64_t* d_off, int64_t n_groups,
                                  int add_bias, int64_t window, int64_t min_size, double lambda, bool expanding, T* d_co, T* d_pr,
                                  uint8_t* d_va) {
    if (int rc = ws_reserve(ctx, rolling_grouped_need(n_feat, add_bias, n_rows, sizeof(T)))) return rc;
    DeviceCols<T> dc;
    if (int rc = make_device_cols<T>(ctx, d_cols, (const T*)nullptr, n_feat, n_rows, PDS_DEVICE, dc)) return rc;
    return launch_rolling_grouped<T>(ctx, dc, n_feat, n_rows, add_bias, window, min_size, lambda, expanding, d_off, n_groups, d_co, d_pr,
                                     d_va);
}

template <typename T>
static int rolling_grouped_impl(pds_ctx* ctx, const T* const* cols, int n_feat, int64_t n_rows, const int64_t* group_offsets,
                                int64_t n_groups, pds_space space, int add_bias, int64_t window, int64_t min_size, double lambda,
                                bool expanding, T* coeffs, T* pred, uint8_t* valid) {
    if (!ctx || !cols || !group_offsets || !coeffs || !pred || !valid) return fail(PDS_ERR_INVALID, "null argument");
    if (int rc = check_grouped_window(n_feat, add_bias, n_rows, window, min_size)) return rc;
    if (n_groups < 1) return fail(PDS_ERR_INVALID, "n_groups must be >= 1");
    PDS_HIP_CHECK(hipSetDevice(ctx->device));
    const int pp = n_feat + (add_bias ? 1 : 0), nc = n_feat + 1;
    // the offsets on the host: validated (the kernels walk rows with them)
    std::vector<int64_t> h_off_store;
    const int64_t* h_off = nullptr;
    if (int rc = host_offsets(ctx, group_offsets, n_groups, space, h_off_store, h_off)) return rc;
    if (h_off[0] != 0 || h_off[n_groups] != n_rows) return fail(PDS_ERR_INVALID, "group offsets must start at 0 and end at n_rows");
    for (int64_t g = 0; g < n_groups; ++g)
        if (h_off[g + 1] < h_off[g]) return fail(PDS_ERR_INVALID, "group offsets must be non-decreasing");
    if (space == PDS_DEVICE) {
        if (int rc = rolling_grouped_device<T>(ctx, cols, n_feat, n_rows, group_offsets, n_groups, add_bias, window, min_size, lambda,
                                               expanding, coeffs, pred, valid))
            return rc;
        PDS_HIP_CHECK(hipStreamSynchronize(ctx->stream));  // (synchronous on return; dc's pointer table is an async copy source)
        return PDS_OK;
    }
    // host frame: columns, offsets and outputs staged in the keyed workspace (the ws arena belongs to the launch)
    const auto up = Bump::up;
    const size_t col_bytes = up((size_t)n_rows * sizeof(T));
    T *d_co, *d_pr;
    uint8_t* d_va;
    StagedOuts outs(true, (size_t)n_rows);
    outs.add(&d_co, coeffs, pp);
    outs.add(&d_pr, pred, 1);
    outs.add(&d_va, valid, 1);
    const size_t need = col_bytes * nc + up((size_t)(n_groups + 1) * 8) + outs.bytes() + 4096;
    if (int rc = ensure_ws(ctx, ctx->keyed, need)) return rc;
    Bump w{static_cast<char*>(ctx->keyed.ptr)};
    std::vector<const T*> src = frame_cols<T>(cols, n_feat);
    if (int rc = cols_to_device<T>(ctx, w, src, n_rows)) return rc;
    int64_t* d_off = w.take<int64_t>((size_t)n_groups + 1);
    PDS_HIP_CHECK(hipMemcpyAsync(d_off, group_offsets, (size_t)(n_groups + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
    outs.place(w);
    if (int rc = rolling_grouped_device<T>(ctx, src.data(), n_feat, n_rows, d_off, n_groups, add_bias, window, min_size, lambda, expanding,
                                           d_co, d_pr, d_va))
        return rc;
    if (int rc = staged_copy_back(ctx, outs, (size_t)n_rows)) return rc;
    PDS_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return PDS_OK;
}

// int64 keys in any row order.  Ordered keys: the order check's run marks give the offsets, nothing moves.  Otherwise the stable
// radix sort of (key, row) (rows keep their order inside a group), the frame gather, the offsets form on the sorted frame and a
// scatter of coeffs / pred / valid back to frame order.
template <typename T>
static int rolling_by_key_impl(pds_ctx* ctx, const T* const* cols, const int64_t* keys, int n_feat, int64_t n_rows, pds_space space,
                               int add_bias, int64_t window, int64_t min_size, double lambda, bool expanding, T* coeffs, T* pred,
                               uint8_t* valid) {
    if (!ctx || !cols || !keys || !coeffs || !pred || !valid) return fail(PDS_ERR_INVALID, "null argument");
    if (int rc = check_grouped_window(n_feat, add_bias, n_rows, window, min_size)) return rc;
    PDS_HIP_CHECK(hipSetDevice(ctx->device));
    const int pp = n_feat + (add_bias ? 1 : 0);
    const bool host = space == PDS_HOST;
    // the fit's outputs go through the workspace on a host frame and whenever the keys are not in order (they are then scattered
    // back to frame order: into the caller's buffers on the device, else into a second staged set)
    T *d_co, *d_pr, *o_co = nullptr, *o_pr = nullptr;
    uint8_t *d_va, *o_va = nullptr;
    StagedOuts fit(host, (size_t)n_rows), scattered(host, (size_t)n_rows);
    bool sorted = true;
    auto declare = [&](bool keys_sorted) {  // (asked once, when the order check has answered)
        sorted = keys_sorted;
        fit = StagedOuts(host, (size_t)n_rows, !sorted);
        fit.add(&d_co, coeffs, pp);
        fit.add(&d_pr, pred, 1);
        fit.add(&d_va, valid, 1);
        if (sorted) return fit.bytes();
        scattered.add(&o_co, coeffs, pp);
        scattered.add(&o_pr, pred, 1);
        scattered.add(&o_va, valid, 1);
        return fit.bytes() + scattered.bytes();
    };
    KeyedFrame<T> kf;
    kf.src = frame_cols<T>(cols, n_feat);
    Bump w{};
    if (int rc = keyed_frame_open<T>(ctx, keys, n_rows, space, /*max_groups=*/n_rows, declare, nullptr, kf, w)) return rc;
    fit.place(w);
    if (int rc = rolling_grouped_device<T>(ctx, kf.src.data(), n_feat, n_rows, kf.d_offsets, kf.ng, add_bias, window, min_size, lambda, expanding,
                                           d_co, d_pr, d_va))
        return rc;
    if (!sorted) {
        scattered.place(w);
        if (int rc = launch_rolling_scatter<T>(ctx, d_co, d_pr, d_va, kf.d_perm, n_rows, pp, o_co, o_pr, o_va)) return rc;
    }
    if (int rc = staged_copy_back(ctx, sorted ? fit : scattered, (size_t)n_rows)) return rc;
    PDS_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return PDS_OK;
}
