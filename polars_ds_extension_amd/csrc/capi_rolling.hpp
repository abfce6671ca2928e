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
    if (space == PDS_HOST) need += (size_t)n_rows * ((pp + 1) * sizeof(T) + 1) + 4096;
    if (pp > 12) need += rolling_wide_workspace(n_feat, n_rows, sizeof(T));
    if (int rc = ws_reserve(ctx, need)) return rc;
    DeviceCols<T> dc;
    if (int rc = make_device_cols<T>(ctx, cols, (const T*)nullptr, n_feat, n_rows, space, dc)) return rc;
    T* d_co = coeffs;
    T* d_pr = pred;
    uint8_t* d_va = valid;
    if (space == PDS_HOST) {
        d_co = reinterpret_cast<T*>(ws_take(ctx, (size_t)n_rows * pp * sizeof(T)));
        d_pr = reinterpret_cast<T*>(ws_take(ctx, (size_t)n_rows * sizeof(T)));
        d_va = reinterpret_cast<uint8_t*>(ws_take(ctx, (size_t)n_rows));
    }
    if (int rc = launch_rolling<T>(ctx, dc, n_feat, n_rows, add_bias, window, min_size, lambda, expanding,
                                   seed.empty() ? nullptr : seed.data(), d_co, d_pr, d_va))
        return rc;
    if (space == PDS_HOST) {
        PDS_HIP_CHECK(hipMemcpyAsync(coeffs, d_co, (size_t)n_rows * pp * sizeof(T), hipMemcpyDeviceToHost, ctx->stream));
        PDS_HIP_CHECK(hipMemcpyAsync(pred, d_pr, (size_t)n_rows * sizeof(T), hipMemcpyDeviceToHost, ctx->stream));
        PDS_HIP_CHECK(hipMemcpyAsync(valid, d_va, (size_t)n_rows, hipMemcpyDeviceToHost, ctx->stream));
    }
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
    std::vector<int64_t> h_off((size_t)n_groups + 1);
    if (space == PDS_DEVICE) {
        PDS_HIP_CHECK(hipMemcpyAsync(h_off.data(), group_offsets, h_off.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
        PDS_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    } else {
        std::copy(group_offsets, group_offsets + n_groups + 1, h_off.begin());
    }
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
    const size_t need = col_bytes * nc + up(h_off.size() * 8) + up((size_t)n_rows * pp * sizeof(T)) + col_bytes + up((size_t)n_rows) + 4096;
    if (int rc = ensure_ws(ctx, ctx->keyed, need)) return rc;
    Bump w{static_cast<char*>(ctx->keyed.ptr)};
    std::vector<const T*> src = frame_cols<T>(cols, n_feat);
    if (int rc = cols_to_device<T>(ctx, w, src, n_rows)) return rc;
    int64_t* d_off = w.take<int64_t>(h_off.size());
    PDS_HIP_CHECK(hipMemcpyAsync(d_off, h_off.data(), h_off.size() * 8, hipMemcpyHostToDevice, ctx->stream));
    T* d_co = w.take<T>((size_t)n_rows * pp);
    T* d_pr = w.take<T>((size_t)n_rows);
    uint8_t* d_va = w.take<uint8_t>((size_t)n_rows);
    if (int rc = rolling_grouped_device<T>(ctx, src.data(), n_feat, n_rows, d_off, n_groups, add_bias, window, min_size, lambda, expanding,
                                           d_co, d_pr, d_va))
        return rc;
    PDS_HIP_CHECK(hipMemcpyAsync(coeffs, d_co, (size_t)n_rows * pp * sizeof(T), hipMemcpyDeviceToHost, ctx->stream));
    PDS_HIP_CHECK(hipMemcpyAsync(pred, d_pr, (size_t)n_rows * sizeof(T), hipMemcpyDeviceToHost, ctx->stream));
    PDS_HIP_CHECK(hipMemcpyAsync(valid, d_va, (size_t)n_rows, hipMemcpyDeviceToHost, ctx->stream));
    PDS_HIP_CHECK(hipStreamSynchronize(ctx->stream));  // (h_off: source of an async copy)
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
    const int nc = n_feat + 1, pp = n_feat + (add_bias ? 1 : 0);
    KeyOrder ko;
    if (int rc = keyed_order_check(ctx, keys, n_rows, space, false, -1, ko)) return rc;
    const bool sorted = ko.sorted;
    const int64_t run_cap = sorted ? ko.n_runs + 1 : n_rows;  // (no max_groups here)
    size_t need = keyed_frame_bytes<T>(sorted, n_rows, nc, space, run_cap);
    const bool stage_out = space == PDS_HOST || !sorted;  // outputs through the workspace (host frame, or scattered back)
    const size_t out_bytes = Bump::up((size_t)n_rows * pp * sizeof(T)) + Bump::up((size_t)n_rows * sizeof(T)) + Bump::up((size_t)n_rows);
    if (stage_out) need += out_bytes;
    if (!sorted && space == PDS_HOST) need += out_bytes;  // the scatter's target
    if (int rc = ensure_ws(ctx, ctx->keyed, need)) return rc;
    Bump w{static_cast<char*>(ctx->keyed.ptr)};
    KeyedFrame<T> kf;
    kf.src = frame_cols<T>(cols, n_feat);
    if (int rc = keyed_frame_build<T>(ctx, ko, w, n_rows, space, run_cap, /*max_groups=*/n_rows, nullptr, kf)) return rc;
    T* d_co = coeffs;
    T* d_pr = pred;
    uint8_t* d_va = valid;
    if (stage_out) {
        d_co = w.take<T>((size_t)n_rows * pp);
        d_pr = w.take<T>((size_t)n_rows);
        d_va = w.take<uint8_t>((size_t)n_rows);
    }
    if (int rc = rolling_grouped_device<T>(ctx, kf.src.data(), n_feat, n_rows, kf.d_offsets, kf.ng, add_bias, window, min_size, lambda, expanding,
                                           d_co, d_pr, d_va))
        return rc;
    if (!sorted) {
        // back to frame order: in place when the caller's buffers are on the device, else into the staged outputs' own slots
        T* o_co = coeffs;
        T* o_pr = pred;
        uint8_t* o_va = valid;
        if (space == PDS_HOST) {
            o_co = w.take<T>((size_t)n_rows * pp);
            o_pr = w.take<T>((size_t)n_rows);
            o_va = w.take<uint8_t>((size_t)n_rows);
        }
        if (int rc = launch_rolling_scatter<T>(ctx, d_co, d_pr, d_va, kf.d_perm, n_rows, pp, o_co, o_pr, o_va)) return rc;
        d_co = o_co;
        d_pr = o_pr;
        d_va = o_va;
    }
    if (space == PDS_HOST) {
        PDS_HIP_CHECK(hipMemcpyAsync(coeffs, d_co, (size_t)n_rows * pp * sizeof(T), hipMemcpyDeviceToHost, ctx->stream));
        PDS_HIP_CHECK(hipMemcpyAsync(pred, d_pr, (size_t)n_rows * sizeof(T), hipMemcpyDeviceToHost, ctx->stream));
        PDS_HIP_CHECK(hipMemcpyAsync(valid, d_va, (size_t)n_rows, hipMemcpyDeviceToHost, ctx->stream));
    }
    PDS_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return PDS_OK;
}
