// capi_rcond_grouped.hpp -- lin_reg_w_rcond per group: contiguous groups (pds_lr_rcond_grouped_*) and int64 keys in any row order
// (pds_lr_rcond_by_key_*) on top of grouped_rcond.hip
// Part of the one translation unit capi.hip (included there, inside namespace pds, in dependency order): the entry-point
// pipelines are templates with internal linkage, split by concern, not by compilation unit.
#pragma once

// Host frames and host outputs are staged in ctx->wkeyed (the by-key form holds its frame in ctx->keyed).
template <typename T>
static int rcond_grouped_impl(pds_ctx* ctx, const T* const* cols, int n_feat, int64_t n_rows, const int64_t* offsets, int64_t n_groups,
                              pds_space space, int add_bias, T l2_reg, T rcond, T* coeffs, T* singular_values, uint8_t* is_null) {
    if (!ctx || !cols || !offsets || !coeffs || !singular_values || !is_null) return fail(PDS_ERR_INVALID, "null argument");
    if (n_feat < 1) return fail(PDS_ERR_INVALID, "need at least one feature column");
    if (n_groups <= 0 || n_rows <= 0) return fail(PDS_ERR_EMPTY, "Empty data");
    if (n_feat > kMaxFeatSmall) return fail(PDS_ERR_UNSUPPORTED, "grouped lin_reg_w_rcond: up to 16 feature columns");
    if (int rc = check_cols<T>(cols, n_feat)) return rc;
    PDS_HIP_CHECK(hipSetDevice(ctx->device));
    const int bias = add_bias ? 1 : 0, pp = n_feat + bias, nc = n_feat + 1;
    const bool host = space == PDS_HOST;
    const auto up = Bump::up;
    T *d_co, *d_sv;
    uint8_t* d_nu;
    StagedOuts outs(host, (size_t)n_groups);
    outs.add(&d_co, coeffs, pp);
    outs.add(&d_sv, singular_values, pp);
    outs.add(&d_nu, is_null, 1);
    size_t need = 4096 + up(sizeof(T*) * 18) + outs.bytes();
    if (host) need += up((size_t)n_rows * sizeof(T)) * nc + up((size_t)(n_groups + 1) * 8);
    if (int rc = ensure_ws(ctx, ctx->wkeyed, need)) return rc;
    Bump w{static_cast<char*>(ctx->wkeyed.ptr)};
    // ---- the frame: device pointers in the kernel's order x_0 .. x_{p-1}, y
    std::vector<const T*> src = frame_cols<T>(cols, n_feat);  // reference order [y, x1..xp]
    if (host)
        if (int rc = cols_to_device<T>(ctx, w, src, n_rows)) return rc;
    std::vector<const T*> tbl;
    const T** d_tbl = nullptr;
    if (int rc = kernel_order_table<T>(ctx, w, src, n_feat, tbl, d_tbl)) return rc;
    const int64_t* d_off = offsets;
    if (host) {
        int64_t* t = w.take<int64_t>((size_t)n_groups + 1);
        PDS_HIP_CHECK(hipMemcpyAsync(t, offsets, (size_t)(n_groups + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
        d_off = t;
    }
    outs.place(w);
    if (int rc = launch_grouped_rcond<T>(ctx, d_tbl, n_feat, bias, n_rows, d_off, n_groups, l2_reg > (T)0 ? (double)l2_reg : 0.0, (double)rcond,
                                         d_co, d_sv, d_nu))
        return rc;
    if (int rc = staged_copy_back(ctx, outs, (size_t)n_groups)) return rc;
    PDS_HIP_CHECK(hipStreamSynchronize(ctx->stream));  // (tbl: source of the table copy)
    return PDS_OK;
}

// int64 keys in any row order through the shared key-ordering stage (capi_keyed_frame.hpp) -- ordered keys: the order check's run
// marks give the offsets and nothing moves; unordered keys: radix sort of (key, row) pairs + frame gather.
template <typename T>
static int rcond_by_key_impl(pds_ctx* ctx, const T* const* cols, const int64_t* keys, int n_feat, int64_t n_rows, pds_space space, int add_bias,
                             T l2_reg, T rcond, int64_t max_groups, int64_t* out_keys, T* coeffs, T* singular_values, uint8_t* is_null,
                             int64_t* n_groups) {
    if (!ctx || !cols || !keys || !out_keys || !coeffs || !singular_values || !is_null || !n_groups) return fail(PDS_ERR_INVALID, "null argument");
    if (n_feat < 1) return fail(PDS_ERR_INVALID, "need at least one feature column");
    if (n_rows <= 0) return fail(PDS_ERR_EMPTY, "Empty data");
    if (n_feat > kMaxFeatSmall) return fail(PDS_ERR_UNSUPPORTED, "grouped lin_reg_w_rcond: up to 16 feature columns");
    if (max_groups < 1) return fail(PDS_ERR_INVALID, "max_groups must be positive");
    if (int rc = check_cols<T>(cols, n_feat)) return rc;
    PDS_HIP_CHECK(hipSetDevice(ctx->device));
    const int pp = n_feat + (add_bias ? 1 : 0);
    T *d_co, *d_sv;
    uint8_t* d_nu;
    StagedOuts outs(space == PDS_HOST, (size_t)std::min<int64_t>(max_groups, n_rows));
    outs.add(&d_co, coeffs, pp);
    outs.add(&d_sv, singular_values, pp);
    outs.add(&d_nu, is_null, 1);
    KeyedFrame<T> kf;
    kf.src = frame_cols<T>(cols, n_feat);
    Bump w{};
    if (int rc = keyed_frame_open<T>(ctx, keys, n_rows, space, max_groups, [&](bool) { return outs.bytes(); }, n_groups, kf, w)) return rc;
    const int64_t ng = kf.ng;
    outs.place(w);
    if (int rc = rcond_grouped_impl<T>(ctx, kf.src.data(), n_feat, n_rows, kf.d_offsets, ng, PDS_DEVICE, add_bias, l2_reg, rcond, d_co, d_sv, d_nu))
        return rc;
    const hipMemcpyKind back = space == PDS_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    PDS_HIP_CHECK(hipMemcpyAsync(out_keys, kf.d_unique, (size_t)ng * 8, back, ctx->stream));
    if (int rc = staged_copy_back(ctx, outs, (size_t)ng)) return rc;
    PDS_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return PDS_OK;
}
