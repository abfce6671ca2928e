// capi_glm_grouped.hpp -- a GLM per group (IRLS): contiguous groups (pds_glm_irls_grouped_*) and int64 keys in any row order
// (pds_glm_irls_by_key_*) on top of grouped_irls.hip; with l1_reg / l2_reg the elastic-net penalised fits (pds_glm_enet_grouped_* /
// pds_glm_enet_by_key_*), a penalty <= 0 meaning none; with a prior-weight and / or an offset column the weighted / offset fits
// (pds_glm_irls_wo_grouped_* / pds_glm_irls_wo_by_key_*)
// Part of the one translation unit capi.hip (included there, inside namespace pds, in dependency order): the entry-point
// pipelines are templates with internal linkage, split by concern, not by compilation unit.
#pragma once

// Groups above this many rows leave the one-wave-per-group kernel for the full-device iteration (glm_irls_impl on the group's row
// range: launches and a blocking copy per iteration and group, but every CU on the one group).  Context option "glm_split_rows".
constexpr int64_t kGlmSplitRowsDefault = 16384;
static int64_t glm_split_rows(const pds_ctx* ctx) {
    return std::max<int64_t>(ctx->opt_glm_split_rows > 0 ? ctx->opt_glm_split_rows : kGlmSplitRowsDefault, 64);
}
// the most groups of more than `split` rows a frame can hold
static int64_t glm_long_cap(int64_t n_groups, int64_t n_rows, int64_t split) { return std::min<int64_t>(n_groups, n_rows / split + 1); }
// entries of the column table (kernel_order_table): 18, and two more with prior weights / offsets
static int glm_table_slots(bool wo) { return wo ? 20 : 18; }

// The long-group protocol of the fit and of the report (capi_glm_report.hpp): the kernel appends the groups above the split
// threshold to a list in device memory, in any order, and counts them; the host takes the list back in ascending order.
struct GlmLongGroups {
    GlmLongList dev{};
    static size_t bytes(int64_t cap) { return Bump::up((size_t)cap * 8) + 256; }  // the workspace term: the list and the count block
    int take(pds_ctx* ctx, Bump& w, int64_t cap) {
        dev.d_list = w.take<int64_t>((size_t)cap);
        dev.d_count = w.take<unsigned>(64);
        dev.cap = cap;
        PDS_HIP_CHECK(hipMemsetAsync(dev.d_count, 0, sizeof(unsigned), ctx->stream));
        return PDS_OK;
    }
    // After the launch.  The synchronisation here is also the one both callers rely on for the host source of the column table's
    // asynchronous copy (kernel_order_table): the table's vector must live until this returns.
    int fetch(pds_ctx* ctx, std::vector<int64_t>& sorted) {
        unsigned h_count = 0;
        PDS_HIP_CHECK(hipMemcpyAsync(&h_count, dev.d_count, sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream));
        PDS_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        if ((int64_t)h_count > dev.cap) return fail(PDS_ERR_INVALID, "group offsets must be non-decreasing and inside the frame");
        sorted.resize(h_count);
        if (h_count == 0) return PDS_OK;
        PDS_HIP_CHECK(hipMemcpy(sorted.data(), dev.d_list, (size_t)h_count * 8, hipMemcpyDeviceToHost));
        std::sort(sorted.begin(), sorted.end());
        return PDS_OK;
    }
};

// the argument checks every grouped GLM entry shares; `what` names the entry in the message ("grouped GLM (IRLS)", "grouped GLM report")
static int glm_args_check(const char* what, int n_feat, int max_iter, int link, int variance) {
    if (max_iter < 1) return fail(PDS_ERR_INVALID, "`max_iter` must be > 1.");  // linear_models.py:756-757
    if (link < 0 || link > 3 || variance < 0 || variance > 3) return fail(PDS_ERR_INVALID, "unknown link / variance function");
    if (n_feat > kMaxFeatSmall) return fail(PDS_ERR_UNSUPPORTED, std::string(what) + ": up to 16 feature columns");
    return PDS_OK;
}
static int glm_penalty_check(bool wo, double l1_reg, double l2_reg) {
    if (wo && (l1_reg > 0 || l2_reg > 0))
        return fail(PDS_ERR_UNSUPPORTED, "grouped GLM (IRLS): l1_reg / l2_reg together with weights / offset is not built");
    return PDS_OK;
}

// d_perm (device, nullable): row r of the frame in
// group order is row d_perm[r] of pred / row_null.  Its buffers come out of ctx->wkeyed: the full-device iteration of a long group
// re-reserves ctx->ws, and the by-key form holds its frame in ctx->keyed.
// weights / offset (nullable, in `space`, n_rows long): with either one the weighted / offset kernels of grouped_irls.hip fit the
// groups and glm_irls_wo_impl the long ones, on their row range of the two columns; with neither the call is the one it was.
template <typename T>
static int glm_grouped_impl(pds_ctx* ctx, const T* const* cols, int n_feat, int64_t n_rows, const int64_t* offsets, int64_t n_groups,
                            pds_space space, int add_bias, int link, int variance, T l1_reg, T l2_reg, T tol, int max_iter, T* coeffs,
                            int32_t* n_iter, uint8_t* is_null, T* pred, uint8_t* row_null, const uint32_t* d_perm = nullptr,
                            const T* weights = nullptr, const T* offset = nullptr) {
    if (!ctx || !cols || !offsets || !coeffs || !n_iter || !is_null) return fail(PDS_ERR_INVALID, "null argument");
    if (n_feat < 1) return fail(PDS_ERR_INVALID, "need at least one feature column");
    if (n_groups <= 0 || n_rows <= 0) return fail(PDS_ERR_EMPTY, "Empty data");
    if (int rc = glm_args_check("grouped GLM (IRLS)", n_feat, max_iter, link, variance)) return rc;
    if (int rc = check_cols<T>(cols, n_feat)) return rc;
    const bool wo = weights || offset;
    if (int rc = glm_penalty_check(wo, (double)l1_reg, (double)l2_reg)) return rc;
    PDS_HIP_CHECK(hipSetDevice(ctx->device));
    const int bias = add_bias ? 1 : 0, pp = n_feat + bias, nc = n_feat + 1 + (weights ? 1 : 0) + (offset ? 1 : 0);
    const bool host_frame = space == PDS_HOST;
    const bool host_out = space == PDS_HOST;
    const int64_t split = glm_split_rows(ctx);
    const int64_t long_cap = glm_long_cap(n_groups, n_rows, split);
    const auto up = Bump::up;
    const size_t col_bytes = up((size_t)n_rows * sizeof(T));
    T *d_co, *d_pred;
    int32_t* d_it;
    uint8_t *d_nu, *d_rn;
    StagedOuts outs(host_out, (size_t)n_groups), row_outs(host_out, (size_t)n_rows);
    outs.add(&d_co, coeffs, pp);
    outs.add(&d_it, n_iter, 1);
    outs.add(&d_nu, is_null, 1);
    row_outs.add(&d_pred, pred, 1);
    row_outs.add(&d_rn, row_null, 1);
    size_t need = 4096 + up(sizeof(T*) * glm_table_slots(wo)) + GlmLongGroups::bytes(long_cap) + outs.bytes() + row_outs.bytes();
    if (host_frame) need += col_bytes * nc;
    if (host_out) need += up((size_t)(n_groups + 1) * 8);
    if (int rc = ensure_ws(ctx, ctx->wkeyed, need)) return rc;
    Bump w{static_cast<char*>(ctx->wkeyed.ptr)};
    // ---- the frame: device pointers in the kernels' order x_0 .. x_{p-1}, y
    std::vector<const T*> src = frame_cols<T>(cols, n_feat);  // reference order [y, x1..xp (, weights) (, offset)], device resident
    if (weights) src.push_back(weights);
    if (offset) src.push_back(offset);
    if (host_frame)
        if (int rc = cols_to_device<T>(ctx, w, src, n_rows)) return rc;
    std::vector<const T*> tbl;
    const T** d_tbl = nullptr;
    const T* const d_wo[2] = {weights ? src[n_feat + 1] : nullptr, offset ? src[nc - 1] : nullptr};  // (device resident by now)
    if (int rc = kernel_order_table<T>(ctx, w, src, n_feat, tbl, d_tbl, wo ? d_wo : nullptr)) return rc;
    GlmLongGroups lng;
    if (int rc = lng.take(ctx, w, long_cap)) return rc;
    const int64_t* d_off = offsets;
    if (host_out) {
        int64_t* t = w.take<int64_t>((size_t)n_groups + 1);
        PDS_HIP_CHECK(hipMemcpyAsync(t, offsets, (size_t)(n_groups + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
        d_off = t;
    }
    outs.place(w);
    row_outs.place(w);
    const GlmGroupsDev<T> groups{d_tbl, n_feat, bias, n_rows, d_off, n_groups, link, variance, split, wo};
    const GlmFitDev<T> fit{(double)tol, max_iter, (double)l1_reg, (double)l2_reg, d_co, d_it, d_nu, d_pred, d_rn, d_perm};
    if (int rc = launch_grouped_irls<T>(ctx, groups, fit, lng.dev)) return rc;
    std::vector<int64_t> lg;
    if (int rc = lng.fetch(ctx, lg)) return rc;  // (synchronises: tbl was the source of the table copy)
    if (!lg.empty()) {
        // ---- long groups, in ascending order: the full-device iteration on the group's row range, its row of the outputs from the host
        std::vector<T> hb(lg.size() * pp);
        std::vector<int32_t> hi(lg.size());
        std::vector<uint8_t> hn(lg.size());
        for (size_t k = 0; k < lg.size(); ++k) {
            const int64_t g = lg[k];
            int64_t rr[2];
            if (host_out) {
                rr[0] = offsets[g];
                rr[1] = offsets[g + 1];
            } else {
                PDS_HIP_CHECK(hipMemcpy(rr, d_off + g, 16, hipMemcpyDeviceToHost));
            }
            std::vector<const T*> gc(n_feat + 1);
            for (int c = 0; c <= n_feat; ++c) gc[c] = src[c] + rr[0];
            int its = 0, wnull = 0;  // (a long group that fails the weight rule is null, like a short one)
            if (wo) {
                if (int rc = glm_irls_wo_impl<T>(ctx, gc.data(), d_wo[0] ? d_wo[0] + rr[0] : nullptr, d_wo[1] ? d_wo[1] + rr[0] : nullptr, n_feat,
                                                 rr[1] - rr[0], PDS_DEVICE, add_bias, link, variance, tol, max_iter, hb.data() + k * pp, &its,
                                                 &wnull))
                    return rc;
            } else if (int rc = glm_irls_impl<T>(ctx, gc.data(), n_feat, rr[1] - rr[0], PDS_DEVICE, add_bias, link, variance, tol, max_iter,
                                                 hb.data() + k * pp, &its, l1_reg, l2_reg)) {
                return rc;
            }
            hi[k] = its;
            bool fin = true;
            for (int j = 0; j < pp; ++j) fin = fin && std::isfinite(hb[k * pp + j]);
            hn[k] = fin ? 0 : 1;
            PDS_HIP_CHECK(hipMemcpyAsync(d_co + g * pp, hb.data() + k * pp, sizeof(T) * pp, hipMemcpyHostToDevice, ctx->stream));
            PDS_HIP_CHECK(hipMemcpyAsync(d_it + g, &hi[k], 4, hipMemcpyHostToDevice, ctx->stream));
            PDS_HIP_CHECK(hipMemcpyAsync(d_nu + g, &hn[k], 1, hipMemcpyHostToDevice, ctx->stream));
            if (int rc = launch_glm_pred_range<T>(ctx, d_tbl, n_feat, bias, rr[0], rr[1], d_co + g * pp, d_nu + g, link, d_pred, d_rn, d_perm,
                                                  d_wo[1]))
                return rc;
        }
        PDS_HIP_CHECK(hipStreamSynchronize(ctx->stream));  // (hb / hi / hn: sources of the copies)
    }
    if (host_out) {
        if (int rc = staged_copy_back(ctx, outs, (size_t)n_groups)) return rc;
        if (int rc = staged_copy_back(ctx, row_outs, (size_t)n_rows)) return rc;
        PDS_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    }
    return PDS_OK;
}

// int64 keys in any row order: the route pds_lr_by_key_pred_* takes without its partition branch (lr_by_key_impl) -- ordered keys: the
// order check's run marks give the offsets and nothing moves; unordered keys: radix sort of (key, row) pairs + frame gather, the
// per-row means sent back through the permutation.
template <typename T>
static int glm_by_key_impl(pds_ctx* ctx, const T* const* cols, const int64_t* keys, int n_feat, int64_t n_rows, pds_space space, int add_bias,
                           int link, int variance, T l1_reg, T l2_reg, T tol, int max_iter, int64_t max_groups, int64_t* out_keys, T* coeffs,
                           int32_t* n_iter, uint8_t* is_null, int64_t* n_groups, T* pred, uint8_t* row_null, const T* weights = nullptr,
                           const T* offset = nullptr) {
    if (!ctx || !cols || !keys || !out_keys || !coeffs || !n_iter || !is_null || !n_groups) return fail(PDS_ERR_INVALID, "null argument");
    if (n_feat < 1) return fail(PDS_ERR_INVALID, "need at least one feature column");
    if (n_rows <= 0) return fail(PDS_ERR_EMPTY, "Empty data");
    if (int rc = glm_args_check("grouped GLM (IRLS)", n_feat, max_iter, link, variance)) return rc;
    if (max_groups < 1) return fail(PDS_ERR_INVALID, "max_groups must be positive");
    if (int rc = check_cols<T>(cols, n_feat)) return rc;
    if (int rc = glm_penalty_check(weights || offset, (double)l1_reg, (double)l2_reg)) return rc;
    PDS_HIP_CHECK(hipSetDevice(ctx->device));
    const int pp = n_feat + (add_bias ? 1 : 0);
    T *d_co, *d_pred;
    int32_t* d_it;
    uint8_t *d_nu, *d_rn;
    StagedOuts outs(space == PDS_HOST, (size_t)std::min<int64_t>(max_groups, n_rows)), row_outs(space == PDS_HOST, (size_t)n_rows);
    outs.add(&d_co, coeffs, pp);
    outs.add(&d_it, n_iter, 1);
    outs.add(&d_nu, is_null, 1);
    row_outs.add(&d_pred, pred, 1, StagedOuts::kOutRoom);
    row_outs.add(&d_rn, row_null, 1, StagedOuts::kOutRoom);
    KeyedFrame<T> kf;
    kf.src = frame_cols<T>(cols, n_feat);  // the two columns ride through the staging, the sort and the gather with the frame
    if (weights) kf.src.push_back(weights);
    if (offset) kf.src.push_back(offset);
    Bump w{};
    if (int rc = keyed_frame_open<T>(ctx, keys, n_rows, space, max_groups, [&](bool) { return outs.bytes() + row_outs.bytes(); }, n_groups, kf, w))
        return rc;
    const int64_t ng = kf.ng;
    outs.place(w);
    row_outs.place(w);
    if (int rc = glm_grouped_impl<T>(ctx, kf.src.data(), n_feat, n_rows, kf.d_offsets, ng, PDS_DEVICE, add_bias, link, variance, l1_reg, l2_reg, tol, max_iter,
                                     d_co, d_it, d_nu, d_pred, d_rn, kf.d_perm, weights ? kf.src[n_feat + 1] : nullptr,
                                     offset ? kf.src.back() : nullptr))
        return rc;
    const hipMemcpyKind back = space == PDS_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    PDS_HIP_CHECK(hipMemcpyAsync(out_keys, kf.d_unique, (size_t)ng * 8, back, ctx->stream));
    if (int rc = staged_copy_back(ctx, outs, (size_t)ng)) return rc;
    if (int rc = staged_copy_back(ctx, row_outs, (size_t)n_rows)) return rc;
    PDS_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return PDS_OK;
}
