// capi_glm_report.hpp -- the grouped GLM report: the fit of capi_glm_grouped.hpp and, at its coefficients, standard errors, z, p,
// confidence intervals, cov, deviances and the dispersion of every group (grouped_glm_report.hip): contiguous groups
// (pds_glm_report_grouped_*) and int64 keys in any row order (pds_glm_report_by_key_*)
// Part of the one translation unit capi.hip (included there, inside namespace pds, in dependency order): the entry-point
// pipelines are templates with internal linkage, split by concern, not by compilation unit.
#pragma once

// rows of a piece of a group above the split threshold: never more than the threshold (no wave walks more rows than a group of the
// one-wave route may have), and short enough that the pieces of one long group fill the device
constexpr int64_t kGlmReportPieceRows = 4096;

// the twelve report outputs, `cap` groups of room: `d` receives the device pointers
template <typename T>
static StagedOuts glm_report_staged_outs(const pds_glm_report_out& out, GlmReportDev<T>& d, bool host, int64_t cap, int pp) {
    StagedOuts so(host, (size_t)cap);
    so.add(&d.se, static_cast<T*>(out.std_err), pp);
    so.add(&d.z, static_cast<T*>(out.z), pp);
    so.add(&d.p, static_cast<T*>(out.p), pp);
    so.add(&d.lo, static_cast<T*>(out.ci_lower), pp);
    so.add(&d.hi, static_cast<T*>(out.ci_upper), pp);
    so.add(&d.cov, static_cast<T*>(out.cov), (size_t)pp * pp);
    so.add(&d.deviance, static_cast<T*>(out.deviance), 1);
    so.add(&d.null_deviance, static_cast<T*>(out.null_deviance), 1);
    so.add(&d.pearson, static_cast<T*>(out.pearson_chi2), 1);
    so.add(&d.dispersion, static_cast<T*>(out.dispersion), 1);
    so.add(&d.df_resid, out.df_resid, 1);
    so.add(&d.report_null, out.report_null, 1);
    return so;
}

// Fit and report of a DEVICE-resident frame (src: reference order [y, x1..xp]; every pointer a device pointer).  The fit is
// glm_grouped_impl as the pds_glm_irls_* entry points call it; the report's own arrays come out of ctx->ws, which the fit has
// finished with (its full-device iteration of long groups re-reserves it).
// d_pw / d_o (device, nullable): prior weights and offsets -- the weighted / offset fit and the weighted / offset report kernels
// (grouped_glm_report_wo.hip); with neither, the calls they always were.
template <typename T>
static int glm_report_device(pds_ctx* ctx, const std::vector<const T*>& src, int n_feat, int64_t n_rows, const int64_t* d_off, int64_t n_groups,
                             int add_bias, int link, int variance, T tol, int max_iter, T* d_co, int32_t* d_it, uint8_t* d_nu,
                             const GlmReportDev<T>& d, const T* d_pw = nullptr, const T* d_o = nullptr) {
    const bool wo = d_pw || d_o;
    if (int rc = glm_grouped_impl<T>(ctx, src.data(), n_feat, n_rows, d_off, n_groups, PDS_DEVICE, add_bias, link, variance, (T)0, (T)0, tol,
                                     max_iter, d_co, d_it, d_nu, (T*)nullptr, (uint8_t*)nullptr, nullptr, d_pw, d_o))
        return rc;
    const int bias = add_bias ? 1 : 0;
    const int64_t split = glm_split_rows(ctx);
    const int64_t piece_rows = std::min(split, kGlmReportPieceRows);
    const int64_t long_cap = glm_long_cap(n_groups, n_rows, split);
    const int64_t piece_cap = n_rows / piece_rows + long_cap + 1;
    const auto up = Bump::up;
    const size_t need = 4096 + up(sizeof(T*) * glm_table_slots(wo)) + GlmLongGroups::bytes(long_cap) + 2 * up((size_t)piece_cap * 24) +
                        up((size_t)piece_cap * kGlmReportRec * 8);
    if (int rc = ws_reserve(ctx, need)) return rc;
    Bump w{static_cast<char*>(ctx->ws.ptr)};
    std::vector<const T*> tbl;
    const T** d_tbl = nullptr;
    const T* const d_wo[2] = {d_pw, d_o};
    std::vector<const T*> frame(src.begin(), src.begin() + n_feat + 1);  // (src may carry the two columns behind the frame)
    if (int rc = kernel_order_table<T>(ctx, w, frame, n_feat, tbl, d_tbl, wo ? d_wo : nullptr)) return rc;
    GlmLongGroups lng;
    if (int rc = lng.take(ctx, w, long_cap)) return rc;
    int64_t* d_pieces = w.take<int64_t>((size_t)piece_cap * 3);
    int64_t* d_fin = w.take<int64_t>((size_t)piece_cap * 3);
    double* d_rec = w.take<double>((size_t)piece_cap * kGlmReportRec);
    const GlmGroupsDev<T> groups{d_tbl, n_feat, bias, n_rows, d_off, n_groups, link, variance, split, wo};
    if (int rc = launch_grouped_glm_report<T>(ctx, groups, d_co, d_nu, d, lng.dev)) return rc;
    std::vector<int64_t> lg, pieces, fin;
    if (int rc = lng.fetch(ctx, lg)) return rc;  // (synchronises: tbl was the source of the table copy)
    if (lg.empty()) return PDS_OK;
    // ---- long groups, in ascending order: pieces of at most piece_rows rows, one record each, added per group in piece order
    for (const int64_t g : lg) {
        int64_t rr[2];
        PDS_HIP_CHECK(hipMemcpy(rr, d_off + g, 16, hipMemcpyDeviceToHost));
        if (rr[0] < 0 || rr[1] > n_rows || rr[1] <= rr[0]) return fail(PDS_ERR_INVALID, "group offsets must be non-decreasing and inside the frame");
        const int64_t first = (int64_t)pieces.size() / 3;
        for (int64_t r = rr[0]; r < rr[1]; r += piece_rows) {
            pieces.push_back(g);
            pieces.push_back(r);
            pieces.push_back(std::min(r + piece_rows, rr[1]));
        }
        fin.push_back(g);
        fin.push_back(first);
        fin.push_back((int64_t)pieces.size() / 3 - first);
    }
    const int64_t n_pieces = (int64_t)pieces.size() / 3, n_fin = (int64_t)fin.size() / 3;
    if (n_pieces > piece_cap) return fail(PDS_ERR_INVALID, "group offsets must be non-decreasing and inside the frame");
    PDS_HIP_CHECK(hipMemcpyAsync(d_pieces, pieces.data(), pieces.size() * 8, hipMemcpyHostToDevice, ctx->stream));
    PDS_HIP_CHECK(hipMemcpyAsync(d_fin, fin.data(), fin.size() * 8, hipMemcpyHostToDevice, ctx->stream));
    if (int rc = launch_grouped_glm_report_pieces<T>(ctx, groups, d_co, d, d_pieces, n_pieces, d_fin, n_fin, d_rec)) return rc;
    PDS_HIP_CHECK(hipStreamSynchronize(ctx->stream));  // (pieces / fin: sources of the copies)
    return PDS_OK;
}

static int glm_report_check(const void* ctx, const void* cols, const void* coeffs, const void* n_iter, const void* is_null, const void* out,
                            int n_feat, int max_iter, int link, int variance) {
    if (!ctx || !cols || !coeffs || !n_iter || !is_null || !out) return fail(PDS_ERR_INVALID, "null argument");
    if (n_feat < 1) return fail(PDS_ERR_INVALID, "need at least one feature column");
    return glm_args_check("grouped GLM report", n_feat, max_iter, link, variance);
}

// A host frame is staged once (ctx->stage: columns, offsets, the fit's and the report's outputs) and fitted and reported as a device
// frame; the fit is the same kernel on the same values, so its outputs are those of pds_glm_irls_grouped_* on the host frame.
template <typename T>
static int glm_report_grouped_impl(pds_ctx* ctx, const T* const* cols, int n_feat, int64_t n_rows, const int64_t* offsets, int64_t n_groups,
                                   pds_space space, int add_bias, int link, int variance, T tol, int max_iter, T* coeffs, int32_t* n_iter,
                                   uint8_t* is_null, const pds_glm_report_out* out, const T* weights = nullptr, const T* offset = nullptr) {
    if (int rc = glm_report_check(ctx, cols, coeffs, n_iter, is_null, out, n_feat, max_iter, link, variance)) return rc;
    if (!offsets) return fail(PDS_ERR_INVALID, "null argument");
    if (n_groups <= 0 || n_rows <= 0) return fail(PDS_ERR_EMPTY, "Empty data");
    if (int rc = check_cols<T>(cols, n_feat)) return rc;
    PDS_HIP_CHECK(hipSetDevice(ctx->device));
    const int pp = n_feat + (add_bias ? 1 : 0);
    const bool host = space == PDS_HOST;
    T* d_co;
    int32_t* d_it;
    uint8_t* d_nu;
    GlmReportDev<T> d;
    StagedOuts fit(host, (size_t)n_groups);
    fit.add(&d_co, coeffs, pp);
    fit.add(&d_it, n_iter, 1);
    fit.add(&d_nu, is_null, 1);
    StagedOuts rep = glm_report_staged_outs<T>(*out, d, host, n_groups, pp);
    std::vector<const T*> src = frame_cols<T>(cols, n_feat);  // [y, x1..xp (, weights) (, offset)]: a host frame stages them together
    if (weights) src.push_back(weights);
    if (offset) src.push_back(offset);
    const int64_t* d_off = offsets;
    if (host) {
        const size_t need = 4096 + Bump::up((size_t)n_rows * sizeof(T)) * src.size() + Bump::up((size_t)(n_groups + 1) * 8) + fit.bytes() + rep.bytes();
        if (int rc = ensure_ws(ctx, ctx->stage, need)) return rc;
        Bump w{static_cast<char*>(ctx->stage.ptr)};
        if (int rc = cols_to_device<T>(ctx, w, src, n_rows)) return rc;
        int64_t* t = w.take<int64_t>((size_t)n_groups + 1);
        PDS_HIP_CHECK(hipMemcpyAsync(t, offsets, (size_t)(n_groups + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
        d_off = t;
        fit.place(w);
        rep.place(w);
    }
    if (int rc = glm_report_device<T>(ctx, src, n_feat, n_rows, d_off, n_groups, add_bias, link, variance, tol, max_iter, d_co, d_it, d_nu, d,
                                      weights ? src[n_feat + 1] : nullptr, offset ? src.back() : nullptr))
        return rc;
    if (host) {
        if (int rc = staged_copy_back(ctx, fit, (size_t)n_groups)) return rc;
        if (int rc = staged_copy_back(ctx, rep, (size_t)n_groups)) return rc;
    }
    PDS_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return PDS_OK;
}

// int64 keys in any row order: the key-ordered frame of glm_by_key_impl (keyed_frame_open), fitted and reported where it lies
template <typename T>
static int glm_report_by_key_impl(pds_ctx* ctx, const T* const* cols, const int64_t* keys, int n_feat, int64_t n_rows, pds_space space,
                                  int add_bias, int link, int variance, T tol, int max_iter, int64_t max_groups, int64_t* out_keys, T* coeffs,
                                  int32_t* n_iter, uint8_t* is_null, int64_t* n_groups, const pds_glm_report_out* out,
                                  const T* weights = nullptr, const T* offset = nullptr) {
    if (int rc = glm_report_check(ctx, cols, coeffs, n_iter, is_null, out, n_feat, max_iter, link, variance)) return rc;
    if (!keys || !out_keys || !n_groups) return fail(PDS_ERR_INVALID, "null argument");
    if (n_rows <= 0) return fail(PDS_ERR_EMPTY, "Empty data");
    if (max_groups < 1) return fail(PDS_ERR_INVALID, "max_groups must be positive");
    if (int rc = check_cols<T>(cols, n_feat)) return rc;
    PDS_HIP_CHECK(hipSetDevice(ctx->device));
    const int pp = n_feat + (add_bias ? 1 : 0);
    const bool host = space == PDS_HOST;
    const int64_t cap = std::min<int64_t>(max_groups, n_rows);
    T* d_co;
    int32_t* d_it;
    uint8_t* d_nu;
    GlmReportDev<T> d;
    StagedOuts fit(host, (size_t)cap);
    fit.add(&d_co, coeffs, pp);
    fit.add(&d_it, n_iter, 1);
    fit.add(&d_nu, is_null, 1);
    StagedOuts rep = glm_report_staged_outs<T>(*out, d, host, cap, pp);
    KeyedFrame<T> kf;
    kf.src = frame_cols<T>(cols, n_feat);  // (the two columns ride through the staging, the sort and the gather with the frame)
    if (weights) kf.src.push_back(weights);
    if (offset) kf.src.push_back(offset);
    Bump w{};
    if (int rc = keyed_frame_open<T>(ctx, keys, n_rows, space, max_groups, [&](bool) { return fit.bytes() + rep.bytes(); }, n_groups, kf, w))
        return rc;
    const int64_t ng = kf.ng;
    fit.place(w);
    rep.place(w);
    if (int rc = glm_report_device<T>(ctx, kf.src, n_feat, n_rows, kf.d_offsets, ng, add_bias, link, variance, tol, max_iter, d_co, d_it, d_nu, d,
                                      weights ? kf.src[n_feat + 1] : nullptr, offset ? kf.src.back() : nullptr))
        return rc;
    PDS_HIP_CHECK(hipMemcpyAsync(out_keys, kf.d_unique, (size_t)ng * 8, host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, ctx->stream));
    if (int rc = staged_copy_back(ctx, fit, (size_t)ng)) return rc;
    if (int rc = staged_copy_back(ctx, rep, (size_t)ng)) return rc;
    PDS_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return PDS_OK;
}
