// capi_glm_sandwich.hpp -- the one-model GLM report with robust (hc0 / hc1) and cluster-robust (cluster / cluster0) standard errors:
// pds_glm_report_robust_* / pds_glm_report_cluster_grouped_* / pds_glm_report_cluster_by_key_*.  ONE model over the whole frame,
// V = c I^-1 M I^-1 with M the sum of the outer products of the rows' (hc) or the clusters' (cluster) scores (Stata's vce(robust |
// cluster id), statsmodels' GLM.fit(cov_type="HC0" | "HC1" | "cluster"), R's sandwich::vcovHC / vcovCL on a glm).
// Part of the one translation unit capi.hip (included there, inside namespace pds, in dependency order): the entry-point
// pipelines are templates with internal linkage, split by concern, not by compilation unit.
//
// The stages: the frame is staged as glm_report_grouped_impl stages it (host frames go to ctx->stage once, weights and offset behind
// the frame; the by-key form brings the frame into key order first, keyed_frame_open); glm_report_device with the single group
// [0, n) gives the fit and the plain report (coeffs, n_iter and the plain fields are therefore bit for bit those of
// pds_glm_report_wo_grouped_* with group_offsets = [0, n]); ONE more pass over the same device frame (glm_meat.hip) gives the meat and
// the cluster and row counts; beta, cov, dispersion and the record come to the host, which forms I^-1 = cov / dispersion, I^-1 M I^-1 and the
// fields in double and writes the outputs.
#pragma once

// bytes of workspace glm_sandwich_device takes out of its Bump: the one-group outputs, the pointer table, the offsets of the single
// group and of the clusters (n_off_upload entries when the device needs a copy), the chunk lists and scores of the long clusters, the
// records.  An upper bound that does not need the plan (the by-key form asks before the clusters are known).
template <typename T>
static size_t glm_sandwich_bytes(const pds_ctx* ctx, int64_t n_rows, int64_t n_off_upload, int pp, int64_t split) {
    const auto up = Bump::up;
    const int64_t max_long = n_rows / split + 1, max_chunks = n_rows / split + max_long + 1;
    const size_t rec_bytes = (size_t)kMixedRecStride * sizeof(double);
    const size_t n_rec = (size_t)cluster_meat_blocks(ctx, n_rows) * 3 + 1;
    return 8192 + up(sizeof(T) * (size_t)pp) * 6 + up(sizeof(T) * (size_t)pp * pp) + 8 * up(16) + up(sizeof(T*) * 20) + up(16) +
           up((size_t)(n_off_upload + 1) * 8) + 4 * up((size_t)(max_chunks + 1) * 8) + up((size_t)(max_chunks + 1) * kClusterScoreStride * 8) +
           up(n_rec * rec_bytes) + up((n_rec / 64 + 1) * rec_bytes) + up(rec_bytes);
}

static int64_t glm_sandwich_split(const pds_ctx* ctx) {
    return std::max<int64_t>(ctx->opt_cluster_split_rows > 0 ? ctx->opt_cluster_split_rows : kClusterSplitRowsDefault, 64);
}

// se_type of a robust (cluster = false) or cluster (cluster = true) entry point
static int glm_sandwich_check_kind(int se_type, bool cluster) {
    if (se_type == PDS_HC2 || se_type == PDS_HC3)
        return fail(PDS_ERR_UNSUPPORTED, "robust GLM report: HC2 / HC3 need the leverages and are not built (hc0, hc1, cluster, cluster0)");
    if (cluster ? (se_type != PDS_CLUSTER && se_type != PDS_CLUSTER0) : (se_type != PDS_HC0 && se_type != PDS_HC1))
        return fail(PDS_ERR_INVALID, cluster ? "cluster-robust GLM report: se_type is PDS_CLUSTER or PDS_CLUSTER0"
                                             : "robust GLM report: se_type is PDS_HC0 or PDS_HC1");
    return PDS_OK;
}

template <typename T>
static int glm_sandwich_check(const void* ctx, const T* const* cols, const void* coeffs, const void* n_iter, const void* out, int n_feat,
                              int64_t n_rows, int max_iter, int link, int variance, int se_type, bool cluster) {
    if (!ctx || !cols || !coeffs || !n_iter || !out) return fail(PDS_ERR_INVALID, "null argument");
    if (n_feat < 1) return fail(PDS_ERR_INVALID, "need at least one feature column");
    if (max_iter < 1) return fail(PDS_ERR_INVALID, "`max_iter` must be > 1.");
    if (link < 0 || link > 3 || variance < 0 || variance > 3) return fail(PDS_ERR_INVALID, "unknown link / variance function");
    if (n_feat > kMaxFeatSmall) return fail(PDS_ERR_UNSUPPORTED, "robust GLM report: up to 16 feature columns");
    if (int rc = glm_sandwich_check_kind(se_type, cluster)) return rc;
    if (n_rows <= 0) return fail(PDS_ERR_EMPTY, "Empty data");
    return check_cols<T>(cols, n_feat);
}

// v = c inv meat inv, made symmetric (the mean of the two halves): pp x pp row-major, pp <= kMaxFeatSmall + 1.  The robust GLM report
// and the fixed-effects GLM (capi_glm_within.hpp) share it: the loop order is part of their results' bits.
static void sandwich_cov(int pp, const double* inv, const double* meat, double c, double* v) {
    double half[(kMaxFeatSmall + 1) * (kMaxFeatSmall + 1)];
    for (int i = 0; i < pp; ++i)
        for (int j = 0; j < pp; ++j) {
            double s = 0.0;
            for (int a = 0; a < pp; ++a) s += inv[i * pp + a] * meat[a * pp + j];
            half[i * pp + j] = s;
        }
    for (int i = 0; i < pp; ++i)
        for (int j = 0; j < pp; ++j) {
            double s = 0.0;
            for (int a = 0; a < pp; ++a) s += half[i * pp + a] * inv[a * pp + j];
            v[i * pp + j] = c * s;
        }
    for (int i = 0; i < pp; ++i)
        for (int j = i + 1; j < pp; ++j) v[i * pp + j] = v[j * pp + i] = 0.5 * (v[i * pp + j] + v[j * pp + i]);
}

// `vals` (host, doubles) -> the caller's buffer of T (nullable), `space`-resident; `keep` owns the source of an asynchronous copy
template <typename T>
static int glm_sandwich_put(pds_ctx* ctx, bool host, void* user, const double* vals, size_t n, std::vector<std::vector<T>>& keep) {
    if (!user) return PDS_OK;
    T* dst = static_cast<T*>(user);
    if (host) {
        for (size_t i = 0; i < n; ++i) dst[i] = (T)vals[i];
        return PDS_OK;
    }
    keep.emplace_back(n);
    for (size_t i = 0; i < n; ++i) keep.back()[i] = (T)vals[i];
    PDS_HIP_CHECK(hipMemcpyAsync(dst, keep.back().data(), n * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
    return PDS_OK;
}

// Fit, plain report and sandwich of a DEVICE-resident frame (src: [y, x1..xp (, weights) (, offset)], device pointers).  Clusters:
// h_off (host, n_clusters + 1 validated-here offsets) and d_off (the same on the device, or null when the device has none: they are
// then uploaded); n_clusters = 0 for the hc kinds.  w: glm_sandwich_bytes of room.  host: the caller's outputs are host memory.
template <typename T>
static int glm_sandwich_device(pds_ctx* ctx, const std::vector<const T*>& src, const T* d_pw, const T* d_o, int n_feat, int64_t n_rows,
                               const int64_t* h_off, const int64_t* d_off, int64_t n_clusters, int add_bias, int link, int variance, T tol,
                               int max_iter, int se_type, Bump w, bool host, T* coeffs, int32_t* n_iter, const pds_glm_report_out* out,
                               int64_t* n_clusters_out) {
    const bool cluster = se_type == PDS_CLUSTER || se_type == PDS_CLUSTER0;
    const int p = n_feat, bias = add_bias ? 1 : 0, pp = p + bias;
    const int64_t split = glm_sandwich_split(ctx);
    if (n_clusters_out) *n_clusters_out = 0;
    if ((se_type == PDS_HC1 || se_type == PDS_CLUSTER) && n_rows <= pp) return fail(PDS_ERR_TOO_FEW_ROWS, "#Data <= #features. No conclusive result.");
    // ---- the clusters on the host: validation, the non-empty clusters, the chunks of the long ones
    GroupChunkPlan pl;
    ClusterChunks ch;
    if (cluster) {
        if (n_clusters < 1) return fail(PDS_ERR_INVALID, "cluster-robust standard errors need at least two non-empty clusters");
        if (int rc = plan_group_chunks(h_off, n_clusters, n_rows, split, /*cover=*/true, d_off == nullptr, /*want_gmap=*/false,
                                       "cluster offsets must be non-decreasing and cover the frame", pl))
            return rc;
        if (n_clusters_out) *n_clusters_out = pl.n_nonempty;
        if (pl.n_nonempty < 2) return fail(PDS_ERR_INVALID, "cluster-robust standard errors need at least two non-empty clusters");
        n_clusters = pl.n_nonempty;  // (the device works on the non-empty clusters alone)
        if (pl.upload_off) {
            int64_t* t = w.take<int64_t>((size_t)n_clusters + 1);
            PDS_HIP_CHECK(hipMemcpyAsync(t, pl.h_off, (size_t)(n_clusters + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
            d_off = t;
        }
        if (int rc = upload_cluster_chunks(ctx, w, pl, ch)) return rc;
    } else {
        n_clusters = 0;
    }
    // ---- the one-group fit and plain report, into this call's own device buffers
    T* d_co = w.take<T>((size_t)pp);
    int32_t* d_it = w.take<int32_t>(1);
    uint8_t* d_nu = w.take<uint8_t>(1);
    GlmReportDev<T> d;
    d.se = w.take<T>((size_t)pp), d.z = w.take<T>((size_t)pp), d.p = w.take<T>((size_t)pp), d.lo = w.take<T>((size_t)pp), d.hi = w.take<T>((size_t)pp);
    d.cov = w.take<T>((size_t)pp * pp);
    d.deviance = w.take<T>(1), d.null_deviance = w.take<T>(1), d.pearson = w.take<T>(1), d.dispersion = w.take<T>(1);
    d.df_resid = w.take<int64_t>(1);
    d.report_null = w.take<uint8_t>(1);
    int64_t* d_one = w.take<int64_t>(2);
    const int64_t one_group[2] = {0, n_rows};
    PDS_HIP_CHECK(hipMemcpyAsync(d_one, one_group, sizeof(one_group), hipMemcpyHostToDevice, ctx->stream));
    const int n_rec = glm_meat_records(ctx, n_rows, n_clusters, ch);
    const size_t rec_bytes = (size_t)kMixedRecStride * sizeof(double);
    double* d_partials = reinterpret_cast<double*>(w.take<char>((size_t)n_rec * rec_bytes));
    double* d_stage = reinterpret_cast<double*>(w.take<char>(((size_t)n_rec / 64 + 1) * rec_bytes));
    double* d_rec = reinterpret_cast<double*>(w.take<char>(rec_bytes));
    std::vector<const T*> tbl;
    const T** d_tbl = nullptr;
    const T* const d_wo[2] = {d_pw, d_o};
    std::vector<const T*> frame(src.begin(), src.begin() + n_feat + 1);
    if (int rc = kernel_order_table<T>(ctx, w, frame, n_feat, tbl, d_tbl, d_wo)) return rc;
    if (int rc = glm_report_device<T>(ctx, src, n_feat, n_rows, d_one, 1, add_bias, link, variance, tol, max_iter, d_co, d_it, d_nu, d, d_pw, d_o))
        return rc;
    // ---- the meat at the coefficients as stored, on the same device frame
    if (int rc = launch_glm_meat<T>(ctx, d_tbl, p, n_rows, d_off, n_clusters, split, ch, d_co, bias, link, variance, d_partials, d_stage, d_rec))
        return rc;
    std::vector<T> beta(pp), cov((size_t)pp * pp);
    T plain[4];  // deviance, null_deviance, pearson_chi2, dispersion
    int32_t it = 0;
    int64_t df_resid = 0;
    uint8_t nu = 0, rnull = 0;
    double rec[kMixedRecStride];
    const auto d2h = hipMemcpyDeviceToHost;
    PDS_HIP_CHECK(hipMemcpyAsync(beta.data(), d_co, sizeof(T) * pp, d2h, ctx->stream));
    PDS_HIP_CHECK(hipMemcpyAsync(cov.data(), d.cov, sizeof(T) * pp * pp, d2h, ctx->stream));
    PDS_HIP_CHECK(hipMemcpyAsync(&plain[0], d.deviance, sizeof(T), d2h, ctx->stream));
    PDS_HIP_CHECK(hipMemcpyAsync(&plain[1], d.null_deviance, sizeof(T), d2h, ctx->stream));
    PDS_HIP_CHECK(hipMemcpyAsync(&plain[2], d.pearson, sizeof(T), d2h, ctx->stream));
    PDS_HIP_CHECK(hipMemcpyAsync(&plain[3], d.dispersion, sizeof(T), d2h, ctx->stream));
    PDS_HIP_CHECK(hipMemcpyAsync(&it, d_it, sizeof(it), d2h, ctx->stream));
    PDS_HIP_CHECK(hipMemcpyAsync(&df_resid, d.df_resid, sizeof(df_resid), d2h, ctx->stream));
    PDS_HIP_CHECK(hipMemcpyAsync(&nu, d_nu, 1, d2h, ctx->stream));
    PDS_HIP_CHECK(hipMemcpyAsync(&rnull, d.report_null, 1, d2h, ctx->stream));
    PDS_HIP_CHECK(hipMemcpyAsync(rec, d_rec, sizeof(rec), d2h, ctx->stream));
    PDS_HIP_CHECK(hipStreamSynchronize(ctx->stream));  // (tbl, pl, one_group: sources of the copies)
    // ---- the sandwich, in double on the host
    const int64_t n_pos = (int64_t)std::llround(rec[kMixedRecCM]);  // the rows of positive weight, counted by the pass
    const int64_t n_cl = cluster ? (int64_t)std::llround(rec[kMixedRecLD]) : 0;
    if (n_clusters_out) *n_clusters_out = n_cl;
    if (cluster && n_cl < 2) return fail(PDS_ERR_INVALID, "cluster-robust standard errors need at least two non-empty clusters");
    if ((se_type == PDS_HC1 || se_type == PDS_CLUSTER) && n_pos <= pp) return fail(PDS_ERR_TOO_FEW_ROWS, "#Data <= #features. No conclusive result.");
    const double nan = std::nan("");
    std::vector<double> inv((size_t)pp * pp), meat((size_t)pp * pp, 0.0), v((size_t)pp * pp);
    const double disp = (double)plain[3];
    for (size_t k = 0; k < inv.size(); ++k) inv[k] = (double)cov[k] / disp;  // cov = dispersion I^-1: the dispersion cancels in the sandwich
    for (int i = 0; i < p; ++i) {
        for (int j = 0; j < p; ++j) meat[(size_t)i * pp + j] = rec[kMixedRecW + i * 16 + j];
        if (bias) meat[(size_t)i * pp + p] = meat[(size_t)p * pp + i] = rec[kMixedRecXY + i];
    }
    if (bias) meat[(size_t)p * pp + p] = cluster ? rec[kMixedRecC] : rec[kMixedRecYY] + rec[kMixedRecCY];  // (sum r)^2 per cluster; sum r^2, compensated
    double c = 1.0;
    if (se_type == PDS_HC1) c = (double)n_pos / (double)(n_pos - pp);
    if (se_type == PDS_CLUSTER) c = (double)n_cl / (double)(n_cl - 1) * ((double)(n_pos - 1) / (double)(n_pos - pp));
    sandwich_cov(pp, inv.data(), meat.data(), c, v.data());
    bool null = nu != 0 || rnull != 0;
    for (int j = 0; j < pp && !null; ++j) null = !(std::isfinite(v[(size_t)j * pp + j]) && v[(size_t)j * pp + j] >= 0.0);
    std::vector<double> se(pp, nan), z(pp, nan), pv(pp, nan), lo(pp, nan), hi(pp, nan);
    double group[4] = {(double)plain[0], (double)plain[1], (double)plain[2], (double)plain[3]};
    if (null) {
        std::fill(v.begin(), v.end(), nan);
        std::fill(group, group + 4, nan);
    } else {
        for (int j = 0; j < pp; ++j) {
            const double b = (double)beta[j];
            se[j] = std::sqrt(v[(size_t)j * pp + j]);
            z[j] = b / se[j];
            pv[j] = std::erfc(std::fabs(z[j]) / 1.4142135623730951);
            lo[j] = b - 1.959963984540054 * se[j];
            hi[j] = b + 1.959963984540054 * se[j];
        }
    }
    // ---- the outputs: the fit's and the plain fields as the device gave them (their bits), the rest from V
    std::vector<std::vector<T>> keep;
    const auto put_raw = [&](void* user, const void* h, size_t bytes) -> int {
        if (!user) return PDS_OK;
        if (host) std::memcpy(user, h, bytes);
        else PDS_HIP_CHECK(hipMemcpyAsync(user, h, bytes, hipMemcpyHostToDevice, ctx->stream));
        return PDS_OK;
    };
    const uint8_t null_u8 = null ? 1 : 0;
    if (int rc = put_raw(coeffs, beta.data(), sizeof(T) * pp)) return rc;
    if (int rc = put_raw(n_iter, &it, sizeof(it))) return rc;
    if (int rc = glm_sandwich_put<T>(ctx, host, out->std_err, se.data(), pp, keep)) return rc;
    if (int rc = glm_sandwich_put<T>(ctx, host, out->z, z.data(), pp, keep)) return rc;
    if (int rc = glm_sandwich_put<T>(ctx, host, out->p, pv.data(), pp, keep)) return rc;
    if (int rc = glm_sandwich_put<T>(ctx, host, out->ci_lower, lo.data(), pp, keep)) return rc;
    if (int rc = glm_sandwich_put<T>(ctx, host, out->ci_upper, hi.data(), pp, keep)) return rc;
    if (int rc = glm_sandwich_put<T>(ctx, host, out->cov, v.data(), (size_t)pp * pp, keep)) return rc;
    void* const group_out[4] = {out->deviance, out->null_deviance, out->pearson_chi2, out->dispersion};
    for (int k = 0; k < 4; ++k) {
        if (null) {
            if (int rc = glm_sandwich_put<T>(ctx, host, group_out[k], &group[k], 1, keep)) return rc;
        } else if (int rc = put_raw(group_out[k], &plain[k], sizeof(T))) {
            return rc;
        }
    }
    if (int rc = put_raw(out->df_resid, &df_resid, sizeof(df_resid))) return rc;
    if (int rc = put_raw(out->report_null, &null_u8, 1)) return rc;
    PDS_HIP_CHECK(hipStreamSynchronize(ctx->stream));  // (keep and the locals: sources of the copies)
    return PDS_OK;
}

// contiguous clusters (offsets) and the hc kinds (offsets = null, n_clusters = 0)
template <typename T>
static int glm_sandwich_impl(pds_ctx* ctx, const T* const* cols, const T* weights, const T* offset, int n_feat, int64_t n_rows,
                             const int64_t* offsets, int64_t n_clusters, pds_space space, int add_bias, int link, int variance, T tol,
                             int max_iter, int se_type, bool cluster, T* coeffs, int32_t* n_iter, const pds_glm_report_out* out,
                             int64_t* n_clusters_out) {
    if (int rc = glm_sandwich_check<T>(ctx, cols, coeffs, n_iter, out, n_feat, n_rows, max_iter, link, variance, se_type, cluster)) return rc;
    if (cluster && !offsets) return fail(PDS_ERR_INVALID, "null argument");
    if (cluster && n_clusters < 1) return fail(PDS_ERR_INVALID, "cluster-robust standard errors need at least two non-empty clusters");
    PDS_HIP_CHECK(hipSetDevice(ctx->device));
    const int pp = n_feat + (add_bias ? 1 : 0);
    const bool host = space == PDS_HOST;
    std::vector<int64_t> off_copy;
    const int64_t* h_off = nullptr;
    if (cluster)
        if (int rc = host_offsets(ctx, offsets, n_clusters, space, off_copy, h_off)) return rc;
    std::vector<const T*> src = frame_cols<T>(cols, n_feat);  // [y, x1..xp (, weights) (, offset)]: a host frame stages them together
    if (weights) src.push_back(weights);
    if (offset) src.push_back(offset);
    const size_t need = glm_sandwich_bytes<T>(ctx, n_rows, cluster ? n_clusters : 0, pp, glm_sandwich_split(ctx)) +
                        (host ? Bump::up((size_t)n_rows * sizeof(T)) * src.size() : 0);
    if (int rc = ensure_ws(ctx, ctx->stage, need)) return rc;
    Bump w{static_cast<char*>(ctx->stage.ptr)};
    if (host)
        if (int rc = cols_to_device<T>(ctx, w, src, n_rows)) return rc;
    return glm_sandwich_device<T>(ctx, src, weights ? src[n_feat + 1] : nullptr, offset ? src.back() : nullptr, n_feat, n_rows, h_off,
                                  cluster && !host ? offsets : nullptr, cluster ? n_clusters : 0, add_bias, link, variance, tol, max_iter, se_type,
                                  w, host, coeffs, n_iter, out, n_clusters_out);
}

// int64 keys in any row order: the shared key-ordering stage (ordered keys move nothing; weights and offset ride through the gather),
// then the contiguous form on the device frame
template <typename T>
static int glm_sandwich_by_key_impl(pds_ctx* ctx, const T* const* cols, const T* weights, const T* offset, const int64_t* keys, int n_feat,
                                    int64_t n_rows, pds_space space, int add_bias, int link, int variance, T tol, int max_iter, int se_type,
                                    T* coeffs, int32_t* n_iter, const pds_glm_report_out* out, int64_t* n_clusters_out) {
    if (int rc = glm_sandwich_check<T>(ctx, cols, coeffs, n_iter, out, n_feat, n_rows, max_iter, link, variance, se_type, true)) return rc;
    if (!keys) return fail(PDS_ERR_INVALID, "null argument");
    PDS_HIP_CHECK(hipSetDevice(ctx->device));
    const int pp = n_feat + (add_bias ? 1 : 0);
    KeyedFrame<T> kf;
    kf.src = frame_cols<T>(cols, n_feat);
    if (weights) kf.src.push_back(weights);
    if (offset) kf.src.push_back(offset);
    Bump w{};
    const size_t extra = glm_sandwich_bytes<T>(ctx, n_rows, 0, pp, glm_sandwich_split(ctx));
    if (int rc = keyed_frame_open<T>(ctx, keys, n_rows, space, /*max_groups=*/n_rows, [&](bool) { return extra; }, nullptr, kf, w)) return rc;
    std::vector<int64_t> off_copy;
    const int64_t* h_off = nullptr;
    if (int rc = host_offsets(ctx, kf.d_offsets, kf.ng, PDS_DEVICE, off_copy, h_off)) return rc;
    return glm_sandwich_device<T>(ctx, kf.src, weights ? kf.src[n_feat + 1] : nullptr, offset ? kf.src.back() : nullptr, n_feat, n_rows, h_off,
                                  kf.d_offsets, kf.ng, add_bias, link, variance, tol, max_iter, se_type, w, space == PDS_HOST, coeffs, n_iter, out,
                                  n_clusters_out);
}
