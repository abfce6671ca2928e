// capi_within.hpp -- fixed-effects (within) regression with one absorbed factor (pds_lin_reg_within_grouped_* / _by_key_*): ONE model
// with an intercept per group, y_i = alpha_g(i) + x_i' beta + e_i, fitted without ever forming a dummy column.
// Part of the one translation unit capi.hip (included there, inside namespace pds, in dependency order): the entry-point
// pipelines are templates with internal linkage, split by concern, not by compilation unit.
//
// DEFINITIONS (what this file computes; no equivalence with any package's small-sample conventions is claimed).  n rows, G non-empty
// groups, p features, no intercept column (it is absorbed); m_g the mean of [x, y] over group g and
// W = sum_g sum_{i in g} ([x_i, y_i] - m_g)([x_i, y_i] - m_g)' the within scatter:
//     beta solves W_xx beta = W_xy;   alpha_g = m_y,g - m_g' beta;   e_i = y_i - alpha_g - x_i' beta;   pred_i = y_i - e_i
//     PDS_SE        V = s2 W_xx^-1, s2 = sum e^2 / (n - G - p); t, p and the 95 % interval: Student t, n - G - p degrees of freedom
//     PDS_CLUSTER0  V = W_xx^-1 M W_xx^-1, M = sum_g s_g s_g', s_g = sum_{i in g} (x_i - m_g) e_i: the clusters ARE the absorbed groups
//     PDS_CLUSTER   the same V times c = G / (G - 1) * (n - 1) / (n - p - 1): the absorbed effects, nested in the clusters, are not
//                   counted among the parameters, the one intercept is -- a DEFINITION of this library.  Both cluster forms: G - 1
//                   degrees of freedom
//     (clusters on ANY other key, through the struct WithinCluster: capi_within_cluster.hpp has the definitions and the stages)
//     r2 = 1 - sum e^2 / W_yy (the within R^2);   adj_r2 = 1 - (1 - r2)(n - G) / (n - G - p)
//     r2_overall = 1 - sum e^2 / sum (y - ybar)^2,  sum (y - ybar)^2 = W_yy + sum_g n_g (m_y,g - ybar)^2
// A singleton group stays in: it counts in n and G and adds nothing to W or M; its alpha is y - x' beta.  An empty group (offsets
// form) counts nowhere and changes no output bit; its alpha is NaN.
//
// Stages: (1) launch_mixed_stats (mixed.hip, no beta0): W, the group means, the "varies inside some group" bits, in one
// pass without cancellation, long groups cut into chunks; (2) the p x p Cholesky solve with the inverse on the host in f64 -- beta and
// nothing else goes back to the device; (3) launch_within_pass (within_pass.hip): alpha, residuals, predictions, sum e^2 formed from
// the residuals (W_yy - beta' W_xy cancels) and the meat of the centred scores, in ONE more pass over the frame over the same chunks.
// r2_overall's between-group term is G values: the y means come back to the host beside the record.
#pragma once

// Absorbed groups above this many rows are cut into row chunks that are separate work items.  Context option "within_split_rows".
constexpr int64_t kWithinSplitRowsDefault = 16384;

// W_xx = L L' on the host (rec: the statistics record), beta from the two triangular solves, inv = W_xx^-1 (p x p row-major)
static int within_solve(int p, const double* rec, unsigned vary, double* beta, double* inv) {
    for (int j = 0; j < p; ++j)
        if (!((vary >> j) & 1u))
            return fail(PDS_ERR_NUMERIC, "fixed-effects regression: feature column " + std::to_string(j) +
                                             " is constant inside every group (collinear with the absorbed effects)");
    double l[kMaxFeatSmall * kMaxFeatSmall] = {0}, li[kMaxFeatSmall * kMaxFeatSmall] = {0};
    for (int j = 0; j < p; ++j) {
        const double ajj = rec[kMixedRecW + j * 16 + j];
        double d = ajj;
        for (int k = 0; k < j; ++k) d -= l[j * p + k] * l[j * p + k];
        if (!(d > kMixedPivotTol * ajj)) return fail(PDS_ERR_NUMERIC, "fixed-effects regression: the within scatter of the features is not positive definite");
        const double ljj = std::sqrt(d);
        l[j * p + j] = ljj;
        for (int i = j + 1; i < p; ++i) {
            double v = rec[kMixedRecW + i * 16 + j];
            for (int k = 0; k < j; ++k) v -= l[i * p + k] * l[j * p + k];
            l[i * p + j] = v / ljj;
        }
    }
    double z[kMaxFeatSmall];
    for (int i = 0; i < p; ++i) {  // L z = W_xy
        double v = rec[kMixedRecXY + i];
        for (int k = 0; k < i; ++k) v -= l[i * p + k] * z[k];
        z[i] = v / l[i * p + i];
    }
    for (int j = p - 1; j >= 0; --j) {  // L' beta = z
        double v = z[j];
        for (int k = j + 1; k < p; ++k) v -= l[k * p + j] * beta[k];
        beta[j] = v / l[j * p + j];
    }
    for (int j = 0; j < p; ++j) {  // L^-1, then W_xx^-1 = L^-T L^-1
        li[j * p + j] = 1.0 / l[j * p + j];
        for (int i = j + 1; i < p; ++i) {
            double v = 0.0;
            for (int k = j; k < i; ++k) v -= l[i * p + k] * li[k * p + j];
            li[i * p + j] = v / l[i * p + i];
        }
    }
    for (int i = 0; i < p; ++i)
        for (int j = 0; j <= i; ++j) {
            double v = 0.0;
            for (int k = i; k < p; ++k) v += li[k * p + i] * li[k * p + j];
            inv[i * p + j] = inv[j * p + i] = v;
        }
    return PDS_OK;
}

// what: the model's name in front of the message ("fixed-effects regression", "fixed-effects GLM")
static int within_check_se(int se_type, const char* what = "fixed-effects regression") {
    if (se_type >= PDS_HC0 && se_type <= PDS_HC3)
        return fail(PDS_ERR_UNSUPPORTED, std::string(what) + ": HC0 - HC3 standard errors are not available with absorption");
    if (se_type != PDS_SE && se_type != PDS_CLUSTER && se_type != PDS_CLUSTER0)
        return fail(PDS_ERR_INVALID, std::string(what) + ": se_type is PDS_SE, PDS_CLUSTER or PDS_CLUSTER0");
    return PDS_OK;
}

// What the two-factor pipeline (capi_within2.hpp) tells the final stage when it hands it columns that are projected off a second
// factor already.  Absent: the one-factor fit, whose bits do not depend on this struct.
struct WithinMore {
    int64_t extra_df = 0;         // absorbed degrees of freedom beyond one per group
    double tss = 0.0;             // sum (y - ybar)^2 of the ORIGINAL target: r2_overall is formed from it
    const double* css = nullptr;  // [p] sum (x - xbar)^2 of the original features: a feature has to keep ...
    double min_share = 0.0;       // ... more than this share of it, or it is refused as collinear with the absorbed effects
    double* beta_f64 = nullptr;   // [p] out (nullable): beta as solved, before it is rounded to the report's type
};

// cols / offsets live in `space`; the outputs of `extra` (and out_keys' caller) in `out_space`.  d_perm (nullable): row r of this
// frame is row d_perm[r] of the caller's (the by-key form).  R's value type may be narrower than T (f64 columns of an f32 report).
template <typename T, typename R>
static int within_impl(pds_ctx* ctx, const T* const* cols, int n_feat, int64_t n_rows, const int64_t* offsets, int64_t n_groups, pds_space space,
                       pds_space out_space, int se_type, R* out, pds_within_out* extra, const uint32_t* d_perm = nullptr,
                       const WithinMore* more = nullptr, WithinCluster* cl = nullptr) {
    if (!ctx || !cols || !offsets || !out || !out->beta) return fail(PDS_ERR_INVALID, "null argument");
    if (int rc = within_check_se(se_type)) return rc;
    if (n_feat < 1) return fail(PDS_ERR_INVALID, "need at least one feature column");
    if (n_feat > kMaxFeatSmall) return fail(PDS_ERR_UNSUPPORTED, "fixed-effects regression: up to 16 feature columns");
    if (n_rows <= 0 || n_groups <= 0) return fail(PDS_ERR_EMPTY, "Empty data");
    if (int rc = check_cols<T>(cols, n_feat)) return rc;
    // the fit-only call: no standard errors asked for -> beta, r2, adj_r2 alone, and the pass without the meat
    const bool want_se = out->std_err || out->t || out->p || out->ci_lower || out->ci_upper;
    if (want_se && !(out->std_err && out->t && out->p && out->ci_lower && out->ci_upper))
        return fail(PDS_ERR_INVALID, "fixed-effects regression: std_err .. ci_upper are given together or not at all");
    if (int rc = within_cluster_check(cl, se_type, n_rows, want_se)) return rc;
    // a cluster key (capi_within_cluster.hpp): the within pass forms no scores, the meat comes from the gathered row scores
    const bool meat = want_se && se_type != PDS_SE && !cl;
    PDS_HIP_CHECK(hipSetDevice(ctx->device));
    const int p = n_feat;
    // ---- the offsets on the host: validation, the non-empty groups, the chunks of the long ones
    const int64_t split = std::max<int64_t>(ctx->opt_within_split_rows > 0 ? ctx->opt_within_split_rows : kWithinSplitRowsDefault, 64);
    // gmap is the place of a kept group among the caller's groups (alpha)
    GroupFramePlan gp;
    if (int rc = plan_group_frame(ctx, offsets, n_groups, n_rows, space, split, /*cover=*/true, /*want_gmap=*/true,
                                  "absorbed group offsets must be non-decreasing and cover the frame", gp))
        return rc;
    const int64_t n_nonempty = gp.pl.n_nonempty, n_chunks = gp.pl.n_chunks(), n_long = gp.pl.n_long();
    const int64_t extra_df = more ? more->extra_df : 0;
    const int64_t n_all = n_groups, df_se = n_rows - n_nonempty - p - extra_df;
    if (extra) extra->n_groups_used = n_nonempty;
    if (se_type != PDS_SE && !cl && n_nonempty < 2) return fail(PDS_ERR_INVALID, "standard errors clustered on the absorbed key need at least two non-empty groups");
    if (df_se <= 0) return fail(PDS_ERR_TOO_FEW_ROWS, "fixed-effects regression: #rows - #groups - #features <= 0. No conclusive result.");
    const bool empties = gp.pl.dropped();  // (the device works on the non-empty groups alone)
    const int64_t* h_off = gp.pl.h_off;
    n_groups = n_nonempty;
    // ---- workspace (its own block: the by-key form calls this with its ordered frame living in ctx->keyed)
    const bool out_host = out_space == PDS_HOST;
    T *d_alpha = nullptr, *d_pred = nullptr, *d_resid = nullptr;
    StagedOuts g_outs(out_host, (size_t)n_all), row_outs(out_host, (size_t)n_rows);
    if (extra) {
        g_outs.add(&d_alpha, static_cast<T*>(extra->alpha), 1);
        row_outs.add(&d_pred, static_cast<T*>(extra->pred), 1);
        row_outs.add(&d_resid, static_cast<T*>(extra->resid), 1);
    }
    const size_t n_stat = (size_t)mixed_stats_blocks(ctx, n_groups) + (n_chunks > 0 ? (size_t)mixed_stats_blocks(ctx, n_chunks) : 0);
    const size_t n_pass = (size_t)within_pass_blocks(ctx, n_groups) +
                          (n_chunks > 0 ? (size_t)within_pass_blocks(ctx, n_chunks) + (size_t)within_pass_blocks(ctx, n_long) : 0);
    const size_t n_meat = cl ? (size_t)cluster_meat_records(ctx, std::min<int64_t>(n_rows, cl->n_levels)) : 0;
    GroupFrameNeeds needs;
    needs.n_rec = std::max(std::max(n_stat, n_pass), n_meat);
    needs.sum_cols = p + 1;
    needs.scores = true;
    needs.gmap = extra && extra->alpha;
    needs.caller_bytes = g_outs.bytes() + row_outs.bytes() + (cl ? within_cluster_bytes(*cl, n_rows, p, split) : 0);
    GroupFrame<T> f;
    if (int rc = open_group_frame<T>(ctx, gp, cols, nullptr, n_feat, n_rows, space, needs, f)) return rc;
    g_outs.place(f.w);
    row_outs.place(f.w);
    WithinClusterDev cd;
    if (cl)
        if (int rc = within_cluster_open(ctx, f.w, *cl, n_rows, p, split, cd)) return rc;
    // ---- stage 1: the statistics
    if (int rc = launch_mixed_stats<T>(ctx, f.d_tbl, p, f.d_off, n_groups, split, f.ch, nullptr, f.d_means[0], f.d_flags, f.d_partials, f.d_stage,
                                       f.d_rec))
        return rc;
    double stat[kMixedRecStride];
    unsigned vary = 0;
    const bool want_overall = extra != nullptr && !more;
    std::vector<double> my;
    if (want_overall) {
        my.resize((size_t)n_groups);
        PDS_HIP_CHECK(hipMemcpyAsync(my.data(), f.d_means[0] + (size_t)p * n_groups, (size_t)n_groups * 8, hipMemcpyDeviceToHost, ctx->stream));
    }
    PDS_HIP_CHECK(hipMemcpyAsync(stat, f.d_rec, sizeof(stat), hipMemcpyDeviceToHost, ctx->stream));
    PDS_HIP_CHECK(hipMemcpyAsync(&vary, f.d_flags, sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream));
    PDS_HIP_CHECK(hipStreamSynchronize(ctx->stream));  // (f.tbl, gp: sources of the copies)
    if (more && more->css)
        for (int j = 0; j < p; ++j)
            if (!(stat[kMixedRecW + j * 16 + j] > more->min_share * more->css[j]))
                return fail(PDS_ERR_NUMERIC, "fixed-effects regression: feature column " + std::to_string(j) +
                                                 " is a function of the absorbed keys (collinear with the absorbed effects)");
    // ---- stage 2: the solve
    double beta[kMaxFeatSmall] = {0}, inv[kMaxFeatSmall * kMaxFeatSmall];
    if (int rc = within_solve(p, stat, vary, beta, inv)) return rc;
    PDS_HIP_CHECK(hipMemcpyAsync(f.d_beta, beta, sizeof(beta), hipMemcpyHostToDevice, ctx->stream));
    // ---- stage 3: the per-row pass
    if (d_alpha && empties)  // (all bits set is a NaN in both formats: the alpha of an empty group)
        PDS_HIP_CHECK(hipMemsetAsync(d_alpha, 0xFF, (size_t)n_all * sizeof(T), ctx->stream));
    if (int rc = launch_within_pass<T>(ctx, f.d_tbl, p, f.d_off, n_groups, split, f.ch, f.d_scores, f.d_beta, f.d_means[0], meat, f.d_gmap, d_perm,
                                       d_alpha, d_pred, d_resid, f.d_partials, f.d_stage, f.d_rec))
        return rc;
    double rec[kMixedRecStride], crec[kMixedRecStride];
    PDS_HIP_CHECK(hipMemcpyAsync(rec, f.d_rec, sizeof(rec), hipMemcpyDeviceToHost, ctx->stream));
    if (cl) {  // (the records and f.d_rec are free again: the stream has the copy of `rec` in front of these kernels)
        if (int rc = within_cluster_meat<T>(ctx, *cl, cd, f.d_tbl, p, f.d_off, n_groups, split, f.ch, f.d_beta, f.d_means[0], f.d_partials, f.d_stage,
                                            f.d_rec))
            return rc;
        PDS_HIP_CHECK(hipMemcpyAsync(crec, f.d_rec, sizeof(crec), hipMemcpyDeviceToHost, ctx->stream));
    }
    if (int rc = staged_copy_back(ctx, g_outs, (size_t)n_all)) return rc;
    if (int rc = staged_copy_back(ctx, row_outs, (size_t)n_rows)) return rc;
    PDS_HIP_CHECK(hipStreamSynchronize(ctx->stream));  // (beta: source of the copy)
    // ---- the O(p^2) epilogue
    const double sse = rec[kMixedRecYY] + rec[kMixedRecCY], wyy = stat[kMixedRecYY];
    const double nd = (double)n_rows, gd = (double)n_nonempty, xd = (double)extra_df;  // (xd = 0: every term below keeps its bits)
    const double r2 = 1.0 - sse / wyy;
    out->r2 = (T)r2;
    out->adj_r2 = (T)(1.0 - (1.0 - r2) * ((nd - gd - xd) / (double)df_se));
    for (int i = 0; i < p; ++i) out->beta[i] = (T)beta[i];
    if (more && more->beta_f64)
        for (int i = 0; i < p; ++i) more->beta_f64[i] = beta[i];
    const int64_t df = se_type == PDS_SE ? df_se : (cl ? cl->n_clusters : n_nonempty) - 1;
    if (extra && more) {
        extra->r2_overall = 1.0 - sse / more->tss;
        extra->df_resid = df;
    } else if (extra) {
        double ybar = 0.0, between = 0.0;
        for (int64_t g = 0; g < n_groups; ++g) ybar += (double)(h_off[g + 1] - h_off[g]) * my[(size_t)g];
        ybar /= nd;
        for (int64_t g = 0; g < n_groups; ++g) {
            const double d = my[(size_t)g] - ybar;
            between += (double)(h_off[g + 1] - h_off[g]) * d * d;
        }
        extra->r2_overall = 1.0 - sse / (wyy + between);
        extra->df_resid = df;
    }
    if (!want_se) return PDS_OK;
    double se[kMaxFeatSmall];
    if (se_type == PDS_SE) {
        const double s2 = sse / (double)df_se;
        for (int i = 0; i < p; ++i) se[i] = std::sqrt(s2 * inv[i * p + i]);
    } else {
        double factor = se_type == PDS_CLUSTER ? gd / (gd - 1.0) * ((nd - 1.0) / (nd - (double)p - 1.0 - xd)) : 1.0;
        const double* meat_rec = rec;
        if (cl) {  // K counts the effects of a factor that is not nested in the clusters, and one intercept if some factor is
            const int64_t k_par = p + (cl->nested1 ? 0 : n_nonempty) + (cl->nested2 ? 0 : extra_df) + (cl->nested1 || cl->nested2 ? 1 : 0);
            const double gc = (double)cl->n_clusters;
            factor = se_type == PDS_CLUSTER ? gc / (gc - 1.0) * ((nd - 1.0) / (nd - (double)k_par)) : 1.0;
            meat_rec = crec;
        }
        for (int i = 0; i < p; ++i) {
            double acc = 0.0;
            for (int a = 0; a < p; ++a) {
                double t = 0.0;
                for (int b = 0; b < p; ++b) t += meat_rec[kMixedRecW + a * 16 + b] * inv[b * p + i];
                acc += inv[a * p + i] * t;
            }
            se[i] = std::sqrt(acc * factor);
        }
    }
    const double t_alpha = student_t_ppf(0.975, (double)df);
    for (int i = 0; i < p; ++i) {
        out->std_err[i] = (T)se[i];
        const double tv = beta[i] / se[i];
        out->t[i] = (T)tv;
        bool err = false;
        const double sf = student_t_sf_wide(std::fabs(tv), (double)df, &err);
        out->p[i] = err ? (T)NAN : (T)(2.0 * sf);
        out->ci_lower[i] = (T)(beta[i] - t_alpha * se[i]);
        out->ci_upper[i] = (T)(beta[i] + t_alpha * se[i]);
    }
    return PDS_OK;
}

// The by-key form of an absorbed fit, after the caller's null and se_type checks: int64 keys in any row order go through the shared
// key-ordering stage (ordered keys move nothing; `more`, nullable: the pair {weights, offset}, each nullable, rides through the gather
// behind the frame), then inner(kf) runs the contiguous form on the device frame.  max_groups / out_keys matter only with want_alpha:
// alpha and out_keys then have room for max_groups entries.  what: the model's name in front of a message.
template <typename T, typename Inner>
static int absorbed_by_key(pds_ctx* ctx, const T* const* cols, const T* const* more, const int64_t* keys, int n_feat, int64_t n_rows, pds_space space,
                           const char* what, bool want_alpha, int64_t max_groups, int64_t* out_keys, int64_t* n_groups, Inner&& inner) {
    if (n_feat < 1) return fail(PDS_ERR_INVALID, "need at least one feature column");
    if (n_feat > kMaxFeatSmall) return fail(PDS_ERR_UNSUPPORTED, std::string(what) + ": up to 16 feature columns");
    if (n_rows <= 0) return fail(PDS_ERR_EMPTY, "Empty data");
    if (int rc = check_cols<T>(cols, n_feat)) return rc;
    if (want_alpha && max_groups < 1) return fail(PDS_ERR_INVALID, "max_groups must be positive");
    PDS_HIP_CHECK(hipSetDevice(ctx->device));
    KeyedFrame<T> kf;
    kf.src = frame_cols<T>(cols, n_feat);
    for (int k = 0; more && k < 2; ++k)
        if (more[k]) kf.src.push_back(more[k]);
    Bump w{};
    if (int rc = keyed_frame_open<T>(ctx, keys, n_rows, space, want_alpha ? max_groups : n_rows, [](bool) { return (size_t)0; }, n_groups, kf, w))
        return rc;
    if (int rc = inner(kf)) return rc;
    if (want_alpha && out_keys) {
        PDS_HIP_CHECK(hipMemcpyAsync(out_keys, kf.d_unique, (size_t)kf.ng * 8, space == PDS_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice,
                                     ctx->stream));
        PDS_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    }
    return PDS_OK;
}

template <typename T, typename R>
static int within_by_key_impl(pds_ctx* ctx, const T* const* cols, const int64_t* keys, int n_feat, int64_t n_rows, pds_space space, int se_type,
                              int64_t max_groups, int64_t* out_keys, R* out, pds_within_out* extra, int64_t* n_groups,
                              WithinCluster* cl = nullptr) {
    if (!ctx || !cols || !keys || !out || !out->beta || !n_groups) return fail(PDS_ERR_INVALID, "null argument");
    if (int rc = within_check_se(se_type)) return rc;
    const auto inner = [&](const KeyedFrame<T>& kf) {
        if (cl) cl->d_code_perm = kf.d_perm;  // (the cluster codes stay in the caller's row order and are gathered through the permutation)
        return within_impl<T, R>(ctx, kf.src.data(), n_feat, n_rows, kf.d_offsets, kf.ng, PDS_DEVICE, space, se_type, out, extra, kf.d_perm, nullptr,
                                 cl);
    };
    return absorbed_by_key<T>(ctx, cols, nullptr, keys, n_feat, n_rows, space, "fixed-effects regression", extra && extra->alpha, max_groups, out_keys,
                              n_groups, inner);
}
