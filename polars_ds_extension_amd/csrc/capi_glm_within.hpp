// capi_glm_within.hpp -- the fixed-effects GLM (pds_glm_within_grouped_* / _by_key_*): ONE generalised linear model with an intercept
// per group, g(E y_i) = alpha_g(i) + x_i' beta + o_i, fitted by IRLS without ever forming a dummy column.
// Part of the one translation unit capi.hip (included there, inside namespace pds, in dependency order): the entry-point
// pipelines are templates with internal linkage, split by concern, not by compilation unit.
//
// DEFINITIONS (what this file computes; no equivalence with any package's small-sample conventions is claimed).  n rows, p features
// (1 .. 16), no intercept column (it is absorbed), integer groups g(i), optional prior weights pw_i and offsets o_i, link g and
// variance V as in pds_glm_irls_wo_*.
//   Rows and groups that count.  A weight that is negative or not finite, anywhere: PDS_ERR_INVALID.  A row counts if pw_i > 0.  A
//     group is DROPPED if it has no counting row, if (poisson) every counting row has y == 0, or if (binomial) every counting row has
//     y == 0 or every one has y == 1: its effect would be -inf or +inf.  The comparisons are exact and are made once, before the first
//     iteration.  Rows of dropped groups count nowhere.  Gaussian and gamma drop only groups without a counting row.  Singletons that
//     are not dropped stay in.  n_used, G_used: the counting rows of the kept groups, the kept groups.
//   Start.  binomial: mu = (y + 0.5) / 2; otherwise mu = (y + ybar) / 2, ybar = sum pw y / sum pw over the used rows; eta = g(mu).
//   Iteration.  w_i = pw_i / (g'(mu_i)^2 V(mu_i)),  z_i = (eta_i - o_i) + g'(mu_i)(y_i - mu_i),  m_g the w-weighted mean of [x, z] over
//     group g,  W = sum_g sum_{i in g} w_i ([x_i, z_i] - m_g)([x_i, z_i] - m_g)';  beta solves W_xx beta = W_xz;
//     alpha_g = m_z,g - m_x,g . beta;  eta_i = alpha_g + x_i . beta + o_i;  mu = g^-1(eta).  By Frisch-Waugh this is exactly the IRLS
//     step of the design with one dummy column per kept group.
//   Stopping.  beta starts at 0.  The iteration stops when max_j |beta_new,j - beta_j| < tol, or after max_iter iterations; n_iter
//     counts iterations, converged says which of the two ended it.  A beta or W that is not finite: PDS_ERR_NUMERIC.  No step halving.
//   Refusals.  A feature that does not vary inside any kept group (exact comparison with the group's first counting row, once) is
//     refused by its index, as within_solve does; a pivot below kMixedPivotTol of its diagonal: PDS_ERR_NUMERIC;
//     df_resid = n_used - G_used - p <= 0: PDS_ERR_TOO_FEW_ROWS.
//   Report, at the returned beta, alpha and the last W_xx: deviance and Pearson's chi2 as in pds_glm_report_wo_*, summed over the used
//     rows; dispersion phi = 1 (poisson, binomial), chi2 / df_resid (gaussian, gamma).
//     PDS_SE        V = phi W_xx^-1
//     PDS_CLUSTER0  V = W_xx^-1 M W_xx^-1, M = sum_g s_g s_g', s_g = sum_{i in g} r_i (x_i - m_x,g), r_i = pw_i (y_i - mu_i) / (V(mu_i)
//                   g'(mu_i)): the clusters ARE the absorbed groups
//     PDS_CLUSTER   the same V times G / (G - 1) * (n - 1) / (n - p - 1), G = G_used, n = n_used: the linear within definition
//     z, p and the interval use the normal distribution, as every GLM report here does.  The cluster kinds need G_used >= 2.
//   Optional outputs.  alpha per group, NaN for a dropped or empty group; pred = mu_i per row in the caller's row order, NaN on the rows
//     of dropped groups, a value on the zero-weight rows of kept groups.
//
// Stages: (1) launch_glm_within_pre, once: per group the counting rows, sum pw, sum pw y, the drop flag; the "varies" bits; the per-
// group sums come to the host, which adds them in group order (ybar, n_used, G_used).  (2) per iteration launch_glm_within_iter: one
// pass over the frame, ONE blocking copy of the record, the p x p solve on the host (within_solve), beta back to the device; the state
// between iterations is beta and the group means.  (3) launch_glm_within_final: alpha, mu, the deviance, chi2 and the meat in one more
// pass.  Long groups are the chunks of plan_group_chunks (context option "within_split_rows").
#pragma once

template <typename T>
static int glm_within_impl(pds_ctx* ctx, const T* const* cols, const T* weights, const T* offset, int n_feat, int64_t n_rows,
                           const int64_t* offsets, int64_t n_groups, pds_space space, pds_space out_space, int link, int variance, T tol_t,
                           int max_iter, int se_type, pds_glm_within_out* out, const uint32_t* d_perm = nullptr) {
    if (!ctx || !cols || !offsets || !out) return fail(PDS_ERR_INVALID, "null argument");
    if (int rc = within_check_se(se_type, "fixed-effects GLM")) return rc;
    if (n_feat < 1) return fail(PDS_ERR_INVALID, "need at least one feature column");
    if (max_iter < 1) return fail(PDS_ERR_INVALID, "`max_iter` must be > 1.");
    if (link < 0 || link > 3 || variance < 0 || variance > 3) return fail(PDS_ERR_INVALID, "unknown link / variance function");
    if (n_feat > kMaxFeatSmall) return fail(PDS_ERR_UNSUPPORTED, "fixed-effects GLM: up to 16 feature columns");
    if (n_rows <= 0 || n_groups <= 0) return fail(PDS_ERR_EMPTY, "Empty data");
    if (int rc = check_cols<T>(cols, n_feat)) return rc;
    PDS_HIP_CHECK(hipSetDevice(ctx->device));
    const int p = n_feat;
    const double tol = (double)tol_t;
    const bool meat = se_type != PDS_SE;
    // ---- the offsets on the host: validation, the non-empty groups, the chunks of the long ones
    const int64_t split = std::max<int64_t>(ctx->opt_within_split_rows > 0 ? ctx->opt_within_split_rows : kWithinSplitRowsDefault, 64);
    GroupFramePlan gp;
    if (int rc = plan_group_frame(ctx, offsets, n_groups, n_rows, space, split, /*cover=*/true, /*want_gmap=*/true,
                                  "absorbed group offsets must be non-decreasing and cover the frame", gp))
        return rc;
    const int64_t n_all = n_groups, n_chunks = gp.pl.n_chunks(), n_long = gp.pl.n_long();
    const bool empties = gp.pl.dropped();  // (the device works on the non-empty groups alone)
    n_groups = gp.pl.n_nonempty;
    // ---- workspace (its own block: the by-key form calls this with its ordered frame living in ctx->keyed)
    const auto up = Bump::up;
    const bool out_host = out_space == PDS_HOST;
    T *d_alpha = nullptr, *d_pred = nullptr;
    StagedOuts g_outs(out_host, (size_t)n_all), row_outs(out_host, (size_t)n_rows);
    g_outs.add(&d_alpha, static_cast<T*>(out->alpha), 1);
    row_outs.add(&d_pred, static_cast<T*>(out->pred), 1);
    const size_t n_it = (size_t)glm_within_iter_blocks(ctx, n_groups) + (n_chunks > 0 ? (size_t)glm_within_iter_blocks(ctx, n_chunks) : 0);
    const size_t n_fin = (size_t)glm_within_final_blocks(ctx, n_groups) +
                         (n_chunks > 0 ? (size_t)glm_within_final_blocks(ctx, n_chunks) + (size_t)glm_within_final_blocks(ctx, n_long) : 0);
    const T* const wo[2] = {weights, offset};
    GroupFrameNeeds needs;
    needs.n_means = 2;  // (an iteration reads one table and writes the other)
    needs.n_rec = std::max(n_it, n_fin);
    needs.sum_cols = p + 2;
    needs.scores = true;
    needs.gmap = d_alpha != nullptr;
    // this pipeline's own slices: per group the pre-pass sums (3) and the drop flag, per chunk its pre-pass sums (3 + p); the outputs
    needs.caller_bytes = up(3 * (size_t)n_groups * 8) + up((size_t)n_groups * 4) + up((size_t)n_chunks * (3 + p) * 8) + g_outs.bytes() +
                         row_outs.bytes();
    GroupFrame<T> f;
    if (int rc = open_group_frame<T>(ctx, gp, cols, wo, n_feat, n_rows, space, needs, f)) return rc;
    double* d_gstat = f.w.template take<double>(3 * (size_t)n_groups);
    int32_t* d_drop = f.w.template take<int32_t>((size_t)n_groups);
    double* d_cpre = n_chunks > 0 ? f.w.template take<double>((size_t)n_chunks * (3 + p)) : nullptr;
    g_outs.place(f.w);
    row_outs.place(f.w);
    // ---- stage 1: the pre-pass; the per-group sums are added here in group order
    if (int rc = launch_glm_within_pre<T>(ctx, f.d_tbl, p, f.d_off, n_groups, split, f.ch, variance, d_cpre, d_gstat, d_drop, f.d_flags)) return rc;
    std::vector<double> gstat(3 * (size_t)n_groups);
    std::vector<int32_t> drop((size_t)n_groups);
    unsigned flags[2] = {0, 0};
    PDS_HIP_CHECK(hipMemcpyAsync(gstat.data(), d_gstat, gstat.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
    PDS_HIP_CHECK(hipMemcpyAsync(drop.data(), d_drop, drop.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
    PDS_HIP_CHECK(hipMemcpyAsync(flags, f.d_flags, sizeof(flags), hipMemcpyDeviceToHost, ctx->stream));
    PDS_HIP_CHECK(hipStreamSynchronize(ctx->stream));  // (f.tbl, gp: sources of the copies)
    if (flags[1]) return fail(PDS_ERR_INVALID, "fixed-effects GLM: a weight is negative or not finite");
    int64_t n_used = 0, g_used = 0;
    double spw = 0.0, spwy = 0.0;
    for (int64_t g = 0; g < n_groups; ++g) {
        if (drop[(size_t)g]) continue;
        ++g_used;
        n_used += (int64_t)std::llround(gstat[(size_t)g]);
        spw += gstat[(size_t)(n_groups + g)];
        spwy += gstat[(size_t)(2 * n_groups + g)];
    }
    const int64_t df_resid = n_used - g_used - p;
    out->n_groups_used = g_used;
    out->n_groups_dropped = n_groups - g_used;
    out->n_rows_used = n_used;
    out->df_resid = df_resid;
    out->n_iter = 0;
    out->converged = 0;
    if (meat && g_used < 2) return fail(PDS_ERR_INVALID, "standard errors clustered on the absorbed key need at least two kept groups");
    if (df_resid <= 0) return fail(PDS_ERR_TOO_FEW_ROWS, "fixed-effects GLM: #rows - #groups - #features <= 0. No conclusive result.");
    const double ybar = spwy / spw;
    const unsigned vary = flags[0];
    // ---- stage 2: the iteration
    double beta[kMaxFeatSmall] = {0}, beta_new[kMaxFeatSmall] = {0}, inv[kMaxFeatSmall * kMaxFeatSmall], rec[kMixedRecStride];
    PDS_HIP_CHECK(hipMemcpyAsync(f.d_beta, beta, sizeof(beta), hipMemcpyHostToDevice, ctx->stream));
    int cur = 0, n_iter = 0;
    bool converged = false;
    while (n_iter < max_iter && !converged) {
        if (int rc = launch_glm_within_iter<T>(ctx, f.d_tbl, p, f.d_off, n_groups, split, f.ch, d_drop, link, variance, n_iter == 0, ybar, f.d_beta,
                                               f.d_means[cur], f.d_means[cur ^ 1], f.d_partials, f.d_stage, f.d_rec))
            return rc;
        cur ^= 1;  // (the means this iteration wrote)
        ++n_iter;
        PDS_HIP_CHECK(hipMemcpyAsync(rec, f.d_rec, sizeof(rec), hipMemcpyDeviceToHost, ctx->stream));
        PDS_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        for (int i = 0; i < p; ++i) {
            bool ok = std::isfinite(rec[kMixedRecXY + i]);
            for (int j = 0; j < p; ++j) ok = ok && std::isfinite(rec[kMixedRecW + i * 16 + j]);
            if (!ok) return fail(PDS_ERR_NUMERIC, "fixed-effects GLM: the weighted within scatter is not finite (iteration " + std::to_string(n_iter) + ")");
        }
        if (int rc = within_solve(p, rec, vary, beta_new, inv)) return rc;
        double delta = 0.0;
        for (int j = 0; j < p; ++j) {
            if (!std::isfinite(beta_new[j])) return fail(PDS_ERR_NUMERIC, "fixed-effects GLM: a coefficient is not finite (iteration " + std::to_string(n_iter) + ")");
            delta = std::max(delta, std::fabs(beta_new[j] - beta[j]));
            beta[j] = beta_new[j];
        }
        converged = delta < tol;
        PDS_HIP_CHECK(hipMemcpyAsync(f.d_beta, beta, sizeof(beta), hipMemcpyHostToDevice, ctx->stream));
    }
    // ---- stage 3: the final pass at (beta, the last means)
    if (d_alpha && (empties || g_used != n_groups))  // (all bits set is a NaN in both formats: the alpha of an empty or dropped group)
        PDS_HIP_CHECK(hipMemsetAsync(d_alpha, 0xFF, (size_t)n_all * sizeof(T), ctx->stream));
    if (int rc = launch_glm_within_final<T>(ctx, f.d_tbl, p, f.d_off, n_groups, split, f.ch, f.d_scores, d_drop, link, variance, f.d_beta, f.d_means[cur],
                                            meat, f.d_gmap, d_perm, d_alpha, d_pred, f.d_partials, f.d_stage, f.d_rec))
        return rc;
    double fin[kMixedRecStride];
    PDS_HIP_CHECK(hipMemcpyAsync(fin, f.d_rec, sizeof(fin), hipMemcpyDeviceToHost, ctx->stream));
    if (int rc = staged_copy_back(ctx, g_outs, (size_t)n_all)) return rc;
    if (int rc = staged_copy_back(ctx, row_outs, (size_t)n_rows)) return rc;
    PDS_HIP_CHECK(hipStreamSynchronize(ctx->stream));  // (beta: source of the copy)
    // ---- the O(p^2) epilogue
    const double deviance = fin[kMixedRecYY] + fin[kMixedRecCY], pearson = fin[kMixedRecC] + fin[kMixedRecLD];
    const double phi = (variance == 1 || variance == 2) ? 1.0 : pearson / (double)df_resid;
    const double nd = (double)n_used, gd = (double)g_used;
    out->n_iter = n_iter;
    out->converged = converged ? 1 : 0;
    out->deviance = deviance;
    out->pearson_chi2 = pearson;
    out->dispersion = phi;
    double v[kMaxFeatSmall * kMaxFeatSmall];
    if (!meat) {
        for (int k = 0; k < p * p; ++k) v[k] = phi * inv[k];
    } else {
        const double factor = se_type == PDS_CLUSTER ? gd / (gd - 1.0) * ((nd - 1.0) / (nd - (double)p - 1.0)) : 1.0;
        double m[kMaxFeatSmall * kMaxFeatSmall];  // the meat out of the record's 16-wide rows
        for (int i = 0; i < p; ++i)
            for (int j = 0; j < p; ++j) m[i * p + j] = fin[kMixedRecW + i * 16 + j];
        sandwich_cov(p, inv, m, factor, v);
    }
    for (int i = 0; i < p; ++i) {
        const double se = std::sqrt(v[i * p + i]), zv = beta[i] / se;
        out->beta[i] = beta[i];
        out->std_err[i] = se;
        out->z[i] = zv;
        out->p[i] = std::erfc(std::fabs(zv) / 1.4142135623730951);
        out->ci_lower[i] = beta[i] - 1.959963984540054 * se;
        out->ci_upper[i] = beta[i] + 1.959963984540054 * se;
        for (int j = 0; j < p; ++j) out->cov[i * p + j] = v[i * p + j];
    }
    return PDS_OK;
}

// int64 keys in any row order: the shared key-ordering stage (ordered keys move nothing; weights and offset ride through the gather),
// then the contiguous form on the device frame.  max_groups / out_keys matter only when out->alpha is asked for.
template <typename T>
static int glm_within_by_key_impl(pds_ctx* ctx, const T* const* cols, const T* weights, const T* offset, const int64_t* keys, int n_feat,
                                  int64_t n_rows, pds_space space, int link, int variance, T tol, int max_iter, int se_type, int64_t max_groups,
                                  int64_t* out_keys, pds_glm_within_out* out, int64_t* n_groups) {
    if (!ctx || !cols || !keys || !out || !n_groups) return fail(PDS_ERR_INVALID, "null argument");
    const T* const wo[2] = {weights, offset};
    return absorbed_by_key<T>(ctx, cols, wo, keys, n_feat, n_rows, space, "fixed-effects GLM", out->alpha != nullptr, max_groups, out_keys, n_groups,
                              [&](const KeyedFrame<T>& kf) {
        return glm_within_impl<T>(ctx, kf.src.data(), weights ? kf.src[n_feat + 1] : nullptr, offset ? kf.src.back() : nullptr, n_feat, n_rows,
                                  kf.d_offsets, kf.ng, PDS_DEVICE, space, link, variance, tol, max_iter, se_type, out, kf.d_perm);
    });
}
