// capi_mixed.hpp -- the random-intercept linear mixed model fitted by REML (pds_mixed_reml_grouped_* / _by_key_*,
// pds_mixed_profile_grouped_*): what fit_reml (src/linear/mixed/mod.rs:173-272 of the reference) computes, from per-group moments.
// Part of the one translation unit capi.hip (included there, inside namespace pds, in dependency order): the entry-point
// pipelines are templates with internal linkage, split by concern, not by compilation unit.
//
// The reference evaluates the profiled deviance about 80 times, each a full pass over the rows.  Here the frame is streamed a fixed
// number of times (mixed.hip: group means, the within scatter W, the "varies within some group" bits); an evaluation is then a
// reduction over the groups: M(gamma) = [X y]' H^-1 [X y] = W + sum_g c_g [1, m_g] [1, m_g]', c_g = n_g / (1 + gamma n_g).  The host
// adds W, factors M = L L' (y ordered last) and reads everything off L: beta from the leading block, r' H^-1 r = the last pivot,
// ln det(X' H^-1 X) = 2 sum ln L_jj.  The golden section over gamma is the reference's, line by line.  Per evaluation the host
// round trip is the launches of one reduction and ONE blocking copy of a 296-double record (the pattern of glm_irls_impl).
//
// The last pivot is M_yy minus what X explains of it: taken from y itself it is a difference of sums many times its own size and
// loses their rounding errors' digits (measured: 4.5e-14 relative on the residual variance where the reference's own f64 arithmetic
// is good to 3e-16).  So the frame passes run twice: on y, which gives a first GLS solution beta0 (at gamma = 1), then on
// r0 = y - [1, x] . beta0 formed row by row.  Every evaluation then solves for the small correction to beta0, and r' H^-1 r is a
// sum of squares of residual size minus a small term.
#pragma once

// Groups above this many rows are cut into row chunks that are separate work items.  Context option "mixed_split_rows".
constexpr int64_t kMixedSplitRowsDefault = 16384;
constexpr int kMixedQ = kMaxFeatSmall + 2;  // [1, x_0 .. x_15, y]
// a Cholesky pivot of the leading block below this fraction of its diagonal entry: the design is rank deficient in f64
constexpr double kMixedPivotTol = 1e-13;
// ranks for the containment degrees of freedom: a pivot of the column-pivoted Cholesky counts above this fraction of the first
constexpr double kMixedRankTol = 1e-12;

struct MixedFrame {
    int p = 0;
    int64_t n_groups = 0, n_obs = 0, n_nonempty = 0;
    const int64_t* d_off = nullptr;
    double *d_means = nullptr, *d_partials = nullptr, *d_stage = nullptr, *d_rec = nullptr;
    unsigned between = 0;        // bit j: feature j does not vary inside any group
    double beta0[kMixedQ];       // the target the moments are taken of is y - [1, x] . beta0
    double w[kMixedQ * kMixedQ];  // W over [1, x, y], row-major q x q, lower triangle (the intercept row is zero)
};

struct MixedEval {
    double deviance = 0.0, resid_var = 0.0;
    double beta[kMixedQ];
    double l[kMixedQ * kMixedQ];  // the factor of M(gamma), row-major q x q, lower
    double s[kMixedQ * kMixedQ];  // sum_g c_g [1, m, m_y] [1, m, m_y]', lower
};

// rank of a symmetric positive semi-definite m x m matrix (row-major, overwritten) by column-pivoted Cholesky
static int mixed_rank(double* a, int m) {
    int rank = 0;
    double d00 = 0.0;
    for (int k = 0; k < m; ++k) {
        int piv = k;
        for (int i = k + 1; i < m; ++i)
            if (a[i * m + i] > a[piv * m + piv]) piv = i;
        const double d = a[piv * m + piv];
        if (k == 0) d00 = d;
        if (!(d00 > 0.0) || !(d > kMixedRankTol * d00)) break;
        if (piv != k)
            for (int j = 0; j < m; ++j) std::swap(a[k * m + j], a[piv * m + j]);
        if (piv != k)
            for (int i = 0; i < m; ++i) std::swap(a[i * m + k], a[i * m + piv]);
        const double l = std::sqrt(d);
        for (int i = k + 1; i < m; ++i) a[i * m + k] /= l;
        for (int i = k + 1; i < m; ++i)
            for (int j = k + 1; j < m; ++j) a[i * m + j] -= a[i * m + k] * a[j * m + k];
        ++rank;
    }
    return rank;
}

// M(gamma) = W + S, its factor, beta, the residual variance and the profiled REML deviance (profile, mod.rs:121-165)
static int mixed_solve(const MixedFrame& fr, const double* rec, MixedEval& ev) {
    const int p = fr.p, pp = p + 1, q = p + 2;
    double* s = ev.s;
    std::memset(s, 0, sizeof(ev.s));
    s[0] = rec[kMixedRecC];
    for (int i = 0; i < p; ++i) {
        s[(1 + i) * q] = rec[kMixedRecCM + i];
        for (int j = 0; j <= i; ++j) s[(1 + i) * q + 1 + j] = rec[kMixedRecW + i * 16 + j];
        s[(q - 1) * q + 1 + i] = rec[kMixedRecXY + i];
    }
    s[(q - 1) * q] = rec[kMixedRecCY];
    s[(q - 1) * q + q - 1] = rec[kMixedRecYY];
    double* l = ev.l;
    for (int i = 0; i < q; ++i)
        for (int j = 0; j <= i; ++j) l[i * q + j] = fr.w[i * q + j] + s[i * q + j];
    double rhr = 0.0, logdet = 0.0;
    for (int j = 0; j < q; ++j) {
        const double mjj = l[j * q + j];
        double d = mjj;
        for (int k = 0; k < j; ++k) d -= l[j * q + k] * l[j * q + k];
        if (j == q - 1) {
            rhr = d;
            break;
        }
        if (!(d > kMixedPivotTol * mjj)) return fail(PDS_ERR_NUMERIC, "X'HiX is not positive definite; design may be rank-deficient.");
        const double ljj = std::sqrt(d);
        l[j * q + j] = ljj;
        logdet += std::log(ljj);
        for (int i = j + 1; i < q; ++i) {
            double v = l[i * q + j];
            for (int k = 0; k < j; ++k) v -= l[i * q + k] * l[j * q + k];
            l[i * q + j] = v / ljj;
        }
    }
    const double dof = (double)(fr.n_obs - pp);
    ev.resid_var = rhr / dof;
    if (!(ev.resid_var > 0.0)) return fail(PDS_ERR_NUMERIC, "Residual variance estimate is non-positive.");
    for (int j = pp - 1; j >= 0; --j) {  // L11' beta = l_y
        double v = l[(q - 1) * q + j];
        for (int k = j + 1; k < pp; ++k) v -= l[k * q + j] * ev.beta[k];
        ev.beta[j] = v / l[j * q + j];
    }
    for (int j = 0; j < pp; ++j) ev.beta[j] += fr.beta0[j];
    ev.deviance = dof * std::log(ev.resid_var) + rec[kMixedRecLD] + 2.0 * logdet;
    return PDS_OK;
}

static int mixed_eval(pds_ctx* ctx, const MixedFrame& fr, double gamma, MixedEval& ev) {
    if (int rc = launch_mixed_profile(ctx, fr.d_means, fr.p, fr.d_off, fr.n_groups, gamma, fr.d_partials, fr.d_stage, fr.d_rec)) return rc;
    double rec[kMixedRecStride];
    PDS_HIP_CHECK(hipMemcpyAsync(rec, fr.d_rec, sizeof(rec), hipMemcpyDeviceToHost, ctx->stream));
    PDS_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return mixed_solve(fr, rec, ev);
}

// the frame's one-time passes: offsets on the host, the chunk list, means / W / between bits
template <typename T>
static int mixed_prepare(pds_ctx* ctx, const T* const* cols, int n_feat, int64_t n_rows, const int64_t* offsets, int64_t n_groups,
                         pds_space space, MixedFrame& fr) {
    if (!ctx || !cols || !offsets) return fail(PDS_ERR_INVALID, "null argument");
    if (n_feat < 1) return fail(PDS_ERR_INVALID, "need at least one feature column");
    if (n_feat > kMaxFeatSmall) return fail(PDS_ERR_UNSUPPORTED, "mixed model: up to 16 feature columns");
    if (n_groups <= 0 || n_rows <= 0) return fail(PDS_ERR_EMPTY, "Empty data");
    if (int rc = check_cols<T>(cols, n_feat)) return rc;
    PDS_HIP_CHECK(hipSetDevice(ctx->device));
    const int p = n_feat, q = p + 2;
    // ---- the offsets on the host: row counts, validation, the chunks of the long groups (the device works on the non-empty groups alone)
    const int64_t split = std::max<int64_t>(ctx->opt_mixed_split_rows > 0 ? ctx->opt_mixed_split_rows : kMixedSplitRowsDefault, 64);
    GroupFramePlan gp;
    if (int rc = plan_group_frame(ctx, offsets, n_groups, n_rows, space, split, /*cover=*/false, /*want_gmap=*/false,
                                  "group offsets must be non-decreasing and inside the frame", gp))
        return rc;
    const int64_t n_obs = gp.pl.n_obs, n_chunks = gp.pl.n_chunks();
    n_groups = gp.pl.n_nonempty;
    if (n_obs <= p + 1) return fail(PDS_ERR_TOO_FEW_ROWS, "Not enough rows to fit a mixed model with this many fixed effects.");
    // ---- workspace: the shared part alone (beta0 lives in its beta slot)
    static_assert(kMixedQ <= kGroupBetaSlot, "beta0 = [1, x] has room in the frame's beta slot");
    const int n_part = mixed_stats_blocks(ctx, n_groups) + (n_chunks > 0 ? mixed_stats_blocks(ctx, n_chunks) : 0);
    const int n_prof = mixed_profile_blocks(ctx, n_groups);
    GroupFrameNeeds needs;
    needs.n_rec = (size_t)std::max(n_part, n_prof);
    needs.sum_cols = p + 1;
    GroupFrame<T> f;
    if (int rc = open_group_frame<T>(ctx, gp, cols, nullptr, n_feat, n_rows, space, needs, f)) return rc;
    fr.d_off = f.d_off;
    fr.d_means = f.d_means[0];
    fr.d_partials = f.d_partials;
    fr.d_stage = f.d_stage;
    fr.d_rec = f.d_rec;
    fr.p = p;
    fr.n_groups = n_groups;
    fr.n_obs = n_obs;
    fr.n_nonempty = n_groups;
    std::memset(fr.beta0, 0, sizeof(fr.beta0));
    // one run of the frame passes: means, between bits and W of [x, y - [1, x] . beta0]
    auto pass = [&](const double* d_b0) -> int {
        if (int rc = launch_mixed_stats<T>(ctx, f.d_tbl, p, fr.d_off, n_groups, split, f.ch, d_b0, fr.d_means, f.d_flags, fr.d_partials, fr.d_stage,
                                           fr.d_rec))
            return rc;
        double rec[kMixedRecStride];
        unsigned vary = 0;
        PDS_HIP_CHECK(hipMemcpyAsync(rec, fr.d_rec, sizeof(rec), hipMemcpyDeviceToHost, ctx->stream));
        PDS_HIP_CHECK(hipMemcpyAsync(&vary, f.d_flags, sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream));
        PDS_HIP_CHECK(hipStreamSynchronize(ctx->stream));  // (f.tbl, gp, beta0: sources of the copies)
        fr.between = ~vary & ((1u << p) - 1u);
        std::memset(fr.w, 0, sizeof(fr.w));
        auto within = [&](int j) { return ((vary >> j) & 1u) != 0; };
        for (int i = 0; i < p; ++i) {  // a between column's row and column of W are exactly zero
            for (int j = 0; j <= i; ++j)
                if (within(i) && within(j)) fr.w[(1 + i) * q + 1 + j] = rec[kMixedRecW + i * 16 + j];
            if (within(i)) fr.w[(q - 1) * q + 1 + i] = rec[kMixedRecXY + i];
        }
        fr.w[(q - 1) * q + q - 1] = rec[kMixedRecYY];
        return PDS_OK;
    };
    if (int rc = pass(nullptr)) return rc;
    MixedEval ev;
    if (int rc = mixed_eval(ctx, fr, 1.0, ev)) return rc;  // (a design that is not positive definite, a NaN in y: reported here)
    double b0[kMixedQ] = {0};
    for (int j = 0; j <= p; ++j) b0[j] = ev.beta[j];
    PDS_HIP_CHECK(hipMemcpyAsync(f.d_beta, b0, sizeof(double) * (p + 1), hipMemcpyHostToDevice, ctx->stream));
    if (int rc = pass(f.d_beta)) return rc;
    for (int j = 0; j <= p; ++j) fr.beta0[j] = b0[j];
    return PDS_OK;
}

template <typename T>
static int mixed_reml_impl(pds_ctx* ctx, const T* const* cols, int n_feat, int64_t n_rows, const int64_t* offsets, int64_t n_groups,
                           pds_space space, int max_iter, double tol, double* coeffs, double* std_errors, double* dfs, double* gamma_out,
                           double* resid_variance, int64_t* n_groups_fit, int32_t* n_eval) {
    if (!coeffs || !std_errors || !dfs || !gamma_out || !resid_variance || !n_groups_fit || !n_eval) return fail(PDS_ERR_INVALID, "null argument");
    if (max_iter < 0) return fail(PDS_ERR_INVALID, "`max_iter` must not be negative.");
    if (!std::isfinite(tol)) return fail(PDS_ERR_INVALID, "`tol` must be finite.");
    MixedFrame fr;
    if (int rc = mixed_prepare<T>(ctx, cols, n_feat, n_rows, offsets, n_groups, space, fr)) return rc;
    const int p = fr.p, pp = p + 1, q = p + 2;
    MixedEval ev;
    int evals = 0;
    auto dev = [&](double g, double& out) {
        ++evals;
        if (int rc = mixed_eval(ctx, fr, g, ev)) return rc;
        out = ev.deviance;
        return (int)PDS_OK;
    };
    // ---- golden section over gamma in [0, 1e6]: fit_reml, mod.rs:195-219
    const double phi = (std::sqrt(5.0) - 1.0) / 2.0;
    double lo = 0.0, hi = 1e6;
    double c = hi - phi * (hi - lo), e = lo + phi * (hi - lo);
    double fc = 0.0, fe = 0.0;
    if (int rc = dev(c, fc)) return rc;
    if (int rc = dev(e, fe)) return rc;
    for (int it = 0; it < max_iter; ++it) {
        if (hi - lo < tol) break;
        if (fc < fe) {
            hi = e;
            e = c;
            fe = fc;
            c = hi - phi * (hi - lo);
            if (int rc = dev(c, fc)) return rc;
        } else {
            lo = c;
            c = e;
            fc = fe;
            e = lo + phi * (hi - lo);
            if (int rc = dev(e, fe)) return rc;
        }
    }
    const double gamma = (lo + hi) / 2.0;
    double fg = 0.0;
    if (int rc = dev(gamma, fg)) return rc;
    // ---- standard errors: sqrt(resid_var diag((X' H^-1 X)^-1)), the inverse from the factor's leading block
    double li[kMixedQ * kMixedQ];
    for (int j = 0; j < pp; ++j) {
        li[j * q + j] = 1.0 / ev.l[j * q + j];
        for (int i = j + 1; i < pp; ++i) {
            double v = 0.0;
            for (int k = j; k < i; ++k) v -= ev.l[i * q + k] * li[k * q + j];
            li[i * q + j] = v / ev.l[i * q + i];
        }
    }
    for (int j = 0; j < pp; ++j) {
        double v = 0.0;
        for (int k = j; k < pp; ++k) v += li[k * q + j] * li[k * q + j];
        coeffs[j] = ev.beta[j];
        std_errors[j] = std::sqrt(ev.resid_var * v);
    }
    *gamma_out = gamma;
    *resid_variance = ev.resid_var;
    *n_groups_fit = fr.n_nonempty;
    *n_eval = evals;
    // ---- containment degrees of freedom (mod.rs:233-263).  rank([X | Z]) = G + rank(W_xx); the between columns' Gram matrix is
    // sum_g n_g [1, m_g] [1, m_g]' on those columns: the profile sums at gamma = 0
    MixedEval e0;
    {
        if (int rc = launch_mixed_profile(ctx, fr.d_means, p, fr.d_off, fr.n_groups, 0.0, fr.d_partials, fr.d_stage, fr.d_rec)) return rc;
        double rec[kMixedRecStride];
        PDS_HIP_CHECK(hipMemcpyAsync(rec, fr.d_rec, sizeof(rec), hipMemcpyDeviceToHost, ctx->stream));
        PDS_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        std::memset(e0.s, 0, sizeof(e0.s));
        e0.s[0] = rec[kMixedRecC];
        for (int i = 0; i < p; ++i) {
            e0.s[(1 + i) * q] = rec[kMixedRecCM + i];
            for (int j = 0; j <= i; ++j) e0.s[(1 + i) * q + 1 + j] = rec[kMixedRecW + i * 16 + j];
        }
    }
    int bidx[kMixedQ], nb = 0, widx[kMixedQ], nw = 0;
    bidx[nb++] = 0;
    for (int j = 0; j < p; ++j) {
        if ((fr.between >> j) & 1u) bidx[nb++] = 1 + j;
        else widx[nw++] = 1 + j;
    }
    double a[kMixedQ * kMixedQ];
    for (int i = 0; i < nb; ++i)
        for (int j = 0; j < nb; ++j) a[i * nb + j] = e0.s[std::max(bidx[i], bidx[j]) * q + std::min(bidx[i], bidx[j])];
    const int rank_between = mixed_rank(a, nb);
    for (int i = 0; i < nw; ++i)
        for (int j = 0; j < nw; ++j) a[i * nw + j] = fr.w[std::max(widx[i], widx[j]) * q + std::min(widx[i], widx[j])];
    const int rank_within = nw > 0 ? mixed_rank(a, nw) : 0;
    const double ddf_between = (double)fr.n_nonempty - (double)rank_between;
    const double ddf_within = (double)fr.n_obs - (double)(fr.n_nonempty + rank_within);
    dfs[0] = ddf_between;
    for (int j = 0; j < p; ++j) dfs[1 + j] = ((fr.between >> j) & 1u) ? ddf_between : ddf_within;
    return PDS_OK;
}

template <typename T>
static int mixed_profile_impl(pds_ctx* ctx, const T* const* cols, int n_feat, int64_t n_rows, const int64_t* offsets, int64_t n_groups,
                              pds_space space, const double* gammas, int n_gammas, double* deviance, double* beta, double* resid_variance) {
    if (!gammas || !deviance || !beta || !resid_variance) return fail(PDS_ERR_INVALID, "null argument");
    if (n_gammas < 0) return fail(PDS_ERR_INVALID, "negative number of gamma values");
    for (int k = 0; k < n_gammas; ++k)
        if (!(gammas[k] >= 0.0) || !std::isfinite(gammas[k])) return fail(PDS_ERR_INVALID, "gamma values must be finite and not negative");
    MixedFrame fr;
    if (int rc = mixed_prepare<T>(ctx, cols, n_feat, n_rows, offsets, n_groups, space, fr)) return rc;
    MixedEval ev;
    for (int k = 0; k < n_gammas; ++k) {
        if (int rc = mixed_eval(ctx, fr, gammas[k], ev)) return rc;
        deviance[k] = ev.deviance;
        resid_variance[k] = ev.resid_var;
        for (int j = 0; j <= fr.p; ++j) beta[(size_t)k * (fr.p + 1) + j] = ev.beta[j];
    }
    return PDS_OK;
}

// int64 keys in any row order: the shared key-ordering stage (ordered keys move nothing), then the contiguous form on the device frame
template <typename T>
static int mixed_reml_by_key_impl(pds_ctx* ctx, const T* const* cols, const int64_t* keys, int n_feat, int64_t n_rows, pds_space space,
                                  int max_iter, double tol, double* coeffs, double* std_errors, double* dfs, double* gamma_out,
                                  double* resid_variance, int64_t* n_groups_fit, int32_t* n_eval) {
    if (!ctx || !cols || !keys || !coeffs || !std_errors || !dfs || !gamma_out || !resid_variance || !n_groups_fit || !n_eval)
        return fail(PDS_ERR_INVALID, "null argument");
    if (max_iter < 0) return fail(PDS_ERR_INVALID, "`max_iter` must not be negative.");
    if (!std::isfinite(tol)) return fail(PDS_ERR_INVALID, "`tol` must be finite.");
    if (n_feat < 1) return fail(PDS_ERR_INVALID, "need at least one feature column");
    if (n_feat > kMaxFeatSmall) return fail(PDS_ERR_UNSUPPORTED, "mixed model: up to 16 feature columns");
    if (n_rows <= 0) return fail(PDS_ERR_EMPTY, "Empty data");
    if (n_rows <= n_feat + 1) return fail(PDS_ERR_TOO_FEW_ROWS, "Not enough rows to fit a mixed model with this many fixed effects.");
    if (int rc = check_cols<T>(cols, n_feat)) return rc;
    PDS_HIP_CHECK(hipSetDevice(ctx->device));
    KeyedFrame<T> kf;
    kf.src = frame_cols<T>(cols, n_feat);
    Bump w{};
    if (int rc = keyed_frame_open<T>(ctx, keys, n_rows, space, /*max_groups=*/n_rows, [](bool) { return (size_t)0; }, nullptr, kf, w)) return rc;
    return mixed_reml_impl<T>(ctx, kf.src.data(), n_feat, n_rows, kf.d_offsets, kf.ng, PDS_DEVICE, max_iter, tol, coeffs, std_errors, dfs,
                              gamma_out, resid_variance, n_groups_fit, n_eval);
}
