// capi_within2.hpp -- fixed-effects regression with TWO absorbed factors (pds_lin_reg_within2_grouped_* / _by_key_*): ONE model with an
// intercept per level of each of two keys, y_i = alpha_g1(i) + gamma_g2(i) + x_i' beta + e_i (firm and year effects: the two-way
// fixed-effects model), fitted without ever forming a dummy column.
// Part of the one translation unit capi.hip (included there, inside namespace pds, in dependency order): the entry-point
// pipelines are templates with internal linkage, split by concern, not by compilation unit.
//
// DEFINITIONS (what this file computes; no equivalence with any package's small-sample conventions is claimed beyond this text).
// n rows, p features (1 .. 16), no intercept column.  Factor 1 has G1 occupied levels, factor 2 G2.  C is the number of connected
// components of the bipartite graph whose edges are the occupied (level1, level2) cells; A = G1 + G2 - C is the rank of the absorbed
// dummies.  z~ is the column z projected off both sets of dummies; X~, y~ the projected features and target:
//     beta solves X~'X~ beta = X~'y~;   e = y~ - X~ beta;   pred = y - e
//     PDS_SE        V = s2 (X~'X~)^-1, s2 = sum e^2 / (n - p - A); t, p and the 95 % interval: Student t, n - p - A degrees of freedom
//                   (student_t_sf_wide, as the one-factor fit)
//     PDS_CLUSTER0  V = (X~'X~)^-1 M (X~'X~)^-1, M = sum_g s_g s_g', s_g = sum_{i in g} x~_i e_i: the clusters are the levels of the
//                   FIRST key
//     PDS_CLUSTER   the same V times G1 / (G1 - 1) * (n - 1) / (n - K), K = p + 1 + (A - G1): the effects of the first factor, nested in
//                   the clusters, count as the one intercept, those of the second factor are counted.  With one factor (A = G1) this is
//                   capi_within.hpp's definition.  Both cluster forms: G1 - 1 degrees of freedom
//     r2 = 1 - sum e^2 / sum y~^2;   adj_r2 = 1 - (1 - r2)(n - A) / (n - A - p);   r2_overall = 1 - sum e^2 / sum (y - ybar)^2
// PROJECTION by alternating sweeps over all p + 1 columns in f64 (f32 frames too).  One sweep subtracts the factor-1 level means, then
// the factor-2 level means; delta = max_j max_level |factor-2 mean subtracted from column j in this sweep| / s_j, s_j the population
// standard deviation of the original column j (from one moment pass: only a scale); the sweeps stop when delta <= absorb_tol
// (> 0; 1e-8 is reghdfe's default).  absorb_max_iter sweeps without that: PDS_ERR_NUMERIC, "did not converge" with the last delta,
// nothing returned.  The device keeps the subtracted means as two tables and forms a row's working value from its original value
// (within2_sweep.hip): the same sweep, two reads of the frame and no write.
// ACCELERATION (context option "within2_accel" = 1, Irons-Tuck; 0, the default: plain sweeps; a DEFINITION, stated in
// include/pds_lstsq.h).  The factor-1 step rebuilds a1 from a2 (a1 += mean1(w - a1 - a2) does not depend on the old a1), so the state of
// the iteration is a2 alone, an affine fixed-point map.  A sweep is exactly the plain sweep; m2(k) is the table of factor-2 level means
// sweep k subtracts (what is added to a2; its scaled maximum is delta).  Cycles of two sweeps:
//     1. sweep, Delta1 = its m2; delta <= tol: stop.     2. sweep, Delta2 = its m2; delta <= tol: stop.
//     3. per column j over the occupied codes of factor 2: d = Delta2 - Delta1, c_j = sum Delta2 d / sum d^2,
//        a2[.][j] -= c_j Delta2[.][j];  c_j = 0 (the column is left alone) when the denominator is 0 or a sum or the quotient is not finite.
// Only a2 is extrapolated (a1 is stale for one factor-1 step); convergence is judged by a sweep's delta alone, the call ends on a sweep,
// absorb_max_iter and n_iter count sweeps and nothing else (an extrapolation after the last sweep allowed is not made).  The two sums of
// a column: per wave of the level kernel over the levels it walks, ascending (the grid depends on the number of occupied codes alone),
// the waves' records added in index order by one wave on the device -- no floating-point atomics, nothing read by the host, no extra
// read of the frame.  The unweighted dot products are the choice: weighting by level counts took 2.5 x the sweeps on the few-movers frame.
// COLLINEARITY.  A feature that is a function of the keys is projected to (numerically) nothing: a feature whose projected sum of
// squares is not above kWithin2ShareFloor = 1e-12, or (1e3 absorb_tol)^2 if that is larger (but at most 1e-4) -- 1e-10 at the default
// tolerance --, times its centred sum of squares sum (x - xbar)^2 is refused by index with PDS_ERR_NUMERIC.  (What a sweep at tolerance delta leaves of
// such a column is of the order delta s_j / (1 - rate) per row; 1e3 covers a convergence rate of 0.999.)
// COMPONENTS.  C comes from the device (within2_graph.hip): every row is an edge between its level of factor 1 and its code of factor
// 2, and hook-and-compress rounds of integer atomicMin label every node with the smallest node index of its component, in at most
// 2 ceil(log2(G1 + n_levels2)) + 1 rounds (the trees of a component halve in two rounds: within2_graph.hip has the argument; more: PDS_ERR_NUMERIC, "component labelling did not finish").  The range of the codes is
// checked by a kernel that reads nothing else, before anything is indexed by a code; the level counts of factor 2 are the run
// boundaries of the ordered codes.  The host reads O(n_levels2 + G1) integers, never O(rows).
// EFFECTS (pds_lin_reg_within2_fx_*; a DEFINITION, stated in include/pds_lstsq.h).  With the tables a1 / a2 the sweeps ended with, beta
// and alpha', the one-factor effects of the projected columns (the final stage's alpha: of the order of absorb_tol):
//     alpha_raw[g] = a1[g][y] - sum_j beta_j a1[g][j] + alpha'[g];   gamma_raw[l] = a2[l][y] - sum_j beta_j a2[l][j]
// and, in every component, c = gamma_raw at the LOWEST occupied code of factor 2 in it:  alpha_g = alpha_raw + c, gamma_l = gamma_raw - c.
//
// Stages: the factor-1 offsets and their chunks (plan_group_chunks); the codes of factor 2 in frame order on the device and their range
// check; the row -> level map, the code ordering (launch_within2_order), the level starts and the graph pass (within2_components);
// launch_within2_init (f64 row-major copy, moments); the sweep loop ON THE HOST, one small blocking copy (the per-wave maxima of delta) per sweep; the projected
// columns written column-major (launch_within2_final) and handed to the FINAL STAGE of the one-factor fit -- within_impl on them with
// factor 1's offsets: its statistics pass, host solve, within pass, scores and meat -- told the extra absorbed degrees of freedom
// G2 - C and the original target's sum of squares; pred / resid from the residuals and the ORIGINAL target (launch_within2_rows_out).
#pragma once

// every level of factor 2 is cut into chunks of at most kWithin2GatherChunkRows gathered rows ("within_split_rows", if smaller, takes
// its place): the constant lives in capi_within_cluster.hpp, whose cluster chunks follow the same rule
constexpr double kWithin2ShareFloor = 1e-12, kWithin2ShareTolFactor = 1e3, kWithin2ShareCap = 1e-4;

template <typename T, typename R>
static int within2_impl(pds_ctx* ctx, const T* const* cols, int n_feat, int64_t n_rows, const int64_t* offsets, int64_t n_groups, pds_space space,
                        const int32_t* codes2, pds_space code_space, int64_t n_levels2, pds_space out_space, int se_type, double tol, int max_iter,
                        R* out, pds_within2_out* extra, const uint32_t* d_perm = nullptr, pds_within2_effects* fx = nullptr,
                        WithinCluster* cl = nullptr) {
    if (!ctx || !cols || !offsets || !codes2 || !out || !out->beta) return fail(PDS_ERR_INVALID, "null argument");
    if (fx && n_groups >= (1ll << 31)) return fail(PDS_ERR_UNSUPPORTED, "fixed-effects regression: the effects of fewer than 2^31 groups per call");
    if (int rc = within_check_se(se_type)) return rc;
    if (n_feat < 1) return fail(PDS_ERR_INVALID, "need at least one feature column");
    if (n_feat > kMaxFeatSmall) return fail(PDS_ERR_UNSUPPORTED, "fixed-effects regression: up to 16 feature columns");
    if (n_rows <= 0 || n_groups <= 0) return fail(PDS_ERR_EMPTY, "Empty data");
    if (n_rows >= (1ll << 31)) return fail(PDS_ERR_UNSUPPORTED, "fixed-effects regression with two absorbed keys: fewer than 2^31 rows per call");
    if (n_levels2 < 1 || n_levels2 >= (1ll << 31)) return fail(PDS_ERR_INVALID, "fixed-effects regression: n_levels2 is in [1, 2^31)");
    if (!(tol > 0.0) || !std::isfinite(tol)) return fail(PDS_ERR_INVALID, "fixed-effects regression: absorb_tol must be > 0");
    if (max_iter < 1) return fail(PDS_ERR_INVALID, "fixed-effects regression: absorb_max_iter must be >= 1");
    if (int rc = check_cols<T>(cols, n_feat)) return rc;
    const bool want_se = out->std_err || out->t || out->p || out->ci_lower || out->ci_upper;
    if (want_se && !(out->std_err && out->t && out->p && out->ci_lower && out->ci_upper))
        return fail(PDS_ERR_INVALID, "fixed-effects regression: std_err .. ci_upper are given together or not at all");
    if (int rc = within_cluster_check(cl, se_type, n_rows, want_se)) return rc;
    PDS_HIP_CHECK(hipSetDevice(ctx->device));
    const int p = n_feat, nc = p + 1;
    const int64_t n = n_rows;
    // ---- factor 1: the offsets on the host, the non-empty levels, the chunks of the long ones
    const int64_t split = std::max<int64_t>(ctx->opt_within_split_rows > 0 ? ctx->opt_within_split_rows : kWithinSplitRowsDefault, 64);
    // the effects of factor 1 go out at the caller's group indices: gmap is the place of a kept group among them
    const bool want_fx1 = fx && (fx->effects1 || fx->component1), want_fx = fx && (want_fx1 || fx->effects2 || fx->component2);
    GroupFramePlan gp;  // (the plan step alone: the offsets of the non-empty levels are always sent, with this pipeline's own workspace)
    if (int rc = plan_group_frame(ctx, offsets, n_groups, n, space, split, /*cover=*/true, /*want_gmap=*/want_fx,
                                  "absorbed group offsets must be non-decreasing and cover the frame", gp))
        return rc;
    const GroupChunkPlan& pl = gp.pl;
    const int64_t* h_off = pl.h_off;
    const int64_t n1 = pl.n_nonempty, n_chunks1 = pl.n_chunks(), n_long1 = pl.n_long();
    if (se_type != PDS_SE && !cl && n1 < 2) return fail(PDS_ERR_INVALID, "standard errors clustered on the absorbed key need at least two non-empty groups");
    // ---- workspace (ctx->ws: the by-key form's ordered frame lives in ctx->keyed, the final stage works in ctx->wkeyed)
    const auto up = Bump::up;
    const bool out_host = out_space == PDS_HOST, want_rows = extra && (extra->pred || extra->resid);
    const int64_t chunk2 = std::max<int64_t>(64, std::min<int64_t>(split, kWithin2GatherChunkRows));
    const int64_t lev_cap = std::min<int64_t>(n, n_levels2), c2_cap = n / chunk2 + lev_cap + 1;
    const int n_init = within2_init_records(ctx, n);
    const size_t sort_temp = within2_order_temp_bytes(n);
    T *d_pred = nullptr, *d_resid = nullptr;
    StagedOuts row_outs(out_host, (size_t)n);
    if (extra) {
        row_outs.add(&d_pred, static_cast<T*>(extra->pred), 1);
        row_outs.add(&d_resid, static_cast<T*>(extra->resid), 1);
    }
    const int64_t n_all = n_groups, n_nodes = n1 + n_levels2;
    T *d_eff1 = nullptr, *d_eff2 = nullptr;
    int32_t *d_comp1 = nullptr, *d_comp2 = nullptr;
    StagedOuts g_outs(out_host, (size_t)n_all), l_outs(out_host, (size_t)n_levels2);
    if (fx) {
        g_outs.add(&d_eff1, static_cast<T*>(fx->effects1), 1);
        g_outs.add(&d_comp1, fx->component1, 1);
        l_outs.add(&d_eff2, static_cast<T*>(fx->effects2), 1);
        l_outs.add(&d_comp2, fx->component2, 1);
        fx->n_graph_rounds = 0;
    }
    const size_t graph_bytes = up((size_t)(n_levels2 + 1) * 4) + 2 * up((size_t)n_nodes * 4) + up(within2_graph_flag_bytes()) +
                               up(within2_graph_count_bytes());
    const size_t fx_bytes = want_fx ? 2 * up((size_t)n1 * 8) + up((size_t)n_levels2 * 8) + up((size_t)n1 * 4) + up(kMaxFeatSmall * 8) +
                                          g_outs.bytes() + l_outs.bytes()
                                    : 0;
    size_t need = graph_bytes + fx_bytes + 8192 + up(sizeof(T*) * 18) + up((size_t)(n1 + 1) * 8) + 9 * up((size_t)(n_chunks1 + n_long1 + 1) * 8) +
                  up((size_t)(n_chunks1 + 1) * nc * 8) + up((size_t)(n_chunks1 + 1) * 4) + 6 * up((size_t)n * 4) + sort_temp +
                  up((size_t)n * nc * 8) + up((size_t)n * 8) + up((size_t)n1 * nc * 8) + up((size_t)n_levels2 * nc * 8) + 2 * up((size_t)c2_cap * 8) +
                  up((size_t)c2_cap * 4) + 3 * up((size_t)lev_cap * 8) + up((size_t)lev_cap * 4) + up((size_t)c2_cap * nc * 8) +
                  up((size_t)n_init * 2 * nc * 8) + 3 * up(64 * 8) + up((size_t)within2_delta_blocks(ctx, lev_cap) * 8) + row_outs.bytes();
    if (space == PDS_HOST) need += up((size_t)n * sizeof(T)) * nc;
    const bool accel = ctx->opt_within2_accel == 1;  // (the option as it stands when the call starts)
    if (accel) need += 2 * up((size_t)n_levels2 * nc * 8) + up((size_t)within2_delta_blocks(ctx, lev_cap) * 2 * nc * 8) + up(64 * 8);
    if (int rc = ensure_ws(ctx, ctx->ws, need)) return rc;
    Bump w{static_cast<char*>(ctx->ws.ptr)};
    std::vector<const T*> src = frame_cols<T>(cols, n_feat);  // reference order [y, x1..xp], device resident
    if (space == PDS_HOST)
        if (int rc = cols_to_device<T>(ctx, w, src, n)) return rc;
    std::vector<const T*> tbl;
    const T** d_tbl = nullptr;
    if (int rc = kernel_order_table<T>(ctx, w, src, n_feat, tbl, d_tbl)) return rc;
    Within2Dev dev;
    dev.n_rows = n;
    dev.n1 = n1;
    dev.split1 = split;
    {
        int64_t* t = w.take<int64_t>((size_t)n1 + 1);
        PDS_HIP_CHECK(hipMemcpyAsync(t, h_off, (size_t)(n1 + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
        dev.d_off1 = t;
    }
    if (int rc = upload_mixed_chunks(ctx, w, pl, nc, dev.ch1)) return rc;
    // ---- the codes of factor 2 in frame order on the device, and their range BEFORE any kernel indexes anything by a code
    const int32_t* d_in = codes2;
    if (code_space == PDS_HOST) {
        int32_t* t = w.take<int32_t>((size_t)n);
        PDS_HIP_CHECK(hipMemcpyAsync(t, codes2, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
        d_in = t;
    }
    int* d_flags = w.take<int>(within2_graph_flag_bytes() / sizeof(int));
    {
        int bad = 0;
        PDS_HIP_CHECK(hipMemsetAsync(d_flags, 0, sizeof(int), ctx->stream));
        if (int rc = launch_within2_range_check(ctx, d_in, n, n_levels2, d_flags)) return rc;
        PDS_HIP_CHECK(hipMemcpyAsync(&bad, d_flags, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        PDS_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        if (bad) return fail(PDS_ERR_INVALID, "fixed-effects regression: a code of the second absorbed key is outside [0, n_levels2)");
    }
    dev.d_code2 = d_in;
    if (d_perm) {
        int32_t* t = w.take<int32_t>((size_t)n);
        if (int rc = launch_within2_gather_codes(ctx, d_in, d_perm, n, t)) return rc;
        dev.d_code2 = t;
    }
    // ---- the row -> level map; the rows in code order; the level counts of factor 2 from the ordered codes (run boundaries)
    uint32_t* d_start = w.take<uint32_t>((size_t)n_levels2 + 1);
    {
        uint32_t* g1 = w.take<uint32_t>((size_t)n);
        if (int rc = launch_within2_row_levels(ctx, dev.d_off1, n1, n, g1)) return rc;
        dev.d_g1 = g1;
        uint32_t *iota = w.take<uint32_t>((size_t)n), *sorted = w.take<uint32_t>((size_t)n), *idx2 = w.take<uint32_t>((size_t)n);
        void* temp = w.take<char>(sort_temp);
        if (int rc = launch_within2_order(ctx, dev.d_code2, n, n_levels2, iota, sorted, idx2, temp, sort_temp)) return rc;
        dev.d_idx2 = idx2;
        if (int rc = launch_within2_level_starts(ctx, sorted, n, n_levels2, d_start)) return rc;
    }
    // ---- the components of the graph of the cells, on the device (within2_graph.hip): the host reads O(n_levels2 + G1) integers from here on
    uint32_t *d_label = w.take<uint32_t>((size_t)n_nodes), *d_root = w.take<uint32_t>((size_t)n_nodes);
    int64_t* d_counts = w.take<int64_t>(within2_graph_count_bytes() / sizeof(int64_t));
    int64_t n_comp = 0;
    int n_rounds = 0;
    if (int rc = within2_components(ctx, dev.d_g1, reinterpret_cast<const uint32_t*>(dev.d_code2), n, n1, n_levels2, nullptr, d_label, d_root, d_flags,
                                    d_counts, nullptr, nullptr, &n_comp, &n_rounds))
        return rc;
    if (fx) fx->n_graph_rounds = n_rounds;
    std::vector<uint32_t> start2;
    try {
        start2.resize((size_t)n_levels2 + 1);
    } catch (const std::bad_alloc&) {
        return fail(PDS_ERR_INVALID, "fixed-effects regression: no host memory for the level counts of the second absorbed key");
    }
    PDS_HIP_CHECK(hipMemcpyAsync(start2.data(), d_start, start2.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
    PDS_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    std::vector<int64_t> c_pos, c_n, l_c0, l_nc, l_n;
    std::vector<int32_t> c_code, l_code;
    {
        int64_t pos = 0;
        for (int64_t l = 0; l < n_levels2; ++l) {
            const int64_t m = (int64_t)start2[(size_t)l + 1] - (int64_t)start2[(size_t)l];
            if (m == 0) continue;
            const int64_t k = (m + chunk2 - 1) / chunk2;
            l_c0.push_back((int64_t)c_pos.size());
            l_nc.push_back(k);
            l_n.push_back(m);
            l_code.push_back((int32_t)l);
            for (int64_t i = 0; i < k; ++i) {
                c_pos.push_back(pos + i * chunk2);
                c_n.push_back(std::min<int64_t>(chunk2, m - i * chunk2));
                c_code.push_back((int32_t)l);
            }
            pos += m;
        }
    }
    const int64_t n2 = (int64_t)l_n.size(), rank_a = n1 + n2 - n_comp, extra_df = n2 - n_comp;
    if (extra) {
        extra->n_groups_used = n1;
        extra->n_groups2_used = n2;
        extra->n_components = n_comp;
        extra->n_iter = 0;
    }
    if (n - p - rank_a <= 0)
        return fail(PDS_ERR_TOO_FEW_ROWS, "fixed-effects regression: #rows - #features - rank of the absorbed effects <= 0. No conclusive result.");
    dev.n_chunks2 = (int64_t)c_pos.size();
    dev.n_lev2 = n2;
    auto put = [&](const auto& h, auto*& d) -> int {
        using U = std::remove_const_t<std::remove_reference_t<decltype(h[0])>>;
        U* t = w.take<U>(h.size());
        PDS_HIP_CHECK(hipMemcpyAsync(t, h.data(), h.size() * sizeof(U), hipMemcpyHostToDevice, ctx->stream));
        d = t;
        return PDS_OK;
    };
    if (int rc = put(c_pos, dev.d_c2_pos)) return rc;
    if (int rc = put(c_n, dev.d_c2_n)) return rc;
    if (int rc = put(c_code, dev.d_c2_code)) return rc;
    if (int rc = put(l_c0, dev.d_l2_c0)) return rc;
    if (int rc = put(l_nc, dev.d_l2_nc)) return rc;
    if (int rc = put(l_n, dev.d_l2_n)) return rc;
    if (int rc = put(l_code, dev.d_l2_code)) return rc;
    dev.d_csum2 = w.take<double>((size_t)dev.n_chunks2 * nc);
    // ---- the f64 copy and the moments
    dev.d_w0 = w.take<double>((size_t)n * nc);
    double* d_init = w.take<double>((size_t)n_init * 2 * nc);
    double* d_mom = w.take<double>(64);
    if (int rc = launch_within2_init<T>(ctx, d_tbl, p, n, dev.d_w0, d_init, d_mom)) return rc;
    double mom[2 * (kMaxFeatSmall + 1)];
    PDS_HIP_CHECK(hipMemcpyAsync(mom, d_mom, sizeof(double) * 2 * nc, hipMemcpyDeviceToHost, ctx->stream));
    PDS_HIP_CHECK(hipStreamSynchronize(ctx->stream));  // (tbl, the chunk lists: sources of the copies)
    double css[kMaxFeatSmall + 1], scale[64] = {0};
    for (int c = 0; c < nc; ++c) {  // (kernel order: the features, then y)
        css[c] = std::max(mom[nc + c] - mom[c] * mom[c] / (double)n, 0.0);
        scale[c] = std::sqrt(css[c] / (double)n);
        if (!(scale[c] > 0.0)) {
            if (c < p) return fail(PDS_ERR_NUMERIC, "fixed-effects regression: feature column " + std::to_string(c) + " is constant or not finite");
            scale[c] = 1.0;
        }
    }
    dev.d_scale = w.take<double>(64);
    PDS_HIP_CHECK(hipMemcpyAsync(dev.d_scale, scale, sizeof(scale), hipMemcpyHostToDevice, ctx->stream));
    dev.d_a1 = w.take<double>((size_t)n1 * nc);
    dev.d_a2 = w.take<double>((size_t)n_levels2 * nc);
    PDS_HIP_CHECK(hipMemsetAsync(dev.d_a1, 0, (size_t)n1 * nc * 8, ctx->stream));
    PDS_HIP_CHECK(hipMemsetAsync(dev.d_a2, 0, (size_t)n_levels2 * nc * 8, ctx->stream));
    const int n_delta = within2_delta_blocks(ctx, n2);
    dev.d_delta = w.take<double>((size_t)n_delta);
    if (accel) {  // Delta1 / Delta2 (written and read at occupied codes only: no memset), a record per wave of the level kernel, c_j
        dev.d_dm1 = w.take<double>((size_t)n_levels2 * nc);
        dev.d_dm2 = w.take<double>((size_t)n_levels2 * nc);
        dev.d_arec = w.take<double>((size_t)n_delta * 2 * nc);
        dev.d_coef = w.take<double>(64);
    }
    double* d_e = want_rows ? w.take<double>((size_t)n) : nullptr;
    row_outs.place(w);
    double *d_alpha1 = nullptr, *d_graw = nullptr, *d_beta = nullptr;
    int64_t* d_gmap = nullptr;
    uint32_t* d_ref = nullptr;
    if (want_fx) {
        d_alpha1 = w.take<double>((size_t)n1);
        d_gmap = w.take<int64_t>((size_t)n1);
        d_graw = w.take<double>((size_t)n_levels2);
        d_ref = w.take<uint32_t>((size_t)n1);
        d_beta = w.take<double>(kMaxFeatSmall);
        g_outs.place(w);
        l_outs.place(w);
    }
    // ---- the sweeps: the loop lives here, bounded by absorb_max_iter.  Accelerated: cycles of two sweeps, the second followed by the
    // extrapolation of a2 unless it converged or was the last sweep allowed; only a sweep's delta is ever looked at
    std::vector<double> h_delta((size_t)n_delta);
    double delta = INFINITY;
    int n_iter = 0;
    bool converged = false;
    while (n_iter < max_iter && !converged) {
        const int phase = accel ? 1 + (n_iter & 1) : 0;
        if (int rc = launch_within2_sweep<T>(ctx, d_tbl, p, dev, phase)) return rc;
        ++n_iter;
        PDS_HIP_CHECK(hipMemcpyAsync(h_delta.data(), dev.d_delta, (size_t)n_delta * 8, hipMemcpyDeviceToHost, ctx->stream));
        PDS_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        delta = 0.0;
        for (double v : h_delta) delta = (v > delta || v != v) ? v : delta;
        if (delta != delta) return fail(PDS_ERR_NUMERIC, "fixed-effects regression: a level mean is not finite (NaN or infinite values in the frame)");
        converged = delta <= tol;
        if (phase == 2 && !converged && n_iter < max_iter)
            if (int rc = launch_within2_extrapolate(ctx, p, dev)) return rc;
    }
    if (extra) extra->n_iter = n_iter;
    if (!converged) {
        char msg[256];
        std::snprintf(msg, sizeof(msg), "fixed-effects regression: the alternating sweeps did not converge in %d sweeps (last delta = %.3e, absorb_tol = %.3e)",
                      n_iter, delta, tol);
        return fail(PDS_ERR_NUMERIC, msg);
    }
    // ---- the final stage: the one-factor fit on the projected columns (they take the place of the f64 copy, which is done with)
    double* d_z = dev.d_w0;
    if (int rc = launch_within2_final<T>(ctx, d_tbl, p, dev, d_z)) return rc;
    std::vector<const double*> zc((size_t)nc);
    zc[0] = d_z + (size_t)p * n;
    for (int j = 0; j < p; ++j) zc[(size_t)j + 1] = d_z + (size_t)j * n;
    const double share = std::min(kWithin2ShareCap, std::max(kWithin2ShareFloor, (kWithin2ShareTolFactor * tol) * (kWithin2ShareTolFactor * tol)));
    WithinMore more;
    more.extra_df = extra_df;
    more.tss = css[p];
    more.css = css;
    more.min_share = share;
    double beta_h[kMaxFeatSmall] = {0};
    more.beta_f64 = want_fx ? beta_h : nullptr;
    pds_within_out wo{};
    wo.resid = d_e;
    wo.alpha = d_alpha1;  // (the one-factor effects of the projected columns: of the order of absorb_tol, they close the identity)
    if (cl) {  // the cluster codes are gathered through the row permutation; factor 2's nestedness walks its ordered row index
        cl->d_code_perm = d_perm;
        cl->d_idx2 = dev.d_idx2;
        cl->d_start2 = d_start;
        cl->n_levels2 = n_levels2;
    }
    if (int rc = within_impl<double, R>(ctx, zc.data(), p, n, dev.d_off1, n1, PDS_DEVICE, PDS_DEVICE, se_type, out, &wo, nullptr, &more, cl)) return rc;
    if (extra) {
        extra->r2_overall = wo.r2_overall;
        extra->df_resid = wo.df_resid;
    }
    if (want_rows) {
        if (int rc = launch_within2_rows_out<T>(ctx, tbl[(size_t)p], d_e, d_perm, n, d_pred, d_resid)) return rc;
        if (int rc = staged_copy_back(ctx, row_outs, (size_t)n)) return rc;
    }
    // ---- the effects: from the tables the sweeps ended with, beta as solved and the labels of the graph pass
    if (want_fx) {
        // beta_h and the plan's map are sources of asynchronous copies: the stream is synchronised at once, so that no error path
        // below can leave this frame while a copy still reads it
        PDS_HIP_CHECK(hipMemcpyAsync(d_beta, beta_h, sizeof(beta_h), hipMemcpyHostToDevice, ctx->stream));
        if (pl.dropped()) PDS_HIP_CHECK(hipMemcpyAsync(d_gmap, pl.gmap.data(), (size_t)n1 * 8, hipMemcpyHostToDevice, ctx->stream));
        PDS_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        if (pl.dropped()) {  // (all bits set: NaN in both formats and -1, what an empty group of the caller's gets)
            if (d_eff1) PDS_HIP_CHECK(hipMemsetAsync(d_eff1, 0xFF, (size_t)n_all * sizeof(T), ctx->stream));
            if (d_comp1) PDS_HIP_CHECK(hipMemsetAsync(d_comp1, 0xFF, (size_t)n_all * 4, ctx->stream));
        }
        if (int rc = launch_within2_effects<T>(ctx, dev.d_a1, dev.d_a2, d_beta, d_alpha1, d_label, pl.dropped() ? d_gmap : nullptr, p, n1, n_levels2, d_graw,
                                               d_ref, d_eff1, d_eff2, d_comp1, d_comp2))
            return rc;
        if (int rc = staged_copy_back(ctx, g_outs, (size_t)n_all)) return rc;
        if (int rc = staged_copy_back(ctx, l_outs, (size_t)n_levels2)) return rc;
    }
    if (want_rows || want_fx) PDS_HIP_CHECK(hipStreamSynchronize(ctx->stream));  // (the staged outputs are with the caller)
    return PDS_OK;
}

// int64 keys of factor 1 in any row order: the shared key-ordering stage, then the contiguous form on the ordered frame; the codes of
// factor 2 stay in the caller's row order and are gathered through the row permutation.
template <typename T, typename R>
static int within2_by_key_impl(pds_ctx* ctx, const T* const* cols, const int64_t* keys, const int32_t* codes2, int64_t n_levels2, int n_feat,
                               int64_t n_rows, pds_space space, int se_type, double tol, int max_iter, R* out, pds_within2_out* extra,
                               int64_t* n_groups, pds_within2_effects* fx = nullptr, WithinCluster* cl = nullptr) {
    if (!ctx || !cols || !keys || !codes2 || !out || !out->beta || !n_groups) return fail(PDS_ERR_INVALID, "null argument");
    // fx->cap1 matters only when an output per level of key 1 is asked for: each then has room for cap1 entries
    const bool want_keys = fx && (fx->effects1 || fx->component1 || fx->keys1);
    if (want_keys && fx->cap1 < 1) return fail(PDS_ERR_INVALID, "max_groups must be positive");
    if (int rc = within_check_se(se_type)) return rc;
    if (n_feat < 1) return fail(PDS_ERR_INVALID, "need at least one feature column");
    if (n_feat > kMaxFeatSmall) return fail(PDS_ERR_UNSUPPORTED, "fixed-effects regression: up to 16 feature columns");
    if (n_rows <= 0) return fail(PDS_ERR_EMPTY, "Empty data");
    if (n_rows >= (1ll << 31)) return fail(PDS_ERR_UNSUPPORTED, "fixed-effects regression with two absorbed keys: fewer than 2^31 rows per call");
    if (int rc = check_cols<T>(cols, n_feat)) return rc;
    PDS_HIP_CHECK(hipSetDevice(ctx->device));
    KeyedFrame<T> kf;
    kf.src = frame_cols<T>(cols, n_feat);
    Bump w{};
    if (int rc = keyed_frame_open<T>(ctx, keys, n_rows, space, want_keys ? fx->cap1 : n_rows, [](bool) { return (size_t)0; }, n_groups, kf, w))
        return rc;
    if (int rc = within2_impl<T, R>(ctx, kf.src.data(), n_feat, n_rows, kf.d_offsets, kf.ng, PDS_DEVICE, codes2, space, n_levels2, space, se_type, tol,
                                    max_iter, out, extra, kf.d_perm, fx, cl))
        return rc;
    if (fx && fx->keys1) {
        PDS_HIP_CHECK(hipMemcpyAsync(fx->keys1, kf.d_unique, (size_t)kf.ng * 8, space == PDS_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice,
                                     ctx->stream));
        PDS_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    }
    return PDS_OK;
}

// The graph pass alone: two dense code columns in any row order -> the component of every level ("mobility groups").
static int absorb_components_impl(pds_ctx* ctx, const int32_t* codes1, int64_t n_levels1, const int32_t* codes2, int64_t n_levels2, int64_t n_rows,
                                  pds_space space, int32_t* component1, int32_t* component2, int64_t* n1, int64_t* n2, int64_t* n_components,
                                  int* n_rounds) {
    if (!ctx || !codes1 || !codes2) return fail(PDS_ERR_INVALID, "null argument");
    if (n_rows <= 0) return fail(PDS_ERR_EMPTY, "Empty data");
    if (n_rows >= (1ll << 31)) return fail(PDS_ERR_UNSUPPORTED, "components of two absorbed keys: fewer than 2^31 rows per call");
    if (n_levels1 < 1 || n_levels1 >= (1ll << 31)) return fail(PDS_ERR_INVALID, "components of two absorbed keys: n_levels1 is in [1, 2^31)");
    if (n_levels2 < 1 || n_levels2 >= (1ll << 31)) return fail(PDS_ERR_INVALID, "components of two absorbed keys: n_levels2 is in [1, 2^31)");
    PDS_HIP_CHECK(hipSetDevice(ctx->device));
    const auto up = Bump::up;
    const bool host = space == PDS_HOST;
    const int64_t n = n_rows, n_nodes = n_levels1 + n_levels2;
    int32_t *d_comp1 = nullptr, *d_comp2 = nullptr;
    StagedOuts outs1(host, (size_t)n_levels1), outs2(host, (size_t)n_levels2);
    outs1.add(&d_comp1, component1, 1);
    outs2.add(&d_comp2, component2, 1);
    const size_t need = 8192 + (host ? 2 * up((size_t)n * 4) : 0) + up(within2_graph_flag_bytes()) + up(within2_graph_count_bytes()) +
                        2 * up((size_t)n_nodes * 4) + up((size_t)n_levels1 * 4) + outs1.bytes() + outs2.bytes();
    if (int rc = ensure_ws(ctx, ctx->ws, need)) return rc;
    Bump w{static_cast<char*>(ctx->ws.ptr)};
    const int32_t* d_c[2] = {codes1, codes2};
    if (host)
        for (const int32_t*& c : d_c) {
            int32_t* t = w.take<int32_t>((size_t)n);
            PDS_HIP_CHECK(hipMemcpyAsync(t, c, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
            c = t;
        }
    // the range of both columns before anything is indexed by a code
    int* d_flags = w.take<int>(within2_graph_flag_bytes() / sizeof(int));
    int bad[2] = {0, 0};
    PDS_HIP_CHECK(hipMemsetAsync(d_flags, 0, sizeof(bad), ctx->stream));
    if (int rc = launch_within2_range_check(ctx, d_c[0], n, n_levels1, d_flags)) return rc;
    if (int rc = launch_within2_range_check(ctx, d_c[1], n, n_levels2, d_flags + 1)) return rc;
    PDS_HIP_CHECK(hipMemcpyAsync(bad, d_flags, sizeof(bad), hipMemcpyDeviceToHost, ctx->stream));
    PDS_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    if (bad[0]) return fail(PDS_ERR_INVALID, "components of two absorbed keys: a code of the first key is outside [0, n_levels1)");
    if (bad[1]) return fail(PDS_ERR_INVALID, "components of two absorbed keys: a code of the second key is outside [0, n_levels2)");
    int64_t* d_counts = w.take<int64_t>(within2_graph_count_bytes() / sizeof(int64_t));
    uint32_t *d_label = w.take<uint32_t>((size_t)n_nodes), *d_root = w.take<uint32_t>((size_t)n_nodes), *d_occ = w.take<uint32_t>((size_t)n_levels1);
    outs1.place(w);
    outs2.place(w);
    const uint32_t *d_u = reinterpret_cast<const uint32_t*>(d_c[0]), *d_v = reinterpret_cast<const uint32_t*>(d_c[1]);
    PDS_HIP_CHECK(hipMemsetAsync(d_occ, 0, (size_t)n_levels1 * 4, ctx->stream));
    if (int rc = launch_within2_mark(ctx, d_u, n, d_occ)) return rc;
    if (int rc = within2_components(ctx, d_u, d_v, n, n_levels1, n_levels2, d_occ, d_label, d_root, d_flags, d_counts, n1, n2, n_components, n_rounds))
        return rc;
    if (d_comp1 || d_comp2) {
        if (int rc = launch_within2_components_out(ctx, d_label, d_occ, n_levels1, n_levels2, d_comp1, d_comp2)) return rc;
        if (int rc = staged_copy_back(ctx, outs1, (size_t)n_levels1)) return rc;
        if (int rc = staged_copy_back(ctx, outs2, (size_t)n_levels2)) return rc;
        PDS_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    }
    return PDS_OK;
}
