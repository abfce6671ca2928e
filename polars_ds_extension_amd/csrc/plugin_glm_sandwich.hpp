// plugin_glm_sandwich.hpp -- pl_glm_report_robust (+ _f32): the report of ONE GLM over the whole frame with robust (hc0 / hc1) or
// cluster-robust (cluster / cluster0) standard errors, the clusters given by a key column
// Part of the one translation unit plugin.cpp (included there, inside its anonymous namespace, behind plugin_keyed.hpp and plugin_glm.hpp).
//
// inputs: [cluster key (integer, any row order, nulls = one cluster)]? [weights]? [offset]? y, x1..xp -- which of the three leading
// columns are there is in the kwargs.  kwargs: bias, null_policy, family, tol, max_iter, std_err ("hc0", "hc1", "cluster",
// "cluster0"), has_cluster, has_weights, has_offset.  One Struct "glm_report" of p' rows {features, beta, std_err, z, p>|z|, 0.025,
// 0.975, deviance, null_deviance, dispersion, n_iter, n_clusters}, coefficients in input order with __bias__ last, the model's fields
// broadcast -- from ONE call (pds_glm_report_robust_* / pds_glm_report_cluster_by_key_*).  z and p come from the normal distribution;
// n_clusters is there for a caller who wants t(G - 1) (0 for the hc kinds).  A null report keeps its rows with null numeric fields
// behind beta.  The null key is its own cluster (null_key_stand_in).  A null in the weights or the offset is an error whatever the
// policy.  Nulls in y / x: "raise" fails on the first one; under the other policies the rows are prepared on the host (the row rule of
// the policy; with a key prepare_keyed_rows: rows in key order, a dropped row leaves with its key) and go to
// pds_glm_report_cluster_grouped_* / pds_glm_report_robust_*.  A cluster whose rows were all dropped is empty there and is not counted.
#pragma once

constexpr const char* kGlmRobustFields[12] = {"features", "beta", "std_err", "z", "p>|z|", "0.025", "0.975", "deviance", "null_deviance",
                                              "dispersion", "n_iter", "n_clusters"};

template <typename T> struct GlmRobustApi;
template <> struct GlmRobustApi<double> {
    static constexpr auto robust = pds_glm_report_robust_f64;
    static constexpr auto cluster_grouped = pds_glm_report_cluster_grouped_f64;
    static constexpr auto cluster_by_key = pds_glm_report_cluster_by_key_f64;
};
template <> struct GlmRobustApi<float> {
    static constexpr auto robust = pds_glm_report_robust_f32;
    static constexpr auto cluster_grouped = pds_glm_report_cluster_grouped_f32;
    static constexpr auto cluster_by_key = pds_glm_report_cluster_by_key_f32;
};

template <typename T>
void do_glm_report_robust(SeriesExport* in, size_t n_in, const Kwargs& kw, SeriesExport* out) {
    const char* who = "pl_glm_report_robust";
    const bool has_c = kw_bool(kw, "has_cluster"), has_w = kw_bool(kw, "has_weights"), has_o = kw_bool(kw, "has_offset");
    const size_t n_key = has_c ? 1 : 0, n_extra = (has_w ? 1 : 0) + (has_o ? 1 : 0);
    if (n_in < n_key + n_extra + 2) raise("pl_glm_report_robust needs a target and at least one feature");
    const std::string se = kw_str(kw, "std_err", "hc1");
    int se_type = 0;
    if (se == "hc0") se_type = PDS_HC0;
    else if (se == "hc1") se_type = PDS_HC1;
    else if (se == "cluster") se_type = PDS_CLUSTER;
    else if (se == "cluster0") se_type = PDS_CLUSTER0;
    else if (se == "hc2" || se == "hc3") raise("pl_glm_report_robust: hc2 / hc3 need the leverages and are not built");
    else raise("pl_glm_report_robust: std_err is \"hc0\", \"hc1\", \"cluster\" or \"cluster0\"");
    const bool cluster = se_type == PDS_CLUSTER || se_type == PDS_CLUSTER0;
    if (cluster != has_c) raise("pl_glm_report_robust: a cluster key goes with std_err \"cluster\" / \"cluster0\", and only with them");
    int link = 0, variance = 0;
    glm_family_codes(kw_str(kw, "family", "gaussian"), &link, &variance);
    const int max_iter = (int)kw_i64(kw, "max_iter", 100);
    if (max_iter < 1) raise("`max_iter` must be > 1.");
    const T tol = (T)std::fabs(kw_f64(kw, "tol", 1e-8));
    const int bias = kw_bool(kw, "bias") ? 1 : 0;
    const int n_feat = (int)(n_in - n_key - n_extra - 1);
    if (n_feat > 16) raise("robust GLM report: up to 16 feature columns");
    const int pp = n_feat + bias;
    KeyedInputs<T> ki;  // cols: [weights?, offset?, y, x1..xp]
    if (has_c) {
        ki = keyed_import<T>(in, n_in, kw);
    } else {  // (the same checks in the same order, without a key)
        for (size_t i = 0; i < n_in; ++i) ki.cols.push_back(import_series<T>(in[i]));
        ki.pol = parse_policy(kw_str(kw, "null_policy", "raise"));
        for (auto& c : ki.cols) ki.any_null |= c.null_count > 0;
        if (ki.any_null && ki.pol.kind == Policy::RAISE) raise("Nulls found in data");
        ki.n = ki.cols[0].size();
    }
    for (size_t k = 0; k < n_extra; ++k)
        if (ki.cols[k].null_count > 0) raise("pl_glm_report_robust: nulls in the weights or the offset are an error whatever the null policy");
    keyed_check_lengths(ki);
    std::rotate(ki.cols.begin(), ki.cols.begin() + n_extra, ki.cols.end());  // cols: [y, x1..xp, weights?, offset?]
    if (has_c) keyed_settle(ki, who);
    else if (ki.n == 0) raise("Empty data");
    const size_t iw = (size_t)n_feat + 1, io = iw + (has_w ? 1 : 0);
    std::vector<T> b(pp), s(pp), z(pp), p(pp), lo(pp), hi(pp);
    T group[3];  // deviance, null_deviance, dispersion
    int32_t it = 0;
    uint8_t rnull = 0;
    int64_t ng = 0;
    pds_glm_report_out rep{};  // (cov, pearson_chi2, df_resid: not asked for)
    rep.std_err = s.data(); rep.z = z.data(); rep.p = p.data(); rep.ci_lower = lo.data(); rep.ci_upper = hi.data();
    rep.deviance = &group[0]; rep.null_deviance = &group[1]; rep.dispersion = &group[2];
    rep.report_null = &rnull;
    if (!ki.any_null) {
        std::vector<const T*> ptrs;
        for (auto& c : ki.cols) ptrs.push_back(c.data());
        const T* w = has_w ? ptrs[iw] : nullptr;
        const T* o = has_o ? ptrs[io] : nullptr;
        check(has_c ? GlmRobustApi<T>::cluster_by_key(thread_ctx(), ptrs.data(), w, o, ki.ikey, n_feat, ki.n, PDS_HOST, bias, link, variance, tol,
                                                      max_iter, se_type, b.data(), &it, &rep, &ng)
                    : GlmRobustApi<T>::robust(thread_ctx(), ptrs.data(), w, o, n_feat, ki.n, PDS_HOST, bias, link, variance, tol, max_iter, se_type,
                                              b.data(), &it, &rep, &ng));
    } else if (has_c) {
        RawVec<int64_t> keys;
        const PreparedRows<T> pr = prepare_keyed_rows(ki, keys);
        check(GlmRobustApi<T>::cluster_grouped(thread_ctx(), pr.ptrs.data(), has_w ? pr.ptrs[iw] : nullptr, has_o ? pr.ptrs[io] : nullptr, n_feat,
                                               pr.rows(), pr.off.data(), (int64_t)keys.size(), PDS_HOST, bias, link, variance, tol, max_iter,
                                               se_type, b.data(), &it, &rep, &ng));
    } else {
        std::vector<std::vector<T>> kept(ki.cols.size());
        for (int64_t r = 0; r < ki.n; ++r) push_kept_row(ki.cols, r, ki.pol, kept);
        if (kept[0].empty()) raise("Empty data");
        std::vector<const T*> ptrs;
        for (auto& v : kept) ptrs.push_back(v.data());
        check(GlmRobustApi<T>::robust(thread_ctx(), ptrs.data(), has_w ? ptrs[iw] : nullptr, has_o ? ptrs[io] : nullptr, n_feat,
                                      (int64_t)kept[0].size(), PDS_HOST, bias, link, variance, tol, max_iter, se_type, b.data(), &it, &rep, &ng));
    }
    std::vector<std::string> names;
    for (int i = 1; i <= n_feat; ++i) names.push_back(ki.cols[i].name);
    if (bias) names.push_back("__bias__");
    const std::vector<uint8_t> valid((size_t)pp, rnull ? 0 : 1);
    const uint8_t* vr = rnull ? valid.data() : nullptr;
    std::vector<std::unique_ptr<ArrowArray>> kids;
    kids.push_back(utf8_array(names));
    kids.push_back(prim_array<T>(b.data(), pp, nullptr));
    for (auto* v : {&s, &z, &p, &lo, &hi}) kids.push_back(prim_array<T>(v->data(), pp, vr));
    for (int k = 0; k < 3; ++k) {
        const std::vector<T> wide((size_t)pp, group[k]);
        kids.push_back(prim_array<T>(wide.data(), pp, vr));
    }
    const std::vector<int32_t> its((size_t)pp, it);
    const std::vector<int64_t> ncl((size_t)pp, ng);
    kids.push_back(prim_array<int32_t>(its.data(), pp, nullptr));
    kids.push_back(prim_array<int64_t>(ncl.data(), pp, nullptr));
    std::vector<std::unique_ptr<ArrowSchema>> sk;
    sk.push_back(make_schema("U", kGlmRobustFields[0]));
    for (int i = 1; i < 10; ++i) sk.push_back(make_schema(fmt_of<T>(), kGlmRobustFields[i]));
    sk.push_back(make_schema("i", kGlmRobustFields[10]));
    sk.push_back(make_schema("l", kGlmRobustFields[11]));
    export_series(out, make_schema("+s", "glm_report", std::move(sk)), struct_array(pp, std::move(kids)));
}
