// plugin_cluster.hpp -- pl_lin_reg_report_cluster (+ _f32): lin_reg_report of ONE model over the whole frame with cluster-robust
// standard errors, the clusters given by a key column
// Part of the one translation unit plugin.cpp (included there, inside its anonymous namespace, behind plugin_keyed.hpp).
//
// inputs: [key (integer, any row order, nulls = one cluster), y, x1..xp] -- no var(y) input: it is derived from the target.  kwargs:
// bias, std_err ("cluster": CR1, "cluster0": CR0), null_policy.  One Struct "lin_reg_report" of the report's nine columns, p' rows
// {features, beta, cluster_se | cluster0_se, t, p>|t|, 0.025, 0.975, r2, adj_r2}, coefficients in input order with __bias__ last --
// the shape of pl_lin_reg_report -- from ONE call (pds_lin_reg_report_cluster_by_key_*).  The null key is its own cluster
// (null_key_stand_in), as it is its own group elsewhere.  Nulls in y / x: "raise" fails on the first one; under the other policies
// the rows are prepared on the host (prepare_keyed_rows: rows in key order, the row rule of the policy, a dropped row leaves with
// its key) and go to the offsets entry point with var(y) of the ORIGINAL non-null target values, what Polars' `target.var()` hands
// pl_lin_reg_report.  A cluster whose rows were all dropped is empty there and is not counted.
#pragma once

template <typename T>
void do_report_cluster(SeriesExport* in, size_t n_in, const Kwargs& kw, SeriesExport* out) {
    if (n_in < 3) raise("need a key, a target and at least one feature");
    const bool bias = kw_bool(kw, "bias");
    const std::string se = kw_str(kw, "std_err", "cluster");
    if (se != "cluster" && se != "cluster0") raise("pl_lin_reg_report_cluster: std_err is \"cluster\" or \"cluster0\"");
    const int se_type = se == "cluster" ? PDS_CLUSTER : PDS_CLUSTER0;
    KeyedInputs<T> ki = keyed_inputs<T>(in, n_in, kw, "pl_lin_reg_report_cluster");
    const auto& cols = ki.cols;  // [y, x1..xp]
    const int n_feat = (int)(n_in - 2);
    const int pp = n_feat + (bias ? 1 : 0);
    std::vector<T> b(pp), s(pp), t(pp), p(pp), lo(pp), hi(pp);
    typename Api<T>::Report rep;
    rep.beta = b.data(); rep.std_err = s.data(); rep.t = t.data(); rep.p = p.data(); rep.ci_lower = lo.data(); rep.ci_upper = hi.data();
    if (!ki.any_null) {
        std::vector<const T*> ptrs;
        for (auto& c : cols) ptrs.push_back(c.data());
        int64_t ng = 0;
        check(Api<T>::report_cluster_by_key(thread_ctx(), ptrs.data(), ki.ikey, n_feat, ki.n, PDS_HOST, bias, se_type | PDS_REPORT_DERIVE_YVAR,
                                            (T)0, &rep, &ng));
    } else {
        RawVec<int64_t> keys;
        const PreparedRows<T> pr = prepare_keyed_rows(ki, keys);
        // var(y): the sample variance (ddof = 1) of the ORIGINAL non-null target values, dropped rows included, two passes in f64
        double sum = 0.0, ss = 0.0;
        int64_t m = 0;
        for (int64_t r = 0; r < ki.n; ++r)
            if (!is_null_at(cols[0], r)) sum += (double)cols[0].data()[r], ++m;
        const double mean = sum / (double)m;
        for (int64_t r = 0; r < ki.n; ++r)
            if (!is_null_at(cols[0], r)) {
                const double d = (double)cols[0].data()[r] - mean;
                ss += d * d;
            }
        const T y_var = m < 2 ? std::numeric_limits<T>::quiet_NaN() : (T)(ss / (double)(m - 1));
        check(Api<T>::report_cluster_grouped(thread_ctx(), pr.ptrs.data(), n_feat, pr.rows(), pr.off.data(), (int64_t)keys.size(), PDS_HOST, bias,
                                             se_type, y_var, &rep));
    }
    std::vector<std::string> names;
    for (size_t i = 1; i < cols.size(); ++i) names.push_back(cols[i].name);
    if (bias) names.push_back("__bias__");
    std::vector<T> r2(pp, rep.r2), ar2(pp, rep.adj_r2);
    const char* fnames[9] = {"features", "beta", se_type == PDS_CLUSTER ? "cluster_se" : "cluster0_se", "t", "p>|t|", "0.025", "0.975", "r2",
                             "adj_r2"};
    std::vector<std::unique_ptr<ArrowArray>> kids;
    kids.push_back(utf8_array(names));
    for (auto* v : {&b, &s, &t, &p, &lo, &hi, &r2, &ar2}) kids.push_back(prim_array<T>(v->data(), pp, nullptr));
    std::vector<std::unique_ptr<ArrowSchema>> sk;
    sk.push_back(make_schema("U", fnames[0]));
    for (int i = 1; i < 9; ++i) sk.push_back(make_schema(fmt_of<T>(), fnames[i]));
    export_series(out, make_schema("+s", "lin_reg_report", std::move(sk)), struct_array(pp, std::move(kids)));
}
