// plugin_within.hpp -- pl_lin_reg_report_within (+ _f32): the fixed-effects regression -- ONE model with an intercept per group of a
// key column, the within estimator (pds_lin_reg_within_*; include/pds_lstsq.h states the definitions)
// Part of the one translation unit plugin.cpp (included there, inside its anonymous namespace, behind plugin_keyed.hpp).
//
// inputs: [key (integer, any row order, nulls = one group), y, x1..xp] -- no intercept column and no `bias`: it is absorbed.  kwargs:
// std_err ("se", "cluster": the clusters are the absorbed groups, "cluster0"), null_policy.  One Struct "lin_reg_report" of the
// report's nine columns, p rows {features, beta, std_err | cluster_se | cluster0_se, t, p>|t|, 0.025, 0.975, r2, adj_r2}; r2 and
// adj_r2 are the within values.  Null key and null policies come from the keyed scaffold exactly as in plugin_cluster.hpp: the null key
// is its own group; nulls in y / x fail under "raise" and are otherwise prepared on the host (prepare_keyed_rows) for the offsets
// entry point, where a group whose rows were all dropped is empty and is not counted.  The effects and the per-row outputs are not
// exported here (lstsq.lin_reg_report(absorb=, return_effects=, return_pred=) has them).
#pragma once

template <typename T>
void do_report_within(SeriesExport* in, size_t n_in, const Kwargs& kw, SeriesExport* out) {
    if (n_in < 3) raise("need a key, a target and at least one feature");
    if (kw_bool(kw, "bias")) raise("pl_lin_reg_report_within: the intercept is absorbed by the group effects (bias must be false)");
    const std::string se = kw_str(kw, "std_err", "se");
    if (se != "se" && se != "cluster" && se != "cluster0") raise("pl_lin_reg_report_within: std_err is \"se\", \"cluster\" or \"cluster0\"");
    const int se_type = se == "se" ? PDS_SE : (se == "cluster" ? PDS_CLUSTER : PDS_CLUSTER0);
    KeyedInputs<T> ki = keyed_inputs<T>(in, n_in, kw, "pl_lin_reg_report_within");
    const auto& cols = ki.cols;  // [y, x1..xp]
    const int n_feat = (int)(n_in - 2);
    const int pp = n_feat;
    std::vector<T> b(pp), s(pp), t(pp), p(pp), lo(pp), hi(pp);
    typename Api<T>::Report rep;
    rep.beta = b.data(); rep.std_err = s.data(); rep.t = t.data(); rep.p = p.data(); rep.ci_lower = lo.data(); rep.ci_upper = hi.data();
    if (!ki.any_null) {
        std::vector<const T*> ptrs;
        for (auto& c : cols) ptrs.push_back(c.data());
        int64_t ng = 0;
        check(Api<T>::within_by_key(thread_ctx(), ptrs.data(), ki.ikey, n_feat, ki.n, PDS_HOST, se_type, ki.n, nullptr, &rep, nullptr, &ng));
    } else {
        RawVec<int64_t> keys;
        const PreparedRows<T> pr = prepare_keyed_rows(ki, keys);
        check(Api<T>::within_grouped(thread_ctx(), pr.ptrs.data(), n_feat, pr.rows(), pr.off.data(), (int64_t)keys.size(), PDS_HOST, se_type, &rep,
                                     nullptr));
    }
    std::vector<std::string> names;
    for (size_t i = 1; i < cols.size(); ++i) names.push_back(cols[i].name);
    std::vector<T> r2(pp, rep.r2), ar2(pp, rep.adj_r2);
    const char* fnames[9] = {"features", "beta", se_type == PDS_SE ? "std_err" : (se_type == PDS_CLUSTER ? "cluster_se" : "cluster0_se"), "t", "p>|t|",
                             "0.025", "0.975", "r2", "adj_r2"};
    std::vector<std::unique_ptr<ArrowArray>> kids;
    kids.push_back(utf8_array(names));
    for (auto* v : {&b, &s, &t, &p, &lo, &hi, &r2, &ar2}) kids.push_back(prim_array<T>(v->data(), pp, nullptr));
    std::vector<std::unique_ptr<ArrowSchema>> sk;
    sk.push_back(make_schema("U", fnames[0]));
    for (int i = 1; i < 9; ++i) sk.push_back(make_schema(fmt_of<T>(), fnames[i]));
    export_series(out, make_schema("+s", "lin_reg_report", std::move(sk)), struct_array(pp, std::move(kids)));
}
