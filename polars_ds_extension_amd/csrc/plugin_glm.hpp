// plugin_glm.hpp -- pl_logistic_coeffs / pl_logistic_pred (the reference's symbols, src/num_ext/logistic_regression.rs) and the
// key-aware pl_glm_by / pl_glm_by_pred (+ _f32): GLM fits by IRLS through pds_glm_irls_grouped_* / pds_glm_irls_by_key_* (with prior
// weights / an offset: pds_glm_irls_wo_grouped_* / pds_glm_irls_wo_by_key_*); pl_glm_report_by
// (+ _f32): the fit and its report per group through pds_glm_report_grouped_* / pds_glm_report_by_key_*
// Part of the one translation unit plugin.cpp (included there, inside its anonymous namespace, after plugin_exprs.hpp).
#pragma once

template <typename T> struct GlmApi;
template <> struct GlmApi<double> {
    static constexpr auto grouped = pds_glm_irls_grouped_f64;
    static constexpr auto by_key = pds_glm_irls_by_key_f64;
    static constexpr auto enet_grouped = pds_glm_enet_grouped_f64;
    static constexpr auto enet_by_key = pds_glm_enet_by_key_f64;
    static constexpr auto wo_grouped = pds_glm_irls_wo_grouped_f64;
    static constexpr auto wo_by_key = pds_glm_irls_wo_by_key_f64;
};
template <> struct GlmApi<float> {
    static constexpr auto grouped = pds_glm_irls_grouped_f32;
    static constexpr auto by_key = pds_glm_irls_by_key_f32;
    static constexpr auto enet_grouped = pds_glm_enet_grouped_f32;
    static constexpr auto enet_by_key = pds_glm_enet_by_key_f32;
    static constexpr auto wo_grouped = pds_glm_irls_wo_grouped_f32;
    static constexpr auto wo_by_key = pds_glm_irls_wo_by_key_f32;
};

// family -> (link, variance) ids of include/pds_lstsq.h, the names of linear_models.GLM_FAMILIES
inline void glm_family_codes(const std::string& family, int* link, int* variance) {
    std::string s;
    for (char c : family) s.push_back((char)std::tolower((unsigned char)c));
    int id = -1;
    if (s == "gaussian" || s == "normal") id = 0;
    else if (s == "poisson") id = 1;
    else if (s == "binomial" || s == "logistic") id = 2;
    else if (s == "gamma") id = 3;
    if (id < 0) raise("unknown GLM family '" + family + "': gaussian / normal, poisson, binomial / logistic, gamma");
    *link = id;
    *variance = id;
}

// test seam: the first capacity guess of pl_glm_by / pl_glm_report_by (<= 0: first_group_capacity's rule), so that the retry can be exercised
int64_t g_glm_by_first_cap = 0;

// ------------------------------------------------------------------------------------------------- pl_glm_by / pl_glm_by_pred (new)
// inputs: [key (integer, any row order, nulls = one group), y, x1..xp]; kwargs bias, null_policy, family, tol, max_iter, and
// l1_reg / l2_reg (absent or <= 0: none): the elastic-net penalised fits through pds_glm_enet_*, called only when a penalty is
// positive -- an unpenalised call goes to the pds_glm_irls_* symbols it always went to.
// pl_glm_by: Struct{<key>, coeffs: List<T>, n_iter: Int32}, one row per group, keys ascending (the null key's group last, with a null
// key), a null list for a null group (fewer rows than coefficients, or a fit that does not end in finite coefficients).
// pl_glm_by_pred: the fitted mean of every row, row for row, null where the row's group is null or a null policy dropped the row.
// Null-free frames make ONE pds_glm_irls_by_key_* call (by_key_with_retry); frames with nulls are prepared on the host
// (prepare_keyed_rows; "ignore" keeps the rows with NaN for the nulls: that group's fit is not finite, so it is a null group) and go
// to the offsets entry point.
// kwargs has_weights / has_offset (absent: false, the call it always was): the inputs are then [key, weights?, offset?, y, x1..xp]
// -- the place pl_lr_by gives its weights -- and the fit goes through pds_glm_irls_wo_by_key_* / _wo_grouped_* (prior weights and an
// offset per row).  A null in the weights or the offset is an error whatever the null policy; nulls elsewhere follow the host
// preparation above, the two columns going through the same row rule.  Not together with a penalty.
template <typename T>
void do_glm_by(SeriesExport* in, size_t n_in, const Kwargs& kw, SeriesExport* out, bool want_pred) {
    const bool has_w = kw_bool(kw, "has_weights"), has_o = kw_bool(kw, "has_offset");
    const size_t n_extra = (has_w ? 1 : 0) + (has_o ? 1 : 0);
    if (n_in < 3 + n_extra) raise("pl_glm_by needs a key, a target and at least one feature");
    int link = 0, variance = 0;
    glm_family_codes(kw_str(kw, "family", "gaussian"), &link, &variance);
    const int max_iter = (int)kw_i64(kw, "max_iter", 100);
    if (max_iter < 1) raise("`max_iter` must be > 1.");
    const T tol = (T)std::fabs(kw_f64(kw, "tol", 1e-8));
    const int bias = kw_bool(kw, "bias") ? 1 : 0;
    const T l1_reg = (T)std::max(kw_f64(kw, "l1_reg"), 0.0), l2_reg = (T)std::max(kw_f64(kw, "l2_reg"), 0.0);
    const bool penalised = l1_reg > T(0) || l2_reg > T(0);
    if (n_extra && penalised) raise("pl_glm_by: l1_reg / l2_reg together with weights / offset is not built");
    const int n_feat = (int)(n_in - 2 - n_extra);
    if (n_feat > 16) raise("grouped GLM (IRLS): up to 16 feature columns");
    const int pp = n_feat + bias;
    // the three steps of keyed_inputs apart: the check of the two columns comes before the lengths', and they move behind the frame
    KeyedInputs<T> ki = keyed_import<T>(in, n_in, kw);  // cols: [weights?, offset?, y, x1..xp]
    for (size_t k = 0; k < n_extra; ++k)
        if (ki.cols[k].null_count > 0) raise("pl_glm_by: nulls in the weights or the offset are an error whatever the null policy");
    keyed_check_lengths(ki);
    std::rotate(ki.cols.begin(), ki.cols.begin() + n_extra, ki.cols.end());  // cols: [y, x1..xp, weights?, offset?]
    keyed_settle(ki, "pl_glm_by");
    const int64_t n = ki.n;
    const size_t iw = (size_t)n_feat + 1, io = iw + (has_w ? 1 : 0);  // where the two columns stand behind the frame
    RawVec<int64_t> keys;
    ByteVec cobuf, itbuf, pred_b;
    RawVec<uint8_t> nulls, row_null;
    std::vector<uint8_t> row_valid;  // pred: one validity byte per row of the frame
    int64_t ng = 0;
    auto size_outputs = [&](int64_t cap) {
        keys.resize(cap);
        cobuf = raw_buffer<T>((size_t)cap * pp);
        itbuf = raw_buffer<int32_t>((size_t)cap);
        nulls.resize(cap);
    };
    if (!ki.any_null) {
        std::vector<const T*> ptrs;
        for (auto& c : ki.cols) ptrs.push_back(c.data());
        if (want_pred) {
            pred_b = raw_buffer<T>((size_t)n);
            row_null.resize(n);
        }
        T* const pr = want_pred ? as<T>(pred_b) : nullptr;
        uint8_t* const rn = want_pred ? row_null.data() : nullptr;
        by_key_with_retry(first_group_capacity(n, g_glm_by_first_cap), size_outputs, [&](int64_t cap) {
            if (n_extra)
                return GlmApi<T>::wo_by_key(thread_ctx(), ptrs.data(), has_w ? ptrs[iw] : nullptr, has_o ? ptrs[io] : nullptr, ki.ikey, n_feat, n,
                                            PDS_HOST, bias, link, variance, tol, max_iter, cap, keys.data(), as<T>(cobuf), as<int32_t>(itbuf),
                                            nulls.data(), &ng, pr, rn);
            return penalised ? GlmApi<T>::enet_by_key(thread_ctx(), ptrs.data(), ki.ikey, n_feat, n, PDS_HOST, bias, link, variance, l1_reg, l2_reg,
                                                      tol, max_iter, cap, keys.data(), as<T>(cobuf), as<int32_t>(itbuf), nulls.data(), &ng, pr, rn)
                             : GlmApi<T>::by_key(thread_ctx(), ptrs.data(), ki.ikey, n_feat, n, PDS_HOST, bias, link, variance, tol, max_iter, cap,
                                                 keys.data(), as<T>(cobuf), as<int32_t>(itbuf), nulls.data(), &ng, pr, rn);
        }, ng);
        if (want_pred) {
            row_valid.resize((size_t)n);
            for (int64_t i = 0; i < n; ++i) row_valid[i] = row_null[i] ? 0 : 1;
        }
    } else {
        const PreparedRows<T> rows = prepare_keyed_rows(ki, keys);
        ng = (int64_t)keys.size();
        const int64_t nk = rows.rows();
        size_outputs(ng);  // (keys already holds its ng values)
        ByteVec pk;
        RawVec<uint8_t> rk;
        if (want_pred) {
            pk = raw_buffer<T>((size_t)nk);
            rk.resize(nk);
        }
        T* const pr = want_pred ? as<T>(pk) : nullptr;
        uint8_t* const rn = want_pred ? rk.data() : nullptr;
        check(n_extra ? GlmApi<T>::wo_grouped(thread_ctx(), rows.ptrs.data(), has_w ? rows.ptrs[iw] : nullptr, has_o ? rows.ptrs[io] : nullptr,
                                              n_feat, nk, rows.off.data(), ng, PDS_HOST, bias, link, variance, tol, max_iter, as<T>(cobuf),
                                              as<int32_t>(itbuf), nulls.data(), pr, rn)
              : penalised ? GlmApi<T>::enet_grouped(thread_ctx(), rows.ptrs.data(), n_feat, nk, rows.off.data(), ng, PDS_HOST, bias, link, variance,
                                                    l1_reg, l2_reg, tol, max_iter, as<T>(cobuf), as<int32_t>(itbuf), nulls.data(), pr, rn)
                          : GlmApi<T>::grouped(thread_ctx(), rows.ptrs.data(), n_feat, nk, rows.off.data(), ng, PDS_HOST, bias, link, variance, tol,
                                               max_iter, as<T>(cobuf), as<int32_t>(itbuf), nulls.data(), pr, rn));
        if (want_pred) {  // back to the frame's rows: a dropped row is a null row
            pred_b = raw_buffer<T>((size_t)n);
            row_valid.assign((size_t)n, 0);
            T* pd = as<T>(pred_b);
            for (int64_t i = 0; i < n; ++i) pd[i] = std::numeric_limits<T>::quiet_NaN();
            const T* ps = as<T>(pk);
            for (int64_t k = 0; k < nk; ++k) {
                pd[rows.src_row[k]] = ps[k];
                row_valid[rows.src_row[k]] = rk[k] ? 0 : 1;
            }
        }
    }
    if (want_pred) {
        bool all_valid = true;
        for (int64_t i = 0; i < n && all_valid; ++i) all_valid = row_valid[i] != 0;
        export_series(out, make_schema(fmt_of<T>(), "pred"), prim_array_take<T>(std::move(pred_b), n, all_valid ? nullptr : row_valid.data()));
        return;
    }
    std::vector<uint8_t> ok;
    group_flags_to_row_valid(nulls.data(), ng, 1, ok);
    std::vector<std::unique_ptr<ArrowArray>> kids;
    kids.push_back(key_array(ki, keys, ng, 1));
    kids.push_back(list_array_take_rows<T>(std::move(cobuf), ng, pp, ok.data()));
    kids.push_back(prim_array_take<int32_t>(std::move(itbuf), ng, nullptr));
    std::vector<std::unique_ptr<ArrowSchema>> sk;
    sk.push_back(key_schema(ki));
    sk.push_back(list_schema<T>("coeffs"));
    sk.push_back(make_schema("i", "n_iter"));
    export_series(out, make_schema("+s", "", std::move(sk)), struct_array(ng, std::move(kids)));
}

// the fields of pl_glm_report_by's Struct behind the key: large-utf8, nine floats, int32
constexpr const char* kGlmReportFields[11] = {"features", "beta", "std_err", "z", "p>|z|", "0.025", "0.975", "deviance", "null_deviance",
                                              "dispersion", "n_iter"};

// ------------------------------------------------------------------------------------------------- pl_glm_report_by (new)
// inputs and kwargs: those of pl_glm_by; a positive l1_reg / l2_reg is an error (penalised fits have no report).  One Struct
// "glm_report" in long format (key_array, features_array, broadcast_rows): n_groups x p' rows {<key>, features,
// beta, std_err, z, p>|z|, 0.025, 0.975, deviance, null_deviance, dispersion, n_iter}, groups in ascending key order (the null key's
// group last, with a null key), coefficients in input order with __bias__ last, the per-group fields broadcast over a group's rows.
// A group with a null report keeps its p' rows with key, features and n_iter set and null numeric fields (beta stays when the fit
// itself is not null).  z and p come from the normal distribution for every family.  Null-free frames make ONE
// pds_glm_report_by_key_* call (by_key_with_retry); frames with nulls are prepared on the host (prepare_keyed_rows) and go to the
// offsets entry point.
template <typename T> struct GlmReportApi;
template <> struct GlmReportApi<double> {
    static constexpr auto grouped = pds_glm_report_grouped_f64;
    static constexpr auto by_key = pds_glm_report_by_key_f64;
    static constexpr auto wo_grouped = pds_glm_report_wo_grouped_f64;
    static constexpr auto wo_by_key = pds_glm_report_wo_by_key_f64;
};
template <> struct GlmReportApi<float> {
    static constexpr auto grouped = pds_glm_report_grouped_f32;
    static constexpr auto by_key = pds_glm_report_by_key_f32;
    static constexpr auto wo_grouped = pds_glm_report_wo_grouped_f32;
    static constexpr auto wo_by_key = pds_glm_report_wo_by_key_f32;
};

template <typename T>
void do_glm_report_by(SeriesExport* in, size_t n_in, const Kwargs& kw, SeriesExport* out) {
    // has_weights / has_offset: as in pl_glm_by -- inputs [key, weights?, offset?, y, x1..xp], pds_glm_report_wo_*
    const bool has_w = kw_bool(kw, "has_weights"), has_o = kw_bool(kw, "has_offset");
    const size_t n_extra = (has_w ? 1 : 0) + (has_o ? 1 : 0);
    if (n_in < 3 + n_extra) raise("pl_glm_report_by needs a key, a target and at least one feature");
    int link = 0, variance = 0;
    glm_family_codes(kw_str(kw, "family", "gaussian"), &link, &variance);
    const int max_iter = (int)kw_i64(kw, "max_iter", 100);
    if (max_iter < 1) raise("`max_iter` must be > 1.");
    if (kw_f64(kw, "l1_reg") > 0.0 || kw_f64(kw, "l2_reg") > 0.0) raise("pl_glm_report_by: penalised fits have no report");
    const T tol = (T)std::fabs(kw_f64(kw, "tol", 1e-8));
    const int bias = kw_bool(kw, "bias") ? 1 : 0;
    const int n_feat = (int)(n_in - 2 - n_extra);
    if (n_feat > 16) raise("grouped GLM (IRLS): up to 16 feature columns");
    const int pp = n_feat + bias;
    KeyedInputs<T> ki = keyed_import<T>(in, n_in, kw);  // cols: [weights?, offset?, y, x1..xp]
    for (size_t k = 0; k < n_extra; ++k)
        if (ki.cols[k].null_count > 0) raise("pl_glm_report_by: nulls in the weights or the offset are an error whatever the null policy");
    keyed_check_lengths(ki);
    std::rotate(ki.cols.begin(), ki.cols.begin() + n_extra, ki.cols.end());  // cols: [y, x1..xp, weights?, offset?]
    keyed_settle(ki, "pl_glm_report_by");
    const size_t iw = (size_t)n_feat + 1, io = iw + (has_w ? 1 : 0);
    RawVec<int64_t> keys;
    ByteVec vb[6], gb[3], itbuf;  // beta, se, z, p, lo, hi [ng][p']; deviance, null_deviance, dispersion [ng]; n_iter [ng]
    RawVec<uint8_t> nulls, rnulls;
    int64_t ng = 0;
    pds_glm_report_out rep{};  // (cov, pearson_chi2, df_resid: not asked for)
    auto size_outputs = [&](int64_t cap) {
        keys.resize(cap);
        for (auto& b : vb) b = raw_buffer<T>((size_t)cap * pp);
        for (auto& b : gb) b = raw_buffer<T>((size_t)cap);
        itbuf = raw_buffer<int32_t>((size_t)cap);
        nulls.resize(cap);
        rnulls.resize(cap);
        rep.std_err = as<T>(vb[1]); rep.z = as<T>(vb[2]); rep.p = as<T>(vb[3]); rep.ci_lower = as<T>(vb[4]); rep.ci_upper = as<T>(vb[5]);
        rep.deviance = as<T>(gb[0]); rep.null_deviance = as<T>(gb[1]); rep.dispersion = as<T>(gb[2]);
        rep.report_null = rnulls.data();
    };
    if (!ki.any_null) {
        std::vector<const T*> ptrs;
        for (auto& c : ki.cols) ptrs.push_back(c.data());
        by_key_with_retry(first_group_capacity(ki.n, g_glm_by_first_cap), size_outputs, [&](int64_t cap) {
            if (n_extra)
                return GlmReportApi<T>::wo_by_key(thread_ctx(), ptrs.data(), has_w ? ptrs[iw] : nullptr, has_o ? ptrs[io] : nullptr, ki.ikey,
                                                  n_feat, ki.n, PDS_HOST, bias, link, variance, tol, max_iter, cap, keys.data(), as<T>(vb[0]),
                                                  as<int32_t>(itbuf), nulls.data(), &ng, &rep);
            return GlmReportApi<T>::by_key(thread_ctx(), ptrs.data(), ki.ikey, n_feat, ki.n, PDS_HOST, bias, link, variance, tol, max_iter, cap,
                                           keys.data(), as<T>(vb[0]), as<int32_t>(itbuf), nulls.data(), &ng, &rep);
        }, ng);
    } else {
        const PreparedRows<T> pr = prepare_keyed_rows(ki, keys);
        ng = (int64_t)keys.size();
        size_outputs(ng);  // (keys already holds its ng values)
        check(n_extra ? GlmReportApi<T>::wo_grouped(thread_ctx(), pr.ptrs.data(), has_w ? pr.ptrs[iw] : nullptr, has_o ? pr.ptrs[io] : nullptr,
                                                    n_feat, pr.rows(), pr.off.data(), ng, PDS_HOST, bias, link, variance, tol, max_iter,
                                                    as<T>(vb[0]), as<int32_t>(itbuf), nulls.data(), &rep)
                      : GlmReportApi<T>::grouped(thread_ctx(), pr.ptrs.data(), n_feat, pr.rows(), pr.off.data(), ng, PDS_HOST, bias, link, variance,
                                                 tol, max_iter, as<T>(vb[0]), as<int32_t>(itbuf), nulls.data(), &rep));
    }
    ki.cols.erase(ki.cols.begin() + n_feat + 1, ki.cols.end());  // (the two columns are no features: the names below are [y, x1..xp]'s)
    // ---- the long frame
    const int64_t rows = ng * pp;
    std::vector<std::unique_ptr<ArrowArray>> kids;
    kids.push_back(key_array(ki, keys, ng, pp));
    kids.push_back(features_array(ki.cols, 1, bias != 0, ng));
    std::vector<uint8_t> fit_valid, rep_valid;
    const uint8_t* vfit = group_flags_to_row_valid(nulls.data(), ng, pp, fit_valid) ? nullptr : fit_valid.data();
    const uint8_t* vr = group_flags_to_row_valid(rnulls.data(), ng, pp, rep_valid) ? nullptr : rep_valid.data();
    kids.push_back(prim_array_take<T>(std::move(vb[0]), rows, vfit));
    for (int k = 1; k < 6; ++k) kids.push_back(prim_array_take<T>(std::move(vb[k]), rows, vr));
    for (auto& b : gb) kids.push_back(prim_array_take<T>(broadcast_rows<T>(b, ng, pp), rows, vr));
    kids.push_back(prim_array_take<int32_t>(broadcast_rows<int32_t>(itbuf, ng, pp), rows, nullptr));
    std::vector<std::unique_ptr<ArrowSchema>> sk;
    sk.push_back(key_schema(ki));
    sk.push_back(make_schema("U", kGlmReportFields[0]));
    for (int i = 1; i < 10; ++i) sk.push_back(make_schema(fmt_of<T>(), kGlmReportFields[i]));
    sk.push_back(make_schema("i", kGlmReportFields[10]));
    export_series(out, make_schema("+s", "glm_report", std::move(sk)), struct_array(rows, std::move(kids)));
}

// ------------------------------------------------------------------------------------------------- pl_logistic_coeffs / pl_logistic_pred
// inputs [y, x1..xp] (Float64, as the reference casts them), kwargs = the reference's lr_kwargs dict (bias, null_policy, l1_reg,
// l2_reg, solver, tol, max_iter).  Deliberate deviation: the reference minimises the mean log loss with L-BFGS from a seeded random
// start; this backend runs IRLS (binomial family, logit link) to the same unpenalised maximum-likelihood point through
// pds_glm_irls_grouped_f64 with ONE group (offsets [0, n]): a frame above the context's glm_split_rows takes the full-device
// iteration, a shorter one the one-wave kernel.  A positive l1_reg / l2_reg is an error, not an unpenalised fit.
// Nulls as series_to_mat_for_lr's mask has them (logistic_regression.rs:76-94; push_kept_row); pred is null where the mask drops a row.
inline void do_logistic(SeriesExport* in, size_t n_in, const Kwargs& kw, SeriesExport* out, bool want_pred) {
    if (n_in < 2) raise("pl_logistic needs a target and at least one feature");
    if (kw_f64(kw, "l1_reg") > 0.0 || kw_f64(kw, "l2_reg") > 0.0)
        raise("logistic_reg: l1_reg / l2_reg are not supported on this backend; use GLM(family='binomial', l2_reg=...) or by=");
    const int max_iter = (int)kw_i64(kw, "max_iter", 200);
    if (max_iter < 1) raise("Input `max_iter` must be a positive.");
    const double tol = std::fabs(kw_f64(kw, "tol", 1e-5));
    const int bias = kw_bool(kw, "bias") ? 1 : 0;
    const int n_feat = (int)n_in - 1, pp = n_feat + bias;
    std::vector<Column<double>> cols = import_all<double>(in, n_in);
    const Policy pol = parse_policy(kw_str(kw, "null_policy", "raise"));
    bool any_null = false;
    for (auto& c : cols) any_null |= c.null_count > 0;
    if (any_null && pol.kind == Policy::RAISE) raise("Nulls found in data");
    const int64_t n = cols[0].size();
    for (auto& c : cols)
        if (c.size() != n) raise("input columns differ in length");
    if (n == 0) raise("Empty data");
    std::vector<int64_t> src_row;  // non-empty: the fit runs on these rows of the frame
    std::vector<std::vector<double>> kept;
    std::vector<const double*> ptrs;
    int64_t nk = n;
    if (any_null) {
        kept.resize(cols.size());
        for (int64_t r = 0; r < n; ++r)
            if (push_kept_row(cols, r, pol, kept)) src_row.push_back(r);
        nk = (int64_t)src_row.size();
        for (auto& v : kept) ptrs.push_back(v.data());
    } else {
        for (auto& c : cols) ptrs.push_back(c.data());
    }
    if (nk == 0) raise("Empty data");
    if (nk < pp) raise("#Data < #features. No conclusive result.");
    const int64_t off[2] = {0, nk};
    ByteVec cobuf = raw_buffer<double>((size_t)pp), pk;
    int32_t its = 0;
    uint8_t gnull = 0;
    RawVec<uint8_t> rk;
    if (want_pred) {
        pk = raw_buffer<double>((size_t)nk);
        rk.resize(nk);
    }
    check(pds_glm_irls_grouped_f64(thread_ctx(), ptrs.data(), n_feat, nk, off, 1, PDS_HOST, bias, 2, 2, tol, max_iter, as<double>(cobuf), &its,
                                   &gnull, want_pred ? as<double>(pk) : nullptr, want_pred ? rk.data() : nullptr));
    if (!want_pred) {
        const uint8_t ok = 1;  // (a fit that did not end in finite coefficients shows them as they are)
        std::vector<int64_t> lo = {0, (int64_t)pp};
        export_series(out, list_schema<double>("coeffs"), list_array<double>(lo, &ok, as<double>(cobuf), pp));
        return;
    }
    if (src_row.empty() && !gnull) {
        export_series(out, make_schema("g", "pred"), prim_array_take<double>(std::move(pk), n, nullptr));
        return;
    }
    ByteVec pf = raw_buffer<double>((size_t)n);
    std::vector<uint8_t> valid((size_t)n, 0);
    double* pd = as<double>(pf);
    for (int64_t i = 0; i < n; ++i) pd[i] = std::numeric_limits<double>::quiet_NaN();
    const double* ps = as<double>(pk);
    for (int64_t k = 0; k < nk; ++k) {
        const int64_t r = src_row.empty() ? k : src_row[k];
        pd[r] = ps[k];
        valid[r] = rk[k] ? 0 : 1;
    }
    export_series(out, make_schema("g", "pred"), prim_array_take<double>(std::move(pf), n, valid.data()));
}
