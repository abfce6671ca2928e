// plugin_multi_by.hpp -- the key-aware pl_lr_multi_by / pl_lr_multi_by_pred (+ _f32): the multi-target fit per group through
// pds_lr_multi_by_key_*
// Part of the one translation unit plugin.cpp (included there, inside its anonymous namespace, after plugin_rcond.hpp).
#pragma once

template <typename T> struct MultiByApi;
template <> struct MultiByApi<double> { static constexpr auto by_key = pds_lr_multi_by_key_f64; };
template <> struct MultiByApi<float> { static constexpr auto by_key = pds_lr_multi_by_key_f32; };

// test seam: the first capacity guess of pl_lr_multi_by (<= 0: first_group_capacity's rule), so that the retry can be exercised
int64_t g_multi_by_first_cap = 0;

// inputs: [key (integer, any row order, nulls = one group), t_0 .. t_{k-1}, x_1 .. x_p]; kwargs: those of pl_lr_multi (bias,
// null_policy, l2_reg, solver, singular_x_tol, last_target_idx = k, counting the targets behind the key).
//   pl_lr_multi_by       Struct{<key>, <t_0 name>: List<T>, ..}, one row per group, keys ascending (the null key's group last, with a
//                        null key); a null group (fewer rows than coefficients, gated, NaN / inf in its rows) has a null list in
//                        EVERY target field
//   pl_lr_multi_by_pred  Struct{<t>_pred, <t>_resid, ..}, one row per INPUT row in the frame's row order; the rows of a null group
//                        are null in every field
// Null policies are series_to_mat_for_multi_lr's (linear_regression.rs:270-349): "raise" on any null; a numeric fill applies to the
// features only, with the reference's error when a target holds a null; every other policy is not supported by the multi-target fit.
// Either way the device sees a null-free frame and ONE pds_lr_multi_by_key_* call serves all k targets.
template <typename T>
void do_lr_multi_by(SeriesExport* in, size_t n_in, const Kwargs& kw, SeriesExport* out, bool want_pred) {
    const int k = (int)kw_i64(kw, "last_target_idx");
    if (k < 1 || n_in < 3 || (size_t)k + 1 >= n_in) raise("pl_lr_multi_by needs a key, targets and at least one feature");
    const int n_feat = (int)n_in - 1 - k;
    if (n_feat > 16 || k > 15) raise("grouped multi-target lin_reg: up to 16 feature columns and 15 targets");
    const int bias = kw_bool(kw, "bias") ? 1 : 0;
    const int pp = n_feat + bias;
    const std::string sv = kw_str(kw, "solver", "qr");
    const int solver = sv == "svd" ? PDS_SOLVER_SVD : (sv == "choleskey" ? PDS_SOLVER_CHOLESKEY : PDS_SOLVER_QR);
    const T l2 = (T)kw_f64(kw, "l2_reg"), tol = (T)kw_f64(kw, "singular_x_tol");
    KeyedInputs<T> ki = keyed_import<T>(in, n_in, kw);  // cols: [t_0 .. t_{k-1}, x_1 .. x_p]; "raise" on a null is raised here
    if (ki.any_null) {
        if (ki.pol.kind != Policy::FILL) raise("The null policy is not supported by multi-target linear regression.");
        for (int t = 0; t < k; ++t)
            if (ki.cols[t].null_count > 0) raise("Filling null doesn't work for multi-target lstsq when there are nulls in any of the targets.");
        for (size_t c = (size_t)k; c < ki.cols.size(); ++c) {
            auto& col = ki.cols[c];
            if (!col.null_count) continue;
            auto& v = col.own();
            for (int64_t r = 0; r < col.size(); ++r)
                if (!bit_get(col.validity.data(), r)) v[r] = (T)ki.pol.fill;
            col.validity.clear();
            col.null_count = 0;
        }
        ki.any_null = false;
    }
    keyed_check_lengths(ki);
    keyed_settle(ki, "pl_lr_multi_by");
    const int64_t n = ki.n;
    std::vector<const T*> ptrs;
    for (auto& c : ki.cols) ptrs.push_back(c.data());
    std::vector<std::unique_ptr<ArrowArray>> kids;
    std::vector<std::unique_ptr<ArrowSchema>> sk;
    if (want_pred) {
        ByteVec pred_b = raw_buffer<T>((size_t)k * n), resid_b = raw_buffer<T>((size_t)k * n);
        RawVec<uint8_t> row_null;
        row_null.resize(n);
        check(MultiByApi<T>::by_key(thread_ctx(), ptrs.data(), ki.ikey, k, n_feat, n, PDS_HOST, bias, l2, solver, tol, n, nullptr, nullptr, nullptr,
                                    nullptr, as<T>(pred_b), as<T>(resid_b), row_null.data()));
        std::vector<uint8_t> valid((size_t)n);
        for (int64_t r = 0; r < n; ++r) valid[r] = row_null[r] ? 0 : 1;
        for (int t = 0; t < k; ++t) {
            kids.push_back(prim_array<T>(as<T>(pred_b) + (size_t)t * n, n, valid.data()));
            kids.push_back(prim_array<T>(as<T>(resid_b) + (size_t)t * n, n, valid.data()));
            sk.push_back(make_schema(fmt_of<T>(), ki.cols[t].name + "_pred"));
            sk.push_back(make_schema(fmt_of<T>(), ki.cols[t].name + "_resid"));
        }
        export_series(out, make_schema("+s", "all_preds", std::move(sk)), struct_array(n, std::move(kids)));
        return;
    }
    RawVec<int64_t> keys;
    ByteVec cobuf;
    RawVec<uint8_t> nulls;
    int64_t ng = 0;
    auto size_outputs = [&](int64_t cap) {
        keys.resize(cap);
        cobuf = raw_buffer<T>((size_t)cap * k * pp);
        nulls.resize(cap);
    };
    by_key_with_retry(first_group_capacity(n, g_multi_by_first_cap), size_outputs, [&](int64_t cap) {
        return MultiByApi<T>::by_key(thread_ctx(), ptrs.data(), ki.ikey, k, n_feat, n, PDS_HOST, bias, l2, solver, tol, cap, keys.data(), as<T>(cobuf),
                                     nulls.data(), &ng, nullptr, nullptr, nullptr);
    }, ng);
    std::vector<uint8_t> ok;
    group_flags_to_row_valid(nulls.data(), ng, 1, ok);
    kids.push_back(key_array(ki, keys, ng, 1));
    sk.push_back(key_schema(ki));
    const T* co = as<T>(cobuf);
    for (int t = 0; t < k; ++t) {  // [g][t][p'] -> one list column per target
        ByteVec one = raw_buffer<T>((size_t)ng * pp);
        T* d = as<T>(one);
        for (int64_t g = 0; g < ng; ++g) std::memcpy(d + g * pp, co + ((size_t)g * k + t) * pp, sizeof(T) * (size_t)pp);
        kids.push_back(list_array_take_rows<T>(std::move(one), ng, pp, ok.data()));
        sk.push_back(list_schema<T>(ki.cols[t].name));
    }
    export_series(out, make_schema("+s", "coeffs", std::move(sk)), struct_array(ng, std::move(kids)));
}
