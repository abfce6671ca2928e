// plugin_rcond.hpp -- the key-aware pl_lr_w_rcond_by (+ _f32): lin_reg_w_rcond per group through pds_lr_rcond_by_key_* /
// pds_lr_rcond_grouped_*
// Part of the one translation unit plugin.cpp (included there, inside its anonymous namespace, after plugin_glm.hpp).
#pragma once

template <typename T> struct RcondByApi;
template <> struct RcondByApi<double> {
    static constexpr auto grouped = pds_lr_rcond_grouped_f64;
    static constexpr auto by_key = pds_lr_rcond_by_key_f64;
};
template <> struct RcondByApi<float> {
    static constexpr auto grouped = pds_lr_rcond_grouped_f32;
    static constexpr auto by_key = pds_lr_rcond_by_key_f32;
};

// test seam: the first capacity guess of pl_lr_w_rcond_by (<= 0: first_group_capacity's rule), so that the retry can be exercised
int64_t g_rcond_by_first_cap = 0;

// inputs: [key (integer, any row order, nulls = one group), y, x1..xp]; kwargs: the dict lin_reg_w_rcond sends (bias, null_policy,
// l2_reg, tol = rcond; the floor eps * max(n_g, p') is the device's, per group).
// Struct{<key>, coeffs: List<T>, singular_values: List<T>}, one row per group, keys ascending (the null key's group last, with a null
// key), null lists for a null group (fewer rows than coefficients, NaN / inf in its rows, the all-zero system).
// Null-free frames make ONE pds_lr_rcond_by_key_* call (by_key_with_retry); "raise" on a frame with nulls is the single call's error;
// other policies prepare the rows on the host (prepare_keyed_rows; "ignore" keeps the rows with NaN for the nulls: that group is a
// null group) and go to the offsets entry point.
template <typename T>
void do_lr_rcond_by(SeriesExport* in, size_t n_in, const Kwargs& kw, SeriesExport* out) {
    if (n_in < 3) raise("pl_lr_w_rcond_by needs a key, a target and at least one feature");
    const int bias = kw_bool(kw, "bias") ? 1 : 0;
    const int n_feat = (int)n_in - 2;
    if (n_feat > 16) raise("grouped lin_reg_w_rcond: up to 16 feature columns");
    const int pp = n_feat + bias;
    const T rcond = (T)std::fabs(kw_f64(kw, "tol"));
    const T l2 = (T)kw_f64(kw, "l2_reg");
    const KeyedInputs<T> ki = keyed_inputs<T>(in, n_in, kw, "pl_lr_w_rcond_by");  // cols: [y, x1..xp]
    RawVec<int64_t> keys;
    ByteVec cobuf, svbuf;
    RawVec<uint8_t> nulls;
    int64_t ng = 0;
    auto size_outputs = [&](int64_t cap) {
        keys.resize(cap);
        cobuf = raw_buffer<T>((size_t)cap * pp);
        svbuf = raw_buffer<T>((size_t)cap * pp);
        nulls.resize(cap);
    };
    if (!ki.any_null) {
        std::vector<const T*> ptrs;
        for (auto& c : ki.cols) ptrs.push_back(c.data());
        by_key_with_retry(first_group_capacity(ki.n, g_rcond_by_first_cap), size_outputs, [&](int64_t cap) {
            return RcondByApi<T>::by_key(thread_ctx(), ptrs.data(), ki.ikey, n_feat, ki.n, PDS_HOST, bias, l2, rcond, cap, keys.data(), as<T>(cobuf),
                                         as<T>(svbuf), nulls.data(), &ng);
        }, ng);
    } else {
        const PreparedRows<T> pr = prepare_keyed_rows(ki, keys);
        ng = (int64_t)keys.size();
        size_outputs(ng);  // (keys already holds its ng values)
        check(RcondByApi<T>::grouped(thread_ctx(), pr.ptrs.data(), n_feat, pr.rows(), pr.off.data(), ng, PDS_HOST, bias, l2, rcond, as<T>(cobuf),
                                     as<T>(svbuf), nulls.data()));
    }
    std::vector<uint8_t> ok;
    group_flags_to_row_valid(nulls.data(), ng, 1, ok);
    std::vector<std::unique_ptr<ArrowArray>> kids;
    kids.push_back(key_array(ki, keys, ng, 1));
    kids.push_back(list_array_take_rows<T>(std::move(cobuf), ng, pp, ok.data()));
    kids.push_back(list_array_take_rows<T>(std::move(svbuf), ng, pp, ok.data()));
    std::vector<std::unique_ptr<ArrowSchema>> sk;
    sk.push_back(key_schema(ki));
    sk.push_back(list_schema<T>("coeffs"));
    sk.push_back(list_schema<T>("singular_values"));
    export_series(out, make_schema("+s", "", std::move(sk)), struct_array(ng, std::move(kids)));
}
