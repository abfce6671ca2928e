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

// test seam: the first capacity guess of pl_lr_w_rcond_by (<= 0: the default rule of do_lr_by), so that the retry can be exercised
int64_t g_rcond_by_first_cap = 0;

// inputs: [key (integer, any row order, nulls = one group), y, x1..xp]; kwargs: the dict lin_reg_w_rcond sends (bias, null_policy,
// l2_reg, tol = rcond; the floor eps * max(n_g, p') is the device's, per group).
// Struct{<key>, coeffs: List<T>, singular_values: List<T>}, one row per group, keys ascending (the null key's group last, with a null
// key), null lists for a null group (fewer rows than coefficients, NaN / inf in its rows, the all-zero system).
// Null-free frames make ONE pds_lr_rcond_by_key_* call (capacity guess and one retry as do_lr_by); "raise" on a frame with nulls is the
// single call's error; other policies prepare the rows on the host as do_glm_by does -- rows in key order, the policy applied row by
// row inside every group ("skip" drops a row with any null, a fill policy fills the features and drops the rows whose target is
// null, "ignore" keeps the rows with NaN for the nulls: that group is a null group) -- and go to the offsets entry point.
template <typename T>
void do_lr_rcond_by(SeriesExport* in, size_t n_in, const Kwargs& kw, SeriesExport* out) {
    if (n_in < 3) raise("pl_lr_w_rcond_by needs a key, a target and at least one feature");
    const int bias = kw_bool(kw, "bias") ? 1 : 0;
    const int n_feat = (int)n_in - 2;
    if (n_feat > 16) raise("grouped lin_reg_w_rcond: up to 16 feature columns");
    const int pp = n_feat + bias;
    const T rcond = (T)std::fabs(kw_f64(kw, "tol"));
    const T l2 = (T)kw_f64(kw, "l2_reg");
    auto key = import_series<int64_t>(in[0]);
    std::vector<Column<T>> cols;  // [y, x1..xp]
    for (size_t i = 1; i < n_in; ++i) cols.push_back(import_series<T>(in[i]));
    const Policy pol = parse_policy(kw_str(kw, "null_policy", "raise"));
    bool any_null = false;
    for (auto& c : cols) any_null |= c.null_count > 0;
    if (any_null && pol.kind == Policy::RAISE) raise("Nulls found in data");
    const int64_t n = key.size();
    for (auto& c : cols)
        if (c.size() != n) raise("input columns differ in length");
    if (n == 0) raise("Empty data");
    int64_t null_stand_in = 0;
    const bool null_group = null_key_stand_in(key, n, "pl_lr_w_rcond_by", &null_stand_in);
    const int64_t* ikey = key.data();
    RawVec<int64_t> keys;
    ByteVec cobuf, svbuf;
    RawVec<uint8_t> nulls;
    int64_t ng = 0;
    if (!any_null) {
        std::vector<const T*> ptrs;
        for (auto& c : cols) ptrs.push_back(c.data());
        int64_t cap = g_rcond_by_first_cap > 0 ? std::min<int64_t>(g_rcond_by_first_cap, n)
                                               : (n <= ((int64_t)1 << 20) ? n : std::max<int64_t>((int64_t)1 << 20, n / 16));
        for (int attempt = 0;; ++attempt) {
            keys.resize(cap);
            cobuf = raw_buffer<T>((size_t)cap * pp);
            svbuf = raw_buffer<T>((size_t)cap * pp);
            nulls.resize(cap);
            const int rc = RcondByApi<T>::by_key(thread_ctx(), ptrs.data(), ikey, n_feat, n, PDS_HOST, bias, l2, rcond, cap, keys.data(),
                                                 as<T>(cobuf), as<T>(svbuf), nulls.data(), &ng);
            if (rc != 0 && attempt == 0 && ng > cap) {
                cap = ng;
                continue;
            }
            check(rc);
            break;
        }
    } else {
        std::vector<int64_t> perm(n);
        for (int64_t i = 0; i < n; ++i) perm[i] = i;
        bool ordered = true;
        for (int64_t i = 1; i < n && ordered; ++i) ordered = ikey[i] >= ikey[i - 1];
        if (!ordered) std::stable_sort(perm.begin(), perm.end(), [&](int64_t a, int64_t b) { return ikey[a] < ikey[b]; });
        const bool fill = pol.kind == Policy::FILL, skip = pol.kind == Policy::SKIP;
        const size_t nc = cols.size();
        auto is_null = [&](size_t c, int64_t r) { return cols[c].null_count > 0 && !bit_get(cols[c].validity.data(), r); };
        std::vector<std::vector<T>> kept(nc);
        for (auto& v : kept) v.reserve((size_t)n);
        std::vector<int64_t> off;
        const T nanv = std::numeric_limits<T>::quiet_NaN();
        for (int64_t i = 0; i < n; ++i) {
            const int64_t r = perm[i];
            if (i == 0 || ikey[r] != ikey[perm[i - 1]]) {
                off.push_back((int64_t)kept[0].size());
                keys.push_back(ikey[r]);
            }
            bool keep = true;
            if (skip)
                for (size_t c = 0; c < nc && keep; ++c) keep = !is_null(c, r);
            else if (fill)
                keep = !is_null(0, r);
            if (!keep) continue;
            for (size_t c = 0; c < nc; ++c) kept[c].push_back(is_null(c, r) ? (fill ? (T)pol.fill : nanv) : cols[c].data()[r]);
        }
        off.push_back((int64_t)kept[0].size());
        ng = (int64_t)keys.size();
        const int64_t nk = (int64_t)kept[0].size();
        if (nk == 0) raise("Empty data");
        std::vector<const T*> ptrs;
        for (auto& v : kept) ptrs.push_back(v.data());
        cobuf = raw_buffer<T>((size_t)ng * pp);
        svbuf = raw_buffer<T>((size_t)ng * pp);
        nulls.resize(ng);
        check(RcondByApi<T>::grouped(thread_ctx(), ptrs.data(), n_feat, nk, off.data(), ng, PDS_HOST, bias, l2, rcond, as<T>(cobuf), as<T>(svbuf),
                                     nulls.data()));
    }
    std::vector<uint8_t> ok(ng);
    for (int64_t g = 0; g < ng; ++g) ok[g] = nulls[g] ? 0 : 1;
    std::vector<std::unique_ptr<ArrowArray>> kids;
    {
        std::vector<uint8_t> kvalid;
        if (null_group) {
            kvalid.assign(ng, 1);
            for (int64_t g = 0; g < ng; ++g)
                if (keys[g] == null_stand_in) kvalid[g] = 0;
        }
        kids.push_back(prim_array_take<int64_t>(bytes_of(keys.data(), (size_t)ng), ng, null_group ? kvalid.data() : nullptr));
    }
    kids.push_back(list_array_take_rows<T>(std::move(cobuf), ng, pp, ok.data()));
    kids.push_back(list_array_take_rows<T>(std::move(svbuf), ng, pp, ok.data()));
    std::vector<std::unique_ptr<ArrowSchema>> sk;
    sk.push_back(make_schema("l", key.name.empty() ? "key" : key.name));
    sk.push_back(list_schema<T>("coeffs"));
    sk.push_back(list_schema<T>("singular_values"));
    export_series(out, make_schema("+s", "", std::move(sk)), struct_array(ng, std::move(kids)));
}
