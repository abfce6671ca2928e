// plugin_keyed.hpp -- what the key-aware entry points share on the host: the import of [key, value columns] and its checks, the null
// key's stand-in, the capacity guess and the one retry of a by-key call, the preparation of a frame with nulls for an offsets entry
// point, and the children of a per-group result (key, features, broadcast fields, validity)
// Part of the one translation unit plugin.cpp (included there, inside its anonymous namespace, before plugin_exprs.hpp).
#pragma once

// ------------------------------------------------------------------------------------------------- inputs
// Polars' group_by / over make the null keys ONE group.  They take a key value no valid row uses -- max + 1, so that group comes
// last (min - 1 when the maximum is INT64_MAX); returns whether there were null keys (and the stand-in)
inline bool null_key_stand_in(Column<int64_t>& key, int64_t n, const char* who, int64_t* stand_in) {
    if (key.null_count <= 0) return false;
    const int64_t* k = key.data();
    int64_t mx = std::numeric_limits<int64_t>::min(), mn = std::numeric_limits<int64_t>::max();
    bool any_valid = false;
    for (int64_t i = 0; i < n; ++i)
        if (bit_get(key.validity.data(), i)) {
            mx = std::max(mx, k[i]);
            mn = std::min(mn, k[i]);
            any_valid = true;
        }
    int64_t v = 0;
    if (!any_valid) v = 0;
    else if (mx < std::numeric_limits<int64_t>::max()) v = mx + 1;
    else if (mn > std::numeric_limits<int64_t>::min()) v = mn - 1;
    else raise(std::string(who) + ": the keys span the whole int64 range, no value is left for the null group");
    auto& kv = key.own();
    for (int64_t i = 0; i < n; ++i)
        if (!bit_get(key.validity.data(), i)) kv[i] = v;
    *stand_in = v;
    return true;
}

// inputs [key (integer, any row order, nulls = one group), value columns...] and the null policy of a key-aware symbol
template <typename T>
struct KeyedInputs {
    Column<int64_t> key;           // an Int64 key column is borrowed as it is; other integer widths are widened
    std::vector<Column<T>> cols;   // everything behind the key
    Policy pol{Policy::RAISE};     // kwargs["null_policy"]
    int64_t n = 0;                 // rows
    bool any_null = false;         // a value column holds a null
    bool null_group = false;       // the key holds nulls: the group that carries null_stand_in is reported with a null key
    int64_t null_stand_in = 0;
    const int64_t* ikey = nullptr; // the keys, stand-in in place (set by keyed_settle)
};

// The checks of a key-aware symbol, in the order every one of them keeps: the import, the policy, "Nulls found in data" under
// "raise" (keyed_import); the column lengths (keyed_check_lengths); "Empty data" and the null keys' stand-in (keyed_settle).  A
// symbol with a check or a step of its own in between calls the three itself, the others call keyed_inputs.
template <typename T>
KeyedInputs<T> keyed_import(SeriesExport* in, size_t n_in, const Kwargs& kw) {
    KeyedInputs<T> ki;
    ki.key = import_series<int64_t>(in[0]);
    for (size_t i = 1; i < n_in; ++i) ki.cols.push_back(import_series<T>(in[i]));
    ki.pol = parse_policy(kw_str(kw, "null_policy", "raise"));
    for (auto& c : ki.cols) ki.any_null |= c.null_count > 0;
    if (ki.any_null && ki.pol.kind == Policy::RAISE) raise("Nulls found in data");
    ki.n = ki.key.size();
    return ki;
}
template <typename T>
void keyed_check_lengths(const KeyedInputs<T>& ki) {
    for (auto& c : ki.cols)
        if (c.size() != ki.n) raise("input columns differ in length");
}
// (an empty key column holds no null, so the stand-in step cannot raise on it: which of the two comes first cannot be observed)
template <typename T>
void keyed_settle(KeyedInputs<T>& ki, const char* who) {
    if (ki.n == 0) raise("Empty data");
    ki.null_group = null_key_stand_in(ki.key, ki.n, who, &ki.null_stand_in);
    ki.ikey = ki.key.data();
}
template <typename T>
KeyedInputs<T> keyed_inputs(SeriesExport* in, size_t n_in, const Kwargs& kw, const char* who) {
    KeyedInputs<T> ki = keyed_import<T>(in, n_in, kw);
    keyed_check_lengths(ki);
    keyed_settle(ki, who);
    return ki;
}

// ------------------------------------------------------------------------------------------------- the by-key call
// Output capacity of a by-key call: the number of distinct keys is unknown until the device has counted the runs -- start from a
// guess (every row its own group is always enough but costs n x p' of host memory) ...  `seam` > 0: a test's first guess instead
inline int64_t first_group_capacity(int64_t n, int64_t seam) {
    if (seam > 0) return std::min(seam, n);
    return n <= ((int64_t)1 << 20) ? n : std::max<int64_t>((int64_t)1 << 20, n / 16);
}
// ... and repeat once with the count `call` left in `ng` when the guess was too small.  size_outputs(cap) sizes the result storage
// -- never zeroed (RawVec / raw_buffer): pages the device-to-host copies do not write are never touched (a zeroed 1M-group guess cost
// 16 ms of page faults per call) -- and call(cap) makes the C ABI call and returns its code.
template <typename Size, typename Call>
void by_key_with_retry(int64_t cap, Size&& size_outputs, Call&& call, const int64_t& ng) {
    size_outputs(cap);
    int rc = call(cap);
    if (rc != 0 && ng > cap) {
        cap = ng;
        size_outputs(cap);
        rc = call(cap);
    }
    check(rc);
}

// ------------------------------------------------------------------------------------------------- frames with nulls
// row index -> frame row in ascending key order: a stable sort of the row indices, empty when the keys are in order already
inline std::vector<int64_t> key_order(const int64_t* ikey, int64_t n) {
    bool ordered = true;
    for (int64_t i = 1; i < n && ordered; ++i) ordered = ikey[i] >= ikey[i - 1];
    std::vector<int64_t> perm;
    if (ordered) return perm;
    perm.resize((size_t)n);
    for (int64_t i = 0; i < n; ++i) perm[i] = i;
    std::stable_sort(perm.begin(), perm.end(), [&](int64_t a, int64_t b) { return ikey[a] < ikey[b]; });
    return perm;
}

template <typename T>
bool is_null_at(const Column<T>& c, int64_t r) { return c.null_count > 0 && !bit_get(c.validity.data(), r); }

// The row rule of series_to_mat_for_lr (linear_regression.rs:187-248) on row r of [y, x1..xp]: "skip" drops a row with any null, a
// fill policy fills the features and drops the rows whose target is null, everything else keeps the row with NaN for the nulls.
// A surviving row is appended to `kept` column by column; returns whether it survived.
template <typename T>
bool push_kept_row(const std::vector<Column<T>>& cols, int64_t r, const Policy& pol, std::vector<std::vector<T>>& kept) {
    const bool fill = pol.kind == Policy::FILL;
    bool keep = true;
    if (pol.kind == Policy::SKIP)
        for (size_t c = 0; c < cols.size() && keep; ++c) keep = !is_null_at(cols[c], r);
    else if (fill)
        keep = !is_null_at(cols[0], r);
    if (!keep) return false;
    for (size_t c = 0; c < cols.size(); ++c)
        kept[c].push_back(is_null_at(cols[c], r) ? (fill ? (T)pol.fill : std::numeric_limits<T>::quiet_NaN()) : cols[c].data()[r]);
    return true;
}

// A frame with nulls, prepared on the host for an offsets entry point (pds_*_grouped_*): rows in key order (key_order), the row rule
// of ki.pol applied inside every group (push_kept_row) -- what the reference's per-group call does with that group's rows alone.
template <typename T>
struct PreparedRows {
    std::vector<std::vector<T>> kept;  // the surviving rows, column by column, in key order
    std::vector<int64_t> off;          // n_groups + 1 offsets into kept
    std::vector<int64_t> src_row;      // the frame row of every surviving row
    std::vector<int64_t> perm, first;  // all rows: group g is row(first[g]) .. row(first[g + 1] - 1), dropped rows included
    int64_t row(int64_t i) const { return perm.empty() ? i : perm[i]; }
    int64_t rows() const { return (int64_t)src_row.size(); }
    std::vector<const T*> ptrs;        // kept[c].data(), the `cols` argument of the entry point
};
// `keys`: one entry per group, ascending (a group whose rows were all dropped stays, empty).  No surviving row is "Empty data".
template <typename T>
PreparedRows<T> prepare_keyed_rows(const KeyedInputs<T>& ki, RawVec<int64_t>& keys) {
    PreparedRows<T> pr;
    pr.perm = key_order(ki.ikey, ki.n);
    pr.kept.assign(ki.cols.size(), {});
    for (auto& v : pr.kept) v.reserve((size_t)ki.n);
    pr.src_row.reserve((size_t)ki.n);
    for (int64_t i = 0; i < ki.n; ++i) {
        const int64_t r = pr.row(i);
        if (i == 0 || ki.ikey[r] != ki.ikey[pr.row(i - 1)]) {
            pr.first.push_back(i);
            pr.off.push_back(pr.rows());
            keys.push_back(ki.ikey[r]);
        }
        if (push_kept_row(ki.cols, r, ki.pol, pr.kept)) pr.src_row.push_back(r);
    }
    pr.first.push_back(ki.n);
    pr.off.push_back(pr.rows());
    if (pr.rows() == 0) raise("Empty data");
    for (auto& v : pr.kept) pr.ptrs.push_back(v.data());
    return pr;
}

// ------------------------------------------------------------------------------------------------- per-group results
// the key child: every group's key `repeat` times (1: one row per group; p': the long format), null for the null key's stand-in
template <typename T>
std::unique_ptr<ArrowArray> key_array(const KeyedInputs<T>& ki, const RawVec<int64_t>& keys, int64_t ng, int repeat) {
    const int64_t rows = ng * repeat;
    ByteVec kb = raw_buffer<int64_t>((size_t)rows);
    int64_t* kd = as<int64_t>(kb);
    std::vector<uint8_t> kvalid;
    if (ki.null_group) kvalid.assign((size_t)rows, 1);
    for (int64_t g = 0; g < ng; ++g)
        for (int i = 0; i < repeat; ++i) {
            kd[g * repeat + i] = keys[g];
            if (ki.null_group && keys[g] == ki.null_stand_in) kvalid[g * repeat + i] = 0;
        }
    return prim_array_take<int64_t>(std::move(kb), rows, ki.null_group ? kvalid.data() : nullptr);
}
// ... and its field: Int64 under the key column's name
template <typename T>
std::unique_ptr<ArrowSchema> key_schema(const KeyedInputs<T>& ki) { return make_schema("l", ki.key.name.empty() ? "key" : ki.key.name); }

// the long format's `features` child: the names of cols[first_x..] (+ __bias__ last), once per group (large-utf8: int64 offsets)
template <typename T>
std::unique_ptr<ArrowArray> features_array(const std::vector<Column<T>>& cols, size_t first_x, bool bias, int64_t ng) {
    std::string one;
    std::vector<int64_t> o1 = {0};
    for (size_t i = first_x; i < cols.size() + (bias ? 1 : 0); ++i) {
        one += i < cols.size() ? cols[i].name : "__bias__";
        o1.push_back((int64_t)one.size());
    }
    const int pp = (int)o1.size() - 1;
    const int64_t rows = ng * pp;
    ByteVec ob = raw_buffer<int64_t>((size_t)rows + 1), db = raw_buffer<char>((size_t)ng * one.size());
    int64_t* od = as<int64_t>(ob);
    for (int64_t g = 0; g < ng; ++g) {
        for (int i = 0; i < pp; ++i) od[g * pp + i] = g * (int64_t)one.size() + o1[i];
        if (!one.empty()) std::memcpy(db.data() + g * one.size(), one.data(), one.size());
    }
    od[rows] = ng * (int64_t)one.size();
    std::vector<ByteVec> bufs;
    bufs.emplace_back();
    bufs.push_back(std::move(ob));
    bufs.push_back(std::move(db));
    return make_array(rows, 0, std::move(bufs), {false, true, true});
}

// a per-group value over the group's pp rows
template <typename V>
ByteVec broadcast_rows(const ByteVec& per_group, int64_t ng, int pp) {
    ByteVec wide = raw_buffer<V>((size_t)(ng * pp));
    const V* sv = reinterpret_cast<const V*>(per_group.data());
    V* dv = as<V>(wide);
    for (int64_t g = 0; g < ng; ++g)
        for (int i = 0; i < pp; ++i) dv[g * pp + i] = sv[g];
    return wide;
}

// per-group null flags -> one validity byte for each of the group's pp rows; returns whether NO group is null (the array then
// takes a null pointer and carries no validity buffer).  pp = 1 is the plain inversion null flag -> valid flag of the one-row-per-group
// results, whose list children always take the flags (the return value is not needed there)
inline bool group_flags_to_row_valid(const uint8_t* nulls, int64_t ng, int pp, std::vector<uint8_t>& valid) {
    valid.resize((size_t)(ng * pp));
    bool none = true;
    for (int64_t g = 0; g < ng; ++g) {
        if (nulls[g]) none = false;
        for (int i = 0; i < pp; ++i) valid[g * pp + i] = nulls[g] ? 0 : 1;
    }
    return none;
}
