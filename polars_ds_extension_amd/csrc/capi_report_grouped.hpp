// capi_report_grouped.hpp -- the grouped lin_reg_report: one report per group of a frame in one call
// Part of the one translation unit capi.hip (included there, inside namespace pds, in dependency order): the entry-point
// pipelines are templates with internal linkage, split by concern, not by compilation unit.
//
// Per chunk of groups: grouped Gram records (launch_grouped_moments) -> batched pivoted QR with (X'X)^-1 (launch_solve, no gate:
// report_impl's factorisation) -> the residual / leverage / meat stream (grouped_report_pass.hip) -> the epilogue on the device.
// Chunking bounds the records, inverses and meats (at 1e6 groups x 17^2 each would be 2.3 - 2.6 GB); context option
// "report_chunk_groups" overrides the chunk size.
//
// With a weight column (pds_wls_report_grouped_* / _by_key_*) the same pipeline is pl_wls_report per group (linear_regression.rs:
// 982-1117): the records are Z'WZ (the WEIGHTED Gram kernels: the weights are read as one more column, never a scaled copy of the
// frame), the pass adds sum w e^2 to every item's sums slot and the epilogue's mse reads it.  r2 keeps the unweighted sum e^2 and
// the unweighted var(y), as the reference does.  Plain standard error only.
#pragma once

double student_t_lng_term(double df);  // stats.cpp

template <typename T>
struct ReportGroupedOut {  // the layout of pds_report_grouped_f64 / _f32
    T *beta, *std_err, *t, *p, *ci_lower, *ci_upper, *r2, *adj_r2;
    uint8_t* is_null;
};

// the nine outputs of a grouped report, `cap` groups of room: `d` receives the device pointers
template <typename T>
static StagedOuts report_staged_outs(const ReportGroupedOut<T>& out, ReportGroupedOut<T>& d, pds_space space, int64_t cap, int pp) {
    StagedOuts so(space == PDS_HOST, (size_t)cap);
    so.add(&d.beta, out.beta, pp);
    so.add(&d.std_err, out.std_err, pp);
    so.add(&d.t, out.t, pp);
    so.add(&d.p, out.p, pp);
    so.add(&d.ci_lower, out.ci_lower, pp);
    so.add(&d.ci_upper, out.ci_upper, pp);
    so.add(&d.r2, out.r2, 1);
    so.add(&d.adj_r2, out.adj_r2, 1);
    so.add(&d.is_null, out.is_null, 1);
    return so;
}

// t quantile and ln-gamma term per distinct dof = n_g - p' of the non-null groups (host functions, once each)
template <typename T>
static int report_dof_table(pds_ctx* ctx, const int64_t* off, int64_t n_groups, int pp, std::vector<double>& dense,
                            std::vector<int64_t>& large_keys, std::vector<double>& large, ReportDofTable& tab) {
    constexpr int64_t kDense = 1 << 16;
    std::vector<uint8_t> used;
    int64_t top = -1;
    for (int64_t g = 0; g < n_groups; ++g) {
        const int64_t k = off[g + 1] - off[g] - pp;
        if (k < 0) continue;
        if (k < kDense) {
            if (k >= (int64_t)used.size()) used.resize((size_t)std::max<int64_t>(k + 1, 2 * (int64_t)used.size()), 0);
            used[k] = 1;
            top = std::max(top, k);
        } else {
            large_keys.push_back(k);
        }
    }
    std::sort(large_keys.begin(), large_keys.end());
    large_keys.erase(std::unique(large_keys.begin(), large_keys.end()), large_keys.end());
    auto entry = [&](int64_t k, double* e) {
        const double dof = (double)((T)(k + pp) - (T)pp);  // report_epilogue's dof, in the frame's type
        e[0] = student_t_ppf(0.975, dof);
        e[1] = student_t_lng_term(dof);
    };
    dense.assign((size_t)(top + 1) * 2, (double)NAN);
    for (int64_t k = 0; k <= top; ++k)
        if (used[k]) entry(k, dense.data() + 2 * k);
    large.assign(large_keys.size() * 2, 0.0);
    for (size_t i = 0; i < large_keys.size(); ++i) entry(large_keys[i], large.data() + 2 * i);
    tab.dense_len = top + 1;
    tab.n_large = (int64_t)large_keys.size();
    double* d_dense = reinterpret_cast<double*>(ws_take(ctx, std::max<size_t>(dense.size(), 2) * 8));
    int64_t* d_lk = reinterpret_cast<int64_t*>(ws_take(ctx, std::max<size_t>(large_keys.size(), 1) * 8));
    double* d_large = reinterpret_cast<double*>(ws_take(ctx, std::max<size_t>(large.size(), 2) * 8));
    if (!d_dense || !d_lk || !d_large) return fail(PDS_ERR_HIP, "workspace allocation failed");
    if (!dense.empty()) PDS_HIP_CHECK(hipMemcpyAsync(d_dense, dense.data(), dense.size() * 8, hipMemcpyHostToDevice, ctx->stream));
    if (!large.empty()) {
        PDS_HIP_CHECK(hipMemcpyAsync(d_lk, large_keys.data(), large_keys.size() * 8, hipMemcpyHostToDevice, ctx->stream));
        PDS_HIP_CHECK(hipMemcpyAsync(d_large, large.data(), large.size() * 8, hipMemcpyHostToDevice, ctx->stream));
    }
    tab.dense = d_dense;
    tab.large_keys = d_lk;
    tab.large = d_large;
    return PDS_OK;
}

template <typename T>
static size_t report_dof_table_bytes(int64_t n_groups) {
    return (size_t)2 * 8 * (1 << 16) + (size_t)3 * 8 * (size_t)n_groups + 3 * 512;
}

// cols [y, x1..xp]; weights (nullable: the unweighted report) n_rows values; offsets n_groups + 1 (absolute rows, non-decreasing);
// d_yvar (nullable) n_groups values; all in `space`
template <typename T>
static int report_grouped_impl(pds_ctx* ctx, const T* const* cols, const T* weights, int n_feat, int64_t n_rows, const int64_t* offsets,
                               int64_t n_groups, pds_space space, int add_bias, int se_type, const T* y_var,
                               const ReportGroupedOut<T>* out) {
    if (!ctx || !cols || !offsets || !out) return fail(PDS_ERR_INVALID, "null argument");
    if (!out->beta || !out->std_err || !out->t || !out->p || !out->ci_lower || !out->ci_upper || !out->r2 || !out->adj_r2 || !out->is_null)
        return fail(PDS_ERR_INVALID, "null output pointer");
    if (n_feat < 1) return fail(PDS_ERR_INVALID, "need at least one feature column");
    if (n_feat > kMaxFeatWide) return fail(PDS_ERR_UNSUPPORTED, "grouped lin_reg_report: at most 64 features");
    if (n_groups <= 0 || n_rows <= 0) return fail(PDS_ERR_EMPTY, "Empty data");
    if (se_type < PDS_SE || se_type > PDS_HC3) return fail(PDS_ERR_INVALID, "unknown standard-error type");
    const bool weighted = weights != nullptr;
    if (weighted) se_type = PDS_SE;  // pl_wls_report only knows "std_err"
    PDS_HIP_CHECK(hipSetDevice(ctx->device));
    const int p = n_feat, bias = add_bias ? 1 : 0, pp = p + bias, q = p + 2;
    const int hc = (se_type == PDS_SE) ? 0 : (se_type == PDS_HC2 ? 2 : (se_type == PDS_HC3 ? 3 : 1));
    // the offsets on the host: validated (the kernels index rows with them) and the source of the dof table
    std::vector<int64_t> h_off_store;
    const int64_t* h_off = nullptr;
    if (int rc = host_offsets(ctx, offsets, n_groups, space, h_off_store, h_off)) return rc;
    if (h_off[0] < 0 || h_off[n_groups] > n_rows) return fail(PDS_ERR_INVALID, "group offsets outside the frame");
    for (int64_t g = 0; g < n_groups; ++g)
        if (h_off[g + 1] < h_off[g]) return fail(PDS_ERR_INVALID, "group offsets must be non-decreasing");
    int64_t chunk = ctx->opt_report_chunk_groups > 0 ? ctx->opt_report_chunk_groups
                                                     : std::max<int64_t>(1024, (int64_t)(128ll << 20) / (int64_t)(sizeof(T) * q * q));
    chunk = std::min(chunk, n_groups);
    // groups of more than piece_rows rows stream on several waves (grouped_report.hpp): the extra pieces of each chunk, and the
    // largest count any chunk has (their sums / meat slots follow the chunk's own)
    const int64_t piece_rows = p > kMaxFeatSmall ? 16384 : 4096;
    std::vector<int64_t> chunk_pieces;  // per chunk: number of extra pieces
    int64_t max_pieces = 0, max_fin = 0;
    for (int64_t g0 = 0; g0 < n_groups; g0 += chunk) {
        int64_t np_ = 0, nf = 0;
        for (int64_t g = g0; g < std::min(n_groups, g0 + chunk); ++g) {
            const int64_t ng = h_off[g + 1] - h_off[g];
            if (ng >= pp && ng > piece_rows) {
                np_ += (ng - 1) / piece_rows;
                ++nf;
            }
        }
        chunk_pieces.push_back(np_);
        max_pieces = std::max(max_pieces, np_);
        max_fin = std::max(max_fin, nf);
    }
    const int64_t slots = chunk + max_pieces;
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    size_t need = 131072 + up(sizeof(T*) * (size_t)(p + 64)) + report_dof_table_bytes<T>(n_groups);
    need += up(sizeof(T) * (size_t)chunk * q * q) + up(sizeof(T) * (size_t)chunk * pp * pp) + up((size_t)chunk) + up((size_t)slots * 32);
    need += up((size_t)std::max<int64_t>(max_pieces, 1) * 24) + up((size_t)std::max<int64_t>(max_fin, 1) * 24);
    if (hc) need += up((size_t)slots * pp * pp * 8);
    // pass 1 of split groups: one Gram record per piece (virtual groups), summed back per group
    if (max_pieces > 0) need += up(sizeof(T) * (size_t)slots * q * q) + up((size_t)(slots + 1) * 8) + up((size_t)(chunk + 1) * 8);
    ReportGroupedOut<T> d;
    StagedOuts outs = report_staged_outs<T>(*out, d, space, n_groups, pp);
    need += outs.bytes();
    if (space == PDS_HOST) need += up((size_t)(n_groups + 1) * 8) + (y_var ? up((size_t)n_groups * sizeof(T)) : 0);
    if (int rc = ws_reserve(ctx, need)) return rc;
    DeviceCols<T> dc;
    if (int rc = make_device_cols<T>(ctx, cols, weights, p, n_rows, space, dc)) return rc;
    if (!dc.d_ptrs) return fail(PDS_ERR_HIP, "workspace allocation failed");
    bool ws_ok = true;
    auto take = [&](size_t b) { void* r = ws_take(ctx, b); if (!r) ws_ok = false; return r; };
    const int64_t* d_off = offsets;
    const T* d_yv = y_var;
    if (space == PDS_HOST) {
        int64_t* o = reinterpret_cast<int64_t*>(take((size_t)(n_groups + 1) * 8));
        if (y_var) d_yv = reinterpret_cast<const T*>(take((size_t)n_groups * sizeof(T)));
        outs.place(take);
        if (!ws_ok) return fail(PDS_ERR_HIP, "workspace allocation failed");
        PDS_HIP_CHECK(hipMemcpyAsync(o, offsets, (size_t)(n_groups + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
        if (y_var) PDS_HIP_CHECK(hipMemcpyAsync(const_cast<T*>(d_yv), y_var, (size_t)n_groups * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
        d_off = o;
    }
    T* d_mom = reinterpret_cast<T*>(take(sizeof(T) * (size_t)chunk * q * q));
    T* d_inv = reinterpret_cast<T*>(take(sizeof(T) * (size_t)chunk * pp * pp));
    uint8_t* d_flag = reinterpret_cast<uint8_t*>(take((size_t)chunk));
    double* d_sums = reinterpret_cast<double*>(take((size_t)slots * 32));
    double* d_meat = hc ? reinterpret_cast<double*>(take((size_t)slots * pp * pp * 8)) : nullptr;
    int64_t* d_pieces = reinterpret_cast<int64_t*>(take((size_t)std::max<int64_t>(max_pieces, 1) * 24));
    int64_t* d_fin = reinterpret_cast<int64_t*>(take((size_t)std::max<int64_t>(max_fin, 1) * 24));
    T* d_vmom = max_pieces > 0 ? reinterpret_cast<T*>(take(sizeof(T) * (size_t)slots * q * q)) : nullptr;
    int64_t* d_vofs = max_pieces > 0 ? reinterpret_cast<int64_t*>(take((size_t)(slots + 1) * 8)) : nullptr;
    int64_t* d_vfirst = max_pieces > 0 ? reinterpret_cast<int64_t*>(take((size_t)(chunk + 1) * 8)) : nullptr;
    if (!ws_ok) return fail(PDS_ERR_HIP, "workspace allocation failed");
    std::vector<double> dense, large;
    std::vector<int64_t> large_keys;
    ReportDofTable tab;
    if (int rc = report_dof_table<T>(ctx, h_off, n_groups, pp, dense, large_keys, large, tab)) return rc;
    // xtx.col_piv_qr() -> inverse() and the solve, per group, no gate (report_impl, linear_regression.rs:855-858)
    const SolveParams sp{p, bias, PDS_SOLVER_QR, 0.0, 0.0, 0};
    std::vector<int64_t> pieces, fin, vofs, vfirst;  // (host sources of the async copies: synchronised before they are refilled)
    for (int64_t g0 = 0, ci = 0; g0 < n_groups; g0 += chunk, ++ci) {
        const int64_t gc = std::min(chunk, n_groups - g0);
        const int64_t* d_o = d_off + g0;
        T* beta = d.beta + g0 * pp;
        if (chunk_pieces[ci] > 0) {
            PDS_HIP_CHECK(hipStreamSynchronize(ctx->stream));  // (the previous chunk's copies have left the vectors)
            pieces.clear();
            fin.clear();
            vofs.clear();
            vfirst.clear();
            for (int64_t g = g0; g < g0 + gc; ++g) {
                const int64_t r0 = h_off[g], r1 = h_off[g + 1];
                vfirst.push_back((int64_t)vofs.size());
                const bool split = r1 - r0 >= pp && r1 - r0 > piece_rows;
                for (int64_t r = r0; r < r1 || r == r0; r += (split ? piece_rows : std::max<int64_t>(r1 - r0, 1))) vofs.push_back(r);
                if (!split) continue;
                fin.push_back(g - g0);
                fin.push_back(gc + (int64_t)pieces.size() / 3);
                for (int64_t r = r0 + piece_rows; r < r1; r += piece_rows) {
                    pieces.push_back(g - g0);
                    pieces.push_back(r);
                    pieces.push_back(std::min(r + piece_rows, r1));
                }
                fin.push_back(gc + (int64_t)pieces.size() / 3 - fin[fin.size() - 1]);
            }
            vfirst.push_back((int64_t)vofs.size());
            vofs.push_back(h_off[g0 + gc]);
            PDS_HIP_CHECK(hipMemcpyAsync(d_vofs, vofs.data(), vofs.size() * 8, hipMemcpyHostToDevice, ctx->stream));
            PDS_HIP_CHECK(hipMemcpyAsync(d_vfirst, vfirst.data(), vfirst.size() * 8, hipMemcpyHostToDevice, ctx->stream));
            PDS_HIP_CHECK(hipMemcpyAsync(d_pieces, pieces.data(), pieces.size() * 8, hipMemcpyHostToDevice, ctx->stream));
            PDS_HIP_CHECK(hipMemcpyAsync(d_fin, fin.data(), fin.size() * 8, hipMemcpyHostToDevice, ctx->stream));
        }
        const int64_t n_pieces = chunk_pieces[ci] > 0 ? (int64_t)pieces.size() / 3 : 0;
        const int64_t n_fin = chunk_pieces[ci] > 0 ? (int64_t)fin.size() / 3 : 0;
        if (n_pieces > 0) {  // groups longer than a piece: their rows' records on many waves, summed back in piece order
            const int64_t nv = (int64_t)vofs.size() - 1;
            if (int rc = launch_grouped_moments<T>(ctx, dc, p, d_vofs, nv, d_vmom, nullptr, weighted)) return rc;
            if (int rc = launch_grouped_report_sum_records<T>(ctx, d_vmom, d_vfirst, gc, q * q, d_mom)) return rc;
        } else if (int rc = launch_grouped_moments<T>(ctx, dc, p, d_o, gc, d_mom, nullptr, weighted)) {
            return rc;
        }
        if (int rc = launch_solve<T>(ctx, d_mom, gc, sp, beta, d_flag, d_inv, nullptr)) return rc;
        if (int rc = launch_grouped_report_pass<T>(ctx, dc.d_ptrs, p, bias, d_o, gc, beta, d_inv, hc, d_sums, d_meat, d_pieces, n_pieces,
                                                   piece_rows, d_fin, n_fin, weighted))
            return rc;
        if (int rc = launch_grouped_report_epilogue<T>(ctx, d_o, gc, p, bias, se_type, d_yv ? d_yv + g0 : nullptr, beta, d_inv, d_sums,
                                                       d_meat, tab, d.std_err + g0 * pp, d.t + g0 * pp, d.p + g0 * pp,
                                                       d.ci_lower + g0 * pp, d.ci_upper + g0 * pp, d.r2 + g0, d.adj_r2 + g0,
                                                       d.is_null + g0, weighted))
            return rc;
    }
    if (int rc = staged_copy_back(ctx, outs, (size_t)n_groups)) return rc;
    PDS_HIP_CHECK(hipStreamSynchronize(ctx->stream));  // (also: the dof table's host vectors are the sources of async copies)
    return PDS_OK;
}

// int64 keys in any row order: ordered keys take the order check's run marks (nothing moves); otherwise the stable radix sort of
// (key, row) and the frame gather (capi_keyed_frame.hpp).  Groups come back in ascending key order.
template <typename T>
static int report_by_key_impl(pds_ctx* ctx, const T* const* cols, const T* weights, const int64_t* keys, int n_feat, int64_t n_rows,
                              pds_space space, int add_bias, int se_type, int64_t max_groups, int64_t* out_keys,
                              const ReportGroupedOut<T>* out, int64_t* n_groups) {
    if (!ctx || !cols || !keys || !out || !out_keys || !n_groups) return fail(PDS_ERR_INVALID, "null argument");
    if (n_feat < 1) return fail(PDS_ERR_INVALID, "need at least one feature column");
    if (n_feat > kMaxFeatWide) return fail(PDS_ERR_UNSUPPORTED, "grouped lin_reg_report: at most 64 features");
    if (n_rows <= 0) return fail(PDS_ERR_EMPTY, "Empty data");
    if (max_groups < 1) return fail(PDS_ERR_INVALID, "max_groups must be positive");
    if (se_type < PDS_SE || se_type > PDS_HC3) return fail(PDS_ERR_INVALID, "unknown standard-error type");
    PDS_HIP_CHECK(hipSetDevice(ctx->device));
    // (a weight column rides through the staging, the sort and the gather as one more column of the frame: kf.src[n_feat + 1])
    const int pp = n_feat + (add_bias ? 1 : 0);
    ReportGroupedOut<T> d;
    StagedOuts outs = report_staged_outs<T>(*out, d, space, std::min<int64_t>(max_groups, n_rows), pp);
    KeyedFrame<T> kf;
    kf.src = frame_cols<T>(cols, n_feat, weights);
    Bump w{};
    if (int rc = keyed_frame_open<T>(ctx, keys, n_rows, space, max_groups, [&](bool) { return outs.bytes(); }, n_groups, kf, w)) return rc;
    const int64_t ng = kf.ng;
    outs.place(w);
    if (int rc = report_grouped_impl<T>(ctx, kf.src.data(), weights ? kf.src[n_feat + 1] : (const T*)nullptr, n_feat, n_rows, kf.d_offsets, ng,
                                        PDS_DEVICE, add_bias, se_type, (const T*)nullptr, &d))
        return rc;
    if (int rc = staged_copy_back(ctx, outs, (size_t)ng)) return rc;
    PDS_HIP_CHECK(hipMemcpyAsync(out_keys, kf.d_unique, (size_t)ng * 8, space == PDS_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, ctx->stream));
    PDS_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return PDS_OK;
}

// the device p-value function on a host grid (tests: within 1e-13 relative of pds_student_t_sf)
static int student_t_sf_device_impl(pds_ctx* ctx, const double* x, const double* df, int64_t n, double* out) {
    if (!ctx || !x || !df || !out) return fail(PDS_ERR_INVALID, "null argument");
    if (n <= 0) return PDS_OK;
    PDS_HIP_CHECK(hipSetDevice(ctx->device));
    std::vector<double> lng((size_t)n);
    for (int64_t i = 0; i < n; ++i) lng[i] = student_t_lng_term(df[i]);
    if (int rc = ws_reserve(ctx, 4 * ((size_t)n * 8 + 256))) return rc;
    double* d_x = reinterpret_cast<double*>(ws_take(ctx, (size_t)n * 8));
    double* d_df = reinterpret_cast<double*>(ws_take(ctx, (size_t)n * 8));
    double* d_lng = reinterpret_cast<double*>(ws_take(ctx, (size_t)n * 8));
    double* d_out = reinterpret_cast<double*>(ws_take(ctx, (size_t)n * 8));
    if (!d_x || !d_df || !d_lng || !d_out) return fail(PDS_ERR_HIP, "workspace allocation failed");
    PDS_HIP_CHECK(hipMemcpyAsync(d_x, x, (size_t)n * 8, hipMemcpyHostToDevice, ctx->stream));
    PDS_HIP_CHECK(hipMemcpyAsync(d_df, df, (size_t)n * 8, hipMemcpyHostToDevice, ctx->stream));
    PDS_HIP_CHECK(hipMemcpyAsync(d_lng, lng.data(), (size_t)n * 8, hipMemcpyHostToDevice, ctx->stream));
    if (int rc = launch_student_t_sf_grid(ctx, d_x, d_df, d_lng, n, d_out)) return rc;
    PDS_HIP_CHECK(hipMemcpyAsync(out, d_out, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->stream));
    PDS_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return PDS_OK;
}
