// capi_report_cluster.hpp -- lin_reg_report with cluster-robust standard errors (pds_lin_reg_report_cluster_grouped_* / _by_key_*):
// ONE model over the whole frame, V = c inv (sum_g s_g s_g') inv with s_g = X_g' e_g the score of cluster g (Stata's vce(cluster),
// statsmodels' cov_type="cluster", R's vcovCL).
// Part of the one translation unit capi.hip (included there, inside namespace pds, in dependency order): the entry-point
// pipelines are templates with internal linkage, split by concern, not by compilation unit.
//
// The stages are report_impl's: the moment pass, the pivoted-QR solve with the inverse, ONE more pass over the frame
// (cluster_meat.hip: residuals, sum e^2 and the meat together), the copy back and report_epilogue's cluster branch.  The clusters
// are contiguous row ranges; the by-key form brings an int64 key column in any row order there first (keyed_frame_open; ordered keys
// move nothing).
#pragma once

// Clusters above this many rows are cut into row chunks that are separate work items.  Context option "cluster_split_rows".
constexpr int64_t kClusterSplitRowsDefault = 16384;

template <typename T, typename R>
static int report_cluster_impl(pds_ctx* ctx, const T* const* cols, int n_feat, int64_t n_rows, const int64_t* offsets, int64_t n_clusters,
                               pds_space space, int add_bias, int se_type, T y_var, R* out, int64_t* n_clusters_used = nullptr) {
    if (!ctx || !cols || !offsets || !out) return fail(PDS_ERR_INVALID, "null argument");
    const bool derive_var = (se_type & PDS_REPORT_DERIVE_YVAR) != 0;
    se_type &= ~PDS_REPORT_DERIVE_YVAR;
    if (se_type != PDS_CLUSTER && se_type != PDS_CLUSTER0) return fail(PDS_ERR_INVALID, "cluster-robust report: se_type is PDS_CLUSTER or PDS_CLUSTER0");
    if (n_feat < 1) return fail(PDS_ERR_INVALID, "need at least one feature column");
    if (n_feat > kMaxFeatSmall) return fail(PDS_ERR_UNSUPPORTED, "cluster-robust report: up to 16 feature columns");
    if (n_rows <= 0) return fail(PDS_ERR_EMPTY, "Empty data");
    if (n_clusters < 1) return fail(PDS_ERR_INVALID, "cluster-robust standard errors need at least two non-empty clusters");
    if (int rc = check_cols<T>(cols, n_feat)) return rc;
    PDS_HIP_CHECK(hipSetDevice(ctx->device));
    const int p = n_feat, bias = add_bias ? 1 : 0, pp = p + bias, q = p + 2;
    // ---- the offsets on the host: validation, the non-empty clusters, the chunks of the long ones
    std::vector<int64_t> off_copy;
    const int64_t* h_off = nullptr;
    if (int rc = host_offsets(ctx, offsets, n_clusters, space, off_copy, h_off)) return rc;
    const int64_t split = std::max<int64_t>(ctx->opt_cluster_split_rows > 0 ? ctx->opt_cluster_split_rows : kClusterSplitRowsDefault, 64);
    GroupChunkPlan pl;
    if (int rc = plan_group_chunks(h_off, n_clusters, n_rows, split, /*cover=*/true, space == PDS_HOST, /*want_gmap=*/false,
                                   "cluster offsets must be non-decreasing and cover the frame", pl))
        return rc;
    const int64_t n_nonempty = pl.n_nonempty;
    if (n_clusters_used) *n_clusters_used = n_nonempty;
    if (n_nonempty < 2) return fail(PDS_ERR_INVALID, "cluster-robust standard errors need at least two non-empty clusters");
    if (n_rows <= pp) return fail(PDS_ERR_TOO_FEW_ROWS, "#Data <= #features. No conclusive result.");
    const bool upload_off = pl.upload_off;  // (the device works on the non-empty clusters alone)
    h_off = pl.h_off;
    n_clusters = n_nonempty;
    ClusterChunks ch;
    ch.n_chunks = pl.n_chunks();
    ch.n_long = pl.n_long();
    // ---- workspace
    const auto up = Bump::up;
    const size_t n_rec = (size_t)cluster_meat_blocks(ctx, n_clusters) +
                         (ch.n_chunks > 0 ? (size_t)cluster_meat_blocks(ctx, ch.n_chunks) + (size_t)cluster_meat_blocks(ctx, ch.n_long) : 0);
    const size_t rec_bytes = (size_t)kMixedRecStride * sizeof(double);
    size_t need = 131072 + 65536 + sizeof(T) * (size_t)(q * q + pp * pp + pp + 8) + sizeof(T*) * (size_t)(p + 64) + up(n_rec * rec_bytes) +
                  up((n_rec / 64 + 1) * rec_bytes) + up(rec_bytes) + 4 * up((size_t)(ch.n_chunks + 1) * 8) +
                  up((size_t)(ch.n_chunks + 1) * kClusterScoreStride * 8) + 4096;
    if (upload_off) need += up((size_t)(n_clusters + 1) * 8);
    if (int rc = ws_reserve(ctx, need)) return rc;
    DeviceCols<T> dc;
    if (int rc = make_device_cols<T>(ctx, cols, nullptr, p, n_rows, space, dc)) return rc;
    const int64_t* d_off = offsets;
    if (upload_off) {
        int64_t* t = reinterpret_cast<int64_t*>(ws_take(ctx, (size_t)(n_clusters + 1) * 8));
        PDS_HIP_CHECK(hipMemcpyAsync(t, h_off, (size_t)(n_clusters + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
        d_off = t;
    }
    if (int rc = upload_cluster_chunks(ctx, [&](size_t bytes) { return ws_take(ctx, bytes); }, pl, ch)) return rc;
    T* d_mom = reinterpret_cast<T*>(ws_take(ctx, sizeof(T) * q * q));
    T* d_beta = reinterpret_cast<T*>(ws_take(ctx, sizeof(T) * (pp + 2)));
    T* d_inv = reinterpret_cast<T*>(ws_take(ctx, sizeof(T) * pp * pp));
    uint8_t* d_flag = reinterpret_cast<uint8_t*>(ws_take(ctx, 16));
    double* d_partials = reinterpret_cast<double*>(ws_take(ctx, n_rec * rec_bytes));
    double* d_stage = reinterpret_cast<double*>(ws_take(ctx, (n_rec / 64 + 1) * rec_bytes));
    double* d_rec = reinterpret_cast<double*>(ws_take(ctx, rec_bytes));
    // ---- the report's stages
    if (int rc = launch_moments<T>(ctx, dc, p, n_rows, false, d_mom)) return rc;
    SolveParams sp{p, bias, PDS_SOLVER_QR, 0.0, 0.0, 0};
    if (int rc = launch_solve<T>(ctx, d_mom, 1, sp, d_beta, d_flag, d_inv, nullptr)) return rc;
    double* d_ys = derive_var ? reinterpret_cast<double*>(ws_take(ctx, 64)) : nullptr;
    if (derive_var)
        if (int rc = launch_y_sums<T>(ctx, dc.h_ptrs[p], n_rows, d_ys, true)) return rc;
    if (int rc = launch_cluster_meat<T>(ctx, dc.d_ptrs, p, d_off, n_clusters, split, ch, d_beta, bias, d_partials, d_stage, d_rec)) return rc;
    std::vector<T> beta(pp), inv((size_t)pp * pp);
    double rec[kMixedRecStride], mom_y[2] = {0.0, 0.0};
    PDS_HIP_CHECK(hipMemcpyAsync(beta.data(), d_beta, sizeof(T) * pp, hipMemcpyDeviceToHost, ctx->stream));
    PDS_HIP_CHECK(hipMemcpyAsync(inv.data(), d_inv, sizeof(T) * pp * pp, hipMemcpyDeviceToHost, ctx->stream));
    PDS_HIP_CHECK(hipMemcpyAsync(rec, d_rec, sizeof(rec), hipMemcpyDeviceToHost, ctx->stream));
    if (derive_var) PDS_HIP_CHECK(hipMemcpyAsync(mom_y, d_ys, sizeof(mom_y), hipMemcpyDeviceToHost, ctx->stream));
    PDS_HIP_CHECK(hipStreamSynchronize(ctx->stream));  // (dc, pl: sources of the copies)
    if (derive_var) {
        const double nn = (double)n_rows, sy = mom_y[0], syy = mom_y[1];
        y_var = (T)((syy - sy * sy / nn) / (nn - 1.0));
    }
    std::vector<double> meat((size_t)pp * pp);
    for (int i = 0; i < p; ++i) {
        for (int j = 0; j < p; ++j) meat[(size_t)i * pp + j] = rec[kMixedRecW + i * 16 + j];
        if (bias) meat[(size_t)i * pp + p] = meat[(size_t)p * pp + i] = rec[kMixedRecXY + i];
    }
    if (bias) meat[(size_t)p * pp + p] = rec[kMixedRecC];
    const double sums[2] = {rec[kMixedRecYY] + rec[kMixedRecCY], 0.0};  // sum e^2: the value and its compensation term
    report_epilogue<T, R>(n_rows, p, bias, se_type, false, y_var, beta.data(), inv.data(), nullptr, sums, out, meat.data(), n_nonempty);
    return PDS_OK;
}

// int64 keys in any row order: the shared key-ordering stage (ordered keys move nothing), then the contiguous form on the device frame
template <typename T, typename R>
static int report_cluster_by_key_impl(pds_ctx* ctx, const T* const* cols, const int64_t* keys, int n_feat, int64_t n_rows, pds_space space,
                                      int add_bias, int se_type, T y_var, R* out, int64_t* n_clusters) {
    if (!ctx || !cols || !keys || !out || !n_clusters) return fail(PDS_ERR_INVALID, "null argument");
    const int st = se_type & ~PDS_REPORT_DERIVE_YVAR;
    if (st != PDS_CLUSTER && st != PDS_CLUSTER0) return fail(PDS_ERR_INVALID, "cluster-robust report: se_type is PDS_CLUSTER or PDS_CLUSTER0");
    if (n_feat < 1) return fail(PDS_ERR_INVALID, "need at least one feature column");
    if (n_feat > kMaxFeatSmall) return fail(PDS_ERR_UNSUPPORTED, "cluster-robust report: up to 16 feature columns");
    if (n_rows <= 0) return fail(PDS_ERR_EMPTY, "Empty data");
    if (int rc = check_cols<T>(cols, n_feat)) return rc;
    PDS_HIP_CHECK(hipSetDevice(ctx->device));
    KeyedFrame<T> kf;
    kf.src = frame_cols<T>(cols, n_feat);
    Bump w{};
    if (int rc = keyed_frame_open<T>(ctx, keys, n_rows, space, /*max_groups=*/n_rows, [](bool) { return (size_t)0; }, nullptr, kf, w)) return rc;
    return report_cluster_impl<T, R>(ctx, kf.src.data(), n_feat, n_rows, kf.d_offsets, kf.ng, PDS_DEVICE, add_bias, se_type, y_var, out, n_clusters);
}
