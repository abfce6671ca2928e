// capi_multi_grouped.hpp -- the multi-target fit per group, lin_reg(target=[..], by=key): contiguous groups (pds_lr_multi_grouped_*)
// and int64 keys in any row order (pds_lr_multi_by_key_*).  k targets share every group's design matrix: the frame is staged once,
// the keys are ordered once, and a group's X'X is factorised once for all k right-hand sides (grouped_multi.hip) -- or, where that
// measures faster, the fused grouped kernel runs once per target on the same staged frame and the same offsets.
// Part of the one translation unit capi.hip (included there, inside namespace pds, in dependency order): the entry-point
// pipelines are templates with internal linkage, split by concern, not by compilation unit.
#pragma once

static const char* const kMultiGroupedLimit = "grouped multi-target lin_reg: up to 16 feature columns and 15 targets";
constexpr int kMultiGroupedMaxTargets = 15;  // the side block of the Gram tile has 16 columns, one of them the ones column

// "grouped_multi_route" = 0: the route per (features, targets), from profiles/grouped_multi_bench.txt (1e6 groups x 100 rows, f64,
// device resident; DESIGN.md 4.2a sets the rule next to its figures).  The one kernel is faster from three targets on at every
// width measured (1, 4, 8, 16 features), by a factor that grows with k (it reads the design matrix once); with two targets the
// per-target launches are, narrowly.  One target is one fused launch: lin_reg_by itself.  The width does not enter.
static int multi_route_auto(int n_feat, int n_targets) {
    (void)n_feat;
    return n_targets >= 3 ? 1 : 2;
}

// The fit on a device-resident frame in group order.  dsrc = [t_0 .. t_{k-1}, x_1 .. x_p] (device); d_co [ng][k][p'], d_nu [ng];
// per-row outputs (each nullable) [k][n_rows] / [n_rows] through d_perm (nullable) in the caller's row order.  Scratch from ctx->ws.
template <typename T>
static int multi_fit_device(pds_ctx* ctx, const std::vector<const T*>& dsrc, int k, int p, int64_t n_rows, const int64_t* d_off, int64_t ng,
                            int bias, double l2_reg, int solver, double gate_tol, T* d_co, uint8_t* d_nu, T* d_pred, T* d_resid, uint8_t* d_rn,
                            const uint32_t* d_perm) {
    const int pp = p + bias, q = p + 2;
    const bool want_pred = d_pred || d_resid || d_rn;
    const bool gated = gate_tol > 0.0;
    int route = (int)ctx->opt_multi_route;
    if (route != 1 && route != 2) route = multi_route_auto(p, k);
    // (a chunk of moment records stays inside the Infinity Cache between the kernel that writes it and the solve: grouped_impl)
    int64_t chunk = std::max<int64_t>(4096, (int64_t)(128ll << 20) / (int64_t)(sizeof(T) * q * q));
    chunk = std::min(chunk, ng);
    const size_t blk = Bump::up((size_t)ng * pp * sizeof(T)) + Bump::up((size_t)ng);
    size_t need = 262144 + Bump::up(sizeof(T) * (size_t)chunk * q * q) + 2 * Bump::up((size_t)ng * 4) +
                  2 * (Bump::up((size_t)chunk * pp * sizeof(T)) + Bump::up((size_t)chunk)) + 2 * blk + Bump::up(sizeof(T*) * ((size_t)k * 18 + 32));
    if (int rc = ws_reserve(ctx, need)) return rc;
    // ---- pointer tables: one per target in the kernels' order x_0 .. x_{p-1}, t (18 entries: the fused kernel, the Gram build of
    // the marked groups and the prediction pass read these), and the multi-target kernel's x_0 .. x_{p-1}, t_0 .. t_{k-1} (32)
    std::vector<const T*> tabs((size_t)k * 18 + 32, dsrc[k]);
    for (int t = 0; t < k; ++t) {
        for (int c = 0; c < p; ++c) tabs[(size_t)t * 18 + c] = dsrc[k + c];
        tabs[(size_t)t * 18 + p] = dsrc[t];
    }
    for (int c = 0; c < p; ++c) tabs[(size_t)k * 18 + c] = dsrc[k + c];
    for (int t = 0; t < k; ++t) tabs[(size_t)k * 18 + p + t] = dsrc[t];
    const T** d_tabs = reinterpret_cast<const T**>(ws_take(ctx, sizeof(T*) * tabs.size()));
    unsigned* d_words = reinterpret_cast<unsigned*>(ws_take(ctx, 256));  // [0] marked groups, [1] bad offsets
    T* d_mom = reinterpret_cast<T*>(ws_take(ctx, sizeof(T) * (size_t)chunk * q * q));
    if (!d_tabs || !d_words || !d_mom) return fail(PDS_ERR_HIP, "workspace allocation failed");
    PDS_HIP_CHECK(hipMemcpyAsync(d_tabs, tabs.data(), sizeof(T*) * tabs.size(), hipMemcpyHostToDevice, ctx->stream));
    PDS_HIP_CHECK(hipMemsetAsync(d_words, 0, 8, ctx->stream));
    std::vector<DeviceCols<T>> dct((size_t)k);
    for (int t = 0; t < k; ++t) {
        dct[t].nc = p + 1;
        dct[t].d_ptrs = d_tabs + (size_t)t * 18;
        dct[t].h_ptrs.assign(tabs.begin() + (size_t)t * 18, tabs.begin() + (size_t)(t + 1) * 18);
    }
    // the one-wave-per-group kernel reads nothing of a group whose offsets leave the frame; the per-target kernels and the
    // prediction pass walk the offsets as they are, so they only ever see offsets that were checked
    if (route == 2 || !gated || want_pred) {
        unsigned h_bad = 0;
        if (int rc = launch_multi_offsets_check(ctx, d_off, ng, n_rows, d_words + 1)) return rc;
        PDS_HIP_CHECK(hipMemcpyAsync(&h_bad, d_words + 1, sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream));
        PDS_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        if (h_bad) {
            if (!gated || want_pred) return fail(PDS_ERR_INVALID, "group_offsets must be non-decreasing and inside the frame");
            route = 1;
        }
    }
    // solver = "svd" maps to the pivoted QR, as in pds_lr_multi_* (lr_multi_impl)
    SolveParams sp{p, bias, solver == PDS_SOLVER_SVD ? PDS_SOLVER_QR : solver, l2_reg, gate_tol, 0};
    if (gated && route == 1) {
        // ---- ONE launch: Gram + one factorisation per group + k substitutions; "choleskey" IS that factorisation, otherwise the
        // groups next to the gate come back as a list and go through the pivoted QR, target by target
        const bool second_pass = sp.solver != PDS_SOLVER_CHOLESKEY;
        int32_t* d_list = second_pass ? reinterpret_cast<int32_t*>(ws_take(ctx, (size_t)ng * sizeof(int32_t))) : nullptr;
        if (second_pass && !d_list) return fail(PDS_ERR_HIP, "workspace allocation failed");
        if (int rc = launch_grouped_multi<T>(ctx, d_tabs + (size_t)k * 18, p, k, bias, n_rows, d_off, ng, l2_reg, gate_tol, second_pass, d_co, d_nu,
                                             d_list, d_words))
            return rc;
        if (second_pass) {
            unsigned h_count = 0;
            PDS_HIP_CHECK(hipMemcpyAsync(&h_count, d_words, sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream));
            PDS_HIP_CHECK(hipStreamSynchronize(ctx->stream));
            const int64_t marked = (int64_t)h_count;
            if (marked > 0) {
                const int64_t mchunk = std::min(chunk, marked);
                T* co_c = reinterpret_cast<T*>(ws_take(ctx, (size_t)mchunk * pp * sizeof(T)));
                uint8_t* fl_c = reinterpret_cast<uint8_t*>(ws_take(ctx, (size_t)mchunk));
                if (!co_c || !fl_c) return fail(PDS_ERR_HIP, "workspace allocation failed");
                for (int64_t k0 = 0; k0 < marked; k0 += mchunk) {
                    const int64_t kc = std::min(mchunk, marked - k0);
                    for (int t = 0; t < k; ++t) {
                        const size_t mark = ctx->ws_used;  // (call-local slices of the launchers: stream order makes the reuse safe)
                        int rc = launch_grouped_moments<T>(ctx, dct[t], p, d_off, kc, d_mom, d_list + k0);
                        if (!rc) rc = launch_solve_marked<T>(ctx, d_mom, kc, sp, co_c, fl_c, nullptr);
                        if (!rc) rc = launch_multi_scatter<T>(ctx, co_c, fl_c, d_list + k0, kc, t, k, pp, t == 0, d_co, d_nu);
                        ctx->ws_used = mark;
                        if (rc) return rc;
                    }
                    if (int rc = launch_multi_null_fill<T>(ctx, d_nu, d_list + k0, kc, k * pp, false, d_co)) return rc;
                }
            }
        }
    } else {
        // ---- per target, what pds_lr_grouped_* runs for that target alone: the fused grouped kernel (gate on), or the grouped
        // Gram records and the pivoted QR (gate off) -- on the one staged frame and the one offsets array
        T* t_co = reinterpret_cast<T*>(ws_take(ctx, (size_t)ng * pp * sizeof(T)));
        uint8_t* t_fl = reinterpret_cast<uint8_t*>(ws_take(ctx, (size_t)ng));
        if (!t_co || !t_fl) return fail(PDS_ERR_HIP, "workspace allocation failed");
        for (int t = 0; t < k; ++t) {
            const size_t mark = ctx->ws_used;
            int rc = PDS_OK;
            if (gated && ng < (1ll << 31)) {
                rc = launch_grouped_fused<T>(ctx, dct[t], p, n_rows, d_off, ng, sp, t_co, t_fl, d_mom, chunk);
            } else {
                for (int64_t g0 = 0; g0 < ng && !rc; g0 += chunk) {
                    const int64_t gc = std::min(chunk, ng - g0);
                    rc = launch_grouped_moments<T>(ctx, dct[t], p, d_off + g0, gc, d_mom);
                    if (!rc) rc = launch_solve<T>(ctx, d_mom, gc, sp, t_co + g0 * pp, t_fl + g0, nullptr, d_off + g0);
                }
            }
            if (!rc) rc = launch_multi_scatter<T>(ctx, t_co, t_fl, nullptr, ng, t, k, pp, t == 0, d_co, d_nu);
            ctx->ws_used = mark;
            if (rc) return rc;
        }
        // (the gate depends on X alone, and a gated fit passes a regular X'X whatever the right-hand side holds: a NaN in one target
        //  comes back as NaN coefficients of that target under a clear flag -- the group is null for every target, as in the one kernel.
        //  Without the gate the flags are those of pds_lr_grouped_*, target by target, and a group is null when any of them is.)
        if (int rc = launch_multi_null_fill<T>(ctx, d_nu, nullptr, ng, k * pp, gated, d_co)) return rc;
    }
    if (want_pred) {
        T* blk_t = k == 1 ? d_co : reinterpret_cast<T*>(ws_take(ctx, (size_t)ng * pp * sizeof(T)));
        if (!blk_t) return fail(PDS_ERR_HIP, "workspace allocation failed");
        for (int t = 0; t < k; ++t) {
            if (k > 1)
                if (int rc = launch_multi_extract<T>(ctx, d_co, ng, t, k, pp, blk_t)) return rc;
            if (int rc = launch_grouped_pred<T>(ctx, d_tabs + (size_t)t * 18, p, bias, n_rows, d_off, ng, blk_t, d_nu, d_perm,
                                                d_pred ? d_pred + (size_t)t * n_rows : nullptr, d_resid ? d_resid + (size_t)t * n_rows : nullptr,
                                                t == 0 ? d_rn : nullptr))
                return rc;
        }
    }
    PDS_HIP_CHECK(hipStreamSynchronize(ctx->stream));  // (tabs: source of the table copy)
    return PDS_OK;
}

static int multi_grouped_check(int n_targets, int n_feat) {
    if (n_targets < 1) return fail(PDS_ERR_INVALID, "need at least one target");
    if (n_feat < 1) return fail(PDS_ERR_INVALID, "need at least one feature column");
    if (n_feat > kMaxFeatSmall || n_targets > kMultiGroupedMaxTargets) return fail(PDS_ERR_UNSUPPORTED, kMultiGroupedLimit);
    return PDS_OK;
}

// Host frames and host outputs are staged in ctx->wkeyed.
template <typename T>
static int multi_grouped_impl(pds_ctx* ctx, const T* const* cols, int n_targets, int n_feat, int64_t n_rows, const int64_t* offsets,
                              int64_t n_groups, pds_space space, int add_bias, T l2_reg, int solver, T singular_x_tol, T* coeffs, uint8_t* is_null,
                              T* pred, T* resid, uint8_t* row_null) {
    if (!ctx || !cols || !offsets || !coeffs || !is_null) return fail(PDS_ERR_INVALID, "null argument");
    if (int rc = multi_grouped_check(n_targets, n_feat)) return rc;
    if (n_groups <= 0 || n_rows <= 0) return fail(PDS_ERR_EMPTY, "Empty data");
    const int k = n_targets, nc = n_feat + k;
    if (int rc = check_cols<T>(cols, nc - 1)) return rc;
    PDS_HIP_CHECK(hipSetDevice(ctx->device));
    const int bias = add_bias ? 1 : 0, pp = n_feat + bias;
    const bool host = space == PDS_HOST;
    const auto up = Bump::up;
    T *d_co, *d_pred, *d_resid;
    uint8_t *d_nu, *d_rn;
    StagedOuts outs(host, (size_t)n_groups), row_outs(host, (size_t)n_rows);
    outs.add(&d_co, coeffs, (size_t)k * pp);
    outs.add(&d_nu, is_null, 1);
    row_outs.add(&d_pred, pred, k);
    row_outs.add(&d_resid, resid, k);
    row_outs.add(&d_rn, row_null, 1);
    size_t need = 4096 + outs.bytes() + row_outs.bytes();
    if (host) need += up((size_t)n_rows * sizeof(T)) * nc + up((size_t)(n_groups + 1) * 8);
    if (int rc = ensure_ws(ctx, ctx->wkeyed, need)) return rc;
    Bump w{static_cast<char*>(ctx->wkeyed.ptr)};
    std::vector<const T*> src(cols, cols + nc);  // [t_0 .. t_{k-1}, x_1 .. x_p]: staged ONCE for all targets
    const int64_t* d_off = offsets;
    if (host) {
        if (int rc = cols_to_device<T>(ctx, w, src, n_rows)) return rc;
        int64_t* t = w.take<int64_t>((size_t)n_groups + 1);
        PDS_HIP_CHECK(hipMemcpyAsync(t, offsets, (size_t)(n_groups + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
        d_off = t;
    }
    outs.place(w);
    row_outs.place(w);
    if (int rc = multi_fit_device<T>(ctx, src, k, n_feat, n_rows, d_off, n_groups, bias, l2_reg > (T)0 ? (double)l2_reg : 0.0, solver,
                                     (double)singular_x_tol, d_co, d_nu, d_pred, d_resid, d_rn, nullptr))
        return rc;
    if (int rc = staged_copy_back(ctx, outs, (size_t)n_groups)) return rc;
    if (int rc = staged_copy_back(ctx, row_outs, (size_t)n_rows)) return rc;
    PDS_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return PDS_OK;
}

// int64 keys in any row order through the shared key-ordering stage (capi_keyed_frame.hpp): the keys are ordered ONCE and all p + k
// columns ride through the gather together; per-row outputs go back to the frame's own row order through the sort permutation.
template <typename T>
static int multi_by_key_impl(pds_ctx* ctx, const T* const* cols, const int64_t* keys, int n_targets, int n_feat, int64_t n_rows, pds_space space,
                             int add_bias, T l2_reg, int solver, T singular_x_tol, int64_t max_groups, int64_t* out_keys, T* coeffs,
                             uint8_t* is_null, int64_t* n_groups, T* pred, T* resid, uint8_t* row_null) {
    // (a caller that only wants the per-row outputs passes no out_keys / coeffs / is_null / n_groups: pds_lr_by_key_pred_*'s rule)
    const bool want_pred = pred || resid || row_null;
    const bool want_coef = out_keys || coeffs;
    if (!ctx || !cols || !keys) return fail(PDS_ERR_INVALID, "null argument");
    if (want_coef ? (!out_keys || !coeffs || !is_null || !n_groups) : !want_pred) return fail(PDS_ERR_INVALID, "null argument");
    if (int rc = multi_grouped_check(n_targets, n_feat)) return rc;
    if (n_rows <= 0) return fail(PDS_ERR_EMPTY, "Empty data");
    if (!want_coef) max_groups = n_rows;
    if (max_groups < 1) return fail(PDS_ERR_INVALID, "max_groups must be positive");
    const int k = n_targets, nc = n_feat + k;
    if (int rc = check_cols<T>(cols, nc - 1)) return rc;
    PDS_HIP_CHECK(hipSetDevice(ctx->device));
    const int bias = add_bias ? 1 : 0, pp = n_feat + bias;
    const bool host = space == PDS_HOST;
    T *d_co, *d_pred, *d_resid;
    uint8_t *d_nu, *d_rn;
    StagedOuts outs(host, (size_t)std::min<int64_t>(max_groups, n_rows)), row_outs(host, (size_t)n_rows);
    outs.add(&d_co, coeffs, (size_t)k * pp, StagedOuts::kScratch);  // (the fit needs both whether or not the caller asked for them)
    outs.add(&d_nu, is_null, 1, StagedOuts::kScratch);
    row_outs.add(&d_pred, pred, k);
    row_outs.add(&d_resid, resid, k);
    row_outs.add(&d_rn, row_null, 1);
    KeyedFrame<T> kf;
    kf.src.assign(cols, cols + nc);
    Bump w{};
    if (int rc = keyed_frame_open<T>(ctx, keys, n_rows, space, max_groups, [&](bool) { return outs.bytes() + row_outs.bytes(); }, n_groups, kf, w))
        return rc;
    const int64_t ng = kf.ng;
    outs.place(w);
    row_outs.place(w);
    if (int rc = multi_fit_device<T>(ctx, kf.src, k, n_feat, n_rows, kf.d_offsets, ng, bias, l2_reg > (T)0 ? (double)l2_reg : 0.0, solver,
                                     (double)singular_x_tol, d_co, d_nu, d_pred, d_resid, d_rn, kf.d_perm))
        return rc;
    if (out_keys)
        PDS_HIP_CHECK(hipMemcpyAsync(out_keys, kf.d_unique, (size_t)ng * 8, host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, ctx->stream));
    if (int rc = staged_copy_back(ctx, outs, (size_t)ng)) return rc;
    if (int rc = staged_copy_back(ctx, row_outs, (size_t)n_rows)) return rc;
    PDS_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return PDS_OK;
}
