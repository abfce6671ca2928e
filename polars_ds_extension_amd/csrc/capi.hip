// capi.hip -- the extern "C" surface declared in include/pds_lstsq.h: context management, host <-> HBM
// staging, and the per-expression pipelines that string the kernels together.
#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <mutex>
#include <thread>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <mutex>

#include <hipcub/hipcub.hpp>

#include "common.hpp"
#include "grouped_report.hpp"
#include "grouped_split_dev.hpp"

namespace pds {

#include "capi_core.hpp"
#include "capi_staging.hpp"
#include "capi_lr.hpp"
#include "capi_report.hpp"
#include "capi_staged_out.hpp"
#include "capi_keyed_frame.hpp"
#include "capi_group_chunks.hpp"
#include "capi_grouped.hpp"
#include "capi_report_grouped.hpp"
#include "capi_multi.hpp"
#include "capi_rolling.hpp"
#include "capi_models.hpp"
#include "capi_glm_grouped.hpp"
#include "capi_glm_report.hpp"
#include "capi_rcond_grouped.hpp"
#include "capi_multi_grouped.hpp"
#include "capi_mixed.hpp"
#include "capi_report_cluster.hpp"
#include "capi_within_cluster.hpp"
#include "capi_within.hpp"
#include "capi_within2.hpp"
#include "capi_glm_sandwich.hpp"
#include "capi_glm_within.hpp"

}  // namespace pds

// =============================================================================================
// extern "C"
// =============================================================================================
using namespace pds;

// pds_cluster_key -> the WithinCluster the pipelines take (null: the call without a cluster key); its outputs back to the caller
template <typename F>
static int with_cluster_key(pds_cluster_key* cl, pds_space space, F&& call) {
    if (!cl) return call(nullptr);
    pds::WithinCluster wc;
    wc.codes = cl->codes;
    wc.code_space = space;
    wc.n_levels = cl->n_levels;
    const int rc = call(&wc);
    cl->n_clusters = wc.n_clusters;
    cl->nested1 = wc.nested1;
    cl->nested2 = wc.nested2;
    return rc;
}

extern "C" {

const char* pds_last_error(void) { return g_err.c_str(); }
const char* pds_version(void) { return "pds_lstsq_hip 0.1.0 (gfx950)"; }

int pds_ctx_create(int device, pds_ctx** out) {
    if (!out) return fail(PDS_ERR_INVALID, "null out pointer");
    int ndev = 0;
    PDS_HIP_CHECK(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail(PDS_ERR_HIP, "no such HIP device");
    hipDeviceProp_t prop;
    PDS_HIP_CHECK(hipGetDeviceProperties(&prop, device));
    if (std::string(prop.gcnArchName).rfind("gfx950", 0) != 0)
        return fail(PDS_ERR_HIP, std::string("libpds_lstsq_hip is built for gfx950 only, device is ") + prop.gcnArchName);
    PDS_HIP_CHECK(hipSetDevice(device));
    pds_ctx* c = new pds_ctx();
    c->device = device;
    c->num_cus = prop.multiProcessorCount;
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
        delete c;
        return fail(PDS_ERR_HIP, "hipStreamCreate failed");
    }
    c->own_stream = true;
    {   // option defaults from the environment, once per context (pds_ctx_set_option changes them afterwards)
        const char* ks = std::getenv("PDS_KEYED_SORT");
        c->opt_keyed_sort = ks && ks[0] == '1';
        const char* wn = std::getenv("PDS_WIDE_F32_NATIVE");
        c->opt_wide_f32_native = wn && wn[0] == '1';
    }
    const size_t pbytes = (size_t)c->num_cus * 8 * kPartStride * sizeof(double);
    if (hipMalloc(reinterpret_cast<void**>(&c->partials), pbytes) != hipSuccess) {
        (void)hipStreamDestroy(c->stream);
        delete c;
        return fail(PDS_ERR_HIP, "hipMalloc(partials) failed");
    }
    *out = c;
    return PDS_OK;
}

void pds_ctx_destroy(pds_ctx* ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    if (ctx->partials) (void)hipFree(ctx->partials);
    if (ctx->ws.ptr) (void)hipFree(ctx->ws.ptr);
    for (void* q : ctx->ws_spill) (void)hipFree(q);
    if (ctx->stage.ptr) (void)hipFree(ctx->stage.ptr);
    if (ctx->solve_ws.ptr) (void)hipFree(ctx->solve_ws.ptr);
    if (ctx->keyed.ptr) (void)hipFree(ctx->keyed.ptr);
    if (ctx->wkeyed.ptr) (void)hipFree(ctx->wkeyed.ptr);
    if (ctx->mark_count) (void)hipFree(ctx->mark_count);
    if (ctx->col_table_dev) (void)hipFree(ctx->col_table_dev);
    if (ctx->wait_timeouts) (void)hipFree(ctx->wait_timeouts);
    if (ctx->mark_host) (void)hipHostFree(ctx->mark_host);
    if (ctx->pinned) (void)hipHostFree(ctx->pinned);
    if (ctx->pinned_in) (void)hipHostFree(ctx->pinned_in);
    for (auto& e : ctx->ev_pending) {
        (void)hipEventDestroy(e.a);
        (void)hipEventDestroy(e.b);
    }
    for (auto e : ctx->ev_pool) (void)hipEventDestroy(e);
    if (ctx->own_stream && ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

int pds_ctx_set_stream(pds_ctx* ctx, void* hip_stream) {
    if (!ctx) return fail(PDS_ERR_INVALID, "null ctx");
    PDS_HIP_CHECK(hipSetDevice(ctx->device));
    PDS_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    if (ctx->own_stream && ctx->stream) (void)hipStreamDestroy(ctx->stream);
    // NULL is a valid hipStream_t: the (legacy) default stream, which is what torch uses unless told otherwise
    ctx->stream = reinterpret_cast<hipStream_t>(hip_stream);
    ctx->own_stream = false;
    ctx->caller_stream = true;  // (the caller orders its own work on it: device-resident grouped fits may return stream-ordered)
    ctx->col_table_valid = false;  // (the cached pointer table was written on the old stream: the next call writes it again)
    return PDS_OK;
}

int pds_ctx_synchronize(pds_ctx* ctx) {
    if (!ctx) return fail(PDS_ERR_INVALID, "null ctx");
    PDS_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return PDS_OK;
}

int pds_ctx_num_cus(const pds_ctx* ctx) { return ctx ? ctx->num_cus : 0; }

int pds_ctx_set_option(pds_ctx* ctx, const char* name, long long value) {
    if (!ctx || !name) return fail(PDS_ERR_INVALID, "null argument");
    const std::string n(name);
    if (n == "keyed_sort") ctx->opt_keyed_sort = value != 0;
    else if (n == "wide_f32_native") ctx->opt_wide_f32_native = value != 0;
    else if (n == "glm_split_rows") ctx->opt_glm_split_rows = value > 0 ? (int64_t)value : 0;
    else if (n == "mixed_split_rows") ctx->opt_mixed_split_rows = value > 0 ? (int64_t)value : 0;
    else if (n == "cluster_split_rows") ctx->opt_cluster_split_rows = value > 0 ? (int64_t)value : 0;
    else if (n == "cluster_waves") ctx->opt_cluster_waves = value > 0 ? (int64_t)value : 0;
    else if (n == "within_split_rows") ctx->opt_within_split_rows = value > 0 ? (int64_t)value : 0;
    else if (n == "within2_accel") {
        if (value != 0 && value != 1) return fail(PDS_ERR_INVALID, "within2_accel: 0 (plain sweeps) or 1 (Irons-Tuck)");
        ctx->opt_within2_accel = (int64_t)value;
    } else if (n == "report_chunk_groups") ctx->opt_report_chunk_groups = value > 0 ? (int64_t)value : 0;
    else if (n == "grouped_fused_waves") ctx->opt_fused_waves = value > 0 ? (int64_t)value : 0;
    else if (n == "grouped_fused_late_permille") {
        if (value < 0 || value > 999) return fail(PDS_ERR_INVALID, "grouped_fused_late_permille: 0 (the default rule) or 1 .. 999");
        ctx->opt_fused_late_permille = (int64_t)value;
    } else if (n == "grouped_multi_route") {
        if (value < 0 || value > 2) return fail(PDS_ERR_INVALID, "grouped_multi_route: 0 (choose), 1 (one kernel) or 2 (per target)");
        ctx->opt_multi_route = (int64_t)value;
    } else if (n == "grouped_multi_waves") ctx->opt_multi_waves = value > 0 ? (int64_t)value : 0;
    else if (n == "rolling_waves") ctx->opt_rolling_waves = value > 0 ? (int64_t)value : 0;
    else if (n == "blocking_return") {
        if (value != 0 && value != 1) return fail(PDS_ERR_INVALID, "blocking_return: 0 (stream-ordered where the header allows it) or 1 (always synchronise)");
        PDS_HIP_CHECK(hipStreamSynchronize(ctx->stream));  // (what earlier stream-ordered calls left queued)
        ctx->opt_blocking_return = (int64_t)value;
    } else return fail(PDS_ERR_INVALID, "unknown context option: " + n);
    return PDS_OK;
}

int pds_ctx_get_option(const pds_ctx* ctx, const char* name, long long* value) {
    if (!ctx || !name || !value) return fail(PDS_ERR_INVALID, "null argument");
    const std::string n(name);
    if (n == "keyed_sort") *value = ctx->opt_keyed_sort ? 1 : 0;
    else if (n == "wide_f32_native") *value = ctx->opt_wide_f32_native ? 1 : 0;
    else if (n == "glm_split_rows") *value = ctx->opt_glm_split_rows;
    else if (n == "mixed_split_rows") *value = ctx->opt_mixed_split_rows;
    else if (n == "cluster_split_rows") *value = ctx->opt_cluster_split_rows;
    else if (n == "cluster_waves") *value = ctx->opt_cluster_waves;
    else if (n == "within_split_rows") *value = ctx->opt_within_split_rows;
    else if (n == "within2_accel") *value = ctx->opt_within2_accel;
    else if (n == "report_chunk_groups") *value = ctx->opt_report_chunk_groups;
    else if (n == "grouped_fused_waves") *value = ctx->opt_fused_waves;
    else if (n == "grouped_fused_late_permille") *value = ctx->opt_fused_late_permille;
    else if (n == "grouped_multi_route") *value = ctx->opt_multi_route;
    else if (n == "grouped_multi_waves") *value = ctx->opt_multi_waves;
    else if (n == "rolling_waves") *value = ctx->opt_rolling_waves;
    else if (n == "blocking_return") *value = ctx->opt_blocking_return;
    else return fail(PDS_ERR_INVALID, "unknown context option: " + n);
    return PDS_OK;
}

int pds_grouped_fused_split(const int64_t* group_offsets, int64_t n_groups, int waves, int late_permille, int64_t* first_group,
                            int64_t* end_group) {
    if (!group_offsets || !first_group || !end_group) return fail(PDS_ERR_INVALID, "null argument");
    if (n_groups < 0 || waves < 1 || late_permille < 0 || late_permille > 999) return fail(PDS_ERR_INVALID, "pds_grouped_fused_split: bad argument");
    // the kernel's own rule, on the host: first group whose start row is >= the wave's first row (lower bound over offsets[0 .. n_groups))
    const int64_t base = group_offsets[0], total = group_offsets[n_groups] - base;
    auto bound = [&](int64_t w) -> int64_t {
        if (w == 0) return 0;
        if (w == waves) return n_groups;
        return std::lower_bound(group_offsets, group_offsets + n_groups, base + pds::fused_split_row(w, waves, total, late_permille)) - group_offsets;
    };
    for (int w = 0; w < waves; ++w) {
        first_group[w] = bound(w);
        end_group[w] = std::max(bound(w + 1), first_group[w]);
    }
    return PDS_OK;
}

int pds_glm_irls_f64(pds_ctx* ctx, const double* const* cols, int n_feat, int64_t n_rows, pds_space space, int add_bias, int link,
                     int variance, double tol, int max_iter, double* coeffs, int* n_iter) {
    return pds::glm_irls_impl<double>(ctx, cols, n_feat, n_rows, space, add_bias, link, variance, tol, max_iter, coeffs, n_iter);
}
int pds_glm_irls_f32(pds_ctx* ctx, const float* const* cols, int n_feat, int64_t n_rows, pds_space space, int add_bias, int link,
                     int variance, float tol, int max_iter, float* coeffs, int* n_iter) {
    return pds::glm_irls_impl<float>(ctx, cols, n_feat, n_rows, space, add_bias, link, variance, tol, max_iter, coeffs, n_iter);
}

int pds_glm_irls_grouped_f64(pds_ctx* ctx, const double* const* cols, int n_feat, int64_t n_rows, const int64_t* group_offsets,
                             int64_t n_groups, pds_space space, int add_bias, int link, int variance, double tol, int max_iter,
                             double* coeffs, int32_t* n_iter, uint8_t* is_null, double* pred, uint8_t* row_null) {
    return pds::glm_grouped_impl<double>(ctx, cols, n_feat, n_rows, group_offsets, n_groups, space, add_bias, link, variance, 0.0, 0.0, tol,
                                         max_iter, coeffs, n_iter, is_null, pred, row_null);
}
int pds_glm_irls_grouped_f32(pds_ctx* ctx, const float* const* cols, int n_feat, int64_t n_rows, const int64_t* group_offsets,
                             int64_t n_groups, pds_space space, int add_bias, int link, int variance, float tol, int max_iter,
                             float* coeffs, int32_t* n_iter, uint8_t* is_null, float* pred, uint8_t* row_null) {
    return pds::glm_grouped_impl<float>(ctx, cols, n_feat, n_rows, group_offsets, n_groups, space, add_bias, link, variance, 0.0f, 0.0f, tol,
                                        max_iter, coeffs, n_iter, is_null, pred, row_null);
}
int pds_glm_irls_by_key_f64(pds_ctx* ctx, const double* const* cols, const int64_t* keys, int n_feat, int64_t n_rows, pds_space space,
                            int add_bias, int link, int variance, double tol, int max_iter, int64_t max_groups, int64_t* out_keys,
                            double* coeffs, int32_t* n_iter, uint8_t* is_null, int64_t* n_groups, double* pred, uint8_t* row_null) {
    return pds::glm_by_key_impl<double>(ctx, cols, keys, n_feat, n_rows, space, add_bias, link, variance, 0.0, 0.0, tol, max_iter, max_groups,
                                        out_keys, coeffs, n_iter, is_null, n_groups, pred, row_null);
}
int pds_glm_irls_by_key_f32(pds_ctx* ctx, const float* const* cols, const int64_t* keys, int n_feat, int64_t n_rows, pds_space space,
                            int add_bias, int link, int variance, float tol, int max_iter, int64_t max_groups, int64_t* out_keys,
                            float* coeffs, int32_t* n_iter, uint8_t* is_null, int64_t* n_groups, float* pred, uint8_t* row_null) {
    return pds::glm_by_key_impl<float>(ctx, cols, keys, n_feat, n_rows, space, add_bias, link, variance, 0.0f, 0.0f, tol, max_iter, max_groups,
                                       out_keys, coeffs, n_iter, is_null, n_groups, pred, row_null);
}

// prior weights and an offset per row: the argument lists of pds_glm_irls_* / _grouped_* / _by_key_* with `weights`, `offset` after
// `cols` (both nullable; both null: the twin's call)
int pds_glm_irls_wo_f64(pds_ctx* ctx, const double* const* cols, const double* weights, const double* offset, int n_feat, int64_t n_rows,
                        pds_space space, int add_bias, int link, int variance, double tol, int max_iter, double* coeffs, int* n_iter) {
    return pds::glm_irls_wo_impl<double>(ctx, cols, weights, offset, n_feat, n_rows, space, add_bias, link, variance, tol, max_iter, coeffs,
                                         n_iter);
}
int pds_glm_irls_wo_f32(pds_ctx* ctx, const float* const* cols, const float* weights, const float* offset, int n_feat, int64_t n_rows,
                        pds_space space, int add_bias, int link, int variance, float tol, int max_iter, float* coeffs, int* n_iter) {
    return pds::glm_irls_wo_impl<float>(ctx, cols, weights, offset, n_feat, n_rows, space, add_bias, link, variance, tol, max_iter, coeffs,
                                        n_iter);
}
int pds_glm_irls_wo_grouped_f64(pds_ctx* ctx, const double* const* cols, const double* weights, const double* offset, int n_feat,
                                int64_t n_rows, const int64_t* group_offsets, int64_t n_groups, pds_space space, int add_bias, int link,
                                int variance, double tol, int max_iter, double* coeffs, int32_t* n_iter, uint8_t* is_null, double* pred,
                                uint8_t* row_null) {
    return pds::glm_grouped_impl<double>(ctx, cols, n_feat, n_rows, group_offsets, n_groups, space, add_bias, link, variance, 0.0, 0.0, tol,
                                         max_iter, coeffs, n_iter, is_null, pred, row_null, nullptr, weights, offset);
}
int pds_glm_irls_wo_grouped_f32(pds_ctx* ctx, const float* const* cols, const float* weights, const float* offset, int n_feat, int64_t n_rows,
                                const int64_t* group_offsets, int64_t n_groups, pds_space space, int add_bias, int link, int variance,
                                float tol, int max_iter, float* coeffs, int32_t* n_iter, uint8_t* is_null, float* pred, uint8_t* row_null) {
    return pds::glm_grouped_impl<float>(ctx, cols, n_feat, n_rows, group_offsets, n_groups, space, add_bias, link, variance, 0.0f, 0.0f, tol,
                                        max_iter, coeffs, n_iter, is_null, pred, row_null, nullptr, weights, offset);
}
int pds_glm_irls_wo_by_key_f64(pds_ctx* ctx, const double* const* cols, const double* weights, const double* offset, const int64_t* keys,
                               int n_feat, int64_t n_rows, pds_space space, int add_bias, int link, int variance, double tol, int max_iter,
                               int64_t max_groups, int64_t* out_keys, double* coeffs, int32_t* n_iter, uint8_t* is_null, int64_t* n_groups,
                               double* pred, uint8_t* row_null) {
    return pds::glm_by_key_impl<double>(ctx, cols, keys, n_feat, n_rows, space, add_bias, link, variance, 0.0, 0.0, tol, max_iter, max_groups,
                                        out_keys, coeffs, n_iter, is_null, n_groups, pred, row_null, weights, offset);
}
int pds_glm_irls_wo_by_key_f32(pds_ctx* ctx, const float* const* cols, const float* weights, const float* offset, const int64_t* keys,
                               int n_feat, int64_t n_rows, pds_space space, int add_bias, int link, int variance, float tol, int max_iter,
                               int64_t max_groups, int64_t* out_keys, float* coeffs, int32_t* n_iter, uint8_t* is_null, int64_t* n_groups,
                               float* pred, uint8_t* row_null) {
    return pds::glm_by_key_impl<float>(ctx, cols, keys, n_feat, n_rows, space, add_bias, link, variance, 0.0f, 0.0f, tol, max_iter, max_groups,
                                       out_keys, coeffs, n_iter, is_null, n_groups, pred, row_null, weights, offset);
}

// the grouped GLM report: the fit of pds_glm_irls_grouped_* / _by_key_* and its report per group (capi_glm_report.hpp)
int pds_glm_report_grouped_f64(pds_ctx* ctx, const double* const* cols, int n_feat, int64_t n_rows, const int64_t* group_offsets,
                               int64_t n_groups, pds_space space, int add_bias, int link, int variance, double tol, int max_iter,
                               double* coeffs, int32_t* n_iter, uint8_t* is_null, const pds_glm_report_out* out) {
    return pds::glm_report_grouped_impl<double>(ctx, cols, n_feat, n_rows, group_offsets, n_groups, space, add_bias, link, variance, tol,
                                                max_iter, coeffs, n_iter, is_null, out);
}
int pds_glm_report_grouped_f32(pds_ctx* ctx, const float* const* cols, int n_feat, int64_t n_rows, const int64_t* group_offsets,
                               int64_t n_groups, pds_space space, int add_bias, int link, int variance, float tol, int max_iter,
                               float* coeffs, int32_t* n_iter, uint8_t* is_null, const pds_glm_report_out* out) {
    return pds::glm_report_grouped_impl<float>(ctx, cols, n_feat, n_rows, group_offsets, n_groups, space, add_bias, link, variance, tol,
                                               max_iter, coeffs, n_iter, is_null, out);
}
int pds_glm_report_by_key_f64(pds_ctx* ctx, const double* const* cols, const int64_t* keys, int n_feat, int64_t n_rows, pds_space space,
                              int add_bias, int link, int variance, double tol, int max_iter, int64_t max_groups, int64_t* out_keys,
                              double* coeffs, int32_t* n_iter, uint8_t* is_null, int64_t* n_groups, const pds_glm_report_out* out) {
    return pds::glm_report_by_key_impl<double>(ctx, cols, keys, n_feat, n_rows, space, add_bias, link, variance, tol, max_iter, max_groups,
                                               out_keys, coeffs, n_iter, is_null, n_groups, out);
}
int pds_glm_report_by_key_f32(pds_ctx* ctx, const float* const* cols, const int64_t* keys, int n_feat, int64_t n_rows, pds_space space,
                              int add_bias, int link, int variance, float tol, int max_iter, int64_t max_groups, int64_t* out_keys,
                              float* coeffs, int32_t* n_iter, uint8_t* is_null, int64_t* n_groups, const pds_glm_report_out* out) {
    return pds::glm_report_by_key_impl<float>(ctx, cols, keys, n_feat, n_rows, space, add_bias, link, variance, tol, max_iter, max_groups,
                                              out_keys, coeffs, n_iter, is_null, n_groups, out);
}

// the report with prior weights and an offset per row: the argument lists of pds_glm_report_* with `weights`, `offset` after `cols`
int pds_glm_report_wo_grouped_f64(pds_ctx* ctx, const double* const* cols, const double* weights, const double* offset, int n_feat, int64_t n_rows,
                                  const int64_t* group_offsets, int64_t n_groups, pds_space space, int add_bias, int link, int variance,
                                  double tol, int max_iter, double* coeffs, int32_t* n_iter, uint8_t* is_null, const pds_glm_report_out* out) {
    return pds::glm_report_grouped_impl<double>(ctx, cols, n_feat, n_rows, group_offsets, n_groups, space, add_bias, link, variance, tol,
                                                max_iter, coeffs, n_iter, is_null, out, weights, offset);
}
int pds_glm_report_wo_by_key_f64(pds_ctx* ctx, const double* const* cols, const double* weights, const double* offset, const int64_t* keys, int n_feat,
                                 int64_t n_rows, pds_space space, int add_bias, int link, int variance, double tol, int max_iter,
                                 int64_t max_groups, int64_t* out_keys, double* coeffs, int32_t* n_iter, uint8_t* is_null, int64_t* n_groups,
                                 const pds_glm_report_out* out) {
    return pds::glm_report_by_key_impl<double>(ctx, cols, keys, n_feat, n_rows, space, add_bias, link, variance, tol, max_iter, max_groups,
                                               out_keys, coeffs, n_iter, is_null, n_groups, out, weights, offset);
}
int pds_glm_report_wo_grouped_f32(pds_ctx* ctx, const float* const* cols, const float* weights, const float* offset, int n_feat, int64_t n_rows,
                                  const int64_t* group_offsets, int64_t n_groups, pds_space space, int add_bias, int link, int variance,
                                  float tol, int max_iter, float* coeffs, int32_t* n_iter, uint8_t* is_null, const pds_glm_report_out* out) {
    return pds::glm_report_grouped_impl<float>(ctx, cols, n_feat, n_rows, group_offsets, n_groups, space, add_bias, link, variance, tol,
                                                max_iter, coeffs, n_iter, is_null, out, weights, offset);
}
int pds_glm_report_wo_by_key_f32(pds_ctx* ctx, const float* const* cols, const float* weights, const float* offset, const int64_t* keys, int n_feat,
                                 int64_t n_rows, pds_space space, int add_bias, int link, int variance, float tol, int max_iter,
                                 int64_t max_groups, int64_t* out_keys, float* coeffs, int32_t* n_iter, uint8_t* is_null, int64_t* n_groups,
                                 const pds_glm_report_out* out) {
    return pds::glm_report_by_key_impl<float>(ctx, cols, keys, n_feat, n_rows, space, add_bias, link, variance, tol, max_iter, max_groups,
                                               out_keys, coeffs, n_iter, is_null, n_groups, out, weights, offset);
}

// the one-model report with robust / cluster-robust standard errors (capi_glm_sandwich.hpp)
int pds_glm_report_robust_f64(pds_ctx* ctx, const double* const* cols, const double* weights, const double* offset, int n_feat, int64_t n_rows,
                              pds_space space, int add_bias, int link, int variance, double tol, int max_iter, int se_type, double* coeffs,
                              int32_t* n_iter, const pds_glm_report_out* out, int64_t* n_clusters) {
    return pds::glm_sandwich_impl<double>(ctx, cols, weights, offset, n_feat, n_rows, nullptr, 0, space, add_bias, link, variance, tol, max_iter,
                                       se_type, false, coeffs, n_iter, out, n_clusters);
}
int pds_glm_report_cluster_grouped_f64(pds_ctx* ctx, const double* const* cols, const double* weights, const double* offset, int n_feat,
                                       int64_t n_rows, const int64_t* cluster_offsets, int64_t n_offsets, pds_space space, int add_bias,
                                       int link, int variance, double tol, int max_iter, int se_type, double* coeffs, int32_t* n_iter,
                                       const pds_glm_report_out* out, int64_t* n_clusters) {
    return pds::glm_sandwich_impl<double>(ctx, cols, weights, offset, n_feat, n_rows, cluster_offsets, n_offsets, space, add_bias, link, variance,
                                       tol, max_iter, se_type, true, coeffs, n_iter, out, n_clusters);
}
int pds_glm_report_cluster_by_key_f64(pds_ctx* ctx, const double* const* cols, const double* weights, const double* offset, const int64_t* keys,
                                      int n_feat, int64_t n_rows, pds_space space, int add_bias, int link, int variance, double tol,
                                      int max_iter, int se_type, double* coeffs, int32_t* n_iter, const pds_glm_report_out* out,
                                      int64_t* n_clusters) {
    return pds::glm_sandwich_by_key_impl<double>(ctx, cols, weights, offset, keys, n_feat, n_rows, space, add_bias, link, variance, tol, max_iter,
                                              se_type, coeffs, n_iter, out, n_clusters);
}
int pds_glm_report_robust_f32(pds_ctx* ctx, const float* const* cols, const float* weights, const float* offset, int n_feat, int64_t n_rows,
                              pds_space space, int add_bias, int link, int variance, float tol, int max_iter, int se_type, float* coeffs,
                              int32_t* n_iter, const pds_glm_report_out* out, int64_t* n_clusters) {
    return pds::glm_sandwich_impl<float>(ctx, cols, weights, offset, n_feat, n_rows, nullptr, 0, space, add_bias, link, variance, tol, max_iter,
                                       se_type, false, coeffs, n_iter, out, n_clusters);
}
int pds_glm_report_cluster_grouped_f32(pds_ctx* ctx, const float* const* cols, const float* weights, const float* offset, int n_feat,
                                       int64_t n_rows, const int64_t* cluster_offsets, int64_t n_offsets, pds_space space, int add_bias,
                                       int link, int variance, float tol, int max_iter, int se_type, float* coeffs, int32_t* n_iter,
                                       const pds_glm_report_out* out, int64_t* n_clusters) {
    return pds::glm_sandwich_impl<float>(ctx, cols, weights, offset, n_feat, n_rows, cluster_offsets, n_offsets, space, add_bias, link, variance,
                                       tol, max_iter, se_type, true, coeffs, n_iter, out, n_clusters);
}
int pds_glm_report_cluster_by_key_f32(pds_ctx* ctx, const float* const* cols, const float* weights, const float* offset, const int64_t* keys,
                                      int n_feat, int64_t n_rows, pds_space space, int add_bias, int link, int variance, float tol,
                                      int max_iter, int se_type, float* coeffs, int32_t* n_iter, const pds_glm_report_out* out,
                                      int64_t* n_clusters) {
    return pds::glm_sandwich_by_key_impl<float>(ctx, cols, weights, offset, keys, n_feat, n_rows, space, add_bias, link, variance, tol, max_iter,
                                              se_type, coeffs, n_iter, out, n_clusters);
}

// the fixed-effects GLM: IRLS with one absorbed factor (capi_glm_within.hpp)
int pds_glm_within_grouped_f64(pds_ctx* ctx, const double* const* cols, const double* weights, const double* offset, int n_feat, int64_t n_rows,
                               const int64_t* group_offsets, int64_t n_groups, pds_space space, int link, int variance, double tol,
                               int max_iter, int se_type, pds_glm_within_out* out) {
    return pds::glm_within_impl<double>(ctx, cols, weights, offset, n_feat, n_rows, group_offsets, n_groups, space, space, link, variance, tol,
                                        max_iter, se_type, out);
}
int pds_glm_within_grouped_f32(pds_ctx* ctx, const float* const* cols, const float* weights, const float* offset, int n_feat, int64_t n_rows,
                               const int64_t* group_offsets, int64_t n_groups, pds_space space, int link, int variance, float tol,
                               int max_iter, int se_type, pds_glm_within_out* out) {
    return pds::glm_within_impl<float>(ctx, cols, weights, offset, n_feat, n_rows, group_offsets, n_groups, space, space, link, variance, tol,
                                       max_iter, se_type, out);
}
int pds_glm_within_by_key_f64(pds_ctx* ctx, const double* const* cols, const double* weights, const double* offset, const int64_t* keys,
                              int n_feat, int64_t n_rows, pds_space space, int link, int variance, double tol, int max_iter, int se_type,
                              int64_t max_groups, int64_t* out_keys, pds_glm_within_out* out, int64_t* n_groups) {
    return pds::glm_within_by_key_impl<double>(ctx, cols, weights, offset, keys, n_feat, n_rows, space, link, variance, tol, max_iter, se_type,
                                               max_groups, out_keys, out, n_groups);
}
int pds_glm_within_by_key_f32(pds_ctx* ctx, const float* const* cols, const float* weights, const float* offset, const int64_t* keys,
                              int n_feat, int64_t n_rows, pds_space space, int link, int variance, float tol, int max_iter, int se_type,
                              int64_t max_groups, int64_t* out_keys, pds_glm_within_out* out, int64_t* n_groups) {
    return pds::glm_within_by_key_impl<float>(ctx, cols, weights, offset, keys, n_feat, n_rows, space, link, variance, tol, max_iter, se_type,
                                              max_groups, out_keys, out, n_groups);
}

// the elastic-net penalised fits: the argument lists of pds_glm_irls_* with l1_reg, l2_reg after `variance` (<= 0: no penalty)
int pds_glm_enet_f64(pds_ctx* ctx, const double* const* cols, int n_feat, int64_t n_rows, pds_space space, int add_bias, int link,
                     int variance, double l1_reg, double l2_reg, double tol, int max_iter, double* coeffs, int* n_iter) {
    return pds::glm_irls_impl<double>(ctx, cols, n_feat, n_rows, space, add_bias, link, variance, tol, max_iter, coeffs, n_iter, l1_reg, l2_reg);
}
int pds_glm_enet_f32(pds_ctx* ctx, const float* const* cols, int n_feat, int64_t n_rows, pds_space space, int add_bias, int link,
                     int variance, float l1_reg, float l2_reg, float tol, int max_iter, float* coeffs, int* n_iter) {
    return pds::glm_irls_impl<float>(ctx, cols, n_feat, n_rows, space, add_bias, link, variance, tol, max_iter, coeffs, n_iter, l1_reg, l2_reg);
}
int pds_glm_enet_grouped_f64(pds_ctx* ctx, const double* const* cols, int n_feat, int64_t n_rows, const int64_t* group_offsets,
                             int64_t n_groups, pds_space space, int add_bias, int link, int variance, double l1_reg, double l2_reg, double tol,
                             int max_iter, double* coeffs, int32_t* n_iter, uint8_t* is_null, double* pred, uint8_t* row_null) {
    return pds::glm_grouped_impl<double>(ctx, cols, n_feat, n_rows, group_offsets, n_groups, space, add_bias, link, variance, l1_reg, l2_reg, tol,
                                         max_iter, coeffs, n_iter, is_null, pred, row_null);
}
int pds_glm_enet_grouped_f32(pds_ctx* ctx, const float* const* cols, int n_feat, int64_t n_rows, const int64_t* group_offsets,
                             int64_t n_groups, pds_space space, int add_bias, int link, int variance, float l1_reg, float l2_reg, float tol,
                             int max_iter, float* coeffs, int32_t* n_iter, uint8_t* is_null, float* pred, uint8_t* row_null) {
    return pds::glm_grouped_impl<float>(ctx, cols, n_feat, n_rows, group_offsets, n_groups, space, add_bias, link, variance, l1_reg, l2_reg, tol,
                                        max_iter, coeffs, n_iter, is_null, pred, row_null);
}
int pds_glm_enet_by_key_f64(pds_ctx* ctx, const double* const* cols, const int64_t* keys, int n_feat, int64_t n_rows, pds_space space,
                            int add_bias, int link, int variance, double l1_reg, double l2_reg, double tol, int max_iter, int64_t max_groups,
                            int64_t* out_keys, double* coeffs, int32_t* n_iter, uint8_t* is_null, int64_t* n_groups, double* pred,
                            uint8_t* row_null) {
    return pds::glm_by_key_impl<double>(ctx, cols, keys, n_feat, n_rows, space, add_bias, link, variance, l1_reg, l2_reg, tol, max_iter, max_groups,
                                        out_keys, coeffs, n_iter, is_null, n_groups, pred, row_null);
}
int pds_glm_enet_by_key_f32(pds_ctx* ctx, const float* const* cols, const int64_t* keys, int n_feat, int64_t n_rows, pds_space space,
                            int add_bias, int link, int variance, float l1_reg, float l2_reg, float tol, int max_iter, int64_t max_groups,
                            int64_t* out_keys, float* coeffs, int32_t* n_iter, uint8_t* is_null, int64_t* n_groups, float* pred,
                            uint8_t* row_null) {
    return pds::glm_by_key_impl<float>(ctx, cols, keys, n_feat, n_rows, space, add_bias, link, variance, l1_reg, l2_reg, tol, max_iter, max_groups,
                                       out_keys, coeffs, n_iter, is_null, n_groups, pred, row_null);
}

int pds_mixed_reml_grouped_f64(pds_ctx* ctx, const double* const* cols, int n_feat, int64_t n_rows, const int64_t* group_offsets,
                               int64_t n_groups, pds_space space, int max_iter, double tol, double* coeffs, double* std_errors, double* dfs,
                               double* gamma, double* resid_variance, int64_t* n_groups_fit, int32_t* n_eval) {
    return pds::mixed_reml_impl<double>(ctx, cols, n_feat, n_rows, group_offsets, n_groups, space, max_iter, tol, coeffs, std_errors, dfs, gamma,
                                        resid_variance, n_groups_fit, n_eval);
}
int pds_mixed_reml_grouped_f32(pds_ctx* ctx, const float* const* cols, int n_feat, int64_t n_rows, const int64_t* group_offsets,
                               int64_t n_groups, pds_space space, int max_iter, double tol, double* coeffs, double* std_errors, double* dfs,
                               double* gamma, double* resid_variance, int64_t* n_groups_fit, int32_t* n_eval) {
    return pds::mixed_reml_impl<float>(ctx, cols, n_feat, n_rows, group_offsets, n_groups, space, max_iter, tol, coeffs, std_errors, dfs, gamma,
                                       resid_variance, n_groups_fit, n_eval);
}
int pds_mixed_reml_by_key_f64(pds_ctx* ctx, const double* const* cols, const int64_t* keys, int n_feat, int64_t n_rows, pds_space space,
                              int max_iter, double tol, double* coeffs, double* std_errors, double* dfs, double* gamma,
                              double* resid_variance, int64_t* n_groups_fit, int32_t* n_eval) {
    return pds::mixed_reml_by_key_impl<double>(ctx, cols, keys, n_feat, n_rows, space, max_iter, tol, coeffs, std_errors, dfs, gamma,
                                               resid_variance, n_groups_fit, n_eval);
}
int pds_mixed_reml_by_key_f32(pds_ctx* ctx, const float* const* cols, const int64_t* keys, int n_feat, int64_t n_rows, pds_space space,
                              int max_iter, double tol, double* coeffs, double* std_errors, double* dfs, double* gamma,
                              double* resid_variance, int64_t* n_groups_fit, int32_t* n_eval) {
    return pds::mixed_reml_by_key_impl<float>(ctx, cols, keys, n_feat, n_rows, space, max_iter, tol, coeffs, std_errors, dfs, gamma,
                                              resid_variance, n_groups_fit, n_eval);
}
int pds_mixed_profile_grouped_f64(pds_ctx* ctx, const double* const* cols, int n_feat, int64_t n_rows, const int64_t* group_offsets,
                                  int64_t n_groups, pds_space space, const double* gammas, int n_gammas, double* deviance, double* beta,
                                  double* resid_variance) {
    return pds::mixed_profile_impl<double>(ctx, cols, n_feat, n_rows, group_offsets, n_groups, space, gammas, n_gammas, deviance, beta,
                                           resid_variance);
}
int pds_mixed_profile_grouped_f32(pds_ctx* ctx, const float* const* cols, int n_feat, int64_t n_rows, const int64_t* group_offsets,
                                  int64_t n_groups, pds_space space, const double* gammas, int n_gammas, double* deviance, double* beta,
                                  double* resid_variance) {
    return pds::mixed_profile_impl<float>(ctx, cols, n_feat, n_rows, group_offsets, n_groups, space, gammas, n_gammas, deviance, beta,
                                          resid_variance);
}

int pds_lr_rowmajor_f64(pds_ctx* ctx, const double* X, int64_t ld, const double* y, int64_t n_rows, int n_feat, pds_space space,
                        const pds_lr_params* prm, int mode, double* coeffs, int* is_null, double* inv) {
    return pds::lr_rowmajor_impl<double>(ctx, X, ld, y, n_rows, n_feat, space, prm, mode, coeffs, is_null, inv);
}
int pds_lr_rowmajor_f32(pds_ctx* ctx, const float* X, int64_t ld, const float* y, int64_t n_rows, int n_feat, pds_space space,
                        const pds_lr_params* prm, int mode, float* coeffs, int* is_null, float* inv) {
    return pds::lr_rowmajor_impl<float>(ctx, X, ld, y, n_rows, n_feat, space, prm, mode, coeffs, is_null, inv);
}

int pds_rows_to_cols_f64(pds_ctx* ctx, const double* X, int64_t ld, int64_t n_rows, int n_cols, pds_space space, double* out_cols,
                         int64_t col_stride) {
    return pds::rows_to_cols_impl<double>(ctx, X, ld, n_rows, n_cols, space, out_cols, col_stride);
}
int pds_rows_to_cols_f32(pds_ctx* ctx, const float* X, int64_t ld, int64_t n_rows, int n_cols, pds_space space, float* out_cols,
                         int64_t col_stride) {
    return pds::rows_to_cols_impl<float>(ctx, X, ld, n_rows, n_cols, space, out_cols, col_stride);
}

int pds_set_host_staging(double chunk_mb, double resident_max_mb) {
    if (chunk_mb > 0.0) pds::g_host_chunk_mb.store(std::max(chunk_mb, 0.001), std::memory_order_relaxed);
    if (resident_max_mb > 0.0) pds::g_host_resident_mb.store(std::max(resident_max_mb, 0.001), std::memory_order_relaxed);
    return PDS_OK;
}

long long pds_ctx_workspace_spills(const pds_ctx* ctx) { return ctx ? ctx->ws_spill_count : -1; }

long long pds_ctx_workspace_bytes(const pds_ctx* ctx, int which) {
    if (!ctx) return -1;
    const pds::Workspace* w[5] = {&ctx->ws, &ctx->stage, &ctx->solve_ws, &ctx->keyed, &ctx->wkeyed};
    return which >= 0 && which < 5 ? (long long)w[which]->bytes : -1;
}

int pds_ctx_set_timing(pds_ctx* ctx, int enable) {
    if (!ctx) return fail(PDS_ERR_INVALID, "null ctx");
    ctx->timing = enable != 0;
    return PDS_OK;
}

int pds_ctx_get_timing(pds_ctx* ctx, double* ms_sum, long long* counts, int n_kinds, int reset) {
    if (!ctx) return fail(PDS_ERR_INVALID, "null ctx");
    PDS_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    for (auto& e : ctx->ev_pending) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, e.a, e.b) == hipSuccess && e.kind >= 0 && e.kind < pds::kNumKinds) {
            ctx->kind_ms[e.kind] += ms;
            ctx->kind_count[e.kind] += 1;
            auto& sm = ctx->kind_samples[e.kind];
            if (sm.size() >= 4096) sm.erase(sm.begin(), sm.begin() + 2048);
            sm.push_back(ms);
        }
        ctx->ev_pool.push_back(e.a);
        ctx->ev_pool.push_back(e.b);
    }
    ctx->ev_pending.clear();
    for (int k = 0; k < n_kinds && k < pds::kNumKinds; ++k) {
        if (ms_sum) ms_sum[k] = ctx->kind_ms[k];
        if (counts) counts[k] = ctx->kind_count[k];
    }
    if (reset)
        for (int k = 0; k < pds::kNumKinds; ++k) {
            ctx->kind_ms[k] = 0;
            ctx->kind_count[k] = 0;
        }
    return PDS_OK;
}

int pds_ctx_get_timing_samples(pds_ctx* ctx, int kind, double* ms_out, int cap, int reset) {
    if (!ctx || kind < 0 || kind >= pds::kNumKinds) return -1;
    if (pds_ctx_get_timing(ctx, nullptr, nullptr, 0, 0) != PDS_OK) return -1;  // drains the pending event pairs
    auto& sm = ctx->kind_samples[kind];
    const int n = (int)std::min<size_t>(sm.size(), (size_t)std::max(cap, 0));
    for (int i = 0; i < n; ++i) ms_out[i] = sm[sm.size() - n + i];
    if (reset) sm.clear();
    return n;
}

int pds_lr_f64(pds_ctx* ctx, const double* const* cols, const double* weights, int n_feat, int64_t n_rows,
               pds_space space, const pds_lr_params* prm, double* coeffs, int* is_null) {
    return lr_impl<double>(ctx, cols, weights, n_feat, n_rows, space, prm, coeffs, is_null, nullptr, nullptr);
}
int pds_lr_f32(pds_ctx* ctx, const float* const* cols, const float* weights, int n_feat, int64_t n_rows,
               pds_space space, const pds_lr_params* prm, float* coeffs, int* is_null) {
    return lr_impl<float>(ctx, cols, weights, n_feat, n_rows, space, prm, coeffs, is_null, nullptr, nullptr);
}
int pds_lr_pred_f64(pds_ctx* ctx, const double* const* cols, const double* weights, int n_feat, int64_t n_rows,
                    pds_space space, const pds_lr_params* prm, double* coeffs, int* is_null, double* pred,
                    double* resid) {
    if (!pred || !resid) return fail(PDS_ERR_INVALID, "pred / resid buffers required");
    return lr_impl<double>(ctx, cols, weights, n_feat, n_rows, space, prm, coeffs, is_null, pred, resid);
}
int pds_lr_pred_f32(pds_ctx* ctx, const float* const* cols, const float* weights, int n_feat, int64_t n_rows,
                    pds_space space, const pds_lr_params* prm, float* coeffs, int* is_null, float* pred, float* resid) {
    if (!pred || !resid) return fail(PDS_ERR_INVALID, "pred / resid buffers required");
    return lr_impl<float>(ctx, cols, weights, n_feat, n_rows, space, prm, coeffs, is_null, pred, resid);
}

int pds_elastic_net_f64(pds_ctx* ctx, const double* const* cols, int n_feat, int64_t n_rows, pds_space space,
                        const pds_lr_params* prm, double* coeffs) {
    return lr_impl<double>(ctx, cols, nullptr, n_feat, n_rows, space, prm, coeffs, nullptr, nullptr, nullptr, true);
}
int pds_elastic_net_f32(pds_ctx* ctx, const float* const* cols, int n_feat, int64_t n_rows, pds_space space,
                        const pds_lr_params* prm, float* coeffs) {
    return lr_impl<float>(ctx, cols, nullptr, n_feat, n_rows, space, prm, coeffs, nullptr, nullptr, nullptr, true);
}

int pds_lr_nullable_f64(pds_ctx* ctx, const double* const* cols, const uint8_t* const* validity, const int64_t* bit_offsets,
                        int n_feat, int64_t n_rows, pds_space space, int null_policy, double fill_value,
                        const pds_lr_params* prm, double* coeffs, int* is_null, double* pred, double* resid,
                        uint8_t* row_valid, int64_t* n_used) {
    return lr_nullable_impl<double>(ctx, cols, validity, bit_offsets, n_feat, n_rows, space, null_policy, fill_value, prm,
                                    coeffs, is_null, pred, resid, row_valid, n_used);
}
int pds_lr_nullable_f32(pds_ctx* ctx, const float* const* cols, const uint8_t* const* validity, const int64_t* bit_offsets,
                        int n_feat, int64_t n_rows, pds_space space, int null_policy, float fill_value,
                        const pds_lr_params* prm, float* coeffs, int* is_null, float* pred, float* resid,
                        uint8_t* row_valid, int64_t* n_used) {
    return lr_nullable_impl<float>(ctx, cols, validity, bit_offsets, n_feat, n_rows, space, null_policy, fill_value, prm,
                                   coeffs, is_null, pred, resid, row_valid, n_used);
}

int pds_lr_multi_f64(pds_ctx* ctx, const double* const* cols, int n_targets, int n_feat, int64_t n_rows, pds_space space,
                     int add_bias, double l2_reg, int solver, double singular_x_tol, double* coeffs, int* is_null,
                     double* pred, double* resid) {
    return lr_multi_impl<double>(ctx, cols, n_targets, n_feat, n_rows, space, add_bias, l2_reg, solver, singular_x_tol,
                                 coeffs, is_null, pred, resid);
}
int pds_lr_multi_f32(pds_ctx* ctx, const float* const* cols, int n_targets, int n_feat, int64_t n_rows, pds_space space,
                     int add_bias, float l2_reg, int solver, float singular_x_tol, float* coeffs, int* is_null, float* pred,
                     float* resid) {
    return lr_multi_impl<float>(ctx, cols, n_targets, n_feat, n_rows, space, add_bias, l2_reg, solver, singular_x_tol, coeffs,
                                is_null, pred, resid);
}

int pds_lr_rcond_f64(pds_ctx* ctx, const double* const* cols, int n_feat, int64_t n_rows, pds_space space,
                     int add_bias, double l2_reg, double rcond, double* coeffs, double* singular_values) {
    return pds::lr_rcond_impl<double>(ctx, cols, n_feat, n_rows, space, add_bias, l2_reg, rcond, coeffs, singular_values);
}
int pds_lr_rcond_f32(pds_ctx* ctx, const float* const* cols, int n_feat, int64_t n_rows, pds_space space,
                     int add_bias, float l2_reg, float rcond, float* coeffs, float* singular_values) {
    return pds::lr_rcond_impl<float>(ctx, cols, n_feat, n_rows, space, add_bias, (double)l2_reg, (double)rcond, coeffs,
                                     singular_values);
}

int pds_lr_rcond_grouped_f64(pds_ctx* ctx, const double* const* cols, int n_feat, int64_t n_rows, const int64_t* group_offsets,
                             int64_t n_groups, pds_space space, int add_bias, double l2_reg, double rcond, double* coeffs,
                             double* singular_values, uint8_t* is_null) {
    return pds::rcond_grouped_impl<double>(ctx, cols, n_feat, n_rows, group_offsets, n_groups, space, add_bias, l2_reg, rcond, coeffs,
                                           singular_values, is_null);
}
int pds_lr_rcond_grouped_f32(pds_ctx* ctx, const float* const* cols, int n_feat, int64_t n_rows, const int64_t* group_offsets,
                             int64_t n_groups, pds_space space, int add_bias, float l2_reg, float rcond, float* coeffs,
                             float* singular_values, uint8_t* is_null) {
    return pds::rcond_grouped_impl<float>(ctx, cols, n_feat, n_rows, group_offsets, n_groups, space, add_bias, l2_reg, rcond, coeffs,
                                          singular_values, is_null);
}
int pds_lr_rcond_by_key_f64(pds_ctx* ctx, const double* const* cols, const int64_t* keys, int n_feat, int64_t n_rows, pds_space space,
                            int add_bias, double l2_reg, double rcond, int64_t max_groups, int64_t* out_keys, double* coeffs,
                            double* singular_values, uint8_t* is_null, int64_t* n_groups) {
    return pds::rcond_by_key_impl<double>(ctx, cols, keys, n_feat, n_rows, space, add_bias, l2_reg, rcond, max_groups, out_keys, coeffs,
                                          singular_values, is_null, n_groups);
}
int pds_lr_rcond_by_key_f32(pds_ctx* ctx, const float* const* cols, const int64_t* keys, int n_feat, int64_t n_rows, pds_space space,
                            int add_bias, float l2_reg, float rcond, int64_t max_groups, int64_t* out_keys, float* coeffs,
                            float* singular_values, uint8_t* is_null, int64_t* n_groups) {
    return pds::rcond_by_key_impl<float>(ctx, cols, keys, n_feat, n_rows, space, add_bias, l2_reg, rcond, max_groups, out_keys, coeffs,
                                         singular_values, is_null, n_groups);
}

int pds_lr_multi_grouped_f64(pds_ctx* ctx, const double* const* cols, int n_targets, int n_feat, int64_t n_rows, const int64_t* group_offsets,
                             int64_t n_groups, pds_space space, int add_bias, double l2_reg, int solver, double singular_x_tol, double* coeffs,
                             uint8_t* is_null, double* pred, double* resid, uint8_t* row_null) {
    return pds::multi_grouped_impl<double>(ctx, cols, n_targets, n_feat, n_rows, group_offsets, n_groups, space, add_bias, l2_reg, solver,
                                           singular_x_tol, coeffs, is_null, pred, resid, row_null);
}
int pds_lr_multi_grouped_f32(pds_ctx* ctx, const float* const* cols, int n_targets, int n_feat, int64_t n_rows, const int64_t* group_offsets,
                             int64_t n_groups, pds_space space, int add_bias, float l2_reg, int solver, float singular_x_tol, float* coeffs,
                             uint8_t* is_null, float* pred, float* resid, uint8_t* row_null) {
    return pds::multi_grouped_impl<float>(ctx, cols, n_targets, n_feat, n_rows, group_offsets, n_groups, space, add_bias, l2_reg, solver,
                                          singular_x_tol, coeffs, is_null, pred, resid, row_null);
}
int pds_lr_multi_by_key_f64(pds_ctx* ctx, const double* const* cols, const int64_t* keys, int n_targets, int n_feat, int64_t n_rows, pds_space space,
                            int add_bias, double l2_reg, int solver, double singular_x_tol, int64_t max_groups, int64_t* out_keys, double* coeffs,
                            uint8_t* is_null, int64_t* n_groups, double* pred, double* resid, uint8_t* row_null) {
    return pds::multi_by_key_impl<double>(ctx, cols, keys, n_targets, n_feat, n_rows, space, add_bias, l2_reg, solver, singular_x_tol, max_groups,
                                          out_keys, coeffs, is_null, n_groups, pred, resid, row_null);
}
int pds_lr_multi_by_key_f32(pds_ctx* ctx, const float* const* cols, const int64_t* keys, int n_targets, int n_feat, int64_t n_rows, pds_space space,
                            int add_bias, float l2_reg, int solver, float singular_x_tol, int64_t max_groups, int64_t* out_keys, float* coeffs,
                            uint8_t* is_null, int64_t* n_groups, float* pred, float* resid, uint8_t* row_null) {
    return pds::multi_by_key_impl<float>(ctx, cols, keys, n_targets, n_feat, n_rows, space, add_bias, l2_reg, solver, singular_x_tol, max_groups,
                                         out_keys, coeffs, is_null, n_groups, pred, resid, row_null);
}

int pds_lin_reg_report_f64(pds_ctx* ctx, const double* const* cols, const double* weights, int n_feat,
                           int64_t n_rows, pds_space space, int add_bias, int se_type, double y_var,
                           pds_report_f64* out) {
    return report_impl<double, pds_report_f64>(ctx, cols, weights, n_feat, n_rows, space, add_bias, se_type, y_var, out);
}
int pds_lin_reg_report_f32(pds_ctx* ctx, const float* const* cols, const float* weights, int n_feat, int64_t n_rows,
                           pds_space space, int add_bias, int se_type, float y_var, pds_report_f32* out) {
    return report_impl<float, pds_report_f32>(ctx, cols, weights, n_feat, n_rows, space, add_bias, se_type, y_var, out);
}

int pds_lin_reg_report_cluster_grouped_f64(pds_ctx* ctx, const double* const* cols, int n_feat, int64_t n_rows, const int64_t* cluster_offsets,
                                           int64_t n_clusters, pds_space space, int add_bias, int se_type, double y_var, pds_report_f64* out) {
    return report_cluster_impl<double, pds_report_f64>(ctx, cols, n_feat, n_rows, cluster_offsets, n_clusters, space, add_bias, se_type, y_var, out);
}
int pds_lin_reg_report_cluster_grouped_f32(pds_ctx* ctx, const float* const* cols, int n_feat, int64_t n_rows, const int64_t* cluster_offsets,
                                           int64_t n_clusters, pds_space space, int add_bias, int se_type, float y_var, pds_report_f32* out) {
    return report_cluster_impl<float, pds_report_f32>(ctx, cols, n_feat, n_rows, cluster_offsets, n_clusters, space, add_bias, se_type, y_var, out);
}
int pds_lin_reg_report_cluster_by_key_f64(pds_ctx* ctx, const double* const* cols, const int64_t* keys, int n_feat, int64_t n_rows,
                                          pds_space space, int add_bias, int se_type, double y_var, pds_report_f64* out, int64_t* n_clusters) {
    return report_cluster_by_key_impl<double, pds_report_f64>(ctx, cols, keys, n_feat, n_rows, space, add_bias, se_type, y_var, out, n_clusters);
}
int pds_lin_reg_report_cluster_by_key_f32(pds_ctx* ctx, const float* const* cols, const int64_t* keys, int n_feat, int64_t n_rows,
                                          pds_space space, int add_bias, int se_type, float y_var, pds_report_f32* out, int64_t* n_clusters) {
    return report_cluster_by_key_impl<float, pds_report_f32>(ctx, cols, keys, n_feat, n_rows, space, add_bias, se_type, y_var, out, n_clusters);
}
int pds_lin_reg_within_grouped_f64(pds_ctx* ctx, const double* const* cols, int n_feat, int64_t n_rows, const int64_t* group_offsets,
                                   int64_t n_groups, pds_space space, int se_type, pds_report_f64* out, pds_within_out* extra) {
    return within_impl<double, pds_report_f64>(ctx, cols, n_feat, n_rows, group_offsets, n_groups, space, space, se_type, out, extra);
}
int pds_lin_reg_within_grouped_f32(pds_ctx* ctx, const float* const* cols, int n_feat, int64_t n_rows, const int64_t* group_offsets,
                                   int64_t n_groups, pds_space space, int se_type, pds_report_f32* out, pds_within_out* extra) {
    return within_impl<float, pds_report_f32>(ctx, cols, n_feat, n_rows, group_offsets, n_groups, space, space, se_type, out, extra);
}
int pds_lin_reg_within_by_key_f64(pds_ctx* ctx, const double* const* cols, const int64_t* keys, int n_feat, int64_t n_rows, pds_space space,
                                  int se_type, int64_t max_groups, int64_t* out_keys, pds_report_f64* out, pds_within_out* extra,
                                  int64_t* n_groups) {
    return within_by_key_impl<double, pds_report_f64>(ctx, cols, keys, n_feat, n_rows, space, se_type, max_groups, out_keys, out, extra, n_groups);
}
int pds_lin_reg_within_by_key_f32(pds_ctx* ctx, const float* const* cols, const int64_t* keys, int n_feat, int64_t n_rows, pds_space space,
                                  int se_type, int64_t max_groups, int64_t* out_keys, pds_report_f32* out, pds_within_out* extra,
                                  int64_t* n_groups) {
    return within_by_key_impl<float, pds_report_f32>(ctx, cols, keys, n_feat, n_rows, space, se_type, max_groups, out_keys, out, extra, n_groups);
}
int pds_lin_reg_within2_grouped_f64(pds_ctx* ctx, const double* const* cols, int n_feat, int64_t n_rows, const int64_t* group_offsets,
                                    int64_t n_groups, const int32_t* codes2, int64_t n_levels2, pds_space space, int se_type,
                                    double absorb_tol, int absorb_max_iter, pds_report_f64* out, pds_within2_out* extra) {
    return within2_impl<double, pds_report_f64>(ctx, cols, n_feat, n_rows, group_offsets, n_groups, space, codes2, space, n_levels2, space, se_type,
                                                absorb_tol, absorb_max_iter, out, extra);
}
int pds_lin_reg_within2_grouped_f32(pds_ctx* ctx, const float* const* cols, int n_feat, int64_t n_rows, const int64_t* group_offsets,
                                    int64_t n_groups, const int32_t* codes2, int64_t n_levels2, pds_space space, int se_type,
                                    double absorb_tol, int absorb_max_iter, pds_report_f32* out, pds_within2_out* extra) {
    return within2_impl<float, pds_report_f32>(ctx, cols, n_feat, n_rows, group_offsets, n_groups, space, codes2, space, n_levels2, space, se_type,
                                               absorb_tol, absorb_max_iter, out, extra);
}
int pds_lin_reg_within2_by_key_f64(pds_ctx* ctx, const double* const* cols, const int64_t* keys, const int32_t* codes2, int64_t n_levels2,
                                   int n_feat, int64_t n_rows, pds_space space, int se_type, double absorb_tol, int absorb_max_iter,
                                   pds_report_f64* out, pds_within2_out* extra, int64_t* n_groups) {
    return within2_by_key_impl<double, pds_report_f64>(ctx, cols, keys, codes2, n_levels2, n_feat, n_rows, space, se_type, absorb_tol,
                                                       absorb_max_iter, out, extra, n_groups);
}
int pds_lin_reg_within2_by_key_f32(pds_ctx* ctx, const float* const* cols, const int64_t* keys, const int32_t* codes2, int64_t n_levels2,
                                   int n_feat, int64_t n_rows, pds_space space, int se_type, double absorb_tol, int absorb_max_iter,
                                   pds_report_f32* out, pds_within2_out* extra, int64_t* n_groups) {
    return within2_by_key_impl<float, pds_report_f32>(ctx, cols, keys, codes2, n_levels2, n_feat, n_rows, space, se_type, absorb_tol,
                                                      absorb_max_iter, out, extra, n_groups);
}
int pds_lin_reg_within2_fx_grouped_f64(pds_ctx* ctx, const double* const* cols, int n_feat, int64_t n_rows, const int64_t* group_offsets,
                                       int64_t n_groups, const int32_t* codes2, int64_t n_levels2, pds_space space, int se_type,
                                       double absorb_tol, int absorb_max_iter, pds_report_f64* out, pds_within2_out* extra,
                                       pds_within2_effects* fx) {
    return within2_impl<double, pds_report_f64>(ctx, cols, n_feat, n_rows, group_offsets, n_groups, space, codes2, space, n_levels2, space, se_type,
                                                absorb_tol, absorb_max_iter, out, extra, nullptr, fx);
}
int pds_lin_reg_within2_fx_grouped_f32(pds_ctx* ctx, const float* const* cols, int n_feat, int64_t n_rows, const int64_t* group_offsets,
                                       int64_t n_groups, const int32_t* codes2, int64_t n_levels2, pds_space space, int se_type,
                                       double absorb_tol, int absorb_max_iter, pds_report_f32* out, pds_within2_out* extra,
                                       pds_within2_effects* fx) {
    return within2_impl<float, pds_report_f32>(ctx, cols, n_feat, n_rows, group_offsets, n_groups, space, codes2, space, n_levels2, space, se_type,
                                               absorb_tol, absorb_max_iter, out, extra, nullptr, fx);
}
int pds_lin_reg_within2_fx_by_key_f64(pds_ctx* ctx, const double* const* cols, const int64_t* keys, const int32_t* codes2, int64_t n_levels2,
                                      int n_feat, int64_t n_rows, pds_space space, int se_type, double absorb_tol, int absorb_max_iter,
                                      pds_report_f64* out, pds_within2_out* extra, int64_t* n_groups, pds_within2_effects* fx) {
    return within2_by_key_impl<double, pds_report_f64>(ctx, cols, keys, codes2, n_levels2, n_feat, n_rows, space, se_type, absorb_tol,
                                                       absorb_max_iter, out, extra, n_groups, fx);
}
int pds_lin_reg_within2_fx_by_key_f32(pds_ctx* ctx, const float* const* cols, const int64_t* keys, const int32_t* codes2, int64_t n_levels2,
                                      int n_feat, int64_t n_rows, pds_space space, int se_type, double absorb_tol, int absorb_max_iter,
                                      pds_report_f32* out, pds_within2_out* extra, int64_t* n_groups, pds_within2_effects* fx) {
    return within2_by_key_impl<float, pds_report_f32>(ctx, cols, keys, codes2, n_levels2, n_feat, n_rows, space, se_type, absorb_tol,
                                                      absorb_max_iter, out, extra, n_groups, fx);
}
int pds_lin_reg_within_cl_grouped_f64(pds_ctx* ctx, const double* const* cols, int n_feat, int64_t n_rows, const int64_t* group_offsets,
                                      int64_t n_groups, pds_space space, int se_type, pds_report_f64* out, pds_within_out* extra, pds_cluster_key* cl) {
    return with_cluster_key(cl, space, [&](WithinCluster* wc) {
        return within_impl<double, pds_report_f64>(ctx, cols, n_feat, n_rows, group_offsets, n_groups, space, space, se_type, out, extra, nullptr, nullptr, wc);
    });
}
int pds_lin_reg_within_cl_by_key_f64(pds_ctx* ctx, const double* const* cols, const int64_t* keys, int n_feat, int64_t n_rows, pds_space space,
                                     int se_type, int64_t max_groups, int64_t* out_keys, pds_report_f64* out, pds_within_out* extra, int64_t* n_groups,
                                     pds_cluster_key* cl) {
    return with_cluster_key(cl, space, [&](WithinCluster* wc) {
        return within_by_key_impl<double, pds_report_f64>(ctx, cols, keys, n_feat, n_rows, space, se_type, max_groups, out_keys, out, extra, n_groups, wc);
    });
}
int pds_lin_reg_within2_cl_grouped_f64(pds_ctx* ctx, const double* const* cols, int n_feat, int64_t n_rows, const int64_t* group_offsets,
                                       int64_t n_groups, const int32_t* codes2, int64_t n_levels2, pds_space space, int se_type,
                                       double absorb_tol, int absorb_max_iter, pds_report_f64* out, pds_within2_out* extra, pds_within2_effects* fx,
                                       pds_cluster_key* cl) {
    return with_cluster_key(cl, space, [&](WithinCluster* wc) {
        return within2_impl<double, pds_report_f64>(ctx, cols, n_feat, n_rows, group_offsets, n_groups, space, codes2, space, n_levels2, space, se_type, absorb_tol,
                                        absorb_max_iter, out, extra, nullptr, fx, wc);
    });
}
int pds_lin_reg_within2_cl_by_key_f64(pds_ctx* ctx, const double* const* cols, const int64_t* keys, const int32_t* codes2, int64_t n_levels2,
                                      int n_feat, int64_t n_rows, pds_space space, int se_type, double absorb_tol, int absorb_max_iter,
                                      pds_report_f64* out, pds_within2_out* extra, int64_t* n_groups, pds_within2_effects* fx, pds_cluster_key* cl) {
    return with_cluster_key(cl, space, [&](WithinCluster* wc) {
        return within2_by_key_impl<double, pds_report_f64>(ctx, cols, keys, codes2, n_levels2, n_feat, n_rows, space, se_type, absorb_tol, absorb_max_iter, out,
                                               extra, n_groups, fx, wc);
    });
}
int pds_lin_reg_within_cl_grouped_f32(pds_ctx* ctx, const float* const* cols, int n_feat, int64_t n_rows, const int64_t* group_offsets,
                                      int64_t n_groups, pds_space space, int se_type, pds_report_f32* out, pds_within_out* extra, pds_cluster_key* cl) {
    return with_cluster_key(cl, space, [&](WithinCluster* wc) {
        return within_impl<float, pds_report_f32>(ctx, cols, n_feat, n_rows, group_offsets, n_groups, space, space, se_type, out, extra, nullptr, nullptr, wc);
    });
}
int pds_lin_reg_within_cl_by_key_f32(pds_ctx* ctx, const float* const* cols, const int64_t* keys, int n_feat, int64_t n_rows, pds_space space,
                                     int se_type, int64_t max_groups, int64_t* out_keys, pds_report_f32* out, pds_within_out* extra, int64_t* n_groups,
                                     pds_cluster_key* cl) {
    return with_cluster_key(cl, space, [&](WithinCluster* wc) {
        return within_by_key_impl<float, pds_report_f32>(ctx, cols, keys, n_feat, n_rows, space, se_type, max_groups, out_keys, out, extra, n_groups, wc);
    });
}
int pds_lin_reg_within2_cl_grouped_f32(pds_ctx* ctx, const float* const* cols, int n_feat, int64_t n_rows, const int64_t* group_offsets,
                                       int64_t n_groups, const int32_t* codes2, int64_t n_levels2, pds_space space, int se_type,
                                       double absorb_tol, int absorb_max_iter, pds_report_f32* out, pds_within2_out* extra, pds_within2_effects* fx,
                                       pds_cluster_key* cl) {
    return with_cluster_key(cl, space, [&](WithinCluster* wc) {
        return within2_impl<float, pds_report_f32>(ctx, cols, n_feat, n_rows, group_offsets, n_groups, space, codes2, space, n_levels2, space, se_type, absorb_tol,
                                        absorb_max_iter, out, extra, nullptr, fx, wc);
    });
}
int pds_lin_reg_within2_cl_by_key_f32(pds_ctx* ctx, const float* const* cols, const int64_t* keys, const int32_t* codes2, int64_t n_levels2,
                                      int n_feat, int64_t n_rows, pds_space space, int se_type, double absorb_tol, int absorb_max_iter,
                                      pds_report_f32* out, pds_within2_out* extra, int64_t* n_groups, pds_within2_effects* fx, pds_cluster_key* cl) {
    return with_cluster_key(cl, space, [&](WithinCluster* wc) {
        return within2_by_key_impl<float, pds_report_f32>(ctx, cols, keys, codes2, n_levels2, n_feat, n_rows, space, se_type, absorb_tol, absorb_max_iter, out,
                                               extra, n_groups, fx, wc);
    });
}
int pds_absorb_components_i32(pds_ctx* ctx, const int32_t* codes1, int64_t n_levels1, const int32_t* codes2, int64_t n_levels2, int64_t n_rows,
                              pds_space space, int32_t* component1, int32_t* component2, int64_t* n1, int64_t* n2, int64_t* n_components,
                              int* n_rounds) {
    return absorb_components_impl(ctx, codes1, n_levels1, codes2, n_levels2, n_rows, space, component1, component2, n1, n2, n_components, n_rounds);
}

int pds_report_fit_from_moments_f64(pds_ctx* ctx, const double* moments, int n_feat, int add_bias, double* beta, double* inv) {
    return report_fit_impl<double>(ctx, moments, n_feat, add_bias, beta, inv);
}
int pds_report_fit_from_moments_f32(pds_ctx* ctx, const float* moments, int n_feat, int add_bias, float* beta, float* inv) {
    return report_fit_impl<float>(ctx, moments, n_feat, add_bias, beta, inv);
}
int pds_report_partials_f64(pds_ctx* ctx, const double* const* cols, const double* weights, int n_feat, int64_t n_rows,
                            pds_space space, int add_bias, int se_type, const double* beta, const double* inv, double* partials) {
    return report_partials_impl<double>(ctx, cols, weights, n_feat, n_rows, space, add_bias, se_type, beta, inv, partials);
}
int pds_report_partials_f32(pds_ctx* ctx, const float* const* cols, const float* weights, int n_feat, int64_t n_rows,
                            pds_space space, int add_bias, int se_type, const float* beta, const float* inv, double* partials) {
    return report_partials_impl<float>(ctx, cols, weights, n_feat, n_rows, space, add_bias, se_type, beta, inv, partials);
}
int pds_report_finish_f64(int n_feat, int add_bias, int se_type, int weighted, int64_t n_rows_total, double y_var,
                          const double* beta, const double* inv, const double* partials, pds_report_f64* out) {
    return report_finish_impl<double, pds_report_f64>(n_feat, add_bias, se_type, weighted, n_rows_total, y_var, beta, inv, partials, out);
}
int pds_report_finish_f32(int n_feat, int add_bias, int se_type, int weighted, int64_t n_rows_total, float y_var,
                          const float* beta, const float* inv, const double* partials, pds_report_f32* out) {
    return report_finish_impl<float, pds_report_f32>(n_feat, add_bias, se_type, weighted, n_rows_total, y_var, beta, inv, partials, out);
}

int pds_lin_reg_report_nullable_f64(pds_ctx* ctx, const double* const* cols, const uint8_t* const* validity,
                                    const int64_t* bit_offsets, int n_feat, int64_t n_rows, pds_space space, int null_policy,
                                    double fill_value, int add_bias, int se_type, double y_var, pds_report_f64* out,
                                    int64_t* n_used) {
    return report_impl<double, pds_report_f64>(ctx, cols, nullptr, n_feat, n_rows, space, add_bias, se_type, y_var, out, true,
                                               validity, bit_offsets, null_policy, fill_value, n_used);
}
int pds_lin_reg_report_nullable_f32(pds_ctx* ctx, const float* const* cols, const uint8_t* const* validity,
                                    const int64_t* bit_offsets, int n_feat, int64_t n_rows, pds_space space, int null_policy,
                                    float fill_value, int add_bias, int se_type, float y_var, pds_report_f32* out,
                                    int64_t* n_used) {
    return report_impl<float, pds_report_f32>(ctx, cols, nullptr, n_feat, n_rows, space, add_bias, se_type, y_var, out, true,
                                              validity, bit_offsets, null_policy, fill_value, n_used);
}

int pds_lr_grouped_f64(pds_ctx* ctx, const double* const* cols, int n_feat, int64_t n_rows,
                       const int64_t* group_offsets, int64_t n_groups, pds_space space, const pds_lr_params* prm,
                       double* coeffs, uint8_t* is_null) {
    const int rc = grouped_impl<double>(ctx, cols, n_feat, n_rows, group_offsets, n_groups, space, prm, coeffs, is_null, false, nullptr,
                                        nullptr, PDS_NULL_RAISE, 0.0, nullptr, nullptr, nullptr, /*may_stay_on_stream=*/true);
    if (rc && ctx) ctx->col_table_valid = false;  // (a failed call: nothing it queued is trusted to have run)
    return rc;
}
int pds_lr_grouped_f32(pds_ctx* ctx, const float* const* cols, int n_feat, int64_t n_rows,
                       const int64_t* group_offsets, int64_t n_groups, pds_space space, const pds_lr_params* prm,
                       float* coeffs, uint8_t* is_null) {
    const int rc = grouped_impl<float>(ctx, cols, n_feat, n_rows, group_offsets, n_groups, space, prm, coeffs, is_null, false, nullptr,
                                       nullptr, PDS_NULL_RAISE, 0.0f, nullptr, nullptr, nullptr, /*may_stay_on_stream=*/true);
    if (rc && ctx) ctx->col_table_valid = false;
    return rc;
}

int pds_lr_grouped_nullable_f64(pds_ctx* ctx, const double* const* cols, const uint8_t* const* validity,
                                const int64_t* bit_offsets, int n_feat, int64_t n_rows, const int64_t* group_offsets,
                                int64_t n_groups, pds_space space, int null_policy, double fill_value, const pds_lr_params* prm,
                                double* coeffs, uint8_t* is_null) {
    return grouped_impl<double>(ctx, cols, n_feat, n_rows, group_offsets, n_groups, space, prm, coeffs, is_null, true, validity,
                                bit_offsets, null_policy, fill_value);
}
int pds_lr_grouped_nullable_f32(pds_ctx* ctx, const float* const* cols, const uint8_t* const* validity,
                                const int64_t* bit_offsets, int n_feat, int64_t n_rows, const int64_t* group_offsets,
                                int64_t n_groups, pds_space space, int null_policy, float fill_value, const pds_lr_params* prm,
                                float* coeffs, uint8_t* is_null) {
    return grouped_impl<float>(ctx, cols, n_feat, n_rows, group_offsets, n_groups, space, prm, coeffs, is_null, true, validity,
                               bit_offsets, null_policy, fill_value);
}

int pds_lr_with_inv_f64(pds_ctx* ctx, const double* const* cols, int n_feat, int64_t n_rows, pds_space space, int add_bias,
                        double lambda, double* coeffs, double* inv) {
    return pds::lr_with_inv_impl<double>(ctx, cols, n_feat, n_rows, space, add_bias, lambda, coeffs, inv);
}
int pds_lr_with_inv_f32(pds_ctx* ctx, const float* const* cols, int n_feat, int64_t n_rows, pds_space space, int add_bias,
                        float lambda, float* coeffs, float* inv) {
    return pds::lr_with_inv_impl<float>(ctx, cols, n_feat, n_rows, space, add_bias, (double)lambda, coeffs, inv);
}

int pds_lr_grouped_weighted_f64(pds_ctx* ctx, const double* const* cols, const double* weights, int n_feat, int64_t n_rows,
                                const int64_t* group_offsets, int64_t n_groups, pds_space space, const pds_lr_params* prm,
                                double* coeffs, uint8_t* is_null) {
    return pds::grouped_weighted_impl<double>(ctx, cols, weights, n_feat, n_rows, group_offsets, n_groups, space, prm, coeffs, is_null);
}
int pds_lr_grouped_weighted_f32(pds_ctx* ctx, const float* const* cols, const float* weights, int n_feat, int64_t n_rows,
                                const int64_t* group_offsets, int64_t n_groups, pds_space space, const pds_lr_params* prm,
                                float* coeffs, uint8_t* is_null) {
    return pds::grouped_weighted_impl<float>(ctx, cols, weights, n_feat, n_rows, group_offsets, n_groups, space, prm, coeffs, is_null);
}

int pds_lr_by_key_multi_f64(pds_ctx* const* ctxs, int n_ctx, int n_slices, const double* const* cols, const int64_t* keys, int n_feat,
                            int64_t n_rows, const pds_lr_params* prm, int64_t max_groups, int64_t* out_keys, double* coeffs,
                            uint8_t* is_null, int64_t* n_groups) {
    return pds::lr_by_key_multi_impl<double>(ctxs, n_ctx, n_slices, cols, keys, n_feat, n_rows, prm, max_groups, out_keys, coeffs, is_null,
                                             n_groups);
}
int pds_lr_by_key_multi_f32(pds_ctx* const* ctxs, int n_ctx, int n_slices, const float* const* cols, const int64_t* keys, int n_feat,
                            int64_t n_rows, const pds_lr_params* prm, int64_t max_groups, int64_t* out_keys, float* coeffs,
                            uint8_t* is_null, int64_t* n_groups) {
    return pds::lr_by_key_multi_impl<float>(ctxs, n_ctx, n_slices, cols, keys, n_feat, n_rows, prm, max_groups, out_keys, coeffs, is_null,
                                            n_groups);
}
int pds_lr_by_key_pred_multi_f64(pds_ctx* const* ctxs, int n_ctx, int n_slices, const double* const* cols, const double* weights,
                                 const int64_t* keys, int n_feat, int64_t n_rows, const pds_lr_params* prm, double* pred, double* resid,
                                 uint8_t* row_null) {
    return pds::lr_by_key_pred_multi_impl<double>(ctxs, n_ctx, n_slices, cols, weights, keys, n_feat, n_rows, prm, pred, resid, row_null);
}
int pds_lr_by_key_pred_multi_f32(pds_ctx* const* ctxs, int n_ctx, int n_slices, const float* const* cols, const float* weights,
                                 const int64_t* keys, int n_feat, int64_t n_rows, const pds_lr_params* prm, float* pred, float* resid,
                                 uint8_t* row_null) {
    return pds::lr_by_key_pred_multi_impl<float>(ctxs, n_ctx, n_slices, cols, weights, keys, n_feat, n_rows, prm, pred, resid, row_null);
}
// pinned (page-locked, portable) host storage for results: a device-to-host copy into it runs at the link rate instead of the
// pageable rate (7.8 -> ~2.5 ms for the 136 MB of the headline frame's coefficients)
int pds_host_alloc(size_t bytes, void** out) {
    if (!out) return pds::fail(PDS_ERR_INVALID, "null argument");
    *out = nullptr;
    PDS_HIP_CHECK(hipHostMalloc(out, bytes ? bytes : 1, hipHostMallocPortable));
    return PDS_OK;
}
int pds_host_free(void* p) {
    if (p) PDS_HIP_CHECK(hipHostFree(p));
    return PDS_OK;
}
int pds_device_count(int* n) {
    if (!n) return pds::fail(PDS_ERR_INVALID, "null argument");
    *n = 0;
    PDS_HIP_CHECK(hipGetDeviceCount(n));
    return PDS_OK;
}
// result storage a peer PROCESS's kernels write into (the direct gather of the group-sharded step: include/pds_lstsq.h)
static_assert(sizeof(hipIpcMemHandle_t) == PDS_IPC_HANDLE_BYTES, "the handle travels as 64 opaque bytes");
int pds_device_alloc(int device, size_t bytes, int fine_grained, void** out) {
    if (!out) return pds::fail(PDS_ERR_INVALID, "null argument");
    *out = nullptr;
    PDS_HIP_CHECK(hipSetDevice(device));
    if (fine_grained) PDS_HIP_CHECK(hipExtMallocWithFlags(out, bytes ? bytes : 1, hipDeviceMallocFinegrained));
    else PDS_HIP_CHECK(hipMalloc(out, bytes ? bytes : 1));
    return PDS_OK;
}
// stream-ordered completion words of the direct gather (include/pds_lstsq.h)
namespace pds {
__global__ void signal_post_kernel(unsigned* word, unsigned value) {
    __hip_atomic_store(word, value, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
__global__ __launch_bounds__(64) void signal_wait_kernel(const unsigned* words, int n, unsigned value, long long budget_ticks, int* timed_out) {
    const int lane = threadIdx.x;
    const long long t0 = wall_clock64();
    bool ok = lane >= n;
    while (!__all(ok)) {
        if (!ok) ok = (int)(__hip_atomic_load(words + lane, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM) - value) >= 0;  // (wrap-safe >=)
        if (wall_clock64() - t0 > budget_ticks) {
            if (lane == 0) atomicAdd(timed_out, 1);
            break;
        }
        __builtin_amdgcn_s_sleep(8);
    }
}
}  // namespace pds
int pds_signal_post(pds_ctx* ctx, unsigned* word, unsigned value) {
    if (!ctx || !word) return pds::fail(PDS_ERR_INVALID, "null argument");
    PDS_HIP_CHECK(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(pds::signal_post_kernel, dim3(1), dim3(1), 0, ctx->stream, word, value);
    PDS_HIP_CHECK(hipGetLastError());
    return PDS_OK;
}
int pds_signal_wait(pds_ctx* ctx, const unsigned* words, int n_words, unsigned value, int timeout_ms) {
    if (!ctx || !words || n_words < 0 || n_words > 64) return pds::fail(PDS_ERR_INVALID, "pds_signal_wait: up to 64 words");
    if (n_words == 0) return PDS_OK;
    PDS_HIP_CHECK(hipSetDevice(ctx->device));
    if (!ctx->wait_timeouts) {
        PDS_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&ctx->wait_timeouts), 64));
        PDS_HIP_CHECK(hipMemsetAsync(ctx->wait_timeouts, 0, 64, ctx->stream));
    }
    int rate_khz = 100000;  // wall_clock64 ticks per ms
    (void)hipDeviceGetAttribute(&rate_khz, hipDeviceAttributeWallClockRate, ctx->device);
    const long long budget = (long long)(timeout_ms > 0 ? timeout_ms : 2000) * (long long)rate_khz;
    hipLaunchKernelGGL(pds::signal_wait_kernel, dim3(1), dim3(64), 0, ctx->stream, words, n_words, value, budget,
                       ctx->wait_timeouts);
    PDS_HIP_CHECK(hipGetLastError());
    return PDS_OK;
}
int pds_signal_wait_status(pds_ctx* ctx, int* timed_out) {
    if (!ctx || !timed_out) return pds::fail(PDS_ERR_INVALID, "null argument");
    *timed_out = 0;
    if (!ctx->wait_timeouts) return PDS_OK;
    PDS_HIP_CHECK(hipSetDevice(ctx->device));
    PDS_HIP_CHECK(hipMemcpyAsync(timed_out, ctx->wait_timeouts, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    PDS_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return PDS_OK;
}
int pds_device_free(int device, void* p) {
    if (!p) return PDS_OK;
    PDS_HIP_CHECK(hipSetDevice(device));
    PDS_HIP_CHECK(hipFree(p));
    return PDS_OK;
}
int pds_ipc_export(int device, void* p, unsigned char* handle) {
    if (!p || !handle) return pds::fail(PDS_ERR_INVALID, "null argument");
    PDS_HIP_CHECK(hipSetDevice(device));
    hipIpcMemHandle_t h;
    PDS_HIP_CHECK(hipIpcGetMemHandle(&h, p));
    std::memcpy(handle, &h, sizeof(h));
    return PDS_OK;
}
int pds_ipc_open(int device, const unsigned char* handle, void** mapped) {
    if (!handle || !mapped) return pds::fail(PDS_ERR_INVALID, "null argument");
    *mapped = nullptr;
    PDS_HIP_CHECK(hipSetDevice(device));
    hipIpcMemHandle_t h;
    std::memcpy(&h, handle, sizeof(h));
    PDS_HIP_CHECK(hipIpcOpenMemHandle(mapped, h, hipIpcMemLazyEnablePeerAccess));
    return PDS_OK;
}
int pds_ipc_close(int device, void* mapped) {
    if (!mapped) return PDS_OK;
    PDS_HIP_CHECK(hipSetDevice(device));
    PDS_HIP_CHECK(hipIpcCloseMemHandle(mapped));
    return PDS_OK;
}

int pds_lr_grouped_pred_f64(pds_ctx* ctx, const double* const* cols, const double* weights, int n_feat, int64_t n_rows,
                            const int64_t* group_offsets, int64_t n_groups, pds_space space, const pds_lr_params* prm, double* coeffs,
                            uint8_t* is_null, double* pred, double* resid, uint8_t* row_null) {
    if (!pred && !resid && !row_null) return pds::fail(PDS_ERR_INVALID, "pds_lr_grouped_pred: no per-row output requested");
    if (weights)
        return pds::grouped_weighted_impl<double>(ctx, cols, weights, n_feat, n_rows, group_offsets, n_groups, space, prm, coeffs, is_null,
                                                  pred, resid, row_null, nullptr);
    return pds::grouped_impl<double>(ctx, cols, n_feat, n_rows, group_offsets, n_groups, space, prm, coeffs, is_null, false, nullptr,
                                     nullptr, PDS_NULL_RAISE, 0.0, pred, resid, row_null);
}
int pds_lr_grouped_pred_f32(pds_ctx* ctx, const float* const* cols, const float* weights, int n_feat, int64_t n_rows,
                            const int64_t* group_offsets, int64_t n_groups, pds_space space, const pds_lr_params* prm, float* coeffs,
                            uint8_t* is_null, float* pred, float* resid, uint8_t* row_null) {
    if (!pred && !resid && !row_null) return pds::fail(PDS_ERR_INVALID, "pds_lr_grouped_pred: no per-row output requested");
    if (weights)
        return pds::grouped_weighted_impl<float>(ctx, cols, weights, n_feat, n_rows, group_offsets, n_groups, space, prm, coeffs, is_null,
                                                 pred, resid, row_null, nullptr);
    return pds::grouped_impl<float>(ctx, cols, n_feat, n_rows, group_offsets, n_groups, space, prm, coeffs, is_null, false, nullptr,
                                    nullptr, PDS_NULL_RAISE, 0.0f, pred, resid, row_null);
}
int pds_lr_by_key_pred_f64(pds_ctx* ctx, const double* const* cols, const double* weights, const int64_t* keys, int n_feat,
                           int64_t n_rows, pds_space space, const pds_lr_params* prm, int64_t max_groups, int64_t* out_keys,
                           double* coeffs, uint8_t* is_null, int64_t* n_groups, double* pred, double* resid, uint8_t* row_null) {
    return pds::lr_by_key_impl<double>(ctx, cols, keys, n_feat, n_rows, space, prm, max_groups, out_keys, coeffs, is_null, n_groups, weights,
                                       pred, resid, row_null);
}
int pds_lr_by_key_pred_f32(pds_ctx* ctx, const float* const* cols, const float* weights, const int64_t* keys, int n_feat, int64_t n_rows,
                           pds_space space, const pds_lr_params* prm, int64_t max_groups, int64_t* out_keys, float* coeffs,
                           uint8_t* is_null, int64_t* n_groups, float* pred, float* resid, uint8_t* row_null) {
    return pds::lr_by_key_impl<float>(ctx, cols, keys, n_feat, n_rows, space, prm, max_groups, out_keys, coeffs, is_null, n_groups, weights,
                                      pred, resid, row_null);
}

int pds_lin_reg_report_grouped_f64(pds_ctx* ctx, const double* const* cols, int n_feat, int64_t n_rows, const int64_t* group_offsets,
                                   int64_t n_groups, pds_space space, int add_bias, int se_type, const double* y_var,
                                   pds_report_grouped_f64* out) {
    return pds::report_grouped_impl<double>(ctx, cols, (const double*)nullptr, n_feat, n_rows, group_offsets, n_groups, space, add_bias, se_type, y_var,
                                            reinterpret_cast<const pds::ReportGroupedOut<double>*>(out));
}
int pds_lin_reg_report_grouped_f32(pds_ctx* ctx, const float* const* cols, int n_feat, int64_t n_rows, const int64_t* group_offsets,
                                   int64_t n_groups, pds_space space, int add_bias, int se_type, const float* y_var,
                                   pds_report_grouped_f32* out) {
    return pds::report_grouped_impl<float>(ctx, cols, (const float*)nullptr, n_feat, n_rows, group_offsets, n_groups, space, add_bias, se_type, y_var,
                                           reinterpret_cast<const pds::ReportGroupedOut<float>*>(out));
}
int pds_lin_reg_report_by_key_f64(pds_ctx* ctx, const double* const* cols, const int64_t* keys, int n_feat, int64_t n_rows,
                                  pds_space space, int add_bias, int se_type, int64_t max_groups, int64_t* out_keys,
                                  pds_report_grouped_f64* out, int64_t* n_groups) {
    return pds::report_by_key_impl<double>(ctx, cols, (const double*)nullptr, keys, n_feat, n_rows, space, add_bias, se_type, max_groups, out_keys,
                                           reinterpret_cast<const pds::ReportGroupedOut<double>*>(out), n_groups);
}
int pds_lin_reg_report_by_key_f32(pds_ctx* ctx, const float* const* cols, const int64_t* keys, int n_feat, int64_t n_rows,
                                  pds_space space, int add_bias, int se_type, int64_t max_groups, int64_t* out_keys,
                                  pds_report_grouped_f32* out, int64_t* n_groups) {
    return pds::report_by_key_impl<float>(ctx, cols, (const float*)nullptr, keys, n_feat, n_rows, space, add_bias, se_type, max_groups, out_keys,
                                          reinterpret_cast<const pds::ReportGroupedOut<float>*>(out), n_groups);
}
int pds_wls_report_grouped_f64(pds_ctx* ctx, const double* const* cols, const double* weights, int n_feat, int64_t n_rows,
                               const int64_t* group_offsets, int64_t n_groups, pds_space space, int add_bias, const double* y_var,
                               pds_report_grouped_f64* out) {
    if (!weights) return pds::fail(PDS_ERR_INVALID, "null argument");
    return pds::report_grouped_impl<double>(ctx, cols, weights, n_feat, n_rows, group_offsets, n_groups, space, add_bias, PDS_SE, y_var,
                                            reinterpret_cast<const pds::ReportGroupedOut<double>*>(out));
}
int pds_wls_report_by_key_f64(pds_ctx* ctx, const double* const* cols, const double* weights, const int64_t* keys, int n_feat,
                              int64_t n_rows, pds_space space, int add_bias, int64_t max_groups, int64_t* out_keys,
                              pds_report_grouped_f64* out, int64_t* n_groups) {
    if (!weights) return pds::fail(PDS_ERR_INVALID, "null argument");
    return pds::report_by_key_impl<double>(ctx, cols, weights, keys, n_feat, n_rows, space, add_bias, PDS_SE, max_groups, out_keys,
                                           reinterpret_cast<const pds::ReportGroupedOut<double>*>(out), n_groups);
}
int pds_wls_report_grouped_f32(pds_ctx* ctx, const float* const* cols, const float* weights, int n_feat, int64_t n_rows,
                               const int64_t* group_offsets, int64_t n_groups, pds_space space, int add_bias, const float* y_var,
                               pds_report_grouped_f32* out) {
    if (!weights) return pds::fail(PDS_ERR_INVALID, "null argument");
    return pds::report_grouped_impl<float>(ctx, cols, weights, n_feat, n_rows, group_offsets, n_groups, space, add_bias, PDS_SE, y_var,
                                            reinterpret_cast<const pds::ReportGroupedOut<float>*>(out));
}
int pds_wls_report_by_key_f32(pds_ctx* ctx, const float* const* cols, const float* weights, const int64_t* keys, int n_feat,
                              int64_t n_rows, pds_space space, int add_bias, int64_t max_groups, int64_t* out_keys,
                              pds_report_grouped_f32* out, int64_t* n_groups) {
    if (!weights) return pds::fail(PDS_ERR_INVALID, "null argument");
    return pds::report_by_key_impl<float>(ctx, cols, weights, keys, n_feat, n_rows, space, add_bias, PDS_SE, max_groups, out_keys,
                                           reinterpret_cast<const pds::ReportGroupedOut<float>*>(out), n_groups);
}
int pds_student_t_sf_device(pds_ctx* ctx, const double* x, const double* df, int64_t n, double* out) {
    return pds::student_t_sf_device_impl(ctx, x, df, n, out);
}
int pds_lr_by_key_f64(pds_ctx* ctx, const double* const* cols, const int64_t* keys, int n_feat, int64_t n_rows, pds_space space,
                      const pds_lr_params* prm, int64_t max_groups, int64_t* out_keys, double* coeffs, uint8_t* is_null,
                      int64_t* n_groups) {
    return pds::lr_by_key_impl<double>(ctx, cols, keys, n_feat, n_rows, space, prm, max_groups, out_keys, coeffs, is_null, n_groups);
}
int pds_lr_by_key_f32(pds_ctx* ctx, const float* const* cols, const int64_t* keys, int n_feat, int64_t n_rows, pds_space space,
                      const pds_lr_params* prm, int64_t max_groups, int64_t* out_keys, float* coeffs, uint8_t* is_null,
                      int64_t* n_groups) {
    return pds::lr_by_key_impl<float>(ctx, cols, keys, n_feat, n_rows, space, prm, max_groups, out_keys, coeffs, is_null, n_groups);
}

int pds_rolling_lr_f64(pds_ctx* ctx, const double* const* cols, int n_feat, int64_t n_rows, pds_space space,
                       int add_bias, int64_t window, int64_t min_size, double lambda, double* coeffs, double* pred,
                       uint8_t* valid) {
    return rolling_impl<double>(ctx, cols, n_feat, n_rows, space, add_bias, window, min_size, lambda, false, coeffs, pred, valid);
}
int pds_rolling_lr_f32(pds_ctx* ctx, const float* const* cols, int n_feat, int64_t n_rows, pds_space space,
                       int add_bias, int64_t window, int64_t min_size, float lambda, float* coeffs, float* pred,
                       uint8_t* valid) {
    return rolling_impl<float>(ctx, cols, n_feat, n_rows, space, add_bias, window, min_size, lambda, false, coeffs, pred, valid);
}
int pds_recursive_lr_f64(pds_ctx* ctx, const double* const* cols, int n_feat, int64_t n_rows, pds_space space,
                         int add_bias, int64_t start_with, double lambda, double* coeffs, double* pred,
                         uint8_t* valid) {
    return rolling_impl<double>(ctx, cols, n_feat, n_rows, space, add_bias, start_with, 0, lambda, true, coeffs, pred, valid);
}
int pds_recursive_lr_f32(pds_ctx* ctx, const float* const* cols, int n_feat, int64_t n_rows, pds_space space,
                         int add_bias, int64_t start_with, float lambda, float* coeffs, float* pred, uint8_t* valid) {
    return rolling_impl<float>(ctx, cols, n_feat, n_rows, space, add_bias, start_with, 0, lambda, true, coeffs, pred, valid);
}

int pds_rolling_lr_grouped_f64(pds_ctx* ctx, const double* const* cols, int n_feat, int64_t n_rows, const int64_t* group_offsets,
                               int64_t n_groups, pds_space space, int add_bias, int64_t window, int64_t min_size, double lambda,
                               double* coeffs, double* pred, uint8_t* valid) {
    return rolling_grouped_impl<double>(ctx, cols, n_feat, n_rows, group_offsets, n_groups, space, add_bias, window, min_size, lambda, false,
                                        coeffs, pred, valid);
}
int pds_rolling_lr_grouped_f32(pds_ctx* ctx, const float* const* cols, int n_feat, int64_t n_rows, const int64_t* group_offsets,
                               int64_t n_groups, pds_space space, int add_bias, int64_t window, int64_t min_size, float lambda,
                               float* coeffs, float* pred, uint8_t* valid) {
    return rolling_grouped_impl<float>(ctx, cols, n_feat, n_rows, group_offsets, n_groups, space, add_bias, window, min_size, lambda, false,
                                       coeffs, pred, valid);
}
int pds_recursive_lr_grouped_f64(pds_ctx* ctx, const double* const* cols, int n_feat, int64_t n_rows, const int64_t* group_offsets,
                                 int64_t n_groups, pds_space space, int add_bias, int64_t start_with, double lambda, double* coeffs,
                                 double* pred, uint8_t* valid) {
    return rolling_grouped_impl<double>(ctx, cols, n_feat, n_rows, group_offsets, n_groups, space, add_bias, start_with, 0, lambda, true,
                                        coeffs, pred, valid);
}
int pds_recursive_lr_grouped_f32(pds_ctx* ctx, const float* const* cols, int n_feat, int64_t n_rows, const int64_t* group_offsets,
                                 int64_t n_groups, pds_space space, int add_bias, int64_t start_with, float lambda, float* coeffs,
                                 float* pred, uint8_t* valid) {
    return rolling_grouped_impl<float>(ctx, cols, n_feat, n_rows, group_offsets, n_groups, space, add_bias, start_with, 0, lambda, true,
                                       coeffs, pred, valid);
}
int pds_rolling_lr_by_key_f64(pds_ctx* ctx, const double* const* cols, const int64_t* keys, int n_feat, int64_t n_rows, pds_space space,
                              int add_bias, int64_t window, int64_t min_size, double lambda, double* coeffs, double* pred, uint8_t* valid) {
    return rolling_by_key_impl<double>(ctx, cols, keys, n_feat, n_rows, space, add_bias, window, min_size, lambda, false, coeffs, pred, valid);
}
int pds_rolling_lr_by_key_f32(pds_ctx* ctx, const float* const* cols, const int64_t* keys, int n_feat, int64_t n_rows, pds_space space,
                              int add_bias, int64_t window, int64_t min_size, float lambda, float* coeffs, float* pred, uint8_t* valid) {
    return rolling_by_key_impl<float>(ctx, cols, keys, n_feat, n_rows, space, add_bias, window, min_size, lambda, false, coeffs, pred, valid);
}
int pds_recursive_lr_by_key_f64(pds_ctx* ctx, const double* const* cols, const int64_t* keys, int n_feat, int64_t n_rows, pds_space space,
                                int add_bias, int64_t start_with, double lambda, double* coeffs, double* pred, uint8_t* valid) {
    return rolling_by_key_impl<double>(ctx, cols, keys, n_feat, n_rows, space, add_bias, start_with, 0, lambda, true, coeffs, pred, valid);
}
int pds_recursive_lr_by_key_f32(pds_ctx* ctx, const float* const* cols, const int64_t* keys, int n_feat, int64_t n_rows, pds_space space,
                                int add_bias, int64_t start_with, float lambda, float* coeffs, float* pred, uint8_t* valid) {
    return rolling_by_key_impl<float>(ctx, cols, keys, n_feat, n_rows, space, add_bias, start_with, 0, lambda, true, coeffs, pred, valid);
}

int pds_recursive_lr_seeded_f64(pds_ctx* ctx, const double* const* cols, int n_feat, int64_t n_rows, pds_space space,
                                int add_bias, int64_t start_with, double lambda, const double* seed_moments,
                                double* coeffs, double* pred, uint8_t* valid) {
    return rolling_impl<double>(ctx, cols, n_feat, n_rows, space, add_bias, start_with, 0, lambda, true, coeffs, pred, valid,
                                seed_moments);
}
int pds_recursive_lr_seeded_f32(pds_ctx* ctx, const float* const* cols, int n_feat, int64_t n_rows, pds_space space,
                                int add_bias, int64_t start_with, float lambda, const float* seed_moments, float* coeffs,
                                float* pred, uint8_t* valid) {
    return rolling_impl<float>(ctx, cols, n_feat, n_rows, space, add_bias, start_with, 0, lambda, true, coeffs, pred, valid,
                               seed_moments);
}

int pds_moments_f64(pds_ctx* ctx, const double* const* cols, const double* weights, int n_feat, int64_t n_rows,
                    pds_space space, double* moments, pds_space out_space) {
    return moments_impl<double>(ctx, cols, weights, n_feat, n_rows, space, moments, out_space);
}
int pds_moments_f32(pds_ctx* ctx, const float* const* cols, const float* weights, int n_feat, int64_t n_rows,
                    pds_space space, float* moments, pds_space out_space) {
    return moments_impl<float>(ctx, cols, weights, n_feat, n_rows, space, moments, out_space);
}
int pds_lr_from_moments_f64(pds_ctx* ctx, const double* moments, pds_space mom_space, int n_feat,
                            const pds_lr_params* prm, double* coeffs, int* is_null) {
    return from_moments_impl<double>(ctx, moments, mom_space, n_feat, prm, coeffs, is_null);
}
int pds_lr_from_moments_f32(pds_ctx* ctx, const float* moments, pds_space mom_space, int n_feat,
                            const pds_lr_params* prm, float* coeffs, int* is_null) {
    return from_moments_impl<float>(ctx, moments, mom_space, n_feat, prm, coeffs, is_null);
}

// ---- exchange steps between the contexts of one process (capi_multi.hpp)
int pds_allreduce_sum_f64(pds_ctx* const* ctxs, int n_ctx, double* const* bufs, int64_t count, int prefix) {
    return pds::allreduce_sum_impl<double>(ctxs, n_ctx, bufs, count, prefix);
}
int pds_allreduce_sum_f32(pds_ctx* const* ctxs, int n_ctx, float* const* bufs, int64_t count, int prefix) {
    return pds::allreduce_sum_impl<float>(ctxs, n_ctx, bufs, count, prefix);
}
int pds_scatter_rows_f64(pds_ctx* const* ctxs, int n_ctx, const double* const* cols, int n_cols, const int64_t* bounds, double* const* const* dst) {
    return pds::scatter_rows_impl<double>(ctxs, n_ctx, cols, n_cols, bounds, dst);
}
int pds_scatter_rows_f32(pds_ctx* const* ctxs, int n_ctx, const float* const* cols, int n_cols, const int64_t* bounds, float* const* const* dst) {
    return pds::scatter_rows_impl<float>(ctxs, n_ctx, cols, n_cols, bounds, dst);
}
int pds_gather_f64(pds_ctx* const* ctxs, int n_ctx, const double* const* src, const int64_t* counts, double* dst) {
    return pds::gather_impl<double>(ctxs, n_ctx, src, counts, dst);
}
int pds_gather_f32(pds_ctx* const* ctxs, int n_ctx, const float* const* src, const int64_t* counts, float* dst) {
    return pds::gather_impl<float>(ctxs, n_ctx, src, counts, dst);
}
int pds_debug_last_multi_route(void) { return pds::g_multi_route; }
int pds_debug_last_grouped_route(void) { return pds::g_grouped_route; }
// (tests) whether the context's last pds_lr_grouped_* call returned stream-ordered, and -- after waiting for the stream -- the two
// words of the marked-group state: [0] groups marked and not yet re-solved, [1] fix-up blocks counted as gone; both rest at zero
int pds_debug_last_return_async(const pds_ctx* ctx) { return ctx ? ctx->last_return_async : 0; }
int pds_debug_mark_state(pds_ctx* ctx, unsigned* out2) {
    if (!ctx || !out2) return pds::fail(PDS_ERR_INVALID, "null argument");
    out2[0] = out2[1] = 0u;
    PDS_HIP_CHECK(hipSetDevice(ctx->device));
    PDS_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    if (!ctx->mark_count) return PDS_OK;
    PDS_HIP_CHECK(hipMemcpy(out2, ctx->mark_count, 2 * sizeof(unsigned), hipMemcpyDeviceToHost));
    return PDS_OK;
}
int pds_debug_last_by_key_route(int* info /* 4 ints, nullable */) {
    if (info)
        for (int i = 0; i < 4; ++i) info[i] = pds::g_by_key_info[i];
    return pds::g_by_key_route;
}
}  // extern "C"
