// common.hpp -- shared declarations of libpds_lstsq_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/pds_lstsq.h"

// Wave-private LDS hand-off (one lane writes, another lane of the SAME wave reads): LDS operations of a wave
// execute in issue order, so all that is needed is (a) the compiler not moving LDS accesses across this point and
// (b) outstanding LDS traffic drained.  A `fence(acq_rel, "wavefront")` also works but makes the compiler wait for
// EVERY outstanding memory operation (vmcnt(0)) -- which silently serialised the register prefetch of the next tile
// behind every LDS hand-off in the streaming kernels.
#define PDS_WAVE_LDS_SYNC()                                   \
    do {                                                      \
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   \
        __builtin_amdgcn_wave_barrier();                      \
    } while (0)

// Newton steps x <- x + x (1 - d x) behind v_rcp_f64 for the pivot reciprocals of the in-register L D L' solves
// (solve_reg_dev.hpp, rolling_seg_dev.hpp); tools/rcp_accuracy.hip measures what the instruction delivers on its own and after
// each step
#ifndef PDS_RCP_NEWTON
#define PDS_RCP_NEWTON 2
#endif

namespace pds {

// Column base pointers reach the kernels through a device-side table, so the compiler only knows them as generic
// ("flat") addresses.  Flat loads tick lgkmcnt as well as vmcnt -- every wait for an LDS or scalar result then also
// waits for the HBM loads in flight -- and cannot use the SGPR-base + 32-bit-VGPR-offset addressing form.  The
// kernels therefore retag the pointers as global (address space 1) once, where they fetch them.
#if defined(__HIPCC__)
template <typename T>
using gptr = const __attribute__((address_space(1))) T*;
template <typename T>
__device__ __forceinline__ gptr<T> as_global(const T* p) {
    return (gptr<T>)p;
}
#endif


// host side: the kernels templated over a width are instantiated for LO .. HI; f(std::integral_constant<int, N>{}) for the N = n
// among them.  Returns whether there was one (the fallback, if any, is the caller's).
template <int LO, int HI, typename F>
inline bool dispatch_width(int n, F&& f) {
    if constexpr (LO > HI) {
        return false;
    } else {
        if (n != LO) return dispatch_width<LO + 1, HI>(n, f);
        f(std::integral_constant<int, LO>{});
        return true;
    }
}

// ---------------------------------------------------------------------------------------------
// error plumbing: thread-local message, like the plugin ABI's `_polars_plugin_get_last_error_message`
// ---------------------------------------------------------------------------------------------
void set_error(const std::string& msg);
int fail(int code, const std::string& msg);

#define PDS_HIP_CHECK(expr)                                                                     \
    do {                                                                                        \
        hipError_t _e = (expr);                                                                 \
        if (_e != hipSuccess)                                                                   \
            return pds::fail(PDS_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));  \
    } while (0)

// ---------------------------------------------------------------------------------------------
// moment-matrix layout.  For p features: q = p + 2, Z = [x_0 .. x_{p-1} | 1 | y], A = Z'Z stored
// column-major q x q.  Index helpers:
//   A[i + j*q], i,j < p : X'X          A[i + p*q]      : column sums (bias row/col)
//   A[p + p*q]          : n (or sum w) A[i + (p+1)*q]  : X'y
//   A[p + (p+1)*q]      : sum y        A[(p+1)+(p+1)*q]: y'y
// ---------------------------------------------------------------------------------------------
constexpr int kMaxFeatSmall = 16;   // one MFMA 16x16 block of features
constexpr int kMaxFeatWide = 64;    // four blocks; beyond that -> tiled SYRK kernel (f32) / unsupported
constexpr int kTileBytesPerLane = 16;

// per-block partial record of the small-p moment kernel (doubles):
//   [0,256)  D[i + 16*j]   X'X tile     [256,272) xy[f]   [272,288) cs[f]   288 yy  289 ys  290 sw
constexpr int kPartD = 0, kPartXY = 256, kPartCS = 272, kPartYY = 288, kPartYS = 289, kPartSW = 290;
constexpr int kPartY1 = 291, kPartY2 = 292;  // spare slots: sum (y - y[0]), sum (y - y[0])^2 (IrlsArgs::y_sums)
constexpr int kPartStride = 296;

struct Workspace {
    void* ptr = nullptr;
    size_t bytes = 0;
};

}  // namespace pds

struct pds_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    int num_cus = 256;
    double* partials = nullptr; // per-block partial records (num_cus * 8 blocks * kPartStride doubles)
    pds::Workspace ws;       // HBM scratch for call-local arrays (bump allocated per call)
    size_t ws_used = 0;
    std::vector<void*> ws_spill;     // slices ws_take() had to allocate on their own (an under-estimated ws_reserve bound)
    long long ws_spill_count = 0;    // ... counted since the context was created (pds_ctx_workspace_spills)
    pds::Workspace stage;    // HBM staging of PDS_HOST column buffers
    pds::Workspace solve_ws; // factor workspace of the p' > 64 solver (solve_big.hip)
    pds::Workspace keyed;    // pds_lr_by_key_*: staged / sorted keys, permutation, gathered columns, run-length results
    pds::Workspace wkeyed;   // pds_lr_grouped_weighted_*: staged + sqrt(w)-scaled frame (separate: by_key calls it with its frame in `keyed`)
    // fused grouped kernel -> pivoted-QR pass hand-over: device counter of marked groups, and a host-mapped word the kernel
    // raises when it marks its first group (the only thing the host reads in the common case)
    unsigned* mark_count = nullptr;
    unsigned* mark_host = nullptr;      // host address
    unsigned* mark_host_dev = nullptr;  // the same word as the device sees it
    int* wait_timeouts = nullptr;       // device counter of pds_signal_wait kernels that gave up (pds_signal_wait_status)
    bool mark_dirty = false;            // a launch went out and mark_count has not been seen back at zero since (an error path)
    void* pinned = nullptr;  // pinned host scratch (small results, pointer arrays)
    size_t pinned_bytes = 0;
    void* pinned_in = nullptr;  // pinned staging of small PDS_HOST frames: all columns + pointer table, ONE H2D copy
    size_t pinned_in_bytes = 0;
    // optional per-kernel-class HIP-event timing (pds_ctx_set_timing / pds_ctx_get_timing)
    bool timing = false;
    std::vector<hipEvent_t> ev_pool;
    struct EvPair { int kind; hipEvent_t a, b; };
    std::vector<EvPair> ev_pending;
    // behaviour switches of the context (pds_ctx_set_option); their defaults come from the environment once, at pds_ctx_create
    bool opt_keyed_sort = false;       // "keyed_sort" / PDS_KEYED_SORT=1: unordered keys always take the sorting route (determinism)
    bool opt_wide_f32_native = false;  // "wide_f32_native" / PDS_WIDE_F32_NATIVE=1: f32 Gram beyond 64 features on the f32 matrix instructions
    int64_t opt_glm_split_rows = 0;       // "glm_split_rows": groups above this many rows leave the grouped IRLS kernel (0: the default)
    int64_t opt_report_chunk_groups = 0;  // "report_chunk_groups": groups per pass of the grouped report (0: from its record budget)
    int64_t opt_mixed_split_rows = 0;     // "mixed_split_rows": groups above this many rows are cut into row chunks (0: the default)
    int64_t opt_cluster_split_rows = 0;   // "cluster_split_rows": clusters above this many rows are cut into row chunks (0: the default)
    int64_t opt_cluster_waves = 0;        // "cluster_waves": cap on the waves a launch of the cluster report's pass starts (0: the default)
    int64_t opt_fused_waves = 0;          // "grouped_fused_waves": cap on the grid of the fused grouped kernel (0: every wave slot)
    int64_t opt_fused_late_permille = 0;  // "grouped_fused_late_permille": rows, in 1/1000, of the grid's second half (0: grouped_split_dev.hpp)
    double kind_ms[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    long long kind_count[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    std::vector<float> kind_samples[9];  // the individual bracketed durations (ms), newest kept up to 4096 per class
    // (behind everything else: the members above keep their places for the translation units that do not know these)
    int64_t opt_multi_route = 0;  // "grouped_multi_route": 0 choose, 1 the one-wave-per-group kernel, 2 one fused launch per target
    int64_t opt_multi_waves = 0;  // "grouped_multi_waves": cap on the grid of the grouped multi-target kernel (0: every wave slot)
    int64_t opt_within_split_rows = 0;  // "within_split_rows": absorbed groups above this many rows are cut into row chunks (0: the default)
    int64_t opt_within2_accel = 0;      // "within2_accel": 0 plain alternating sweeps, 1 Irons-Tuck cycles (capi_within2.hpp)
    int64_t opt_rolling_waves = 0;      // "rolling_waves": cap on the waves a launch of the tiled rolling / expanding kernels starts (0: the default grid)
    // Stream-ordered return (include/pds_lstsq.h, "Synchronisation"): on a stream the caller handed in, the device-resident grouped
    // fit of up to 16 features leaves its work queued and returns.  mark_count[1] counts the blocks of the marked-group fix-up
    // kernel that have left (the last one puts both words back to zero).
    bool caller_stream = false;         // the stream came from pds_ctx_set_stream
    int64_t opt_blocking_return = 0;    // "blocking_return": 1 = every call synchronises before it returns (tests, A/B)
    int last_return_async = 0;          // the last pds_lr_grouped_* call returned with work still queued (pds_debug_last_return_async)
    // the column pointer table of stream-ordered calls: a slot of its own, written on the stream (write_col_table_kernel) only when
    // the pointers differ from the ones it holds -- a resident frame fitted again and again writes it once
    const void** col_table_dev = nullptr;
    const void* col_table_host[18] = {};
    bool col_table_valid = false;
    bool async_pending = false;         // a stream-ordered call returned and the context has not waited for the stream since
};

namespace pds {

// Development switches -- the A/B alternative of a default that won its measurement, timing experiments -- exist only in libraries
// built with EXTRA=-DPDS_DEV_SWITCHES (tools/README.md).  A product build compiles the default in and never looks them up.
#ifdef PDS_DEV_SWITCHES
inline const char* dev_env(const char* name) { return std::getenv(name); }
#else
inline const char* dev_env(const char*) { return nullptr; }
#endif

// kernel classes for the timing hooks
enum { kKindMoments = 0, kKindGroupedMoments = 1, kKindSolve = 2, kKindPass2 = 3, kKindRolling = 4, kKindIter = 5, kKindSweep1 = 6, kKindSweep2 = 7, kKindGraph = 8,
       kNumKinds = 9 };
// RAII: records a HIP event pair around the launches issued in its scope when ctx->timing is on
struct KernelTimer {
    pds_ctx* ctx;
    int kind;
    hipEvent_t a = nullptr, b = nullptr;
    KernelTimer(pds_ctx* c, int k);
    ~KernelTimer();
};

int ensure_ws(pds_ctx* ctx, Workspace& w, size_t bytes);
int ensure_pinned(pds_ctx* ctx, size_t bytes);
// call-local bump allocation inside ctx->ws: ws_reserve() once per API call with an upper bound, then
// ws_take() hands out 256-byte aligned slices; a request past the reserved bound is served from its own allocation and
// counted (never silently out of bounds).
int ws_reserve(pds_ctx* ctx, size_t total_bytes);
void* ws_take(pds_ctx* ctx, size_t bytes);

// Columns resident in HBM for the duration of one call.  For PDS_DEVICE inputs this is just the
// pointer array copied to the device; for PDS_HOST inputs the column buffers are staged into HBM.
template <typename T>
struct DeviceCols {
    const T** d_ptrs = nullptr;  // device array of nc pointers
    std::vector<const T*> h_ptrs; // the same pointers on the host
    int nc = 0;
};

// order on device: x_0..x_{p-1}, y, [w]
template <typename T>
int make_device_cols(pds_ctx* ctx, const T* const* cols /*[y,x1..xp]*/, const T* weights, int n_feat,
                     int64_t n_rows, pds_space space, DeviceCols<T>& out,
                     // device-resident frames of up to 18 columns: the pointer table goes to the context's own slot, written by a
                     // kernel on the stream (no host-side copy source, nothing for the host to wait for) -- stream-ordered calls
                     bool table_on_stream = false);

// one IRLS step folded into the Gram pass (moments.hip WM = 3): link / variance ids as in pds_lstsq.h, init = first iteration
struct IrlsArgs {
    int link = 0, variance = 0, init = 0;
    double y_mean = 0.0;
    // WM = 4 (HC2 / HC3 meat in the residual pass): (X'X)^-1, p' x p' column-major in the kernel's T, and the power of
    // 1 / (1 - h_i) that scales the squared residual (1: HC2, 2: HC3)
    const void* inv = nullptr;
    int hc_pow = 0;
    // residual-weighted passes of lin_reg_report (WM = 2 / 4): also sum (y - y[0]) and sum (y - y[0])^2 of the rows the pass reads anyway --
    // the target's variance (PDS_REPORT_DERIVE_YVAR) without one more pass over y; they travel in two spare slots of the partial records
    int y_sums = 0;
};

// ---- kernels' host launchers (moments.hip) ----
template <typename T>
int launch_moments(pds_ctx* ctx, const DeviceCols<T>& dc, int n_feat, int64_t n_rows, bool weighted,
                   T* d_moments /*device, (p+2)^2*/,
                   // p <= 16, unweighted frames only: weight of row i = (y_i - x_i . beta [- beta_p])^2 formed inside the pass
                   // (the HC0 / HC1 meat of lin_reg_report); d_sums_resid[0] receives sum of the weights = sum e^2
                   const T* d_beta_resid = nullptr, int bias_resid = 0, double* d_sums_resid = nullptr,
                   // p <= 16: write the record as f64 into this slot instead of d_moments (row chunks of a host frame)
                   double* d_moments_f64 = nullptr,
                   // p <= 16: weights and working response of one IRLS step from d_beta_resid (moments = X'WX | X'Wz)
                   const IrlsArgs* irls = nullptr,
                   // p <= 16, residual-weighted passes (d_beta_resid): sum (y - y[0]), sum (y - y[0])^2 -> d_ysums[0..1] (see IrlsArgs::y_sums)
                   double* d_ysums = nullptr);
// moments.hip: weights and working response of one IRLS step for frames of more than 16 features (the wide Gram build reads them)
template <typename T>
int launch_irls_working_wide(pds_ctx* ctx, const DeviceCols<T>& dc, int n_feat, int64_t n_rows, int bias, const T* d_beta,
                             const IrlsArgs& ia, T* d_w, T* d_z);
// moments.hip: Gram build straight from a row-major device matrix (X[r * ld + c], y[r]), 1..16 features, unweighted
template <typename T>
int launch_moments_rowmajor(pds_ctx* ctx, const T* d_X, int64_t ld, const T* d_y, int n_feat, int64_t n_rows, T* d_moments,
                            double* d_moments_f64 = nullptr);
template <typename T>
int launch_sum_moment_slots(pds_ctx* ctx, const double* d_slots, int nslots, int len, T* d_out);

// moments_wide.hip: p > 16 (tiled MFMA SYRK with split-K); partials come out of ctx->ws (reserve
// moments_wide_workspace() bytes on top of the call's other needs)
template <typename T>
int launch_moments_wide(pds_ctx* ctx, const DeviceCols<T>& dc, int n_feat, int64_t n_rows, bool weighted, T* d_moments);
size_t moments_wide_workspace(int num_cus, int n_feat, int64_t n_rows, bool weighted = false);
// moments_mid.hip: 17 .. 64 f64 features -- the streaming kernel (several 16-feature tile columns); its per-wave
// partial records come out of ctx->ws like the wide kernel's (moments_wide_workspace() covers them)
size_t moments_mid_workspace(int num_cus);
template <typename T>
int launch_moments_mid(pds_ctx* ctx, const DeviceCols<T>& dc, int n_feat, int64_t n_rows, bool weighted, T* d_moments);

// segmented (per-group) moments: d_moments [n_groups][(p+2)^2].  d_group_index (p <= 16 only): record g belongs to group
// d_group_index[g] of the offsets array instead of group g.
template <typename T>
int launch_grouped_moments(pds_ctx* ctx, const DeviceCols<T>& dc, int n_feat, const int64_t* d_offsets,
                           int64_t n_groups, T* d_moments, const int32_t* d_group_index = nullptr, bool weighted = false);

struct SolveParams;
// grouped_fused.hip: per-group Gram + gated Cholesky in one streaming kernel (p <= 16, OLS / ridge); unless the caller asked
// for "choleskey", groups next to the gate go through a second, pivoted-QR pass (d_mom_scratch: room for `scratch_groups`
// moment records of (p+2)^2 values; the pass is chunked by it).  stay_on_stream (nullable, in / out): in = the caller would like
// the call to end without a host synchronisation; then the marked groups of a "qr" fit with up to 16 coefficients are re-solved by
// a kernel queued behind the stream (fixup_marked_kernel) instead of the host-driven pass.  out = nothing in the call waited for the
// device and nothing of it is left for the host to do.
template <typename T>
int launch_grouped_fused(pds_ctx* ctx, const DeviceCols<T>& dc, int n_feat, int64_t n_rows, const int64_t* d_offsets,
                         int64_t n_groups, const SolveParams& sp, T* d_coeffs, uint8_t* d_flags, T* d_mom_scratch,
                         int64_t scratch_groups, bool* stay_on_stream = nullptr);

// ---- solve.hip ----
struct SolveParams {
    int p;         // features (without bias)
    int add_bias;
    int solver;
    double lambda; // l2 added to the first p diagonals (not the bias)
    double gate_tol; // <= 0: no gate
    int lambda_on_bias; // rolling / recursive: lambda on every diagonal
};
// batched: moments [n_sys][(p+2)^2] -> coeffs [n_sys][p+bias], flags [n_sys] (1 = null)
// optional inv_out [n_sys][p'*p'] (column-major) = (X'X + lambda)^-1 via the QR, and logdet.
template <typename T>
int launch_solve(pds_ctx* ctx, const T* d_moments, int64_t n_sys, const SolveParams& sp, T* d_coeffs,
                 uint8_t* d_flags, T* d_inv_out, const int64_t* d_rows_per_sys /*nullable*/);

// capi_lr.hpp: the marked systems of a grouped fit through the reference's factorisation for sp.solver (pivoted QR; "svd": host SVD gate)
template <typename T>
int launch_solve_marked(pds_ctx* ctx, const T* d_rec, int64_t n_sys, const SolveParams& sp, T* d_coeffs, uint8_t* d_flags,
                        const int64_t* d_rows_per_sys);

// solve_big.hip: p' > 64 (Cholesky on an HBM/L2 workspace, one workgroup per system); used by launch_solve
template <typename T>
int launch_solve_big(pds_ctx* ctx, const T* d_moments, int64_t n_sys, const SolveParams& sp, T* d_coeffs, uint8_t* d_flags,
                     T* d_inv_out);

// solve_reg.hip: register-resident variant (p' <= 16, QR, no inverse); used by launch_solve.  `tri` (nullable): the systems are rows
// ids[s] of an id-indexed table of packed upper triangles over [x_0 .. x_{pc-1}, 1, y] (keyed_partition.hip) instead of d_moments
struct TriSource {
    const double* table = nullptr;
    const unsigned* ids = nullptr;
    int nvp = 0, pc = 0;
};
template <typename T>
int launch_solve_reg(pds_ctx* ctx, const T* d_moments, int64_t n_sys, const SolveParams& sp, T* d_coeffs,
                     uint8_t* d_flags, const int64_t* d_rows_per_sys, const TriSource* tri = nullptr);

// solve_wave.hip: 17 .. 64 features, one wave per system, L D L' in registers + a pivoted-QR pass over the systems it marks
// (PDS_ERR_UNSUPPORTED without an error message: not applicable, the caller keeps launch_solve)
template <typename T>
int launch_solve_wave(pds_ctx* ctx, const T* d_moments, int64_t n_sys, const SolveParams& sp, T* d_coeffs, uint8_t* d_flags,
                      const int64_t* d_rows_per_sys, void* d_ws);
size_t solve_wave_workspace(int n_feat, int add_bias, int64_t n_sys, size_t elem);

template <typename T>
int launch_cd(pds_ctx* ctx, const T* d_moments, int p, int add_bias, double l1, double l2, double tol,
              int max_iter, int positive, T* d_coeffs, int* d_info /*per system: [0]=sweeps,[1]=converged; nullable*/,
              int64_t n_sys = 1, uint8_t* d_flags = nullptr, const int64_t* d_rows_per_sys = nullptr,
              double pen_rows = 0.0 /* > 0: the penalties scale with this row count, not with the record's count slot (an IRLS record
                                       holds sum w there), and the bias move counts towards the sweep's largest move */,
              int warm_start = 0 /* the sweeps start from the coefficients d_coeffs holds, not from 0 */);
template <typename T>
int launch_nnls(pds_ctx* ctx, const T* d_moments, int p, int add_bias, double tol, int max_iter, T* d_coeffs,
                int64_t n_sys = 1, uint8_t* d_flags = nullptr, const int64_t* d_rows_per_sys = nullptr);

// ---- grouped_pred.hip: per-row pred / resid of grouped fits (frame in group order; d_perm sends rows back to frame order) ----
template <typename T>
int launch_grouped_pred(pds_ctx* ctx, const T* const* d_cols, int n_feat, int bias, int64_t n_rows, const int64_t* d_off,
                        int64_t n_groups, const T* d_coeffs, const uint8_t* d_flags, const uint32_t* d_perm, T* d_pred, T* d_resid,
                        uint8_t* d_row_null);

template <typename T>
int launch_grouped_pred_by_id(pds_ctx* ctx, const T* const* d_cols, int n_feat, int bias, int64_t n_rows, const int64_t* d_keys,
                              const int64_t* d_kmin, const uint32_t* d_rank, int64_t n_groups, const T* d_coeffs, const uint8_t* d_flags,
                              T* d_pred, T* d_resid, uint8_t* d_row_null);
// elements per row of the id-indexed coefficient table: rows padded to whole 64- or 128-byte lines (wider rows: as they are)
template <typename T>
inline int grouped_pred_table_stride(int pp) {
    const int b = pp * (int)sizeof(T);
    return b <= 64 ? 64 / (int)sizeof(T) : (b <= 128 ? 128 / (int)sizeof(T) : pp);
}
template <typename T>
int launch_grouped_pred_by_id_table(pds_ctx* ctx, const T* const* d_cols, int n_feat, int bias, int64_t n_rows, const int64_t* d_keys,
                                    const int64_t* d_kmin, const uint32_t* d_ids /* dense id of group g */, int64_t n_groups, const T* d_coeffs,
                                    const uint8_t* d_flags, T* d_table /* n_ids x grouped_pred_table_stride(p') workspace */, T* d_pred, T* d_resid, uint8_t* d_row_null);  // grouped_pred.hip
// ---- the grouped GLM kernels (grouped_irls.hip, grouped_glm_report.hip): one description of a launch, shared by the fit and the report.
// The frame as the kernels see it: d_cols holds x_0 .. x_{p-1}, y (18 entries) and, with `wo`, the prior weights and the offsets
// behind y (20 entries), of which either may be null (weights 1, offsets 0).  1 .. 16 features.
template <typename T>
struct GlmGroupsDev {
    const T* const* d_cols;
    int n_feat, bias;
    int64_t n_rows;
    const int64_t* d_off;
    int64_t n_groups;
    int link, variance;
    int64_t split_rows;
    bool wo;  // the weighted / offset kernels; the table carries the two extra entries
};
// Groups of more than `split_rows` rows are not walked by one wave: their indices are appended to d_list (any order, *d_count of
// them, of which the first `cap` are stored; the caller zeroes the count).
struct GlmLongList {
    int64_t* d_list;
    unsigned* d_count;
    int64_t cap;
};
// the fit's controls and outputs.  l1_reg / l2_reg > 0: the elastic-net penalised fit (features only, scaled by the group's row
// count); a penalty <= 0 means none.
template <typename T>
struct GlmFitDev {
    double tol;
    int max_iter;
    double l1_reg, l2_reg;
    T* d_coeffs;
    int32_t* d_n_iter;
    uint8_t* d_null;
    T* d_pred;               // nullable
    uint8_t* d_row_null;     // nullable
    const uint32_t* d_perm;  // nullable: row r of the frame in group order is row d_perm[r] of pred / row_null
};
// ---- grouped_irls.hip: a GLM per group (IRLS), one wave per group, all iterations on chip.  The one fit launcher: it picks the
// kernel set -- weighted / offset (groups.wo: unpenalised), coordinate descent (l1_reg > 0), ridge (l2_reg > 0), plain.
template <typename T>
int launch_grouped_irls(pds_ctx* ctx, const GlmGroupsDev<T>& groups, const GlmFitDev<T>& fit, const GlmLongList& long_list);
// glm_wo_model.hip: the one-model iteration with prior weights d_pw and offsets d_off (device, each nullable).  The side sums of the
// first pass, d_out4 = {rows of positive weight, weights that are negative or not finite, sum pw, sum pw y}; and the weight and the
// working response of one IRLS step as two columns, which the weighted Gram build then reads (every width).
template <typename T>
int launch_glm_wo_sums(pds_ctx* ctx, const T* d_y, const T* d_pw, int64_t n_rows, double* d_out4);
template <typename T>
int launch_irls_working_wo(pds_ctx* ctx, const DeviceCols<T>& dc, int n_feat, int64_t n_rows, int bias, const T* d_beta, const IrlsArgs& ia,
                           const T* d_pw, const T* d_off, T* d_w, T* d_z);
// The penalised IRLS step (l1_reg > 0) is a coordinate descent on the iteration's weighted Gram system: its sweeps end when the
// largest move of a sweep is below kGiCdInner * tol, or at kGiCdSweeps sweeps (not an error: the outer iteration goes on).
constexpr double kGiCdInner = 0.1;
constexpr int kGiCdSweeps = 1000;
// per-row means g^-1(x . beta) of the rows [r0, r1) from one coefficient vector in device memory
template <typename T>
int launch_glm_pred_range(pds_ctx* ctx, const T* const* d_cols, int n_feat, int bias, int64_t r0, int64_t r1, const T* d_beta,
                          const uint8_t* d_null_flag, int link, T* d_pred, uint8_t* d_row_null, const uint32_t* d_perm,
                          const T* d_offset = nullptr /*an offset per row of the frame, added to x . beta*/);
// ---- grouped_glm_report.hip: the report of a GLM per group at the coefficients in d_coeffs (se, z, p, CI, cov, deviances,
// dispersion: the definitions stand at the head of that file), one wave per group; 1 .. 16 features.  Every output is nullable.
// Groups of more than `split_rows` rows are appended to the long list and reported by launch_grouped_glm_report_pieces: d_pieces
// [n_pieces][3] = (group, first row, end row), d_fin [n_fin][3] = (group, first piece, pieces), d_rec n_pieces records of
// kGlmReportRec doubles.  Both launchers take the weighted / offset kernels (grouped_glm_report_wo.hip) when groups.wo is set.
template <typename T>
struct GlmReportDev {
    T *se, *z, *p, *lo, *hi, *cov, *deviance, *null_deviance, *pearson, *dispersion;
    int64_t* df_resid;
    uint8_t* report_null;
};
// a piece's record: [0,256) I [i * 16 + j]; [256,272) X'w; from 272 the scalar sums in the order of grouped_glm_report.hip's GrSum:
// sum w, sum (y - y0), pearson, deviance, the family sum (the weighted / offset form: the last four weighted by pw; then sum pw and
// the rows of positive weight)
constexpr int kGlmReportRec = 280;
template <typename T>
int launch_grouped_glm_report(pds_ctx* ctx, const GlmGroupsDev<T>& groups, const T* d_coeffs, const uint8_t* d_null,
                              const GlmReportDev<T>& out, const GlmLongList& long_list);
template <typename T>
int launch_grouped_glm_report_pieces(pds_ctx* ctx, const GlmGroupsDev<T>& groups, const T* d_coeffs, const GlmReportDev<T>& out,
                                     const int64_t* d_pieces, int64_t n_pieces, const int64_t* d_fin, int64_t n_fin, double* d_rec);
// ---- grouped_rcond.hip: lin_reg_w_rcond per group, one wave per group: Gram, one-sided Jacobi of X'X (+ l2_reg) and the minimum-norm
// solve on chip; 1 .. 16 features.  d_coeffs / d_svals [n_groups][p'] (bias last; singular values descending), d_null [n_groups].
// rcond is the caller's value: the floor eps_T max(n_g, p') is applied per group.
template <typename T>
int launch_grouped_rcond(pds_ctx* ctx, const T* const* d_cols, int n_feat, int bias, int64_t n_rows, const int64_t* d_off,
                         int64_t n_groups, double l2_reg, double rcond, T* d_coeffs, T* d_svals, uint8_t* d_null);
// ---- grouped_multi.hip: the multi-target fit per group (k targets, one design matrix), one wave per group; 1 .. 16 features, 1 .. 15
// targets, the gated L D L' only (gate_tol > 0).  d_cols: x_0 .. x_{p-1}, t_0 .. t_{k-1}, padded to 32 valid entries.  d_coeffs
// [n_groups][k][p'] (bias last), d_flags [n_groups]: 0 fitted, 1 null, 2 next to the gate (mark_suspects only): not answered, its
// index appended to d_mark_list (any order, *d_mark_count of them; the caller zeroes the count) for the reference's factorisation.
template <typename T>
int launch_grouped_multi(pds_ctx* ctx, const T* const* d_cols, int n_feat, int n_targets, int bias, int64_t n_rows, const int64_t* d_off,
                         int64_t n_groups, double l2_reg, double gate_tol, bool mark_suspects, T* d_coeffs, uint8_t* d_flags,
                         int32_t* d_mark_list, unsigned* d_mark_count);
// one target's block d_co [n][p'] / d_fl [n] -> target t of the groups d_list[i] (null: i) of d_coeffs [.][k][p']; the group's flag is
// set (first) or added to
template <typename T>
int launch_multi_scatter(pds_ctx* ctx, const T* d_co, const uint8_t* d_fl, const int32_t* d_list, int64_t n, int t, int k, int pp, bool first,
                         T* d_coeffs, uint8_t* d_flags);
// NaN for all k p' coefficients of the flagged groups among d_list[i] (null: i), i < n; check_finite: a group with a coefficient that
// is not finite is flagged first
template <typename T>
int launch_multi_null_fill(pds_ctx* ctx, uint8_t* d_flags, const int32_t* d_list, int64_t n, int kpp, bool check_finite, T* d_coeffs);
template <typename T>
int launch_multi_extract(pds_ctx* ctx, const T* d_coeffs, int64_t n_groups, int t, int k, int pp, T* d_out);  // target t -> [n_groups][p']
// *d_bad = 1 when the offsets decrease or leave the frame (the caller zeroes it)
int launch_multi_offsets_check(pds_ctx* ctx, const int64_t* d_off, int64_t n_groups, int64_t n_rows, unsigned* d_bad);
// ---- mixed.hip: the random-intercept mixed model's passes (capi_mixed.hpp).  One record layout for the scatter partials and the
// per-gamma sums (doubles): [0,256) the 16 x 16 feature block [i * 16 + j]; [256,272) the y column; [272,288) sum c m_f (profile
// only); 288 the y diagonal; 289 sum c; 290 sum c m_y; 291 sum ln(1 + gamma n_g)
constexpr int kMixedRecW = 0, kMixedRecXY = 256, kMixedRecCM = 272, kMixedRecYY = 288, kMixedRecC = 289, kMixedRecCY = 290, kMixedRecLD = 291;
constexpr int kMixedRecStride = 296;
// records [0, n_rec) of d_rec -> one record at d_out, added in index order entry by entry, in two stages (blocks of 64 records into
// d_stage: room for a 64th of n_rec, rounded up; then the block sums).  compensated: every running sum carries its rounding errors
// (two-sum) and adds them at the end -- other bits than the plain sum, so a pass keeps the one it was defined with.
int launch_sum_records(pds_ctx* ctx, const double* d_rec, int n_rec, double* d_stage, double* d_out, bool compensated);
// the row chunks of the groups above the split threshold (device arrays the host filled); n_chunks = 0: none
struct MixedChunks {
    int64_t n_chunks = 0, n_long = 0;
    const int64_t *d_chunk_r0 = nullptr, *d_chunk_n = nullptr, *d_chunk_g = nullptr, *d_chunk_first = nullptr;  // per chunk
    const int64_t *d_long_g = nullptr, *d_long_c0 = nullptr, *d_long_nc = nullptr, *d_long_first = nullptr, *d_long_n = nullptr;  // per group
    double* d_sums = nullptr;     // n_chunks x (p + 1)
    unsigned* d_varies = nullptr;  // n_chunks
};
int mixed_stats_blocks(const pds_ctx* ctx, int64_t n_work);    // partial records a stats / chunk launch writes
int mixed_profile_blocks(const pds_ctx* ctx, int64_t n_groups);
// group means (feature-major, d_means[(p + 1) x n_groups]: features, then y), the "varies within some group" bits of the features
// (*d_flags) and the within scatter W (one record at d_w).  d_cols: x_0 .. x_{p-1}, y.  d_partials: room for
// mixed_stats_blocks(n_groups) + mixed_stats_blocks(n_chunks) records, d_stage for a 64th of that (rounded up).  d_beta0 (nullable,
// p + 1 values, intercept first): the target is read as y - [1, x] . beta0.
template <typename T>
int launch_mixed_stats(pds_ctx* ctx, const T* const* d_cols, int n_feat, const int64_t* d_off, int64_t n_groups, int64_t split_rows,
                       const MixedChunks& ch, const double* d_beta0, double* d_means, unsigned* d_flags, double* d_partials,
                       double* d_stage, double* d_w);
// one gamma: sum_g c_g [m m' | m m_y | m], sum c, sum c m_y, sum c m_y^2, sum ln(1 + gamma n_g) -> one record at d_out
int launch_mixed_profile(pds_ctx* ctx, const double* d_means, int n_feat, const int64_t* d_off, int64_t n_groups, double gamma,
                         double* d_partials, double* d_stage, double* d_out);
// ---- cluster_meat.hip: the cluster-robust report's pass (capi_report_cluster.hpp).  Records in the layout above: [0,256) the feature
// block of the meat, [256,272) its bias column, 288 sum e^2 and 290 its compensation term (the sum is their sum), 289 the bias diagonal.
constexpr int kClusterScoreStride = 18;  // doubles per chunk score: 16 features, the bias entry, one of padding
// the row chunks of the clusters above the split threshold (device arrays the host filled); n_chunks = 0: none
struct ClusterChunks {
    int64_t n_chunks = 0, n_long = 0;
    const int64_t *d_chunk_r0 = nullptr, *d_chunk_n = nullptr;  // per chunk
    const int64_t *d_long_c0 = nullptr, *d_long_nc = nullptr;   // per long cluster: first chunk, chunks
    double* d_scores = nullptr;                                  // n_chunks x kClusterScoreStride
};
int cluster_meat_blocks(const pds_ctx* ctx, int64_t n_work);  // partial records a launch over n_work work items writes
// meat and sum e^2 of e = y - [x, 1] . beta (d_beta: features, then the bias when `bias`) -> one record at d_rec.  d_cols: x_0 ..
// x_{p-1}, y.  d_partials: room for cluster_meat_blocks(n_clusters) + cluster_meat_blocks(n_chunks) + cluster_meat_blocks(n_long)
// records, d_stage for a 64th of that (rounded up).
template <typename T>
int launch_cluster_meat(pds_ctx* ctx, const T* const* d_cols, int n_feat, const int64_t* d_off, int64_t n_clusters, int64_t split_rows,
                        const ClusterChunks& ch, const T* d_beta, int bias, double* d_partials, double* d_stage, double* d_rec);
// ---- glm_meat.hip: the meat of the robust / cluster-robust one-model GLM report (capi_glm_sandwich.hpp) at the coefficients d_beta
// (features, then the bias when `bias`) -> one record at d_rec.  d_cols: x_0 .. x_{p-1}, y, weights, offset (a table of n_feat + 3
// device pointers; the last two nullable).  n_clusters > 0: the cluster forms (d_off, split_rows and ch as launch_cluster_meat; the
// record's kMixedRecLD slot counts the clusters that hold a row of positive weight, its kMixedRecC slot is the bias diagonal);
// in both forms the kMixedRecCM slot counts the rows of positive weight;
// n_clusters = 0: the hc forms over row ranges (the bias diagonal is kMixedRecYY + kMixedRecCY).  d_partials: room for
// glm_meat_records() records, d_stage for a 64th of that (rounded up).
int glm_meat_records(const pds_ctx* ctx, int64_t n_rows, int64_t n_clusters, const ClusterChunks& ch);
template <typename T>
int launch_glm_meat(pds_ctx* ctx, const T* const* d_cols, int n_feat, int64_t n_rows, const int64_t* d_off, int64_t n_clusters,
                    int64_t split_rows, const ClusterChunks& ch, const T* d_beta, int bias, int link, int variance, double* d_partials,
                    double* d_stage, double* d_rec);
// ---- within_pass.hip: the fixed-effects regression's per-row pass (capi_within.hpp).  With beta (n_feat doubles) and the group means of
// launch_mixed_stats (d_means, the same d_off / n_groups / split_rows / chunks): alpha_g = m_y - m . beta -> d_alpha[d_gmap ? d_gmap[g] : g],
// e = (y - m_y) - (x - m) . beta -> d_resid, y - e -> d_pred (row r of the frame is row d_perm[r] of the outputs when d_perm is given),
// sum e^2 (record slot 288 + its error term in 290) and, with `meat`, sum_g s_g s_g' of the centred scores (record slots [0,256)) ->
// one record at d_rec.  d_alpha, d_pred, d_resid, d_gmap, d_perm: nullable.  d_scores: n_chunks x kClusterScoreStride doubles
// (`meat` with chunks).  d_partials: room for within_pass_blocks(n_groups) + within_pass_blocks(n_chunks) + within_pass_blocks(n_long)
// records, d_stage for a 64th of that (rounded up).
int within_pass_blocks(const pds_ctx* ctx, int64_t n_work);
template <typename T>
int launch_within_pass(pds_ctx* ctx, const T* const* d_cols, int n_feat, const int64_t* d_off, int64_t n_groups, int64_t split_rows,
                       const MixedChunks& ch, double* d_scores, const double* d_beta, const double* d_means, bool meat, const int64_t* d_gmap,
                       const uint32_t* d_perm, T* d_alpha, T* d_pred, T* d_resid, double* d_partials, double* d_stage, double* d_rec);
// ---- glm_within.hip: the fixed-effects GLM's passes (capi_glm_within.hpp).  d_cols: x_0 .. x_{p-1}, y, weights, offset (a table of
// n_feat + 3 device pointers; the last two nullable); d_off / n_groups: the non-empty groups; ch: the chunks of the groups above
// split_rows (upload_mixed_chunks with nc = p + 2: d_sums holds the chunk sums of an iteration, d_varies the chunks' pre-pass words).
int glm_within_iter_blocks(const pds_ctx* ctx, int64_t n_work);   // partial records a launch of the iteration writes per work list
int glm_within_final_blocks(const pds_ctx* ctx, int64_t n_work);  // ... and of the final pass
// the pre-pass: d_gstat [3 x n_groups] the counting rows (pw > 0), sum pw, sum pw y of every group; d_drop [n_groups] 1 for a group
// that is dropped (no counting row; variance 1: every counting y is 0; variance 2: every one is 0 or every one is 1); d_flags[0]: the
// features that vary inside some kept group, d_flags[1]: a weight is negative or not finite.  d_cpre: n_chunks x (3 + p) doubles.
template <typename T>
int launch_glm_within_pre(pds_ctx* ctx, const T* const* d_cols, int n_feat, const int64_t* d_off, int64_t n_groups, int64_t split_rows,
                          const MixedChunks& ch, int variance, double* d_cpre, double* d_gstat, int32_t* d_drop, unsigned* d_flags);
// one iteration: with eta = alpha_g + x . beta + o from (d_beta, d_means_in) -- or the start rule from ybar when `first` -- the weighted
// group means -> d_means_out [(p + 1) x n_groups] (features, then z) and the centred weighted scatter -> one record at d_rec (W_xx in
// [0,256), W_xz in [256,272)).  d_partials: room for glm_within_iter_blocks(n_groups) + glm_within_iter_blocks(n_chunks) records,
// d_stage for a 64th of that (rounded up).
template <typename T>
int launch_glm_within_iter(pds_ctx* ctx, const T* const* d_cols, int n_feat, const int64_t* d_off, int64_t n_groups, int64_t split_rows,
                           const MixedChunks& ch, const int32_t* d_drop, int link, int variance, bool first, double ybar, const double* d_beta,
                           const double* d_means_in, double* d_means_out, double* d_partials, double* d_stage, double* d_rec);
// the final pass at (d_beta, d_means): alpha_g -> d_alpha[d_gmap ? d_gmap[g] : g] (kept groups only), mu_i -> d_pred (through d_perm;
// NaN on the rows of dropped groups), the deviance (record slots 288 + 290), Pearson's chi2 (289 + 291) and, with `meat`, sum_g s_g s_g'
// of the centred scores ([0,256)) -> one record at d_rec.  d_scores: n_chunks x kClusterScoreStride doubles (`meat` with chunks).
// d_partials: room for glm_within_final_blocks of n_groups, n_chunks and n_long records, d_stage for a 64th of that (rounded up).
template <typename T>
int launch_glm_within_final(pds_ctx* ctx, const T* const* d_cols, int n_feat, const int64_t* d_off, int64_t n_groups, int64_t split_rows,
                            const MixedChunks& ch, double* d_scores, const int32_t* d_drop, int link, int variance, const double* d_beta,
                            const double* d_means, bool meat, const int64_t* d_gmap, const uint32_t* d_perm, T* d_alpha, T* d_pred,
                            double* d_partials, double* d_stage, double* d_rec);
// ---- within_cluster.hip: the fixed-effects regression's errors clustered on any key (capi_within_cluster.hpp).  Row r's score
// x~_r e_r is staged row-major at d_rows[r * cluster_row_stride(p)]: p doubles, padded to an even count.
constexpr int cluster_row_stride(int p) { return (p + 1) & ~1; }
// d_flags[0] |= 1 when a level of factor 1 (rows [d_off1[l], d_off1[l + 1]), n1 levels) holds two cluster codes; d_flags[1] the same
// for factor 2 (d_start2 nullable: one factor; level l is the places [d_start2[l], d_start2[l + 1]) of d_idx2).  d_codes: the
// cluster code of every row, frame order.  Both flags are zeroed here; the caller reads them back.
int launch_cluster_nested(pds_ctx* ctx, const int64_t* d_off1, int64_t n1, const uint32_t* d_start2, int64_t n_levels2, const uint32_t* d_idx2,
                          const int32_t* d_codes, int* d_flags);
// launch_within_pass's arguments (the same d_off / n_groups / split_rows / chunks, beta, the group means): the row scores -> d_rows
template <typename T>
int launch_within_row_scores(pds_ctx* ctx, const T* const* d_cols, int n_feat, const int64_t* d_off, int64_t n_groups, int64_t split_rows,
                             const MixedChunks& ch, const double* d_beta, const double* d_means, double* d_rows);
int cluster_meat_records(const pds_ctx* ctx, int64_t n_clusters);  // partial records launch_cluster_gather_meat writes
// d_idx: the rows in cluster order; chunk k is its places [d_chunk_pos[k], + d_chunk_n[k]), all of one cluster; cluster j is the chunks
// [d_cl_c0[j], + d_cl_nc[j]).  d_scores: n_chunks x kClusterScoreStride doubles.  The meat sum_c s_c s_c' -> slots [0,256) of one
// record at d_rec.  d_partials: room for cluster_meat_records(n_clusters) records, d_stage for a 64th of that (rounded up).
int launch_cluster_gather_meat(pds_ctx* ctx, int n_feat, const double* d_rows, const uint32_t* d_idx, const int64_t* d_chunk_pos,
                               const int64_t* d_chunk_n, int64_t n_chunks, const int64_t* d_cl_c0, const int64_t* d_cl_nc, int64_t n_clusters,
                               double* d_scores, double* d_partials, double* d_stage, double* d_rec);
// ---- within2_sweep.hip: the alternating sweeps of the fixed-effects regression with two absorbed factors (capi_within2.hpp).  The device
// arrays of one call (nc = p + 1): the state is a1 / a2, the accumulated level means; row r is worth (w_r - a1[g1(r)]) - a2[code2(r)].
struct Within2Dev {
    int64_t n_rows = 0, n1 = 0, split1 = 0;  // rows; occupied levels of factor 1; its levels above split1 rows are the chunks ch1
    const int64_t* d_off1 = nullptr;         // n1 + 1 offsets
    MixedChunks ch1;                         // (d_sums: the chunk sums)
    const int32_t* d_code2 = nullptr;        // [n_rows] the code of factor 2 of every row, frame order, its range checked on the device
    const uint32_t* d_idx2 = nullptr;        // [n_rows] the rows in ascending code order (launch_within2_order)
    const uint32_t* d_g1 = nullptr;          // [n_rows] the level of factor 1 of every row (launch_within2_row_levels)
    int64_t n_chunks2 = 0, n_lev2 = 0;       // chunks of idx2 (every level is cut from the start); occupied levels of factor 2
    const int64_t *d_c2_pos = nullptr, *d_c2_n = nullptr;                       // per chunk: first place in idx2, rows
    const int32_t* d_c2_code = nullptr;                                         // ... and the code
    const int64_t *d_l2_c0 = nullptr, *d_l2_nc = nullptr, *d_l2_n = nullptr;    // per occupied level: first chunk, chunks, rows
    const int32_t* d_l2_code = nullptr;                                         // ... and the code
    double *d_csum2 = nullptr, *d_w0 = nullptr, *d_a1 = nullptr, *d_a2 = nullptr;  // n_chunks2 x nc; n_rows x nc; n1 x nc; codes x nc
    double *d_scale = nullptr, *d_delta = nullptr;  // [nc] s_j; within2_delta_blocks(n_lev2) values per sweep, their maximum is delta
    // the accelerated iteration only ("within2_accel" = 1; null otherwise): the means of the two sweeps of a cycle, codes x nc each; one
    // record [sum Delta2 d (nc) | sum d d (nc)] per wave of the level kernel, within2_delta_blocks(n_lev2) of them; c_j [64]
    double *d_dm1 = nullptr, *d_dm2 = nullptr, *d_arec = nullptr, *d_coef = nullptr;
};
int within2_init_records(const pds_ctx* ctx, int64_t n_rows);    // records of 2 nc doubles launch_within2_init writes to d_partials
int within2_delta_blocks(const pds_ctx* ctx, int64_t n_levels2);
// the frame -> d_w0 (row-major f64) and d_moments[2 nc]: sum (x - x_0), sum (x - x_0)^2 per column, x_0 the first row's value
template <typename T>
int launch_within2_init(pds_ctx* ctx, const T* const* d_cols, int n_feat, int64_t n_rows, double* d_w0, double* d_partials, double* d_moments);
int launch_within2_row_levels(pds_ctx* ctx, const int64_t* d_off, int64_t n_levels, int64_t n_rows, uint32_t* d_g1);
int launch_within2_gather_codes(pds_ctx* ctx, const int32_t* d_in, const uint32_t* d_perm, int64_t n_rows, int32_t* d_out);
size_t within2_order_temp_bytes(int64_t n_rows);
int launch_within2_order(pds_ctx* ctx, const int32_t* d_code2, int64_t n_rows, int64_t n_codes, uint32_t* d_iota, uint32_t* d_sorted,
                         uint32_t* d_idx2, void* d_temp, size_t temp_bytes);
// one sweep: a1, a2 updated, d_delta written.  d_cols: x_0 .. x_{p-1}, y.  accel_phase 0: the plain sweep; 1 / 2: the first / second
// sweep of an accelerated cycle -- the same sweep, which also writes d_dm1 / d_dm2 and (2) the records d_arec
template <typename T>
int launch_within2_sweep(pds_ctx* ctx, const T* const* d_cols, int n_feat, const Within2Dev& d, int accel_phase = 0);
// the extrapolation that ends a cycle: c_j from d_arec into d_coef, a2 -= c_j d_dm2 over the occupied codes.  Tables only
int launch_within2_extrapolate(pds_ctx* ctx, int n_feat, const Within2Dev& d);
// the projected columns, f64, column-major in the kernels' order: d_z[c * n_rows + r]
template <typename T>
int launch_within2_final(pds_ctx* ctx, const T* const* d_cols, int n_feat, const Within2Dev& d, double* d_z);
// resid[ro] = e[r], pred[ro] = y[r] - e[r], ro = d_perm ? d_perm[r] : r; d_pred / d_resid nullable
template <typename T>
int launch_within2_rows_out(pds_ctx* ctx, const T* d_y, const double* d_e, const uint32_t* d_perm, int64_t n_rows, T* d_pred, T* d_resid);
// ---- within2_graph.hip: the graph of the occupied cells (capi_within2.hpp).  Nodes: n_a levels of factor 1, then n_b codes of factor 2;
// row r is the edge (d_u[r], n_a + d_v[r]).
// *d_flag |= 1 if a code is outside [0, n_levels): reads the codes alone.  The caller zeroes the flag and reads it back
int launch_within2_range_check(pds_ctx* ctx, const int32_t* d_codes, int64_t n_rows, int64_t n_levels, int* d_flag);
// d_start[l], l = 0 .. n_levels: the rows whose code is below l, from the ascending codes of launch_within2_order (d_sorted)
int launch_within2_level_starts(pds_ctx* ctx, const uint32_t* d_sorted, int64_t n_rows, int64_t n_levels, uint32_t* d_start);
int launch_within2_mark(pds_ctx* ctx, const uint32_t* d_u, int64_t n_rows, uint32_t* d_occ);  // d_occ[d_u[r]] = 1
size_t within2_graph_count_bytes();  // d_counts of within2_components
size_t within2_graph_flag_bytes();   // d_flags
// Hook and compress, the rounds driven from here (blocking: a few bytes come back per round).  d_label [n_a + n_b] ends as the smallest
// node index of every node's component; d_root: as much scratch.  d_occ (nullable: every level of factor 1 holds a row): the levels
// of factor 1 that hold one.  *n1 / *n2: occupied levels, *n_components: components that hold a row, *n_rounds: rounds taken, at most
// 2 ceil(log2(n_a + n_b)) + 1 -- more is PDS_ERR_NUMERIC, "component labelling did not finish".
int within2_components(pds_ctx* ctx, const uint32_t* d_u, const uint32_t* d_v, int64_t n_rows, int64_t n_a, int64_t n_b, const uint32_t* d_occ,
                       uint32_t* d_label, uint32_t* d_root, int* d_flags, int64_t* d_counts, int64_t* n1, int64_t* n2, int64_t* n_components,
                       int* n_rounds);
// d_comp1 [n_a] / d_comp2 [n_b] (nullable): the label of every level, -1 for one no row uses
int launch_within2_components_out(pds_ctx* ctx, const uint32_t* d_label, const uint32_t* d_occ, int64_t n_a, int64_t n_b, int32_t* d_comp1,
                                  int32_t* d_comp2);
// The estimated effects from the converged tables d_a1 [n_a x (p + 1)] / d_a2 [n_levels2 x (p + 1)], beta (p doubles) and the
// one-factor effects of the projected columns d_alpha1 [n_a] (include/pds_lstsq.h states the normalisation).  d_gmap (nullable): level g
// of factor 1 is entry d_gmap[g] of d_eff1 / d_comp1 and is named so in the components.  d_graw [n_levels2], d_ref [n_a]: scratch.
// Outputs nullable.
template <typename T>
int launch_within2_effects(pds_ctx* ctx, const double* d_a1, const double* d_a2, const double* d_beta, const double* d_alpha1, const uint32_t* d_label,
                           const int64_t* d_gmap, int n_feat, int64_t n_a, int64_t n_levels2, double* d_graw, uint32_t* d_ref, T* d_eff1, T* d_eff2,
                           int32_t* d_comp1, int32_t* d_comp2);
// ---- leverage_mid.hip: HC2 / HC3 leverages of 17 .. 64 f64 features on the matrix cores (PDS_ERR_UNSUPPORTED: not applicable, nothing done)
int launch_grouped_moments_stream(pds_ctx* ctx, const DeviceCols<double>& dc, int n_feat, int64_t n_frame, const int64_t* d_off, int64_t n_groups,
                                  double* d_records);  // grouped_mid.hip: grouped Gram records, 17 .. 64 f64 features, one stream
// grouped_mid.hip: grouped OLS / ridge with 17 .. 32 features as one stream, the solves in the streaming waves (no records)
template <typename T>
int launch_grouped_mid_fused(pds_ctx* ctx, const DeviceCols<T>& dc, int n_feat, int64_t n_frame, const int64_t* d_off, int64_t n_groups,
                             const SolveParams& sp, T* d_coeffs, uint8_t* d_flags, void* d_ws);
size_t grouped_mid_fused_workspace(int num_cus, int n_feat, int add_bias);
int leverage_operand(pds_ctx* ctx, const double* d_inv, int n_feat, int bias, const double** d_lop);
int launch_report_mid(pds_ctx* ctx, const DeviceCols<double>& dc, int n_feat, int bias, int64_t n_rows, const double* d_beta, const double* d_inv,
                      int hc_mode, double* d_sums, double* d_meat);  // moments_mid.hip: residuals + leverages + meat in one stream
int launch_leverage_mid(pds_ctx* ctx, const DeviceCols<double>& dc, int n_feat, int bias, int64_t n_rows, const double* d_inv, int hc_mode,
                        double* d_s_rows);

// ---- pass2.hip ----
// sum y and sum y^2 of one device column in f64 (fixed-order two-stage reduction): d_out[0..1]
template <typename T>
int launch_y_sums(pds_ctx* ctx, const T* d_y, int64_t n_rows, double* d_out, bool shifted = false /* sums of y - y[0] */);
// streaming residual pass: pred/resid (nullable outputs), sums: [0]=sum e^2, [1]=sum w e^2,
// meat (p' x p') = sum s_i x_i x_i' with s_i = e_i^2 * hc_scale(h_ii) when meat != null.
template <typename T>
int launch_pass2(pds_ctx* ctx, const DeviceCols<T>& dc, int n_feat, int64_t n_rows, int add_bias,
                 bool weighted, const T* d_beta, const T* d_inv /*nullable, for HC2/3*/, int hc_mode,
                 T* d_pred, T* d_resid, double* d_sums /*[2]*/, double* d_meat /*p'*p' or null*/,
                 // p <= 16: also sum (y - y[0]), sum (y - y[0])^2 -> d_ysums[0..1] (the report's derived var(y), from the rows this pass reads anyway)
                 double* d_ysums = nullptr);

// ---- nulls.hip ----
template <typename T>
struct NullPrepared {
    std::vector<const T*> cols;  // device pointers, reference order [y, x1..xp]
    int64_t n_kept = 0;
    bool dropped = false;         // rows were removed -> d_keep / d_rank are valid
    uint8_t* d_keep = nullptr;
    int64_t* d_rank = nullptr;
};
template <typename T>
int apply_null_policy(pds_ctx* ctx, const std::vector<const T*>& cols_dev, const std::vector<const uint8_t*>& bm_dev,
                      const std::vector<int64_t>& bit_off, int64_t n_rows, int policy, T fill_value,
                      NullPrepared<T>& out);
template <typename T>
int expand_rows(pds_ctx* ctx, const T* d_compact, const uint8_t* d_keep, const int64_t* d_rank, int64_t n_rows, T* d_out,
                uint8_t* d_valid);
size_t null_policy_workspace(int n_cols, int64_t n_rows, size_t elem);
int remap_group_offsets(pds_ctx* ctx, const int64_t* d_off, int64_t n_groups, const int64_t* d_rank, int64_t n_rows,
                        int64_t n_kept, int64_t* d_out);

// ---- rolling.hip ----
template <typename T>
int launch_rolling(pds_ctx* ctx, const DeviceCols<T>& dc, int n_feat, int64_t n_rows, int add_bias,
                   int64_t window, int64_t min_size, double lambda, bool expanding, const double* seed_moments,
                   T* d_coeffs, T* d_pred, uint8_t* d_valid);
// grouped fits: segmented sums over the groups [d_off[g], d_off[g+1]) (device offsets, ng + 1 entries, already validated);
// 1 .. 64 coefficients; workspace comes out of ctx->ws
template <typename T>
int launch_rolling_grouped(pds_ctx* ctx, const DeviceCols<T>& dc, int n_feat, int64_t n_rows, int add_bias, int64_t window,
                           int64_t min_size, double lambda, bool expanding, const int64_t* d_off, int64_t ng, T* d_coeffs, T* d_pred,
                           uint8_t* d_valid);
// rolling.hip: the grouped outputs of a group-contiguous frame back to frame order (row i -> perm[i])
template <typename T>
int launch_rolling_scatter(pds_ctx* ctx, const T* d_co, const T* d_pr, const uint8_t* d_va, const uint32_t* d_perm, int64_t n, int pp,
                           T* coeffs, T* pred, uint8_t* valid);

// rolling_wide.hip: 13 .. 64 coefficients (per-row moment records + launch_solve); workspace comes out of ctx->ws.
// d_off / ng: the segmented (grouped) form, used from 9 coefficients on
template <typename T>
int launch_rolling_wide(pds_ctx* ctx, const DeviceCols<T>& dc, int n_feat, int64_t n_rows, int add_bias, int64_t window,
                        int64_t min_size, double lambda, bool expanding, const double* seed_moments, T* d_coeffs, T* d_pred,
                        uint8_t* d_valid, const int64_t* d_off = nullptr, int64_t ng = 0);
size_t rolling_wide_workspace(int n_feat, int64_t n_rows, size_t elem);

// ---- keyed.hip: int64 keys in any row order -> sorted keys, permutation, distinct keys, group offsets
int keys_nondecreasing(pds_ctx* ctx, const int64_t* d_keys, int64_t n, unsigned* d_flag, bool* sorted);
size_t keyed_temp_bytes(int64_t n);
size_t keyed_ordered_temp_bytes(int64_t n);
constexpr int kKeySlots = 8192;  // slots of the histogram the order check can take along (keyed.hip / keyed_partition.hip)
int keys_order_minmax(pds_ctx* ctx, const int64_t* d_keys, int64_t n, int64_t* d_state /* 8 slots */, bool* sorted, int64_t* mm,
                      uint32_t* d_run_counts = nullptr /* key_run_slots(n) entries: see keyed_runs_ordered */,
                      unsigned long long* d_run_masks = nullptr /* key_run_mask_bytes(n) */, int64_t* n_runs = nullptr, int hist_shift = -1,
                      unsigned* d_slot_counts = nullptr /* kKeySlots x 8 */, bool* hist_taken = nullptr);
size_t key_run_slots(int64_t n);
size_t key_run_mask_bytes(int64_t n);
int keyed_runs_ordered(pds_ctx* ctx, const int64_t* d_keys, int64_t n, uint32_t* d_counts, uint32_t* d_prefix, const unsigned long long* d_masks,
                       int64_t cap, int64_t* d_unique, int64_t* d_offsets, void* d_temp, size_t temp_bytes);
int keyed_minmax(pds_ctx* ctx, const int64_t* d_keys, int64_t n, void* d_temp, size_t temp_bytes, int64_t* d_minmax, int64_t* mm);
int keyed_sort(pds_ctx* ctx, const int64_t* d_keys, int64_t n, uint32_t* d_idx_in, int64_t* d_sorted_keys, uint32_t* d_perm,
               void* d_temp, size_t temp_bytes, int64_t* d_scratch_keys, const int64_t* d_minmax, const int64_t* mm);
// ---- keyed_partition.hip: grouped moments of a frame in any row order without sorting its rows (dense integer keys)
struct KeyedPartitionState {
    double* table = nullptr;   // [ids][nvp]: upper triangle of Z'Z, Z = [x_0..x_{pc-1}, 1, y], per dense id
    unsigned* ids = nullptr;   // dense id of group r (ascending)
    unsigned* rank = nullptr;  // group of dense id i (valid where the id has rows)
    int pc = 0, nvp = 0;
};
template <typename T>
int64_t keyed_partition_buckets(int n_feat, int64_t n_rows, uint64_t range);  // 0: not applicable (the sorting route)
template <typename T>
size_t keyed_partition_workspace(int n_feat, int64_t n_rows, int64_t n_buckets);
template <typename T>
int keyed_partition_shift(int n_feat);  // log2 of the bucket width (ids per bucket)
template <typename T>
int keyed_partition_build(pds_ctx* ctx, const T* const* d_cols, const int64_t* d_keys, const int64_t* d_kmin /* base: see keyed_partition.hip */,
                          uint64_t range, int n_feat, int64_t n_rows, int64_t n_buckets, char* ws, int64_t max_groups, int64_t* d_out_keys,
                          int64_t* d_offsets, int64_t* n_groups, KeyedPartitionState& st, const unsigned* d_slot_counts = nullptr,
                          unsigned first_slot = 0, int phases = 3 /* 1: the moment table of these rows; 2: the group list from the table */,
                          int64_t n_rows_total = 0 /* rows behind the table when it sums several slices */);
int keyed_partition_add_table(pds_ctx* ctx, const KeyedPartitionState& st, int64_t n_ids, const double* d_other);  // st.table += other
template <typename T>
int64_t keyed_partition_table_ids(int n_feat, int64_t n_buckets);  // rows of the id-indexed table (st.nvp doubles each)
template <typename T>
int keyed_partition_records(pds_ctx* ctx, const KeyedPartitionState& st, int n_feat, int64_t g0, int64_t gc, T* d_records);
int keyed_runs(pds_ctx* ctx, const int64_t* d_sorted_keys, int64_t n, int64_t* d_unique, int64_t* d_counts, int64_t* d_offsets,
               int64_t* d_nruns, void* d_temp, size_t temp_bytes, int64_t* n_groups);
template <typename T>
int launch_gather_rows(pds_ctx* ctx, const T* d_src, const uint32_t* d_perm, int64_t n, T* d_dst);
// layout.hip: rows [0, n_rows) of a row-major device matrix (row stride ld) -> out[c * col_stride + out_row0 + r]
template <typename T>
int launch_rows_to_cols(pds_ctx* ctx, const T* d_X, int64_t ld, int64_t n_rows, int n_cols, T* d_out, int64_t col_stride, int64_t out_row0);
// keyed.hip: the whole frame through the permutation by way of row-major records (one random access per row, not per element)
template <typename T>
int launch_gather_frame(pds_ctx* ctx, const T* const* d_src, const uint32_t* d_perm, int nc, int64_t n, T* d_records, T* const* d_dst);
// the transposition tile of launch_gather_frame (256 rows x nc columns) must fit the 64 KB of LDS a launch gets without raising
// the kernel's dynamic limit; wider frames take the column-by-column gather (launch_gather_rows), which has no width limit
constexpr size_t kGatherFrameLdsLimit = 64 * 1024;
template <typename T>
inline bool gather_frame_fits(int nc) { return (size_t)256 * (size_t)(nc | 1) * sizeof(T) <= kGatherFrameLdsLimit; }
template <typename T>
int launch_scale_sqrt_w(pds_ctx* ctx, const T* d_src /*nullable: ones*/, const T* d_w, int64_t n, T* d_dst);

// ---- stats.cpp ----
double student_t_sf(double x, double df, bool* err);
double student_t_sf_wide(double x, double df, bool* err);  // the same tail with a cancellation-free prefactor (capi_within.hpp)
double student_t_ppf(double q, double df);

}  // namespace pds
