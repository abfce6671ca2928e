/*
 * include/pds_lstsq.h -- C ABI of libpds_lstsq_hip.so, the MI355X (gfx950) implementation of the
 * polars_ds least-squares expression path.
 *
 * This is the drop-in boundary: the entry points are what the reference's Rust plugin functions
 * (`#[polars_expr] fn pl_lr / pl_lr_pred / pl_lin_reg_report / pl_rolling_lr / pl_recursive_lr`,
 * /root/reference/src/num_ext/linear_regression.rs:419,704,822,1121,1206 and the *_f32 twins in
 * linear_regression_f32.rs) would bind over `extern "C"` after unwrapping the Arrow column buffers.
 * They replace the calls those functions make into src/linear/lr/lr_solvers.rs and
 * src/linear/online_lr/lr_online_solvers.rs; pds_glm_irls_* and pds_mixed_reml_* stand behind the pyclasses PyGLM and
 * PyMixedModel (src/linear/glm/glm_solvers.rs, src/linear/mixed/mod.rs); pds_glm_enet_* are their elastic-net penalised fits
 * (l1_reg / l2_reg of the reference's logistic_reg, expr_linear.py:277-353, for every family, per model and per group).  INTEGRATION.md shows the Rust-side binding.
 *
 * Conventions
 *   - plain pointers and sizes only; no torch / HIP types in any signature.
 *   - `cols` is an array (in HOST memory) of n_feat + 1 column pointers in the reference's input
 *     order [y, x1, ..., xp] (expr_linear.py:250-258; weighted variants take `weights` separately).
 *     Each column is a contiguous buffer of n_rows values, exactly an Arrow Float64/Float32 values
 *     buffer.  `space` says where the column *buffers* live (PDS_DEVICE: already resident in HBM; PDS_HOST: host
 *     memory, copied to HBM by the library -- frames of more than one chunk (256 MiB, pds_set_host_staging) cross
 *     PCIe one row range at a time into a chunk-sized staging buffer for pds_lr_* / pds_moments_* (p <= 16), so HBM use
 *     is O(chunk) and the frame may be larger than HBM; the other entry points stage the whole frame).
 *   - output buffers are host memory unless the parameter is documented "space-resident".
 *   - every function returns PDS_OK (0) or a negative pds_status; pds_last_error() returns the
 *     message (thread-local), with the reference's error strings where the reference has one.
 *   - all launches go to the stream of the context (pds_ctx_set_stream); calls are synchronous with
 *     respect to the host on return (results are ready), except the *_async moment builders and the
 *     stream-ordered return described next.
 *   - Synchronisation.  pds_lr_grouped_f64 / _f32 may return STREAM-ORDERED: all of the call's work is queued on the context's
 *     stream and the function returns without waiting for it, as a stream-taking library does.  Whatever the caller queues on that
 *     stream afterwards -- a kernel that reads `coeffs`, a copy to the host, the next pds_* call -- runs behind it; a host read
 *     of the outputs needs pds_ctx_synchronize (or the caller's own synchronisation of the stream) first, and the inputs must
 *     stay alive and unchanged until then.  This happens only when ALL of the following hold, and every other call blocks as
 *     before:
 *       . the context's stream was handed in with pds_ctx_set_stream (a context on its private stream always blocks: nobody
 *         else can order work behind that stream);
 *       . space == PDS_DEVICE and `coeffs` is given (every input and output in device space);
 *       . OLS / ridge with the rank gate on and up to 16 features, i.e. the fused kernel's route, with solver "qr" and at most
 *         16 coefficients, or solver "choleskey" ("svd" runs on host threads; 16 features with an intercept re-solve their
 *         marked groups on a solver the host drives);
 *       . the timing hooks (pds_ctx_set_timing) are off and context option "blocking_return" is 0.
 *     The results are the same bits either way.  One context serves one stream at a time: pds_ctx_set_stream waits for the
 *     old stream first.
 *   - f64 symbols end in _f64, the f32 twins in _f32 (LIN_REG_EXPR_F64=False path, config.py:15-16).
 */
#ifndef PDS_LSTSQ_H
#define PDS_LSTSQ_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pds_ctx pds_ctx; /* opaque: device, stream, HBM workspace, pinned staging */

typedef enum { PDS_HOST = 0, PDS_DEVICE = 1 } pds_space;

typedef enum {
    PDS_OK = 0,
    PDS_ERR_INVALID = -1,     /* bad argument */
    PDS_ERR_EMPTY = -2,       /* "Empty data"                       linear_regression.rs:167 */
    PDS_ERR_TOO_FEW_ROWS = -3, /* "#Data < #features. No conclusive result."          :170-172 */
    PDS_ERR_HIP = -4,         /* HIP runtime failure / no gfx950 device */
    PDS_ERR_UNSUPPORTED = -5,
    PDS_ERR_NUMERIC = -6,     /* e.g. "SVD failed."                 lr_solvers.rs:256 */
    PDS_ERR_NULLS = -7        /* "Nulls found in data"              linear_regression.rs:198 */
} pds_status;

/* NullPolicy (src/linear/mod.rs:34-66) as the plugin functions use it for pl_lr / pl_lr_pred:
 * "raise" | "skip" | "zero"/"one"/numeric string -> FILL(value) | "ignore". */
typedef enum { PDS_NULL_RAISE = 0, PDS_NULL_SKIP = 1, PDS_NULL_FILL = 2, PDS_NULL_IGNORE = 3 } pds_null_policy;

/* LRSolverMethods::from(&str): "qr" (default, also any unknown string), "svd", "choleskey"
 * (src/linear/lr/mod.rs:17-26 -- the misspelling is the reference's). */
typedef enum { PDS_SOLVER_QR = 0, PDS_SOLVER_SVD = 1, PDS_SOLVER_CHOLESKEY = 2 } pds_solver;

/* StandardError::from(String): linear_regression.rs:113-132 */
typedef enum {
    PDS_SE = 0,
    PDS_HC0 = 1,
    PDS_HC1 = 2,
    PDS_HC2 = 3,
    PDS_HC3 = 4,
    /* cluster-robust, pds_lin_reg_report_cluster_* only (every other entry point answers PDS_ERR_INVALID): */
    PDS_CLUSTER = 5, /* CR1: G / (G - 1) * (n - 1) / (n - p') */
    PDS_CLUSTER0 = 6 /* CR0: no small-sample factor */
} pds_se_type;
/* OR-ed into the se_type argument of pds_lin_reg_report_* (unweighted form): ignore `y_var` and take the target's sample
 * variance (ddof = 1) from the call's own pass over y (sums kept in f64 for both precisions).  Without the flag `y_var` is
 * used as given -- a NaN (what a null `target.var()` becomes, linear_regression.rs:836) propagates into r2 / adj_r2. */
#define PDS_REPORT_DERIVE_YVAR 0x100

/* ---- library / context ------------------------------------------------------------------- */
const char* pds_last_error(void);
const char* pds_version(void);
/* Creates a context on HIP device `device` (must be gfx950).  */
int pds_ctx_create(int device, pds_ctx** out);
void pds_ctx_destroy(pds_ctx* ctx);
/* Use an existing hipStream_t (passed as void*) for all work of this context instead of the private
 * non-blocking stream created with the context.  NULL selects HIP's default (null) stream. */
int pds_ctx_set_stream(pds_ctx* ctx, void* hip_stream);
int pds_ctx_synchronize(pds_ctx* ctx);
/* Number of compute units of the context's device (256 on MI355X). */
int pds_ctx_num_cus(const pds_ctx* ctx);
/* Behaviour switches of a context; the defaults are read from the environment ONCE, when the context is created:
 *   "keyed_sort"      (PDS_KEYED_SORT=1)      pds_lr_by_key_*: unordered keys always take the sorting route -- the determinism switch: the
 *                                             partition route appends records through cursor atomics, so its sums repeat to rounding only;
 *   "wide_f32_native" (PDS_WIDE_F32_NATIVE=1) f32 Gram builds beyond 64 features on the f32 matrix instructions (v_mfma_f32_32x32x2_f32,
 *                                             2.5e-7 from the f64 Gram) instead of three exact bf16 planes on the bf16 matrix cores (2e-6).
 *   "report_chunk_groups"                     pds_lin_reg_report_grouped_* / _by_key_*, pds_wls_report_*: groups per pass (<= 0: the default).
 *   "glm_split_rows"                          pds_glm_irls_grouped_* / _by_key_*: groups of more rows are fitted by the full-device
 *                                             iteration, one by one (<= 0: the default, 16384; at least 64).
 *   "mixed_split_rows"                        pds_mixed_*: groups of more rows are cut into row chunks that are separate work items
 *                                             (<= 0: the default, 16384; at least 64).
 *   "cluster_split_rows"                      pds_lin_reg_report_cluster_*: clusters of more rows are cut into row chunks that are separate
 *                                             work items (<= 0: the default, 16384; at least 64).
 *   "within_split_rows"                       pds_lin_reg_within_*: absorbed groups of more rows are cut into row chunks that are separate
 *                                             work items, in the statistics pass and in the per-row pass alike (<= 0: the default,
 *                                             16384; at least 64).  Few, very long groups are the common fixed-effects shape.
 *   "within2_accel"                           pds_lin_reg_within2_* (the _fx_ forms included): 0 plain alternating sweeps, the default;
 *                                             1 Irons-Tuck cycles of two sweeps and one extrapolation (see there).  Any other value is
 *                                             PDS_ERR_INVALID.  A call reads the option once, when it starts.
 *   "cluster_waves"                           pds_lin_reg_report_cluster_*: cap on the number of waves a launch of the cluster pass starts
 *                                             (<= 0: the default, 12 per compute unit).  Each wave adds up the clusters it walks, so
 *                                             another cap gives other sums, to rounding; one setting repeats its bits.
 *   "grouped_fused_waves"                     pds_lr_grouped_* / pds_lr_by_key_* up to 16 features: cap on the number of waves the fused
 *                                             kernel starts (<= 0: the default, every wave slot of the device).
 *   "grouped_fused_late_permille"             the same kernel: share of the frame's rows, in 1/1000, dealt to the second half of its
 *                                             waves (1 .. 999; 0: the default -- equal shares unless the grid fills the device, see
 *                                             pds_grouped_fused_split).  Neither option changes a result bit: which wave fits a group
 *                                             does not enter the group's arithmetic.
 *   "grouped_multi_route" / "grouped_multi_waves"  pds_lr_multi_grouped_* / pds_lr_multi_by_key_*: see there (0 / 1 / 2; a count).
 *   "blocking_return"                         1: every call synchronises before it returns, also the ones that may return
 *                                             stream-ordered (see "Synchronisation" at the top); 0, the default: they may.  Setting
 *                                             it waits for the stream.  For tests, A/B runs and callers that read results from the host
 *                                             right away.
 *   "rolling_waves"                           pds_rolling_lr_* / pds_recursive_lr_* and their grouped forms, up to 12 coefficients (up to 8
 *                                             when grouped): cap on the number of waves any launch of the tiled kernels starts (<= 0: the
 *                                             default grid; two-wave blocks round down to whole blocks, at least one).  A wave then walks
 *                                             several tiles of a small frame.  The option changes no result bit: a tile's anchor and
 *                                             arithmetic do not depend on which wave walks it.  The per-segment kernels of wider fits
 *                                             have no tile loop and do not take it.
 * value: 0 / 1 (within2_accel: nothing else; report_chunk_groups, glm_split_rows, mixed_split_rows, cluster_split_rows, within_split_rows, cluster_waves, grouped_fused_waves, rolling_waves: a count).  Unknown names are PDS_ERR_INVALID. */
int pds_ctx_set_option(pds_ctx* ctx, const char* name, long long value);
/* The value an option has now, as pds_ctx_set_option stored it (a count given as <= 0 reads back as 0, "the default").  Unknown names
 * are PDS_ERR_INVALID.  A caller that sets an option for one call reads it first and puts that value back. */
int pds_ctx_get_option(const pds_ctx* ctx, const char* name, long long* value);
/* Host restatement of how the fused grouped kernel deals groups to its waves (no device needed): wave w of `waves` fits the groups
 * [first_group[w], end_group[w]) -- those whose first row lies in the wave's share of the row range [group_offsets[0],
 * group_offsets[n_groups]).  late_permille = 0: equal shares of the rows; 1 .. 999: that share of the rows goes to the second half of
 * the waves (a device-filling launch uses an unequal share because the second wave of a SIMD advances more slowly beside the first).
 * The ranges are in order and partition [0, n_groups) for every setting.  first_group / end_group: `waves` values each, host memory. */
int pds_grouped_fused_split(const int64_t* group_offsets, int64_t n_groups, int waves, int late_permille, int64_t* first_group,
                            int64_t* end_group);
/* Host-frame staging (process wide): chunk_mb = bytes of one row chunk of a PDS_HOST frame (default 256, env
 * PDS_HOST_CHUNK_MB); resident_max_mb = largest host frame that pds_lr_pred_* still stages whole (one PCIe trip; larger
 * frames make two chunked trips; default 98304, env PDS_HOST_RESIDENT_MAX_MB).  A value <= 0 leaves the setting as is.
 * Replaces the reference's one-Vec marshalling copy, src/utils/mod.rs:101-206. */
int pds_set_host_staging(double chunk_mb, double resident_max_mb);

/* Diagnostics: how many call-local workspace slices had to be allocated outside the per-call reservation since the context
 * was created (0 unless an entry point under-estimated its bound; the slices are still valid, never out of bounds). */
long long pds_ctx_workspace_spills(const pds_ctx* ctx);
/* Bytes the context currently holds in one of its grow-only HBM workspaces: which = 0 call-local scratch, 1 host-frame staging,
 * 2 solver / key-order scratch, 3 the keyed-grouping workspace (pds_lr_by_key_*), 4 the weighted grouped frame.  -1 on a bad argument.
 * Lets a host size its frames against what a route reserves (the partition route of unordered keys must not reserve the sort
 * route's buffers: tests/test_gpu_parity.py). */
long long pds_ctx_workspace_bytes(const pds_ctx* ctx, int which);
/*
 * Measurement hooks (bench.py): with timing enabled every kernel class is bracketed by a HIP event
 * pair recorded on the context's stream.  pds_ctx_get_timing synchronises and returns, per class,
 * the summed duration in ms and the number of bracketed launches.  Classes: 0 Gram/moments (single
 * system, incl. its finalize), 1 grouped Gram, 2 batched solve, 3 residual pass, 4 rolling, 5 CD/NNLS,
 * 6 / 7 the factor-1 / factor-2 kernels of a sweep of pds_lin_reg_within2_*, 8 its graph pass (level counts, components, effects).
 */
int pds_ctx_set_timing(pds_ctx* ctx, int enable);
int pds_ctx_get_timing(pds_ctx* ctx, double* ms_sum, long long* counts, int n_kinds, int reset);
/* The individual bracketed durations (ms) of one class, oldest first, at most `cap` (the newest are kept, up to 4096 per
 * class): returns how many were written, -1 on a bad argument.  bench.py reports min / median / max of the timed launches. */
int pds_ctx_get_timing_samples(pds_ctx* ctx, int kind, double* ms_out, int cap, int reset);

/* ---- LRKwargs mirror (linear_regression.rs:27-45), minus the strings parsed by the host ---- */
typedef struct {
    int add_bias;          /* kwargs.bias */
    double l1_reg;         /* kwargs.l1_reg */
    double l2_reg;         /* kwargs.l2_reg */
    double tol;            /* kwargs.tol (CD / NNLS convergence; rcond for pds_lr_rcond) */
    int solver;            /* pds_solver, from kwargs.solver.  Grouped fits with PDS_SOLVER_SVD and the rank gate on: the systems a
                            * chunk marks next to the gate go through a host SVD (the reference's thin_svd gate, lr_solvers.rs:358-366)
                            * while the marked set costs no more than 2048 systems of 66 x 66 (5.6e5 systems at 8 features); a larger
                            * set takes the device pivoted QR -- same gate statistic, beta from QR instead of the SVD. */
    int positive;          /* kwargs.positive */
    int max_iter;          /* kwargs.max_iter (the f32 twin ignores it: 2000 CD; NNLS 200 in pl_lr_f32, 2000 in pl_lr_pred_f32) */
    double singular_x_tol; /* kwargs.singular_x_tol: > 0 enables the log-det rank gate */
} pds_lr_params;

/*
 * pds_lr_*: the compute part of `pl_lr` (linear_regression.rs:419-513; f32: linear_regression_f32.rs
 * :289-384) on null-free columns: dispatch on (LRMethods::from((l1,l2)), positive) exactly as
 * :447-497, i.e. faer_solve_lr_gated / faer_solve_lr / faer_nn_lr / faer_coordinate_descent, or
 * faer_weighted_lr when `weights` != NULL (lr_solvers.rs:386-409).
 *   coeffs   out, n_feat + add_bias values (bias last).
 *   is_null  out, 1 when the rank gate fired (the reference returns a 1-row null list,
 *            linear_regression.rs:462-468); coeffs is then filled with NaN.
 */
int pds_lr_f64(pds_ctx* ctx, const double* const* cols, const double* weights, int n_feat,
               int64_t n_rows, pds_space space, const pds_lr_params* prm, double* coeffs,
               int* is_null);
int pds_lr_f32(pds_ctx* ctx, const float* const* cols, const float* weights, int n_feat,
               int64_t n_rows, pds_space space, const pds_lr_params* prm, float* coeffs,
               int* is_null);

/*
 * pds_lr_pred_*: `pl_lr_pred` (linear_regression.rs:704-820): same fit, then pred = X b and
 * resid = y - pred for every row.  pred/resid are `space`-resident buffers of n_rows values.
 */
int pds_lr_pred_f64(pds_ctx* ctx, const double* const* cols, const double* weights, int n_feat,
                    int64_t n_rows, pds_space space, const pds_lr_params* prm, double* coeffs,
                    int* is_null, double* pred, double* resid);
int pds_lr_pred_f32(pds_ctx* ctx, const float* const* cols, const float* weights, int n_feat,
                    int64_t n_rows, pds_space space, const pds_lr_params* prm, float* coeffs,
                    int* is_null, float* pred, float* resid);

/*
 * pds_elastic_net_*: ElasticNet::fit_unchecked of the model-class route (src/linear/lr/lr_solvers.rs:139-164, reached from
 * PyElasticNet.fit src/pymodels/py_lr.rs:112): ALWAYS faer_coordinate_descent with (l1_reg, l2_reg, add_bias, tol, max_iter,
 * positive = false) -- also when l1_reg <= 0, where `pl_lr`'s dispatch would take the closed-form ridge instead (the two
 * differ: coordinate descent penalises with n_rows * l2_reg, :478-480).  max_iter is honoured in both precisions (the 2000
 * of the f32 expression twin is the plugin function's, not the solver's).  Only an empty frame is rejected (lr/mod.rs:114-125).
 */
int pds_elastic_net_f64(pds_ctx* ctx, const double* const* cols, int n_feat, int64_t n_rows, pds_space space,
                        const pds_lr_params* prm, double* coeffs);
int pds_elastic_net_f32(pds_ctx* ctx, const float* const* cols, int n_feat, int64_t n_rows, pds_space space,
                        const pds_lr_params* prm, float* coeffs);

/*
 * pds_lr_nullable_*: `pl_lr` / `pl_lr_pred` on columns that carry Arrow validity bitmaps, i.e. the null handling of
 * series_to_mat_for_lr (linear_regression.rs:151-267) done on the device (stream compaction / fill), then the same
 * fit.  validity[c] is the validity bitmap of cols[c] (LSB-first, one bit per row, NULL = column has no nulls),
 * bit_offsets[c] the Arrow array offset into it; both in the same memory space as the column buffers.
 *   pred / resid / row_valid  optional (all NULL = coefficients only), n_rows entries, `space`-resident.  Dropped rows
 *                             get NaN and row_valid = 0 -- the null re-expansion of linear_regression.rs:790-812.
 *   n_used                    out, rows that took part in the fit.
 * Errors: PDS_ERR_NULLS ("Nulls found in data") under PDS_NULL_RAISE; PDS_ERR_EMPTY / PDS_ERR_TOO_FEW_ROWS are
 * judged on the rows that survive the policy, like the reference (:250-254).
 */
int pds_lr_nullable_f64(pds_ctx* ctx, const double* const* cols, const uint8_t* const* validity,
                        const int64_t* bit_offsets, int n_feat, int64_t n_rows, pds_space space, int null_policy,
                        double fill_value, const pds_lr_params* prm, double* coeffs, int* is_null, double* pred,
                        double* resid, uint8_t* row_valid, int64_t* n_used);
int pds_lr_nullable_f32(pds_ctx* ctx, const float* const* cols, const uint8_t* const* validity,
                        const int64_t* bit_offsets, int n_feat, int64_t n_rows, pds_space space, int null_policy,
                        float fill_value, const pds_lr_params* prm, float* coeffs, int* is_null, float* pred,
                        float* resid, uint8_t* row_valid, int64_t* n_used);

/*
 * pds_lr_multi_*: `pl_lr_multi` / `pl_lr_multi_pred` (linear_regression.rs:517-649): k targets share one design
 * matrix.  cols = [t_0 .. t_{k-1}, x_1 .. x_p] (the expression's input order, MultiLRKwargs.last_target_idx = k).
 * OLS / ridge only; the rank gate depends on X alone, so either every target gets coefficients or none does.
 * One pass over the data builds X'X and all k X't_i together (the extra targets ride in the Gram tile).
 *   coeffs  out, k x (n_feat + add_bias), row-major (target i's coefficients contiguous).
 *   pred / resid  optional, k x n_rows row-major, `space`-resident ("{target}_pred" / "{target}_resid" fields).
 */
int pds_lr_multi_f64(pds_ctx* ctx, const double* const* cols, int n_targets, int n_feat, int64_t n_rows,
                     pds_space space, int add_bias, double l2_reg, int solver, double singular_x_tol, double* coeffs,
                     int* is_null, double* pred, double* resid);
int pds_lr_multi_f32(pds_ctx* ctx, const float* const* cols, int n_targets, int n_feat, int64_t n_rows,
                     pds_space space, int add_bias, float l2_reg, int solver, float singular_x_tol, float* coeffs,
                     int* is_null, float* pred, float* resid);

/*
 * pds_lr_rcond_*: `pl_lr_w_rcond` -> faer_solve_lr_rcond (lr_solvers.rs:216-258).
 * rcond is max(kwargs.tol, eps * max(n, p')) as computed by the caller (linear_regression.rs:651-702).
 */
int pds_lr_rcond_f64(pds_ctx* ctx, const double* const* cols, int n_feat, int64_t n_rows,
                     pds_space space, int add_bias, double l2_reg, double rcond, double* coeffs,
                     double* singular_values);
/* pl_lr_w_rcond_f32 (linear_regression_f32.rs:515-566): rcond = max(tol as f32, f32::EPSILON * max(n, p')). */
int pds_lr_rcond_f32(pds_ctx* ctx, const float* const* cols, int n_feat, int64_t n_rows,
                     pds_space space, int add_bias, float l2_reg, float rcond, float* coeffs,
                     float* singular_values);

/*
 * pds_lin_reg_report_*: the arithmetic of `pl_lin_reg_report` (linear_regression.rs:822-980) and, with
 * weights != NULL, `pl_wls_report` (:982-1117).  y_var is inputs[0][0] of the expression
 * (`target.var()`, ddof = 1, computed by Polars; expr_linear.py:614-617); with se_type | PDS_REPORT_DERIVE_YVAR (unweighted
 * form) the library computes it itself (sum y and sum y^2 in f64 from the rows the report works on).  Each output has
 * n_feat + add_bias entries; r2 / adj_r2 are scalars (the reference broadcasts them).
 */
typedef struct {
    double* beta;
    double* std_err;
    double* t;
    double* p;
    double* ci_lower; /* "0.025" */
    double* ci_upper; /* "0.975" */
    double r2;
    double adj_r2;
} pds_report_f64;
typedef struct {
    float* beta;
    float* std_err;
    float* t;
    float* p;
    float* ci_lower;
    float* ci_upper;
    float r2;
    float adj_r2;
} pds_report_f32;
int pds_lin_reg_report_f64(pds_ctx* ctx, const double* const* cols, const double* weights,
                           int n_feat, int64_t n_rows, pds_space space, int add_bias, int se_type,
                           double y_var, pds_report_f64* out);
int pds_lin_reg_report_f32(pds_ctx* ctx, const float* const* cols, const float* weights,
                           int n_feat, int64_t n_rows, pds_space space, int add_bias, int se_type,
                           float y_var, pds_report_f32* out);

/*
 * pds_lin_reg_report_cluster_*: ONE model over the whole frame with cluster-robust standard errors (Stata's vce(cluster id),
 * statsmodels' cov_type="cluster", R's vcovCL): V = c inv M inv, M = sum_g s_g s_g', s_g = X_g' e_g the score of cluster g.
 * se_type: PDS_CLUSTER (CR1, c = G / (G - 1) * (n - 1) / (n - p')) or PDS_CLUSTER0 (CR0, c = 1), optionally | PDS_REPORT_DERIVE_YVAR;
 * G counts the NON-EMPTY clusters.  t, p and the 95 % interval use the Student t with G - 1 degrees of freedom; beta, r2 and adj_r2
 * are those of pds_lin_reg_report_*.  The report is two streams over the frame: the moment pass, and one pass that forms residuals,
 * sum e^2 and the meat together.  f32 frames: moments and solve as in pds_lin_reg_report_f32, the cluster pass in f64 arithmetic.
 *   grouped: cluster g = rows [cluster_offsets[g], cluster_offsets[g+1]); n_clusters + 1 int64 values, `space`-resident, starting at
 *            0, ending at n_rows, non-decreasing (else PDS_ERR_INVALID).  Empty clusters contribute nothing and change no output bit.
 *   by key:  keys = n_rows int64 values in any row order, `space`-resident; rows with equal keys form a cluster (ordered keys move
 *            nothing; otherwise the stable sort + gather of the other by-key entry points).  *n_clusters receives G.
 * Two calls give the same bits (no floating-point atomics).  Errors: 1 .. 16 feature columns (more: PDS_ERR_UNSUPPORTED); G < 2 is
 * PDS_ERR_INVALID, n_rows <= p' PDS_ERR_TOO_FEW_ROWS -- refused, not approximated.  There is no weighted form.
 */
int pds_lin_reg_report_cluster_grouped_f64(pds_ctx* ctx, const double* const* cols, int n_feat, int64_t n_rows, const int64_t* cluster_offsets,
                                           int64_t n_clusters, pds_space space, int add_bias, int se_type, double y_var, pds_report_f64* out);
int pds_lin_reg_report_cluster_grouped_f32(pds_ctx* ctx, const float* const* cols, int n_feat, int64_t n_rows, const int64_t* cluster_offsets,
                                           int64_t n_clusters, pds_space space, int add_bias, int se_type, float y_var, pds_report_f32* out);
int pds_lin_reg_report_cluster_by_key_f64(pds_ctx* ctx, const double* const* cols, const int64_t* keys, int n_feat, int64_t n_rows,
                                          pds_space space, int add_bias, int se_type, double y_var, pds_report_f64* out, int64_t* n_clusters);
int pds_lin_reg_report_cluster_by_key_f32(pds_ctx* ctx, const float* const* cols, const int64_t* keys, int n_feat, int64_t n_rows,
                                          pds_space space, int add_bias, int se_type, float y_var, pds_report_f32* out, int64_t* n_clusters);

/*
 * pds_lin_reg_within_*: fixed-effects regression -- ONE model with an intercept per group, y_i = alpha_g(i) + x_i' beta + e_i, the
 * within estimator; no dummy column is ever formed.  cols = [y, x1..xp], 1 .. 16 feature columns and NO intercept column (it is
 * absorbed).  What follows is a DEFINITION of what the library computes; no equivalence with the small-sample conventions of any
 * package is claimed.  n rows, G non-empty groups, p features, m_g the mean of [x, y] over group g,
 * W = sum_g sum_{i in g} ([x_i, y_i] - m_g)([x_i, y_i] - m_g)':
 *   beta solves W_xx beta = W_xy;  alpha_g = m_y,g - m_g' beta;  e_i = y_i - alpha_g - x_i' beta;  pred_i = y_i - e_i.
 *   se_type PDS_SE:       V = s2 W_xx^-1, s2 = sum e^2 / (n - G - p); t, p and the 95 % interval use the Student t with n - G - p
 *                         degrees of freedom.
 *   se_type PDS_CLUSTER0: V = W_xx^-1 M W_xx^-1, M = sum_g s_g s_g', s_g = sum_{i in g} (x_i - m_g) e_i: the clusters are the absorbed
 *                         groups.
 *   se_type PDS_CLUSTER:  the same V times c = G / (G - 1) * (n - 1) / (n - p - 1): the absorbed effects, nested in the clusters, are
 *                         not counted among the parameters, the one intercept is.  Both cluster forms use G - 1 degrees of freedom.
 *   out->r2 = 1 - sum e^2 / W_yy (the within R^2), out->adj_r2 = 1 - (1 - r2)(n - G) / (n - G - p),
 *   extra->r2_overall = 1 - sum e^2 / sum (y - ybar)^2.
 * out->beta .. ci_upper: p host values each.  std_err .. ci_upper may ALL be NULL: the fit-only call (beta, r2, adj_r2; the pass
 * then forms no scores).  extra (nullable): alpha / pred / resid are `space`-resident arrays of the frame's type, each nullable;
 * pred and resid come back in the caller's row order.  A singleton group stays in (it counts in n and G and adds nothing to W or M;
 * its alpha is y - x' beta).
 *   grouped: group g = rows [group_offsets[g], group_offsets[g+1]); n_groups + 1 int64 values, `space`-resident, starting at 0,
 *            ending at n_rows, non-decreasing (else PDS_ERR_INVALID).  alpha has n_groups entries.  An empty group counts nowhere and
 *            changes no output bit; its alpha is NaN.
 *   by key:  keys = n_rows int64 values in any row order, `space`-resident (ordered keys move nothing and give the bits of the
 *            grouped form; otherwise the stable sort + gather of the other by-key entry points).  *n_groups receives G.  max_groups
 *            and out_keys matter only when extra->alpha is given: alpha and out_keys (nullable) then have room for max_groups
 *            entries, in ascending key order, and more distinct keys are PDS_ERR_INVALID with *n_groups set (nothing fitted).
 * The call is two streams over the frame: the statistics pass of pds_mixed_* (group means, W, no cancellation) and one pass that forms
 * alpha, residuals, sum e^2 and the scores together; the p x p solve runs on the host in f64.  f32 frames: f64 arithmetic throughout.
 * Two calls give the same bits (no floating-point atomics).  Groups above the context option "within_split_rows" are cut into row
 * chunks.  p-values come from pds_student_t_sf's algorithm with its ln-gamma prefactor evaluated free of cancellation (these entry
 * points have no counterpart in the reference to stay bit-compatible with; at 1e4 .. 1e5 degrees of freedom the two differ by 1e-10).  Refused, never approximated: n - G - p <= 0 PDS_ERR_TOO_FEW_ROWS; a cluster form with G < 2 PDS_ERR_INVALID; a feature
 * that is constant inside every group (collinear with the effects) PDS_ERR_NUMERIC, the message naming the column index; W_xx not
 * positive definite otherwise PDS_ERR_NUMERIC; more than 16 features PDS_ERR_UNSUPPORTED; PDS_HC0 .. PDS_HC3 PDS_ERR_UNSUPPORTED.
 * There is no weighted form.  Clusters on a key other than the absorbed one: pds_lin_reg_within_cl_* below.
 */
typedef struct {           /* every pointer nullable and `space`-resident */
    void* alpha;           /* [n_groups] (by key: [max_groups], ascending key order) */
    void* pred;            /* [n_rows], frame order */
    void* resid;           /* [n_rows], frame order */
    double r2_overall;
    int64_t n_groups_used; /* G */
    int64_t df_resid;      /* n - G - p ("se") or G - 1 (cluster forms) */
} pds_within_out;
int pds_lin_reg_within_grouped_f64(pds_ctx* ctx, const double* const* cols, int n_feat, int64_t n_rows, const int64_t* group_offsets,
                                   int64_t n_groups, pds_space space, int se_type, pds_report_f64* out, pds_within_out* extra);
int pds_lin_reg_within_grouped_f32(pds_ctx* ctx, const float* const* cols, int n_feat, int64_t n_rows, const int64_t* group_offsets,
                                   int64_t n_groups, pds_space space, int se_type, pds_report_f32* out, pds_within_out* extra);
int pds_lin_reg_within_by_key_f64(pds_ctx* ctx, const double* const* cols, const int64_t* keys, int n_feat, int64_t n_rows, pds_space space,
                                  int se_type, int64_t max_groups, int64_t* out_keys, pds_report_f64* out, pds_within_out* extra,
                                  int64_t* n_groups);
int pds_lin_reg_within_by_key_f32(pds_ctx* ctx, const float* const* cols, const int64_t* keys, int n_feat, int64_t n_rows, pds_space space,
                                  int se_type, int64_t max_groups, int64_t* out_keys, pds_report_f32* out, pds_within_out* extra,
                                  int64_t* n_groups);

/*
 * pds_lin_reg_within2_*: fixed-effects regression with TWO absorbed factors -- ONE model with an intercept per level of each of two
 * keys, y_i = alpha_g1(i) + gamma_g2(i) + x_i' beta + e_i (firm and year effects: two-way fixed effects); no dummy column is ever
 * formed.  cols = [y, x1..xp], 1 .. 16 feature columns and NO intercept column.  What follows is a DEFINITION of what the library
 * computes; no equivalence with the small-sample conventions of any package is claimed beyond this text.
 *   n rows, p features.  Factor 1 has G1 occupied levels, factor 2 G2.  C is the number of connected components of the bipartite
 *   graph whose edges are the occupied (level1, level2) cells; A = G1 + G2 - C is the rank of the absorbed dummies.  z~ is the column
 *   z projected off both sets of dummies; X~, y~ the projected features and target.
 *   beta solves X~'X~ beta = X~'y~;  e = y~ - X~ beta;  pred = y - e.
 *   se_type PDS_SE:       V = s2 (X~'X~)^-1, s2 = sum e^2 / (n - p - A); t, p and the 95 % interval use the Student t with n - p - A
 *                         degrees of freedom (the tail of pds_lin_reg_within_*).
 *   se_type PDS_CLUSTER0: V = (X~'X~)^-1 M (X~'X~)^-1, M = sum_g s_g s_g', s_g = sum_{i in g} x~_i e_i: the clusters are the levels of
 *                         the FIRST key.
 *   se_type PDS_CLUSTER:  the same V times G1 / (G1 - 1) * (n - 1) / (n - K), K = p + 1 + (A - G1): the effects of the first factor,
 *                         nested in the clusters, count as the one intercept; those of the second factor are counted.  With one
 *                         factor this is the definition of pds_lin_reg_within_*.  Both cluster forms use G1 - 1 degrees of freedom.
 *   out->r2 = 1 - sum e^2 / sum y~^2, out->adj_r2 = 1 - (1 - r2)(n - A) / (n - A - p), extra->r2_overall = 1 - sum e^2 / sum (y - ybar)^2.
 * The projection is by alternating sweeps over all p + 1 columns in f64 (f32 frames too).  One sweep subtracts the factor-1 level
 * means, then the factor-2 level means.  After each sweep delta = max_j max_level |factor-2 mean subtracted from column j in this
 * sweep| / s_j, s_j the population standard deviation of the original column j (one moment pass; it is only a scale).  The sweeps stop
 * when delta <= absorb_tol (> 0, else PDS_ERR_INVALID; 1e-8 is reghdfe's default).  absorb_max_iter (>= 1) sweeps without that:
 * PDS_ERR_NUMERIC, the message says "did not converge" and gives the last delta; nothing is returned.  extra->n_iter is the number
 * of sweeps used.  The device keeps the subtracted means as two tables and forms every working value from the row's original value:
 * two reads of the frame per sweep, no write, and the rounding of one sweep is not carried into the next.
 *   The first factor enters exactly as in pds_lin_reg_within_*: group_offsets (grouped), or int64 keys in any row order (by key: the
 *   stable sort + gather of the other by-key entry points; *n_groups receives G1).  The second factor enters as dense int32 codes
 *   per row in [0, n_levels2), `space`-resident, in the CALLER's row order (the by-key form gathers them through its row
 *   permutation).  A code outside the range: PDS_ERR_INVALID.  Unused codes count nowhere.  Fewer than 2^31 rows per call.
 * out: as pds_lin_reg_within_* (std_err .. ci_upper may ALL be NULL: the fit-only call).  extra (nullable): pred / resid are
 * `space`-resident arrays of the frame's type, each nullable, in the caller's row order.
 * Refused, never approximated: n - p - A <= 0 PDS_ERR_TOO_FEW_ROWS; a cluster form with G1 < 2 PDS_ERR_INVALID; a feature that is
 * constant PDS_ERR_NUMERIC; a feature whose projected sum of squares sum x~^2 is not above min(1e-4, max(1e-12, (1e3 absorb_tol)^2)) -- 1e-10 at
 * the default tolerance -- times its centred sum of squares sum (x - xbar)^2 (a function of the keys: collinear with the absorbed
 * effects) PDS_ERR_NUMERIC, the message naming the column index; X~'X~ not positive definite otherwise PDS_ERR_NUMERIC; more than 16
 * features PDS_ERR_UNSUPPORTED; PDS_HC0 .. PDS_HC3 PDS_ERR_UNSUPPORTED.  There is no weighted form; the effects themselves come from
 * pds_lin_reg_within2_fx_* below.  A workspace the device cannot hold fails with the allocation's error.
 * C is counted exactly on the device: every row is an edge between its level of factor 1 and its code of factor 2, and rounds of
 * hooking (32-bit integer atomicMin of the smaller root into the larger) and pointer jumping label every level with the smallest
 * level index of its component, in at most 2 ceil(log2(G1 + n_levels2)) + 1 rounds (a root that neither hooks nor is hooked into
 * in one round hooks in the next, so the trees of a component at least halve in two rounds; more: PDS_ERR_NUMERIC,
 * "component labelling did not finish", never a wrong count).  The range of the codes is checked by a kernel that reads nothing else, before anything is indexed
 * by a code; the level counts of factor 2 are exact integers from the ordered codes.  The host reads O(n_levels2 + G1) integers and
 * no row.  Two calls give the same bits (no floating-point atomics; every sum in a fixed order).  Levels of factor 1 above the
 * context option "within_split_rows" are cut into row chunks; every level of factor 2 is cut into chunks of at most 1 024 gathered
 * rows (of "within_split_rows" rows if that is smaller).
 * ACCELERATION (context option "within2_accel" = 1; 0, the default, is the plain iteration above, bit for bit; a DEFINITION).  A sweep
 * is exactly the sweep above.  m2(k) is the table of factor-2 level means sweep k subtracts; its scaled maximum is that sweep's delta.
 * The factor-1 step of a sweep does not depend on the factor-1 means subtracted so far, so the state of the iteration is the table a2
 * of factor-2 means subtracted in all.  The accelerated iteration (Irons-Tuck) runs cycles of two sweeps:
 *     1. sweep; Delta1 = its m2.  delta <= absorb_tol: stop.
 *     2. sweep; Delta2 = its m2.  delta <= absorb_tol: stop.
 *     3. per column j, over the occupied codes of factor 2:  d = Delta2 - Delta1,  c_j = sum Delta2 d / sum d^2,
 *        a2[.][j] <- a2[.][j] - c_j Delta2[.][j].  c_j is 0 -- the column is left alone -- when the denominator is 0 or when a sum or
 *        the quotient is not finite.  The sums are unweighted (not weighted by level counts).
 * Only a2 is extrapolated; the next sweep's factor-1 step rebuilds the factor-1 means from it.  Convergence is judged by a sweep's
 * delta and by nothing else, so the call always ends on a sweep and everything after the sweeps -- the final stage, pred / resid, the
 * effects and their normalisation -- is formed as without acceleration.  absorb_max_iter and extra->n_iter count SWEEPS only; the
 * "did not converge" error is the same (an extrapolation after the last sweep allowed is not made).  The two sums of a column are
 * taken in a fixed order that depends on the number of occupied codes of factor 2 and the device alone -- not on scheduling, on
 * "within_split_rows" or on the row order: two calls give the same bits, and the by-key form on shuffled rows the bits of the
 * grouped form.  An extrapolation reads and writes tables of n_levels2 x (p + 1) doubles; the frame is read twice per sweep as before.
 * All eight pds_lin_reg_within2_* entry points honour the option; none has another argument for it.
 */
typedef struct {            /* every pointer nullable and `space`-resident */
    void* pred;             /* [n_rows], frame order */
    void* resid;            /* [n_rows], frame order */
    double r2_overall;
    int64_t df_resid;       /* n - p - A ("se") or G1 - 1 (cluster forms) */
    int64_t n_groups_used;  /* G1 */
    int64_t n_groups2_used; /* G2 */
    int64_t n_components;   /* C */
    int64_t n_iter;         /* sweeps used */
} pds_within2_out;
int pds_lin_reg_within2_grouped_f64(pds_ctx* ctx, const double* const* cols, int n_feat, int64_t n_rows, const int64_t* group_offsets,
                                    int64_t n_groups, const int32_t* codes2, int64_t n_levels2, pds_space space, int se_type,
                                    double absorb_tol, int absorb_max_iter, pds_report_f64* out, pds_within2_out* extra);
int pds_lin_reg_within2_grouped_f32(pds_ctx* ctx, const float* const* cols, int n_feat, int64_t n_rows, const int64_t* group_offsets,
                                    int64_t n_groups, const int32_t* codes2, int64_t n_levels2, pds_space space, int se_type,
                                    double absorb_tol, int absorb_max_iter, pds_report_f32* out, pds_within2_out* extra);
int pds_lin_reg_within2_by_key_f64(pds_ctx* ctx, const double* const* cols, const int64_t* keys, const int32_t* codes2, int64_t n_levels2,
                                   int n_feat, int64_t n_rows, pds_space space, int se_type, double absorb_tol, int absorb_max_iter,
                                   pds_report_f64* out, pds_within2_out* extra, int64_t* n_groups);
int pds_lin_reg_within2_by_key_f32(pds_ctx* ctx, const float* const* cols, const int64_t* keys, const int32_t* codes2, int64_t n_levels2,
                                   int n_feat, int64_t n_rows, pds_space space, int se_type, double absorb_tol, int absorb_max_iter,
                                   pds_report_f32* out, pds_within2_out* extra, int64_t* n_groups);

/*
 * pds_lin_reg_within2_fx_*: pds_lin_reg_within2_* with the ESTIMATED EFFECTS alpha (per level of factor 1) and gamma (per code of
 * factor 2) of y_i = alpha_g1(i) + gamma_g2(i) + x_i' beta + e_i.  The argument lists are those of pds_lin_reg_within2_* plus a
 * trailing pds_within2_effects* fx (nullable: the call is then pds_lin_reg_within2_* itself); out and extra receive the same bits.
 * The effects are identified only up to one constant per connected component of the cells, so what follows is a DEFINITION of what
 * the library returns; no equivalence with a package's convention is claimed beyond this text.
 *   a1 [level of factor 1][column], a2 [code of factor 2][column]: the level means the sweeps have subtracted in all, columns
 *   x_1 .. x_p, y.  alpha' [level of factor 1]: the one-factor effects pds_lin_reg_within_* defines, of the projected columns (of the
 *   order of absorb_tol; with them y_i - alpha - gamma - x_i' beta - resid_i is zero to rounding).
 *     alpha_raw[g] = a1[g][y] - sum_j beta_j a1[g][j] + alpha'[g];    gamma_raw[l] = a2[l][y] - sum_j beta_j a2[l][j]
 *   NORMALISATION: in every component the reference level is the LOWEST occupied code of factor 2 in it; with c = gamma_raw at that
 *   code, alpha_g = alpha_raw[g] + c and gamma_l = gamma_raw[l] - c.  gamma at every reference level is exactly 0.0: these are the
 *   coefficients of the regression on the features, one dummy per level of factor 1 and one per level of factor 2 less the first
 *   level of factor 2 in every component.  f64 arithmetic, terms in ascending column order; the outputs have the frame's type.
 *   component1 / component2: the component of every level as the index, in effects1, of the smallest level of factor 1 in it.
 *   A code of factor 2 that no row uses: gamma NaN, component -1.
 *   grouped: effects1 / component1 have n_groups entries, indexed by the caller's groups; an empty group: NaN / -1.  cap1 and keys1
 *            are not read.
 *   by key:  effects1 / component1 / keys1 (the distinct keys, ascending) have room for cap1 entries when any of them is given, and
 *            more distinct keys are PDS_ERR_INVALID with *n_groups set (nothing fitted), as pds_lin_reg_within_by_key_*.
 * n_graph_rounds receives the rounds the component labelling took.
 */
typedef struct {              /* every pointer nullable and `space`-resident */
    void* effects1;           /* [n_groups] (by key: [cap1], ascending key order), the frame's type */
    void* effects2;           /* [n_levels2], the frame's type */
    int32_t* component1;      /* as effects1 */
    int32_t* component2;      /* [n_levels2] */
    int64_t* keys1;           /* by key: [cap1] */
    int64_t cap1;             /* by key: room in effects1 / component1 / keys1 */
    int64_t n_graph_rounds;   /* out */
} pds_within2_effects;
int pds_lin_reg_within2_fx_grouped_f64(pds_ctx* ctx, const double* const* cols, int n_feat, int64_t n_rows, const int64_t* group_offsets,
                                       int64_t n_groups, const int32_t* codes2, int64_t n_levels2, pds_space space, int se_type,
                                       double absorb_tol, int absorb_max_iter, pds_report_f64* out, pds_within2_out* extra,
                                       pds_within2_effects* fx);
int pds_lin_reg_within2_fx_grouped_f32(pds_ctx* ctx, const float* const* cols, int n_feat, int64_t n_rows, const int64_t* group_offsets,
                                       int64_t n_groups, const int32_t* codes2, int64_t n_levels2, pds_space space, int se_type,
                                       double absorb_tol, int absorb_max_iter, pds_report_f32* out, pds_within2_out* extra,
                                       pds_within2_effects* fx);
int pds_lin_reg_within2_fx_by_key_f64(pds_ctx* ctx, const double* const* cols, const int64_t* keys, const int32_t* codes2, int64_t n_levels2,
                                      int n_feat, int64_t n_rows, pds_space space, int se_type, double absorb_tol, int absorb_max_iter,
                                      pds_report_f64* out, pds_within2_out* extra, int64_t* n_groups, pds_within2_effects* fx);
int pds_lin_reg_within2_fx_by_key_f32(pds_ctx* ctx, const float* const* cols, const int64_t* keys, const int32_t* codes2, int64_t n_levels2,
                                      int n_feat, int64_t n_rows, pds_space space, int se_type, double absorb_tol, int absorb_max_iter,
                                      pds_report_f32* out, pds_within2_out* extra, int64_t* n_groups, pds_within2_effects* fx);
/*
 * pds_absorb_components_i32: the graph pass of pds_lin_reg_within2_* alone.  codes1 / codes2: n_rows dense int32 codes each, in
 * [0, n_levels1) / [0, n_levels2), `space`-resident, rows in any order (a code outside its range: PDS_ERR_INVALID, found before
 * anything is indexed by a code).  component1 [n_levels1] / component2 [n_levels2] (nullable, `space`-resident): the component of every
 * level as the smallest code of key 1 in it, -1 for a code no row uses.  *n1 / *n2: the codes in use, *n_components: the connected
 * components of the graph of the occupied cells, *n_rounds: the rounds taken (each nullable).  Fewer than 2^31 rows per call.
 */
int pds_absorb_components_i32(pds_ctx* ctx, const int32_t* codes1, int64_t n_levels1, const int32_t* codes2, int64_t n_levels2, int64_t n_rows,
                              pds_space space, int32_t* component1, int32_t* component2, int64_t* n1, int64_t* n2, int64_t* n_components,
                              int* n_rounds);

/*
 * pds_lin_reg_within_cl_* / pds_lin_reg_within2_cl_*: the fixed-effects regressions above with standard errors clustered on ANY key --
 * a key that is not an absorbed key (absorb firm and year, cluster on state), or the second absorbed key.  The argument lists are
 * those of pds_lin_reg_within_* and of pds_lin_reg_within2_fx_* (fx still nullable) plus a trailing pds_cluster_key* cl.  cl == NULL:
 * the call IS the one without the suffix, bit for bit.  What follows is a DEFINITION of what the library computes; no equivalence with
 * the small-sample conventions of any package is claimed.
 *   x~, y~ are the columns projected off the absorbed dummies, B = (X~'X~)^-1, e = y~ - X~ beta: all formed by the fit exactly as
 *   without a cluster key (beta, r2, adj_r2, r2_overall, pred, resid, n_iter and the effects are the same bits).
 *   cl->codes: n_rows dense int32 codes in [0, cl->n_levels), in the CALLER's row order, `space`-resident (the by-key forms gather them
 *   through their row permutation).  A code that no row uses counts nowhere.  A code outside the range: PDS_ERR_INVALID; the range is
 *   checked by a kernel that reads nothing else, before anything is indexed by a code.  Gc is the number of occupied codes.
 *   s_c = sum_{i in c} x~_i e_i,  M = sum_c s_c s_c'.
 *   se_type PDS_CLUSTER0: V = B M B.
 *   se_type PDS_CLUSTER:  the same V times Gc / (Gc - 1) * (n - 1) / (n - K),
 *                         K = p + sum_f (nested_f ? 0 : A_f) + (some factor nested ? 1 : 0),  A_1 = G1,  A_2 = G2 - C (= A - G1).
 *                         Factor f is NESTED when every occupied level of it has all its rows in one cluster: its effects are then
 *                         not counted among the parameters, and the one intercept is counted in their place.  This K reproduces both
 *                         definitions above: one key clustered on itself gives K = p + 1, two keys clustered on the first give
 *                         K = p + 1 + (A - G1).  With no factor nested K = p + A.
 *   t, p and the 95 % interval use the Student t with Gc - 1 degrees of freedom; extra->df_resid = Gc - 1.
 * Refused: Gc < 2 PDS_ERR_INVALID; se_type PDS_SE together with a cluster key PDS_ERR_INVALID (and std_err .. ci_upper must be given);
 * 2^31 rows or more PDS_ERR_UNSUPPORTED; everything the calls without the suffix refuse.  cl->n_clusters receives Gc, cl->nested1 /
 * cl->nested2 whether factor 1 / factor 2 is nested in the clusters (nested2 = 0 with one factor).
 * The meat is a gather: the rows are ordered by a stable radix sort of (code, row), the cluster sizes are exact integers from the run
 * boundaries, every occupied cluster is cut into chunks of at most 1 024 rows of that order ("within_split_rows" rows if that is
 * smaller).  One more contiguous pass over the frame stages every row's score x~_i e_i row-major (p doubles per row, padded to an even
 * count: n x p x 8 bytes of workspace, which fails with the allocation's error if the device cannot hold it); a wave per chunk gathers
 * the staged rows and sums them by a fixed-order butterfly; a cluster's chunk scores are added in chunk order.  Nestedness is decided
 * from integers alone (the minimum and maximum cluster code over every level's rows).  No floating-point atomics: two calls give the
 * same bits, and the by-key form on shuffled rows gives the bits of the grouped form.
 */
typedef struct {
    const int32_t* codes;     /* [n_rows], `space`-resident, the caller's row order */
    int64_t n_levels;
    int64_t n_clusters;       /* out: Gc */
    int32_t nested1, nested2; /* out; nested2 = 0 with one factor */
} pds_cluster_key;
int pds_lin_reg_within_cl_grouped_f64(pds_ctx* ctx, const double* const* cols, int n_feat, int64_t n_rows, const int64_t* group_offsets,
                                      int64_t n_groups, pds_space space, int se_type, pds_report_f64* out, pds_within_out* extra,
                                      pds_cluster_key* cl);
int pds_lin_reg_within_cl_grouped_f32(pds_ctx* ctx, const float* const* cols, int n_feat, int64_t n_rows, const int64_t* group_offsets,
                                      int64_t n_groups, pds_space space, int se_type, pds_report_f32* out, pds_within_out* extra,
                                      pds_cluster_key* cl);
int pds_lin_reg_within_cl_by_key_f64(pds_ctx* ctx, const double* const* cols, const int64_t* keys, int n_feat, int64_t n_rows, pds_space space,
                                     int se_type, int64_t max_groups, int64_t* out_keys, pds_report_f64* out, pds_within_out* extra,
                                     int64_t* n_groups, pds_cluster_key* cl);
int pds_lin_reg_within_cl_by_key_f32(pds_ctx* ctx, const float* const* cols, const int64_t* keys, int n_feat, int64_t n_rows, pds_space space,
                                     int se_type, int64_t max_groups, int64_t* out_keys, pds_report_f32* out, pds_within_out* extra,
                                     int64_t* n_groups, pds_cluster_key* cl);
int pds_lin_reg_within2_cl_grouped_f64(pds_ctx* ctx, const double* const* cols, int n_feat, int64_t n_rows, const int64_t* group_offsets,
                                       int64_t n_groups, const int32_t* codes2, int64_t n_levels2, pds_space space, int se_type,
                                       double absorb_tol, int absorb_max_iter, pds_report_f64* out, pds_within2_out* extra,
                                       pds_within2_effects* fx, pds_cluster_key* cl);
int pds_lin_reg_within2_cl_grouped_f32(pds_ctx* ctx, const float* const* cols, int n_feat, int64_t n_rows, const int64_t* group_offsets,
                                       int64_t n_groups, const int32_t* codes2, int64_t n_levels2, pds_space space, int se_type,
                                       double absorb_tol, int absorb_max_iter, pds_report_f32* out, pds_within2_out* extra,
                                       pds_within2_effects* fx, pds_cluster_key* cl);
int pds_lin_reg_within2_cl_by_key_f64(pds_ctx* ctx, const double* const* cols, const int64_t* keys, const int32_t* codes2, int64_t n_levels2,
                                      int n_feat, int64_t n_rows, pds_space space, int se_type, double absorb_tol, int absorb_max_iter,
                                      pds_report_f64* out, pds_within2_out* extra, int64_t* n_groups, pds_within2_effects* fx,
                                      pds_cluster_key* cl);
int pds_lin_reg_within2_cl_by_key_f32(pds_ctx* ctx, const float* const* cols, const int64_t* keys, const int32_t* codes2, int64_t n_levels2,
                                      int n_feat, int64_t n_rows, pds_space space, int se_type, double absorb_tol, int absorb_max_iter,
                                      pds_report_f32* out, pds_within2_out* extra, int64_t* n_groups, pds_within2_effects* fx,
                                      pds_cluster_key* cl);

/*
 * Row-sharded `pl_lin_reg_report` / `pl_wls_report` (one process per GPU): the stages of
 * pds_lin_reg_report_* as separate calls, the two exchange steps between them left to the caller.
 *   1. every rank: pds_moments_* on its rows                     -> all-reduce(SUM) of the (p+2)^2 block
 *   2. pds_report_fit_from_moments_*: X'X -> col_piv_qr -> inverse, beta (linear_regression.rs:854-858) -- replicated,
 *      deterministic, so every rank holds the same beta / inv without a broadcast.  moments / beta / inv are HOST buffers
 *      (beta: p' values; inv: p'^2, column-major).
 *   3. every rank: pds_report_partials_* on its rows: the residual pass (:863-909)
 *      partials[0] = sum e^2, partials[1] = sum w e^2 (WLS), partials[2 ..] = the (p+2)^2 block whose leading p' x p' part is
 *      the HC meat X' diag(s) X (zeros for plain standard errors); 2 + (p+2)^2 doubles, HOST -> all-reduce(SUM)
 *   4. pds_report_finish_*: the O(p'^2) epilogue (:861-939) on the summed partials; n_rows_total = rows of the whole frame;
 *      y_var as in pds_lin_reg_report_* (of the whole target).  No device work.
 */
int pds_report_fit_from_moments_f64(pds_ctx* ctx, const double* moments, int n_feat, int add_bias, double* beta, double* inv);
int pds_report_fit_from_moments_f32(pds_ctx* ctx, const float* moments, int n_feat, int add_bias, float* beta, float* inv);
int pds_report_partials_f64(pds_ctx* ctx, const double* const* cols, const double* weights, int n_feat, int64_t n_rows,
                            pds_space space, int add_bias, int se_type, const double* beta, const double* inv, double* partials);
int pds_report_partials_f32(pds_ctx* ctx, const float* const* cols, const float* weights, int n_feat, int64_t n_rows,
                            pds_space space, int add_bias, int se_type, const float* beta, const float* inv, double* partials);
int pds_report_finish_f64(int n_feat, int add_bias, int se_type, int weighted, int64_t n_rows_total, double y_var,
                          const double* beta, const double* inv, const double* partials, pds_report_f64* out);
int pds_report_finish_f32(int n_feat, int add_bias, int se_type, int weighted, int64_t n_rows_total, float y_var,
                          const float* beta, const float* inv, const double* partials, pds_report_f32* out);

/*
 * pds_lin_reg_report_nullable_*: `pl_lin_reg_report` on columns with Arrow validity bitmaps: the null policy of
 * series_to_mat_for_lr (linear_regression.rs:151-267, called at :846) on the device, then the same report on the rows
 * that survive it (dof, r2 use that row count).  Arguments as pds_lr_nullable_*; `y_var` stays what Polars computed
 * on the original target.  `pl_wls_report` has no nullable form: the reference does not compact its weights.
 */
int pds_lin_reg_report_nullable_f64(pds_ctx* ctx, const double* const* cols, const uint8_t* const* validity,
                                    const int64_t* bit_offsets, int n_feat, int64_t n_rows, pds_space space,
                                    int null_policy, double fill_value, int add_bias, int se_type, double y_var,
                                    pds_report_f64* out, int64_t* n_used);
int pds_lin_reg_report_nullable_f32(pds_ctx* ctx, const float* const* cols, const uint8_t* const* validity,
                                    const int64_t* bit_offsets, int n_feat, int64_t n_rows, pds_space space,
                                    int null_policy, float fill_value, int add_bias, int se_type, float y_var,
                                    pds_report_f32* out, int64_t* n_used);

/*
 * pds_lr_grouped_*: the key-aware batched symbol of SURVEY.md 8(b) ("pl_lr_by"): what
 * `df.group_by(key).agg(pds.lin_reg(...))` makes Polars compute by calling `pl_lr` once per group
 * (tests/test_linear_exprs.py:918-953).  Rows of one group are contiguous; group g is rows
 * [group_offsets[g], group_offsets[g+1]).  The dispatch on (l1_reg, l2_reg, positive) is pl_lr's (:447-497), per group:
 * OLS / ridge with the rank gate (the default path; streaming Gram + solve in one kernel), lasso / elastic net /
 * positive fits by coordinate descent on the group's Gram matrix (faer_coordinate_descent, faer_nn_lr).
 *   group_offsets  n_groups + 1 int64 values, `space`-resident.
 *   coeffs         out, n_groups x (n_feat + add_bias), row-major, `space`-resident.
 *   is_null        out, n_groups bytes, `space`-resident: 1 = gated or fewer rows than features
 *                  (per-group `pl_lr` raises / returns null there).
 */
int pds_lr_grouped_f64(pds_ctx* ctx, const double* const* cols, int n_feat, int64_t n_rows,
                       const int64_t* group_offsets, int64_t n_groups, pds_space space,
                       const pds_lr_params* prm, double* coeffs, uint8_t* is_null);
int pds_lr_grouped_f32(pds_ctx* ctx, const float* const* cols, int n_feat, int64_t n_rows,
                       const int64_t* group_offsets, int64_t n_groups, pds_space space,
                       const pds_lr_params* prm, float* coeffs, uint8_t* is_null);

/*
 * pds_lr_grouped_nullable_*: the same with Arrow validity bitmaps (arguments as pds_lr_nullable_*): what Polars gets
 * from `group_by(key).agg(pds.lin_reg(..., null_policy=...))` -- every group is fitted on the rows of it that survive the
 * policy; a group left with fewer rows than coefficients is null.  PDS_NULL_RAISE fails on the first null anywhere.
 */
int pds_lr_grouped_nullable_f64(pds_ctx* ctx, const double* const* cols, const uint8_t* const* validity,
                                const int64_t* bit_offsets, int n_feat, int64_t n_rows,
                                const int64_t* group_offsets, int64_t n_groups, pds_space space, int null_policy,
                                double fill_value, const pds_lr_params* prm, double* coeffs, uint8_t* is_null);
int pds_lr_grouped_nullable_f32(pds_ctx* ctx, const float* const* cols, const uint8_t* const* validity,
                                const int64_t* bit_offsets, int n_feat, int64_t n_rows,
                                const int64_t* group_offsets, int64_t n_groups, pds_space space, int null_policy,
                                float fill_value, const pds_lr_params* prm, float* coeffs, uint8_t* is_null);

/*
 * pds_lr_with_inv_*: faer_qr_lr_with_inv (lr_online_solvers.rs:120-143) -- the initial fit of OnlineLR (src/pymodels/py_lr.rs
 * :169, lr_online_solvers.rs:101-113): X'X (+ lambda on the n_feat feature diagonals), column-pivoted QR, its inverse and
 * the solution.  coeffs: n_feat + add_bias values (bias last); inv: (n_feat + add_bias)^2 values, column-major (symmetric).
 * Host outputs.  The per-row `woodbury_step` updates that follow are O(p'^2) host arithmetic on this state.
 */
int pds_lr_with_inv_f64(pds_ctx* ctx, const double* const* cols, int n_feat, int64_t n_rows, pds_space space, int add_bias,
                        double lambda, double* coeffs, double* inv);
int pds_lr_with_inv_f32(pds_ctx* ctx, const float* const* cols, int n_feat, int64_t n_rows, pds_space space, int add_bias,
                        float lambda, float* coeffs, float* inv);

/*
 * pds_lr_grouped_weighted_*: `group_by(key).agg(pds.lin_reg(..., weights=w))` -- per group faer_weighted_lr
 * (lr_solvers.rs:386-409: X'WX, X'Wy, plain solve with `solver`; no gate, no penalties, as pl_lr :436-446).  The frame is
 * scaled by sqrt(w) once on the device and takes the grouped path.  weights: n_rows values, `space`-resident; the other
 * arguments as pds_lr_grouped_*.
 */
int pds_lr_grouped_weighted_f64(pds_ctx* ctx, const double* const* cols, const double* weights, int n_feat, int64_t n_rows,
                                const int64_t* group_offsets, int64_t n_groups, pds_space space, const pds_lr_params* prm,
                                double* coeffs, uint8_t* is_null);
int pds_lr_grouped_weighted_f32(pds_ctx* ctx, const float* const* cols, const float* weights, int n_feat, int64_t n_rows,
                                const int64_t* group_offsets, int64_t n_groups, pds_space space, const pds_lr_params* prm,
                                float* coeffs, uint8_t* is_null);

/*
 * pds_lr_by_key_*: `df.group_by(key).agg(pds.lin_reg(...))` for an int64 key column in ANY row order -- the grouping
 * Polars does on the host before it calls `pl_lr` per group (tests/test_linear_exprs.py:435-474), done on the device:
 * keys already non-decreasing -> no data movement; otherwise a radix sort of (key, row) pairs and a gather of the columns.
 * Then exactly pds_lr_grouped_*.  Groups come back in ascending key order.
 *   keys        n_rows int64 values, `space`-resident.
 *   max_groups  capacity of the outputs (n_rows is always enough).
 *   out_keys    out, the distinct keys;  coeffs  out, n_groups x (n_feat + add_bias);  is_null  out, n_groups bytes
 *               -- all `space`-resident.   n_groups  out (host), number of distinct keys.
 */
int pds_lr_by_key_f64(pds_ctx* ctx, const double* const* cols, const int64_t* keys, int n_feat, int64_t n_rows, pds_space space,
                      const pds_lr_params* prm, int64_t max_groups, int64_t* out_keys, double* coeffs, uint8_t* is_null,
                      int64_t* n_groups);
int pds_lr_by_key_f32(pds_ctx* ctx, const float* const* cols, const int64_t* keys, int n_feat, int64_t n_rows, pds_space space,
                      const pds_lr_params* prm, int64_t max_groups, int64_t* out_keys, float* coeffs, uint8_t* is_null,
                      int64_t* n_groups);

/*
 * pds_lr_by_key_multi_*: pds_lr_by_key_* for a HOST frame with non-decreasing keys, driven through SEVERAL contexts from one
 * process (the Polars plugin is loaded in-process: python/polars_ds/_utils.py:28-38 -- a torch.distributed launcher cannot
 * serve `pl_lr_by`; SURVEY.md 8(e) "each GPU pulls its own shard over its own PCIe link").  The frame is cut into n_slices row
 * ranges at group boundaries (n_slices <= 0: four per context; a slice has at least 2^20 rows), slice s is fitted by context
 * s mod n_ctx on that context's device and stream from its own host thread, and its keys / coefficients / null flags land
 * directly in the piece of the outputs that follows the groups of the slices in front of it.  Contexts on DIFFERENT devices:
 * every device pulls its shard over its own link.  Several contexts on ONE device: a slice's transfer overlaps the previous
 * slice's fit and result copy.  Results are identical to pds_lr_by_key_* (same kernels per group).
 * Keys that are NOT in order (round 4; SURVEY.md 8(e) row C3 "hash(key) % R", here without moving rows): one row slice per context
 * whatever the order; every context builds the id-indexed moment table of its rows (dense integer keys, <= 16 features: the
 * partition route of pds_lr_by_key_*), the tables are summed on ctxs[0] (same device: in place; another device: hipMemcpyPeer),
 * which lists the groups and solves them -- one exchange of (key range) x (p+2)(p+3)/2 doubles per extra context.  Frames the
 * partition route does not take (sparse keys, wider frames, the "keyed_sort" option of ctxs[0]) and n_ctx == 1 take pds_lr_by_key_* on ctxs[0].
 * Arguments as pds_lr_by_key_* (space = PDS_HOST).
 */
int pds_lr_by_key_multi_f64(pds_ctx* const* ctxs, int n_ctx, int n_slices, const double* const* cols, const int64_t* keys, int n_feat,
                            int64_t n_rows, const pds_lr_params* prm, int64_t max_groups, int64_t* out_keys, double* coeffs,
                            uint8_t* is_null, int64_t* n_groups);
int pds_lr_by_key_multi_f32(pds_ctx* const* ctxs, int n_ctx, int n_slices, const float* const* cols, const int64_t* keys, int n_feat,
                            int64_t n_rows, const pds_lr_params* prm, int64_t max_groups, int64_t* out_keys, float* coeffs,
                            uint8_t* is_null, int64_t* n_groups);
/*
 * pds_lr_by_key_pred_multi_*: the per-row predictions of pds_lr_by_key_pred_* (pred / resid / row_null of the frame's length, in the
 * frame's row order; each nullable, not all) for a HOST frame with non-decreasing keys over several contexts -- what
 * `pds.lin_reg(..., return_pred=True).over(key)` (tests/test_linear_exprs.py:435-474) needs for a host frame: slice s + 1 crosses
 * the link while slice s is fitted and its predictions travel back (PCIe is full duplex), and contexts on different devices use
 * their own links.  Slices are independent (no group list comes back).  Keys not in order: pds_lr_by_key_pred_* on ctxs[0].
 *   weights  nullable, n_rows values (per-group faer_weighted_lr).
 */
int pds_lr_by_key_pred_multi_f64(pds_ctx* const* ctxs, int n_ctx, int n_slices, const double* const* cols, const double* weights,
                                 const int64_t* keys, int n_feat, int64_t n_rows, const pds_lr_params* prm, double* pred, double* resid,
                                 uint8_t* row_null);
int pds_lr_by_key_pred_multi_f32(pds_ctx* const* ctxs, int n_ctx, int n_slices, const float* const* cols, const float* weights,
                                 const int64_t* keys, int n_feat, int64_t n_rows, const pds_lr_params* prm, float* pred, float* resid,
                                 uint8_t* row_null);
/*
 * The three exchange steps of SURVEY.md 8(e) for a host that drives SEVERAL devices from ONE process (a Rust plugin inside the
 * Polars process: no launcher, no RCCL communicator) -- peer copies between the contexts' devices plus one kernel, each ordered on
 * the contexts' own streams; every call returns after all of its contexts' streams have been synchronised.  A host with one
 * process per device uses its collective library for the same three steps (python: polars_ds_extension_amd/parallel.py over
 * torch.distributed / RCCL); the compute entry points on either side are the same (pds_moments_*, pds_lr_from_moments_*,
 * pds_report_partials_*, pds_recursive_lr_seeded_*, pds_lr_grouped_*).
 *   pds_allreduce_sum_f64   bufs[c]: `count` doubles resident on ctxs[c]'s device (moment blocks, report partials, the seeds of the
 *                           expanding fit); afterwards every buffer holds the element-wise sum in rank order 0, 1, ..: rows C2 /
 *                           C5 ("all-reduce of the Gram block") and C4 ("prefix Gram": with `prefix != 0` buffer c receives the
 *                           sum of buffers 0 .. c-1 instead -- the exclusive scan the row-sharded expanding fit seeds with).
 *   pds_scatter_rows_f64    a frame resident on ctxs[0]'s device: column k's rows [bounds[c], bounds[c+1]) -> dst[c][k] on ctxs[c]'s
 *                           device (row C3, device-resident frame: "root -> peers, all links at once"); dst[0] may be null (rank
 *                           0 keeps reading the frame in place).
 *   pds_gather_f64          src[c]: counts[c] doubles on ctxs[c]'s device -> dst on ctxs[0]'s device, back to back in rank order
 *                           (row C3: the coefficient blocks of the ranks' groups).
 * f32 twins move floats.  Their all-reduce keeps the running sum as a float: every single addition is formed in f64 and rounded back,
 * so n_ctx addends cost up to n_ctx - 1 float roundings -- not an f64 accumulation (moment blocks that need one travel as f64:
 * pds_moments_* returns f64 records for both precisions).
 */
int pds_allreduce_sum_f64(pds_ctx* const* ctxs, int n_ctx, double* const* bufs, int64_t count, int prefix);
int pds_allreduce_sum_f32(pds_ctx* const* ctxs, int n_ctx, float* const* bufs, int64_t count, int prefix);
int pds_scatter_rows_f64(pds_ctx* const* ctxs, int n_ctx, const double* const* cols, int n_cols, const int64_t* bounds,
                         double* const* const* dst);
int pds_scatter_rows_f32(pds_ctx* const* ctxs, int n_ctx, const float* const* cols, int n_cols, const int64_t* bounds,
                         float* const* const* dst);
int pds_gather_f64(pds_ctx* const* ctxs, int n_ctx, const double* const* src, const int64_t* counts, double* dst);
int pds_gather_f32(pds_ctx* const* ctxs, int n_ctx, const float* const* src, const int64_t* counts, float* dst);

/* Page-locked host storage (hipHostMalloc, portable across devices) for result buffers the caller owns: device-to-host copies
 * into it run at the link rate.  The plugin layer keeps the large Arrow result buffers in such storage (plugin_arrow_out.hpp). */
int pds_host_alloc(size_t bytes, void** out);
int pds_host_free(void* p);
/* number of visible devices (the plugin layer's PDS_DEVICES=all) */
int pds_device_count(int* n);
/*
 * Result storage another PROCESS's kernels can write (one process per device, SURVEY.md 8(e) row C3 "results: gather of n_groups_r x p'
 * f64 + validity to rank 0"): the gathering rank allocates the assembled [n_groups][p'] block with pds_device_alloc (hipMalloc on
 * `device`: an IPC handle names a whole allocation), exports it, hands the 64 handle bytes to its peers (any side channel: the
 * launcher's store, a broadcast), every peer maps it with pds_ipc_open on ITS device (peer access over xGMI is enabled by the
 * mapping) and passes `mapped + its groups' offset` as the `coeffs` / `is_null` arguments of pds_lr_grouped_*: the fit's stores
 * cross the link while the kernel runs -- no staging buffer, no send / receive launches, no separate gather step.  The gathering rank
 * may read the rows once the peer's stream has passed the call (completion: below).
 * pds_ipc_close unmaps (the allocation stays the exporter's, freed with pds_device_free after every peer has closed).
 * python: polars_ds_extension_amd/parallel.py, GroupedShardPlan(direct=True).
 *
 * Completion without a collective: a SIGNAL block (pds_device_alloc with fine_grained = 1: device memory that is coherent across
 * devices, as RCCL's own flag words are) shared the same way holds one 32-bit word per rank.  A peer calls
 * pds_signal_post(ctx, mapped_word, seq) behind its fit -- a one-lane kernel on the context's stream: the fit's stores are complete and
 * visible at the kernel boundary before it, the word is stored with system scope --; the gathering rank calls
 * pds_signal_wait(ctx, words, n, seq) on ITS stream: a one-wave kernel that polls the n words (system-scope loads) until each is
 * >= seq.  Both are stream ordered: no host synchronisation, no collective launch; a step is the fit + one tiny kernel on every rank.
 * The wait gives up after `timeout_ms` (a peer that died must not hang the device): the call then fails at the next synchronisation
 * point through pds_signal_wait_status (0 = every wait so far was satisfied).  fine_grained = 1 also for the RESULT block of a direct
 * gather: the gathering device's L2 must not keep lines of rows another device writes.
 */
#define PDS_IPC_HANDLE_BYTES 64
int pds_device_alloc(int device, size_t bytes, int fine_grained, void** out);
int pds_signal_post(pds_ctx* ctx, unsigned* word, unsigned value);
int pds_signal_wait(pds_ctx* ctx, const unsigned* words, int n_words, unsigned value, int timeout_ms);
int pds_signal_wait_status(pds_ctx* ctx, int* timed_out);
int pds_device_free(int device, void* p);
int pds_ipc_export(int device, void* p, unsigned char* handle);             /* handle: PDS_IPC_HANDLE_BYTES bytes, written */
int pds_ipc_open(int device, const unsigned char* handle, void** mapped);  /* handle: PDS_IPC_HANDLE_BYTES bytes */
int pds_ipc_close(int device, void* mapped);

/*
 * pds_lr_grouped_pred_* / pds_lr_by_key_pred_*: the grouped form of `pl_lr_pred` (linear_regression.rs:704-820) -- what
 * `df.group_by(key).agg(pds.lin_reg(..., return_pred=True))` (tests/test_linear_exprs.py:435-474) and
 * `pds.lin_reg(..., return_pred=True).over(key)` make Polars compute one group at a time: every group is fitted as
 * pds_lr_grouped_* / pds_lr_by_key_* fit it, then ONE more pass over the frame (grouped_pred.hip) writes, for every row,
 *   pred[r] = x_r . beta_g(r) (+ intercept),  resid[r] = y_r - pred[r],  row_null[r] = 1 when the row's group is null
 * (pred / resid are NaN there; the reference returns an all-null struct for such a group, :745-750) -- IN THE FRAME'S OWN ROW
 * ORDER, also when the keys are shuffled.  weights (nullable, n_rows values): per group faer_weighted_lr as in
 * pds_lr_grouped_weighted_*, predictions from the unweighted rows.  pred / resid / row_null are `space`-resident and each may
 * be NULL (at least one is not); coeffs / is_null (grouped) and out_keys / coeffs / is_null / n_groups (by key) may be NULL
 * when only the per-row outputs are wanted (max_groups is then ignored).  Null-free frames only.
 */
int pds_lr_grouped_pred_f64(pds_ctx* ctx, const double* const* cols, const double* weights, int n_feat, int64_t n_rows,
                            const int64_t* group_offsets, int64_t n_groups, pds_space space, const pds_lr_params* prm, double* coeffs,
                            uint8_t* is_null, double* pred, double* resid, uint8_t* row_null);
int pds_lr_grouped_pred_f32(pds_ctx* ctx, const float* const* cols, const float* weights, int n_feat, int64_t n_rows,
                            const int64_t* group_offsets, int64_t n_groups, pds_space space, const pds_lr_params* prm, float* coeffs,
                            uint8_t* is_null, float* pred, float* resid, uint8_t* row_null);
int pds_lr_by_key_pred_f64(pds_ctx* ctx, const double* const* cols, const double* weights, const int64_t* keys, int n_feat,
                           int64_t n_rows, pds_space space, const pds_lr_params* prm, int64_t max_groups, int64_t* out_keys,
                           double* coeffs, uint8_t* is_null, int64_t* n_groups, double* pred, double* resid, uint8_t* row_null);
int pds_lr_by_key_pred_f32(pds_ctx* ctx, const float* const* cols, const float* weights, const int64_t* keys, int n_feat, int64_t n_rows,
                           pds_space space, const pds_lr_params* prm, int64_t max_groups, int64_t* out_keys, float* coeffs,
                           uint8_t* is_null, int64_t* n_groups, float* pred, float* resid, uint8_t* row_null);

/*
 * pds_rolling_lr_* / pds_recursive_lr_*: `pl_rolling_lr` (linear_regression.rs:1206-1283) and
 * `pl_recursive_lr` (:1121-1204) on null-free columns, i.e. faer_rolling_lr / faer_recursive_lr
 * (lr_online_solvers.rs:148-212) plus the plugin's pred_i = x_i . coeffs_i.  SWWLRKwargs: n = window
 * (or start_with), bias, lambda.  As in the reference the ones column is part of the data and lambda is
 * added to every diagonal entry.
 *   coeffs  out, n_rows x (n_feat + add_bias) row-major (the values buffer of the List column),
 *           `space`-resident; rows [0, n-1) are unspecified and marked invalid.
 *   pred    out, n_rows, `space`-resident.
 *   valid   out, n_rows bytes (1 = row has a result), `space`-resident.
 * Coefficients (n_feat + add_bias): <= 8 lane = 4 rows, 9 .. 12 lane = row (one kernel each), 13 .. 64 through per-row
 * moment records and the batched pivoted QR, 65 .. 255 (n_feat <= 254) through a 1024-thread record kernel and the big-system
 * solver (coverage path: the reference's drivers have no limit).
 * min_size > 0 selects the skipping variant (faer_rolling_skipping_lr :218-301): rows holding a
 * non-finite value are left out of the window and a window with fewer than min_size rows is invalid.
 */
int pds_rolling_lr_f64(pds_ctx* ctx, const double* const* cols, int n_feat, int64_t n_rows,
                       pds_space space, int add_bias, int64_t window, int64_t min_size,
                       double lambda, double* coeffs, double* pred, uint8_t* valid);
int pds_rolling_lr_f32(pds_ctx* ctx, const float* const* cols, int n_feat, int64_t n_rows,
                       pds_space space, int add_bias, int64_t window, int64_t min_size,
                       float lambda, float* coeffs, float* pred, uint8_t* valid);
int pds_recursive_lr_f64(pds_ctx* ctx, const double* const* cols, int n_feat, int64_t n_rows,
                         pds_space space, int add_bias, int64_t start_with, double lambda,
                         double* coeffs, double* pred, uint8_t* valid);
int pds_recursive_lr_f32(pds_ctx* ctx, const float* const* cols, int n_feat, int64_t n_rows,
                         pds_space space, int add_bias, int64_t start_with, float lambda,
                         float* coeffs, float* pred, uint8_t* valid);

/*
 * pds_rolling_lr_grouped_* / pds_recursive_lr_grouped_* / pds_rolling_lr_by_key_* / pds_recursive_lr_by_key_*:
 * `pds.rolling_lin_reg(...).over(key)` / `pds.recursive_lin_reg(...).over(key)` in one call.  For group g = rows [s_g, e_g) in
 * frame order (columns, SWWLRKwargs and the non-finite rule as in pds_rolling_lr_* / pds_recursive_lr_*):
 *   rolling    row r is fitted on rows [max(s_g, r - window + 1), r] and is valid iff r - s_g >= window - 1 (and, with
 *              min_size > 0 -- the skipping variant -- the window holds >= min_size finite rows);
 *   expanding  row r is fitted on rows [s_g, r] and is valid iff r - s_g >= start_with - 1;
 * i.e. exactly pds_rolling_lr_* / pds_recursive_lr_* on the group's rows alone.  The sums are segmented -- they restart at every
 * group start and never hold a row of another group -- so a group's outputs depend on its own rows only: a group holding NaN /
 * inf / huge values does not change any other group's coeffs, pred or valid (bit for bit).  Outputs are per row, IN THE FRAME'S
 * OWN ROW ORDER and `space`-resident: coeffs [n_rows][n_feat + add_bias] (bias last), pred [n_rows], valid [n_rows] bytes;
 * coeffs / pred of invalid rows are unspecified (NaN in practice), as in the ungrouped contract.
 * group_offsets: n_groups + 1 non-decreasing int64 row offsets, `space`-resident, starting at 0 and ending at n_rows (anything
 * else: PDS_ERR_INVALID).  keys (by key): n_rows int64 values in any row order, `space`-resident; rows with equal keys form a
 * group (in frame order).  Ordered keys move no data; others take the stable sort of (key, row), the frame gather, the offsets
 * form and a scatter back (fewer than 2^31 rows per call).  Deliberate deviations from a per-group reference call:
 *   1. a group with fewer rows than window / start_with gets all rows invalid (the reference aborts the whole query);
 *   2. empty groups are allowed;
 *   3. 1 .. 64 coefficients (more: PDS_ERR_UNSUPPORTED); window / start_with >= 1 (else PDS_ERR_INVALID).
 * Up to 8 coefficients the lane = 4 rows kernels run with segmented sums (a window of 256 takes the two-stream form, not the
 * register-resident leaving rows); 9 .. 64 the per-row moment records and the batched pivoted QR.  Tile anchors are those of
 * the ungrouped call on the same frame, so a group's bits can differ from a call on its slice alone (same tolerance).
 * Group boundaries are found from the offsets by searches (O(log n_groups) per tile and stage, however many empty groups
 * lie between two rows).  Device-space calls are synchronous on return like every other entry point.
 */
int pds_rolling_lr_grouped_f64(pds_ctx* ctx, const double* const* cols, int n_feat, int64_t n_rows, const int64_t* group_offsets,
                               int64_t n_groups, pds_space space, int add_bias, int64_t window, int64_t min_size, double lambda,
                               double* coeffs, double* pred, uint8_t* valid);
int pds_rolling_lr_grouped_f32(pds_ctx* ctx, const float* const* cols, int n_feat, int64_t n_rows, const int64_t* group_offsets,
                               int64_t n_groups, pds_space space, int add_bias, int64_t window, int64_t min_size, float lambda,
                               float* coeffs, float* pred, uint8_t* valid);
int pds_recursive_lr_grouped_f64(pds_ctx* ctx, const double* const* cols, int n_feat, int64_t n_rows, const int64_t* group_offsets,
                                 int64_t n_groups, pds_space space, int add_bias, int64_t start_with, double lambda, double* coeffs,
                                 double* pred, uint8_t* valid);
int pds_recursive_lr_grouped_f32(pds_ctx* ctx, const float* const* cols, int n_feat, int64_t n_rows, const int64_t* group_offsets,
                                 int64_t n_groups, pds_space space, int add_bias, int64_t start_with, float lambda, float* coeffs,
                                 float* pred, uint8_t* valid);
int pds_rolling_lr_by_key_f64(pds_ctx* ctx, const double* const* cols, const int64_t* keys, int n_feat, int64_t n_rows, pds_space space,
                              int add_bias, int64_t window, int64_t min_size, double lambda, double* coeffs, double* pred, uint8_t* valid);
int pds_rolling_lr_by_key_f32(pds_ctx* ctx, const float* const* cols, const int64_t* keys, int n_feat, int64_t n_rows, pds_space space,
                              int add_bias, int64_t window, int64_t min_size, float lambda, float* coeffs, float* pred, uint8_t* valid);
int pds_recursive_lr_by_key_f64(pds_ctx* ctx, const double* const* cols, const int64_t* keys, int n_feat, int64_t n_rows, pds_space space,
                                int add_bias, int64_t start_with, double lambda, double* coeffs, double* pred, uint8_t* valid);
int pds_recursive_lr_by_key_f32(pds_ctx* ctx, const float* const* cols, const int64_t* keys, int n_feat, int64_t n_rows, pds_space space,
                                int add_bias, int64_t start_with, float lambda, float* coeffs, float* pred, uint8_t* valid);

/*
 * pds_recursive_lr_seeded_*: the expanding fit of a frame that CONTINUES earlier rows -- the row-sharded
 * multi-GPU form of `pl_recursive_lr` ("recursive needs prefix Gram").  `seed_moments` is the
 * HOST-resident augmented moment matrix A = Z'Z ((n_feat+2)^2, layout of pds_moments_*) of all rows in
 * front of this frame (rank r passes the sum of the moment matrices of ranks < r; NULL = no rows = the
 * plain call).  The fit at local row i is over seed + rows [0, i]; the seed's row count (entry [n_feat, n_feat]) counts
 * towards start_with.  The seed must come from finite rows only.
 */
int pds_recursive_lr_seeded_f64(pds_ctx* ctx, const double* const* cols, int n_feat, int64_t n_rows,
                                pds_space space, int add_bias, int64_t start_with, double lambda,
                                const double* seed_moments, double* coeffs, double* pred,
                                uint8_t* valid);
int pds_recursive_lr_seeded_f32(pds_ctx* ctx, const float* const* cols, int n_feat, int64_t n_rows,
                                pds_space space, int add_bias, int64_t start_with, float lambda,
                                const float* seed_moments, float* coeffs, float* pred,
                                uint8_t* valid);

/*
 * Moment-level entry points (what a multi-GPU host composes; also the measured Gram build).
 *
 * pds_moments_*: one streaming pass over [y | X] building the augmented moment matrix
 *     A = Z'Z,  Z = [x1 .. xp | 1 | y]   ((p+2) x (p+2), column-major, symmetric)
 * i.e. X'X (get_xtx_with_lambda lr_solvers.rs:183-198), X'y (build_xty :262-278), the column sums and
 * sum(y) used by the coordinate-descent bias shortcut (:483-484), y'y and n -- every input element is
 * read from HBM exactly once.  With weights != NULL: Z'WZ.  The result is written to `moments`
 * ((n_feat+2)^2 values) in `out_space`; for PDS_DEVICE the call only enqueues work (no host sync), so
 * a caller can all-reduce the buffer across ranks (RCCL) and then call pds_lr_from_moments_*.
 */
int pds_moments_f64(pds_ctx* ctx, const double* const* cols, const double* weights, int n_feat,
                    int64_t n_rows, pds_space space, double* moments, pds_space out_space);
int pds_moments_f32(pds_ctx* ctx, const float* const* cols, const float* weights, int n_feat,
                    int64_t n_rows, pds_space space, float* moments, pds_space out_space);
/* Same dispatch as pds_lr_* but starting from (already all-reduced) moments in `mom_space`. */
int pds_lr_from_moments_f64(pds_ctx* ctx, const double* moments, pds_space mom_space, int n_feat,
                            const pds_lr_params* prm, double* coeffs, int* is_null);
int pds_lr_from_moments_f32(pds_ctx* ctx, const float* moments, pds_space mom_space, int n_feat,
                            const pds_lr_params* prm, float* coeffs, int* is_null);

/* Bit-faithful host restatements of src/stats_utils (beta.rs:24-37, 365-377) used by the report. */
double pds_student_t_sf(double x, double df);
double pds_student_t_ppf(double q, double df);

/* ------------------------------------------------------------------------------------------------
 * The pyclass route (src/pymodels): GLM, fits from row-major matrices
 * ---------------------------------------------------------------------------------------------- */
/* GLM by iteratively re-weighted least squares -- faer_irls (src/linear/glm/glm_solvers.rs:249-368) as GLM::fit_unchecked
 * drives it (:216-240: weighted least squares by pivoted QR, a ones column for add_bias).  link: 0 identity, 1 log, 2 logit,
 * 3 inverse; variance: 0 gaussian, 1 poisson, 2 binomial, 3 gamma (link_functions.rs:5-77; GLMFamily::link_function /
 * variance_function glm_solvers.rs:24-41).  coeffs: n_feat + add_bias values, bias last; *n_iter (nullable): iterations run.
 * Stops when max |beta_new - beta| < tol or after max_iter iterations (the reference does not report non-convergence).
 * Up to 16 feature columns an iteration is ONE pass over the frame (weights and working response formed inside the Gram
 * kernel); wider frames write them as two columns and run the weighted wide Gram build on them. */
int pds_glm_irls_f64(pds_ctx* ctx, const double* const* cols, int n_feat, int64_t n_rows, pds_space space, int add_bias, int link,
                     int variance, double tol, int max_iter, double* coeffs, int* n_iter);
/*
 * pds_glm_irls_grouped_* / pds_glm_irls_by_key_*: a GLM per group in one call -- for every group g what pds_glm_irls_* computes on
 * g's rows alone (faer_irls per group: same start, weights, working response, pivoted-QR weighted solve and stopping rule), all
 * iterations of a group on chip (grouped_irls.hip: one wave per group; a group of up to 128 rows is read from memory once).
 * cols = [y, x1..xp], 1 .. 16 feature columns (more: PDS_ERR_UNSUPPORTED); f32 frames are fitted in f64 arithmetic.
 * Outputs, `space`-resident: coeffs [n_groups][n_feat + add_bias] (bias last), n_iter [n_groups] int32, is_null [n_groups] bytes:
 * 1 for a group with fewer rows than coefficients (NaN coefficients, n_iter = 0) and for a group whose final coefficients are not
 * all finite (a separated binomial group, NaN / inf in its rows); a bad group never changes another group's bits.
 * pred / row_null (each nullable, n_rows): the fitted mean g^-1(x . beta_group) of every row in the frame's row order, NaN and
 * row_null = 1 for the rows of a null group.  Groups longer than the context option "glm_split_rows" are fitted one by one with
 * the full-device iteration of pds_glm_irls_*.  By key: int64 keys in any row order, groups returned in ascending key order
 * (ordered keys: nothing moves; unordered keys: sort + gather, per-row outputs sent back through the permutation); *n_groups
 * receives the number of distinct keys, also when it exceeds max_groups (PDS_ERR_INVALID, nothing fitted).
 */
int pds_glm_irls_grouped_f64(pds_ctx* ctx, const double* const* cols, int n_feat, int64_t n_rows, const int64_t* group_offsets,
                             int64_t n_groups, pds_space space, int add_bias, int link, int variance, double tol, int max_iter,
                             double* coeffs, int32_t* n_iter, uint8_t* is_null, double* pred, uint8_t* row_null);
int pds_glm_irls_grouped_f32(pds_ctx* ctx, const float* const* cols, int n_feat, int64_t n_rows, const int64_t* group_offsets,
                             int64_t n_groups, pds_space space, int add_bias, int link, int variance, float tol, int max_iter,
                             float* coeffs, int32_t* n_iter, uint8_t* is_null, float* pred, uint8_t* row_null);
int pds_glm_irls_by_key_f64(pds_ctx* ctx, const double* const* cols, const int64_t* keys, int n_feat, int64_t n_rows, pds_space space,
                            int add_bias, int link, int variance, double tol, int max_iter, int64_t max_groups, int64_t* out_keys,
                            double* coeffs, int32_t* n_iter, uint8_t* is_null, int64_t* n_groups, double* pred, uint8_t* row_null);
int pds_glm_irls_by_key_f32(pds_ctx* ctx, const float* const* cols, const int64_t* keys, int n_feat, int64_t n_rows, pds_space space,
                            int add_bias, int link, int variance, float tol, int max_iter, int64_t max_groups, int64_t* out_keys,
                            float* coeffs, int32_t* n_iter, uint8_t* is_null, int64_t* n_groups, float* pred, uint8_t* row_null);
/*
 * pds_glm_irls_wo_grouped_* / pds_glm_irls_wo_by_key_*: the grouped fits with a prior weight pw_i and an offset o_i per row (R's
 * glm(weights=, offset=), statsmodels' var_weights=, offset=) -- the argument lists of their twins above with `weights`, `offset`
 * after `cols`: both nullable (pw = 1, o = 0), `space`-resident, n_rows long.  With both null the twin's implementation is called:
 * the same bits.  Per group, everything else as in the twins:
 *     eta_i = x_i . beta + o_i,  mu_i = g^-1(eta_i),  working weight w_i = pw_i / (g'(mu_i)^2 V(mu_i)),
 *     working response z_i = (eta_i - o_i) + g'(mu_i) (y_i - mu_i);
 *     start: mu = (y + 0.5) / 2 (binomial), mu = (y + ybar) / 2 otherwise with ybar = sum pw_i y_i / sum pw_i, then eta = g(mu) --
 *     the offset enters the first iteration only through z;
 *     the same pivoted-QR solve (16 features + bias: weighted centring), stopping rule, n_iter and NaN rule.
 * A row with pw_i = 0 contributes nothing and does not count as a row.  A group is null (NaN coefficients, n_iter = 0, NaN pred and
 * row_null = 1 on its rows) when fewer than n_feat + add_bias of its rows have pw_i > 0 or when any pw_i is negative or not
 * finite; a non-finite offset makes the coefficients non-finite, so the group is null by the twins' rule.  A bad group never changes
 * another group's bits.  pred = g^-1(x_i . beta_group + o_i) for every row of a non-null group, rows of weight 0 included.
 * By key the two columns travel with the frame: ordered keys move nothing, unordered keys take the same sort + gather; a host frame
 * stages them with the other columns.  1 .. 16 feature columns (more: PDS_ERR_UNSUPPORTED).
 * Groups longer than "glm_split_rows" are fitted one by one with the full-device iteration of pds_glm_irls_wo_* on their row range of
 * the two columns; such a group that fails the weight rule is null like any other.
 * pds_glm_irls_wo_*: the one-model form, the argument list of pds_glm_irls_* with `weights`, `offset` after `cols`, any width that
 * pds_glm_irls_* takes.  Each iteration writes the weight and the working response as two columns and runs the weighted Gram build
 * on them (what pds_glm_irls_* does above 16 features).  A negative or non-finite weight, or fewer rows of positive weight than
 * coefficients, is PDS_ERR_INVALID with a message.
 * Not built: a penalty together with either column (the pds_glm_enet_* forms take neither).  The report: pds_glm_report_wo_*.
 */
int pds_glm_irls_wo_f64(pds_ctx* ctx, const double* const* cols, const double* weights, const double* offset, int n_feat, int64_t n_rows,
                        pds_space space, int add_bias, int link, int variance, double tol, int max_iter, double* coeffs, int* n_iter);
int pds_glm_irls_wo_f32(pds_ctx* ctx, const float* const* cols, const float* weights, const float* offset, int n_feat, int64_t n_rows,
                        pds_space space, int add_bias, int link, int variance, float tol, int max_iter, float* coeffs, int* n_iter);
int pds_glm_irls_wo_grouped_f64(pds_ctx* ctx, const double* const* cols, const double* weights, const double* offset, int n_feat,
                                int64_t n_rows, const int64_t* group_offsets, int64_t n_groups, pds_space space, int add_bias, int link,
                                int variance, double tol, int max_iter, double* coeffs, int32_t* n_iter, uint8_t* is_null, double* pred,
                                uint8_t* row_null);
int pds_glm_irls_wo_grouped_f32(pds_ctx* ctx, const float* const* cols, const float* weights, const float* offset, int n_feat, int64_t n_rows,
                                const int64_t* group_offsets, int64_t n_groups, pds_space space, int add_bias, int link, int variance,
                                float tol, int max_iter, float* coeffs, int32_t* n_iter, uint8_t* is_null, float* pred, uint8_t* row_null);
int pds_glm_irls_wo_by_key_f64(pds_ctx* ctx, const double* const* cols, const double* weights, const double* offset, const int64_t* keys,
                               int n_feat, int64_t n_rows, pds_space space, int add_bias, int link, int variance, double tol, int max_iter,
                               int64_t max_groups, int64_t* out_keys, double* coeffs, int32_t* n_iter, uint8_t* is_null, int64_t* n_groups,
                               double* pred, uint8_t* row_null);
int pds_glm_irls_wo_by_key_f32(pds_ctx* ctx, const float* const* cols, const float* weights, const float* offset, const int64_t* keys,
                               int n_feat, int64_t n_rows, pds_space space, int add_bias, int link, int variance, float tol, int max_iter,
                               int64_t max_groups, int64_t* out_keys, float* coeffs, int32_t* n_iter, uint8_t* is_null, int64_t* n_groups,
                               float* pred, uint8_t* row_null);
/*
 * pds_glm_enet_* / pds_glm_enet_grouped_* / pds_glm_enet_by_key_*: the elastic-net penalised fits -- the argument lists of their
 * pds_glm_irls_* twins with l1_reg, l2_reg after `variance`; everything said there holds.  For a frame or group of n rows,
 * coefficients beta with features j < p and an optional unpenalised bias last, the fit minimises
 *     F(beta) = (1/n) sum_i l(y_i, eta_i) + (l2_reg / 2) sum_{j<p} beta_j^2 + l1_reg sum_{j<p} |beta_j|,    eta = X beta (+ bias),
 * l the unit-dispersion negative log-likelihood of the family's canonical link (gaussian (y - eta)^2 / 2, poisson e^eta - y eta,
 * binomial log(1 + e^eta) - y eta, gamma y eta - log eta with eta = 1 / mu); for the binomial family with l1_reg = 0 this is the
 * cost of the reference's logistic_reg (logistic_solver.rs:44-74).  A penalty <= 0 means none, as there; both <= 0 is the
 * pds_glm_irls_* fit, bit for bit.  The links are canonical, so an IRLS step is a Newton step and the penalised step minimises
 * 1/2 beta'Gbeta - c'beta + (n l2_reg / 2) |beta_f|^2 + n l1_reg |beta_f|_1 over the iteration's G = X'WX, c = X'Wz: with l1_reg <= 0
 * the same pivoted-QR solve with n l2_reg on the feature diagonal; with l1_reg > 0 a covariance-update coordinate descent, warm-started
 * from the previous iteration (exact zeros; its sweeps end at a largest move of tol / 10 or after 1000).  Start, stopping rule,
 * n_iter, null rule and pred are those of the unpenalised fit; no line search.  Deliberate deviation: the reference's l1 goes
 * through OWL-QN and may shrink the bias too.  Grouped: 1 .. 16 feature columns (more: PDS_ERR_UNSUPPORTED); one model: any width
 * pds_glm_irls_* takes.
 */
int pds_glm_enet_f64(pds_ctx* ctx, const double* const* cols, int n_feat, int64_t n_rows, pds_space space, int add_bias, int link,
                     int variance, double l1_reg, double l2_reg, double tol, int max_iter, double* coeffs, int* n_iter);
int pds_glm_enet_f32(pds_ctx* ctx, const float* const* cols, int n_feat, int64_t n_rows, pds_space space, int add_bias, int link,
                     int variance, float l1_reg, float l2_reg, float tol, int max_iter, float* coeffs, int* n_iter);
int pds_glm_enet_grouped_f64(pds_ctx* ctx, const double* const* cols, int n_feat, int64_t n_rows, const int64_t* group_offsets,
                             int64_t n_groups, pds_space space, int add_bias, int link, int variance, double l1_reg, double l2_reg, double tol,
                             int max_iter, double* coeffs, int32_t* n_iter, uint8_t* is_null, double* pred, uint8_t* row_null);
int pds_glm_enet_grouped_f32(pds_ctx* ctx, const float* const* cols, int n_feat, int64_t n_rows, const int64_t* group_offsets,
                             int64_t n_groups, pds_space space, int add_bias, int link, int variance, float l1_reg, float l2_reg, float tol,
                             int max_iter, float* coeffs, int32_t* n_iter, uint8_t* is_null, float* pred, uint8_t* row_null);
int pds_glm_enet_by_key_f64(pds_ctx* ctx, const double* const* cols, const int64_t* keys, int n_feat, int64_t n_rows, pds_space space,
                            int add_bias, int link, int variance, double l1_reg, double l2_reg, double tol, int max_iter, int64_t max_groups,
                            int64_t* out_keys, double* coeffs, int32_t* n_iter, uint8_t* is_null, int64_t* n_groups, double* pred,
                            uint8_t* row_null);
int pds_glm_enet_by_key_f32(pds_ctx* ctx, const float* const* cols, const int64_t* keys, int n_feat, int64_t n_rows, pds_space space,
                            int add_bias, int link, int variance, float l1_reg, float l2_reg, float tol, int max_iter, int64_t max_groups,
                            int64_t* out_keys, float* coeffs, int32_t* n_iter, uint8_t* is_null, int64_t* n_groups, float* pred,
                            uint8_t* row_null);
/*
 * pds_glm_report_grouped_* / pds_glm_report_by_key_*: the fit of pds_glm_irls_grouped_* / pds_glm_irls_by_key_* and its report per
 * group in one call -- the argument lists of those entry points without pred / row_null, and a trailing struct of output pointers.
 * The groups returned and their coeffs / n_iter / is_null are bit for bit those of the pds_glm_irls_* call on the same frame; the
 * report is formed afterwards on the device, at the coefficients AS STORED (an f32 frame: the f32 values), in f64 arithmetic
 * (grouped_glm_report.hip: one wave per group, one more weighted Gram build and one p' x p' inverse; groups longer than the
 * context option "glm_split_rows" are cut into pieces that stream on many waves and are added in piece order).  No atomics in any
 * sum: repeated calls are bit-identical.  The unscaled convention of statsmodels' GLM, for a group of n rows, x_i with the
 * constant 1 last when add_bias is set:
 *   eta_i = x_i . beta, mu_i = g^-1(eta_i), w_i = 1 / (g'(mu_i)^2 V(mu_i)), I = sum w_i x_i x_i'
 *   pearson_chi2 = sum (y_i - mu_i)^2 / V(mu_i); df_resid = n - p'
 *   dispersion = 1 (poisson, binomial), pearson_chi2 / df_resid (gaussian, gamma; NaN when df_resid = 0, and se / z / p / CI / cov too)
 *   cov = dispersion I^-1, se_j = sqrt(cov_jj), z_j = beta_j / se_j, p_j = erfc(|z_j| / sqrt 2), lo / hi = beta_j -+ 1.959963984540054
 *   se_j: the normal distribution for every family (statsmodels' use_t = False)
 *   deviance = sum d_i: gaussian (y - mu)^2, poisson 2 [y ln(y / mu) - (y - mu)], binomial 2 [y ln(y / mu) + (1 - y) ln((1 - y) /
 *   (1 - mu))], gamma 2 [-ln(y / mu) + (y - mu) / mu], with 0 ln 0 = 0
 *   null_deviance = the same sum at the constant mean mean_g(y) with a bias, g^-1(0) without (gaussian 0, poisson 1, binomial 0.5;
 *   gamma: NaN)
 *   report_null = 1 when is_null = 1 or the factorisation of I meets a pivot that is not a positive finite number: every other
 *   report field of the group is then NaN except df_resid; the coefficients stay what the fit returned.  A bad group never
 *   changes another group's bits.
 * Penalised fits have no report.  1 .. 16 feature columns (more: PDS_ERR_UNSUPPORTED).
 */
typedef struct {
    /* each nullable and `space`-resident; the numeric fields are double* for the _f64 entry points, float* for _f32 */
    void* std_err;       /* [n_groups][p'] */
    void* z;             /* [n_groups][p'] */
    void* p;             /* [n_groups][p'] */
    void* ci_lower;      /* [n_groups][p']  "0.025" */
    void* ci_upper;      /* [n_groups][p']  "0.975" */
    void* cov;           /* [n_groups][p'][p'] */
    void* deviance;      /* [n_groups] */
    void* null_deviance; /* [n_groups] */
    void* pearson_chi2;  /* [n_groups] */
    void* dispersion;    /* [n_groups] */
    int64_t* df_resid;   /* [n_groups] */
    uint8_t* report_null; /* [n_groups] */
} pds_glm_report_out;
int pds_glm_report_grouped_f64(pds_ctx* ctx, const double* const* cols, int n_feat, int64_t n_rows, const int64_t* group_offsets,
                               int64_t n_groups, pds_space space, int add_bias, int link, int variance, double tol, int max_iter,
                               double* coeffs, int32_t* n_iter, uint8_t* is_null, const pds_glm_report_out* out);
int pds_glm_report_grouped_f32(pds_ctx* ctx, const float* const* cols, int n_feat, int64_t n_rows, const int64_t* group_offsets,
                               int64_t n_groups, pds_space space, int add_bias, int link, int variance, float tol, int max_iter,
                               float* coeffs, int32_t* n_iter, uint8_t* is_null, const pds_glm_report_out* out);
int pds_glm_report_by_key_f64(pds_ctx* ctx, const double* const* cols, const int64_t* keys, int n_feat, int64_t n_rows, pds_space space,
                              int add_bias, int link, int variance, double tol, int max_iter, int64_t max_groups, int64_t* out_keys,
                              double* coeffs, int32_t* n_iter, uint8_t* is_null, int64_t* n_groups, const pds_glm_report_out* out);
int pds_glm_report_by_key_f32(pds_ctx* ctx, const float* const* cols, const int64_t* keys, int n_feat, int64_t n_rows, pds_space space,
                              int add_bias, int link, int variance, float tol, int max_iter, int64_t max_groups, int64_t* out_keys,
                              float* coeffs, int32_t* n_iter, uint8_t* is_null, int64_t* n_groups, const pds_glm_report_out* out);
/*
 * pds_glm_report_wo_grouped_* / pds_glm_report_wo_by_key_*: the fit of pds_glm_irls_wo_grouped_* / _by_key_* and its report per group --
 * the argument lists of pds_glm_report_grouped_* / _by_key_* with `weights`, `offset` after `cols` (both nullable; both null: the
 * twin's call).  The unscaled convention extended: I = sum pw_i w~_i x_i x_i' with w~ = 1 / (g'^2 V) at mu_i = g^-1(x_i . beta + o_i);
 * pearson_chi2 = sum pw_i (y_i - mu_i)^2 / V(mu_i); deviance = sum pw_i d_i; df_resid = n+ - p' (n+: the rows of positive weight);
 * dispersion, cov, se, z, p and the interval from those as in the twins; null_deviance without an offset: the twins' closed form with
 * weighted sums (at ybar = sum pw y / sum pw under a bias, at g^-1(0) without); with an offset: NaN (the intercept-only model under an
 * offset needs an iteration of its own).  A group that is null by the weight rule has a null report.
 */
int pds_glm_report_wo_grouped_f64(pds_ctx* ctx, const double* const* cols, const double* weights, const double* offset, int n_feat, int64_t n_rows,
                                  const int64_t* group_offsets, int64_t n_groups, pds_space space, int add_bias, int link, int variance,
                                  double tol, int max_iter, double* coeffs, int32_t* n_iter, uint8_t* is_null, const pds_glm_report_out* out);
int pds_glm_report_wo_by_key_f64(pds_ctx* ctx, const double* const* cols, const double* weights, const double* offset, const int64_t* keys, int n_feat,
                                 int64_t n_rows, pds_space space, int add_bias, int link, int variance, double tol, int max_iter,
                                 int64_t max_groups, int64_t* out_keys, double* coeffs, int32_t* n_iter, uint8_t* is_null, int64_t* n_groups,
                                 const pds_glm_report_out* out);
int pds_glm_report_wo_grouped_f32(pds_ctx* ctx, const float* const* cols, const float* weights, const float* offset, int n_feat, int64_t n_rows,
                                  const int64_t* group_offsets, int64_t n_groups, pds_space space, int add_bias, int link, int variance,
                                  float tol, int max_iter, float* coeffs, int32_t* n_iter, uint8_t* is_null, const pds_glm_report_out* out);
int pds_glm_report_wo_by_key_f32(pds_ctx* ctx, const float* const* cols, const float* weights, const float* offset, const int64_t* keys, int n_feat,
                                 int64_t n_rows, pds_space space, int add_bias, int link, int variance, float tol, int max_iter,
                                 int64_t max_groups, int64_t* out_keys, float* coeffs, int32_t* n_iter, uint8_t* is_null, int64_t* n_groups,
                                 const pds_glm_report_out* out);
/*
 * pds_glm_report_robust_* / pds_glm_report_cluster_grouped_* / pds_glm_report_cluster_by_key_*: ONE model over the whole frame with
 * robust (PDS_HC0 / PDS_HC1) or cluster-robust (PDS_CLUSTER / PDS_CLUSTER0) standard errors -- Stata's glm, vce(robust | cluster id),
 * statsmodels' GLM.fit(cov_type="HC0" | "HC1" | "cluster"), R's sandwich::vcovHC / vcovCL on a glm.  cols = [y, x1..xp], 1 .. 16
 * feature columns, the four families, `weights` / `offset` nullable with the meaning of pds_glm_irls_wo_*.  The fit is the existing
 * one: coeffs, n_iter, deviance, null_deviance, pearson_chi2, dispersion and df_resid are bit for bit those of
 * pds_glm_report_wo_grouped_* with group_offsets = [0, n_rows] on the same frame (the offsets and hc forms; the by-key form on the
 * key-ordered frame).  What is new is the covariance.  At the coefficients AS STORED, x_i carrying the constant 1 last under a bias,
 * everything in f64 for f64 and f32 frames alike:
 *   eta_i = x_i . beta + o_i, mu_i = g^-1(eta_i); I = sum pw_i x_i x_i' / (g'(mu_i)^2 V(mu_i)), the information the plain report inverts
 *   r_i = pw_i (y_i - mu_i) / (V(mu_i) g'(mu_i)): the score residual, general in (link, variance); a row with pw_i = 0 has r_i = 0
 *   exactly (a select, so that whatever its mu is reaches no sum)
 *   n = the rows of positive weight (all rows without weights), p' = coefficients
 *   PDS_HC0:      M = sum_i r_i^2 x_i x_i', V = I^-1 M I^-1
 *   PDS_HC1:      the same times n / (n - p')
 *   PDS_CLUSTER0: s_g = sum_{i in g} r_i x_i, M = sum_g s_g s_g', V = I^-1 M I^-1
 *   PDS_CLUSTER:  the same times G / (G - 1) * (n - 1) / (n - p'): statsmodels' default correction, the c of
 *                 pds_lin_reg_report_cluster_*; G counts the clusters that hold at least one row of positive weight
 *   The dispersion cancels in the sandwich and does not enter it (I^-1 = the plain report's cov / dispersion).
 *   se_j = sqrt V_jj, z_j = beta_j / se_j, p_j = erfc(|z_j| / sqrt 2), lo / hi = beta_j -+ 1.959963984540054 se_j: the normal
 *   distribution, as in every GLM report here; *n_clusters (a host int64, nullable) receives G for a caller who wants t(G - 1), 0 for
 *   the hc kinds.  out->cov = V.  `out` has one group's room; its fields and coeffs / n_iter are `space`-resident.
 *   report_null = 1 when the fit is null, I cannot be factorised or a diagonal entry of V is not a non-negative finite number: every
 *   report field is then NaN except df_resid; the coefficients stay what the fit returned.
 * cluster_offsets (grouped): n_offsets + 1 `space`-resident offsets, starting at 0, ending at n_rows, non-decreasing (else
 * PDS_ERR_INVALID); empty clusters change no output bit.  keys (by key): n_rows int64 values in any row order (ordered keys move
 * nothing; weights and offset travel with the frame).  Clusters above the context option "cluster_split_rows" are cut into row
 * chunks; "cluster_waves" caps the waves of the pass.  No floating-point atomic: two calls give the same bits.
 * Refused, never approximated: more than 16 features PDS_ERR_UNSUPPORTED; PDS_HC2 / PDS_HC3 (they need the leverages)
 * PDS_ERR_UNSUPPORTED; any other se_type PDS_ERR_INVALID; a cluster form with G < 2 PDS_ERR_INVALID; PDS_HC1 / PDS_CLUSTER with
 * n <= p' PDS_ERR_TOO_FEW_ROWS.  Penalties have no argument.
 */
int pds_glm_report_robust_f64(pds_ctx* ctx, const double* const* cols, const double* weights, const double* offset, int n_feat, int64_t n_rows,
                              pds_space space, int add_bias, int link, int variance, double tol, int max_iter, int se_type, double* coeffs,
                              int32_t* n_iter, const pds_glm_report_out* out, int64_t* n_clusters);
int pds_glm_report_robust_f32(pds_ctx* ctx, const float* const* cols, const float* weights, const float* offset, int n_feat, int64_t n_rows,
                              pds_space space, int add_bias, int link, int variance, float tol, int max_iter, int se_type, float* coeffs,
                              int32_t* n_iter, const pds_glm_report_out* out, int64_t* n_clusters);
int pds_glm_report_cluster_grouped_f64(pds_ctx* ctx, const double* const* cols, const double* weights, const double* offset, int n_feat,
                                       int64_t n_rows, const int64_t* cluster_offsets, int64_t n_offsets, pds_space space, int add_bias,
                                       int link, int variance, double tol, int max_iter, int se_type, double* coeffs, int32_t* n_iter,
                                       const pds_glm_report_out* out, int64_t* n_clusters);
int pds_glm_report_cluster_grouped_f32(pds_ctx* ctx, const float* const* cols, const float* weights, const float* offset, int n_feat,
                                       int64_t n_rows, const int64_t* cluster_offsets, int64_t n_offsets, pds_space space, int add_bias,
                                       int link, int variance, float tol, int max_iter, int se_type, float* coeffs, int32_t* n_iter,
                                       const pds_glm_report_out* out, int64_t* n_clusters);
int pds_glm_report_cluster_by_key_f64(pds_ctx* ctx, const double* const* cols, const double* weights, const double* offset, const int64_t* keys,
                                      int n_feat, int64_t n_rows, pds_space space, int add_bias, int link, int variance, double tol,
                                      int max_iter, int se_type, double* coeffs, int32_t* n_iter, const pds_glm_report_out* out,
                                      int64_t* n_clusters);
int pds_glm_report_cluster_by_key_f32(pds_ctx* ctx, const float* const* cols, const float* weights, const float* offset, const int64_t* keys,
                                      int n_feat, int64_t n_rows, pds_space space, int add_bias, int link, int variance, float tol,
                                      int max_iter, int se_type, float* coeffs, int32_t* n_iter, const pds_glm_report_out* out,
                                      int64_t* n_clusters);
/*
 * pds_glm_within_grouped_* / pds_glm_within_by_key_*: the fixed-effects GLM -- ONE generalised linear model with an intercept per
 * group, g(E y_i) = alpha_g(i) + x_i' beta + o_i, fitted by IRLS with the group effects absorbed (Stata's ppmlhdfe y x, absorb(firm),
 * fixest::fepois(y ~ x | firm) / feglm): no dummy column is ever formed.  cols = [y, x1..xp], 1 .. 16 feature columns and NO intercept
 * column (it is absorbed); `weights` / `offset` nullable, link / variance as in pds_glm_irls_wo_*.  What follows is a DEFINITION of what
 * the library computes; no equivalence with the small-sample conventions of any package is claimed.
 *   Rows and groups that count.  A weight that is negative or not finite, anywhere: PDS_ERR_INVALID.  A row counts if pw_i > 0.  A
 *     group is DROPPED if it has no counting row, if (variance poisson) every counting row has y == 0, or if (variance binomial) every
 *     counting row has y == 0 or every one has y == 1: its effect would be -inf or +inf (fepois and ppmlhdfe drop such groups too).  The
 *     comparisons are exact and are made once, before the first iteration.  Rows of dropped groups count nowhere.  Gaussian and gamma
 *     drop only groups without a counting row.  Singletons that are not dropped stay in.  n_rows_used and n_groups_used are the counting
 *     rows of the kept groups and the kept groups; n_groups_dropped counts the non-empty groups that were dropped.
 *   Start.  binomial: mu = (y + 0.5) / 2; otherwise mu = (y + ybar) / 2 with ybar = sum pw y / sum pw over the used rows; eta = g(mu).
 *   Iteration.  w_i = pw_i / (g'(mu_i)^2 V(mu_i));  z_i = (eta_i - o_i) + g'(mu_i)(y_i - mu_i);  m_g the w-weighted mean of [x, z] over
 *     group g;  W = sum_g sum_{i in g} w_i ([x_i, z_i] - m_g)([x_i, z_i] - m_g)';  beta solves W_xx beta = W_xz;
 *     alpha_g = m_z,g - m_x,g . beta;  eta_i = alpha_g + x_i . beta + o_i;  mu = g^-1(eta).  By Frisch-Waugh this is exactly the IRLS
 *     step of the design with one dummy column per kept group.
 *   Stopping.  beta starts at 0; the iteration stops when max_j |beta_new,j - beta_j| < tol or after max_iter iterations.  n_iter
 *     counts iterations, converged says which of the two ended it.  A beta or W that is not finite: PDS_ERR_NUMERIC.  There is no step
 *     halving.
 *   Report, at the returned beta, alpha and the last W_xx: deviance and pearson_chi2 as in pds_glm_report_wo_*, summed over the used
 *     rows; df_resid = n_rows_used - n_groups_used - p; dispersion phi = 1 (poisson, binomial), pearson_chi2 / df_resid (gaussian, gamma).
 *     PDS_SE        V = phi W_xx^-1
 *     PDS_CLUSTER0  V = W_xx^-1 M W_xx^-1, M = sum_g s_g s_g', s_g = sum_{i in g} r_i (x_i - m_x,g),
 *                   r_i = pw_i (y_i - mu_i) / (V(mu_i) g'(mu_i)): the clusters ARE the absorbed groups
 *     PDS_CLUSTER   the same V times G / (G - 1) * (n - 1) / (n - p - 1), G = n_groups_used, n = n_rows_used (the definition of
 *                   pds_lin_reg_within_*)
 *     z_j = beta_j / se_j, p_j = erfc(|z_j| / sqrt 2), lo / hi = beta_j -+ 1.959963984540054 se_j: the normal distribution, as in every
 *     GLM report here.  out->cov = V, p x p row-major.
 * The report fields are host doubles for both precisions (an f32 frame is fitted in f64 arithmetic).  alpha / pred: nullable,
 * `space`-resident arrays of the frame's type.  alpha: one value per group, NaN for a dropped or empty group; pred = mu_i per row in the
 * caller's row order, NaN on the rows of dropped groups, a value on the zero-weight rows of kept groups.
 *   grouped: group g = rows [group_offsets[g], group_offsets[g+1]); n_groups + 1 int64 values, `space`-resident, starting at 0, ending
 *            at n_rows, non-decreasing (else PDS_ERR_INVALID).  alpha has n_groups entries.  An empty group changes no output bit.
 *   by key:  keys = n_rows int64 values in any row order (ordered keys move nothing and give the bits of the grouped form; weights and
 *            offset travel with the frame).  *n_groups receives the distinct keys.  max_groups and out_keys matter only when out->alpha
 *            is given: alpha and out_keys (nullable) then have room for max_groups entries, in ascending key order, and more distinct
 *            keys are PDS_ERR_INVALID with *n_groups set (nothing fitted).
 * The call is one pre-pass, one stream over the frame per iteration (the state between iterations is beta and the group means; one
 * blocking copy of a record and a p x p host solve per iteration) and one final pass.  No floating-point atomic: two calls give the same
 * bits.  Groups above the context option "within_split_rows" are cut into row chunks.  Refused, never approximated: a feature that does
 * not vary inside any kept group (exact comparison with the group's first counting row) PDS_ERR_NUMERIC, the message naming the column
 * index; a pivot of W_xx below 1e-13 of its diagonal PDS_ERR_NUMERIC; df_resid <= 0 PDS_ERR_TOO_FEW_ROWS; a cluster kind with fewer than
 * two kept groups PDS_ERR_INVALID; more than 16 features PDS_ERR_UNSUPPORTED; PDS_HC0 .. PDS_HC3 PDS_ERR_UNSUPPORTED.  Two absorbed
 * keys, clusters on another key and penalties have no argument.
 */
typedef struct {
    double beta[16], std_err[16], z[16], p[16], ci_lower[16], ci_upper[16]; /* the first p entries */
    double cov[256];                                                         /* p x p, row-major */
    double deviance, pearson_chi2, dispersion;
    int64_t n_groups_used, n_groups_dropped, n_rows_used, df_resid;
    int32_t n_iter, converged;
    void* alpha; /* in, nullable: [n_groups] (by key: [max_groups], ascending key order) */
    void* pred;  /* in, nullable: [n_rows], frame order */
} pds_glm_within_out;
int pds_glm_within_grouped_f64(pds_ctx* ctx, const double* const* cols, const double* weights, const double* offset, int n_feat, int64_t n_rows,
                               const int64_t* group_offsets, int64_t n_groups, pds_space space, int link, int variance, double tol,
                               int max_iter, int se_type, pds_glm_within_out* out);
int pds_glm_within_grouped_f32(pds_ctx* ctx, const float* const* cols, const float* weights, const float* offset, int n_feat, int64_t n_rows,
                               const int64_t* group_offsets, int64_t n_groups, pds_space space, int link, int variance, float tol,
                               int max_iter, int se_type, pds_glm_within_out* out);
int pds_glm_within_by_key_f64(pds_ctx* ctx, const double* const* cols, const double* weights, const double* offset, const int64_t* keys,
                              int n_feat, int64_t n_rows, pds_space space, int link, int variance, double tol, int max_iter, int se_type,
                              int64_t max_groups, int64_t* out_keys, pds_glm_within_out* out, int64_t* n_groups);
int pds_glm_within_by_key_f32(pds_ctx* ctx, const float* const* cols, const float* weights, const float* offset, const int64_t* keys,
                              int n_feat, int64_t n_rows, pds_space space, int link, int variance, float tol, int max_iter, int se_type,
                              int64_t max_groups, int64_t* out_keys, pds_glm_within_out* out, int64_t* n_groups);
/*
 * pds_lr_rcond_grouped_* / pds_lr_rcond_by_key_*: `lin_reg_w_rcond` per group in one call -- for every group g what pds_lr_rcond_*
 * computes on g's rows alone (faer_solve_lr_rcond, lr_solvers.rs:225-254): X'X (+ l2_reg on the feature diagonals) is decomposed on
 * chip by the one-sided Jacobi iteration of the single-system call, singular values below the cut are dropped, the coefficients are
 * the minimum-norm solution (grouped_rcond.hip: one wave per group, one pass over its rows).
 * cols = [y, x1..xp], 1 .. 16 feature columns (more: PDS_ERR_UNSUPPORTED); f32 frames are fitted in f64 arithmetic.
 * rcond is the caller's value (kwargs.tol); the floor of pl_lr_w_rcond is applied per group with the group's own row count:
 * rcond_g = max(rcond, eps_T * max(n_g, p')), eps_T the epsilon of the frame type.
 * Outputs, `space`-resident: coeffs and singular_values [n_groups][n_feat + add_bias] (bias last; singular values descending),
 * is_null [n_groups] bytes: 1 (NaN coefficients and singular values) for a group whose offsets leave the frame (nothing is read), a
 * group with fewer rows than coefficients, a group with a non-finite entry in its moments (the single-system call answers
 * "SVD failed.") and a group whose final coefficients are not all finite (the all-zero system); a bad group never changes another
 * group's bits.  Two calls give the same bits, and a group's bits do not depend on its place in the frame.
 * By key: int64 keys in any row order, groups returned in ascending key order (ordered keys: nothing moves; unordered keys: sort +
 * gather); *n_groups receives the number of distinct keys, also when it exceeds max_groups (PDS_ERR_INVALID, nothing fitted).
 */
int pds_lr_rcond_grouped_f64(pds_ctx* ctx, const double* const* cols, int n_feat, int64_t n_rows, const int64_t* group_offsets,
                             int64_t n_groups, pds_space space, int add_bias, double l2_reg, double rcond, double* coeffs,
                             double* singular_values, uint8_t* is_null);
int pds_lr_rcond_grouped_f32(pds_ctx* ctx, const float* const* cols, int n_feat, int64_t n_rows, const int64_t* group_offsets,
                             int64_t n_groups, pds_space space, int add_bias, float l2_reg, float rcond, float* coeffs,
                             float* singular_values, uint8_t* is_null);
int pds_lr_rcond_by_key_f64(pds_ctx* ctx, const double* const* cols, const int64_t* keys, int n_feat, int64_t n_rows, pds_space space,
                            int add_bias, double l2_reg, double rcond, int64_t max_groups, int64_t* out_keys, double* coeffs,
                            double* singular_values, uint8_t* is_null, int64_t* n_groups);
int pds_lr_rcond_by_key_f32(pds_ctx* ctx, const float* const* cols, const int64_t* keys, int n_feat, int64_t n_rows, pds_space space,
                            int add_bias, float l2_reg, float rcond, int64_t max_groups, int64_t* out_keys, float* coeffs,
                            float* singular_values, uint8_t* is_null, int64_t* n_groups);
/*
 * pds_lr_multi_grouped_* / pds_lr_multi_by_key_*: `lin_reg(target=[t_0 .. t_{k-1}], by=key)` -- for every group g what pds_lr_multi_*
 * computes on g's rows alone (pl_lr_multi under group_by / over): k targets share the group's design matrix.  The frame is staged
 * once and the keys are ordered once for all k targets.
 * cols = [t_0 .. t_{k-1}, x_1 .. x_p], the order of pds_lr_multi_*.  1 .. 16 feature columns, 1 .. 15 targets; anything beyond is
 * PDS_ERR_UNSUPPORTED ("grouped multi-target lin_reg: up to 16 feature columns and 15 targets"), never an approximate answer.
 * OLS / ridge (l2_reg on the feature diagonals, never on the intercept); f32 frames are fitted in f64 arithmetic.
 * The gate and the null rule are pds_lr_grouped_*'s, group for group: null (is_null = 1, NaN coefficients) are a group whose offsets
 * leave the frame (nothing is read), a group with fewer rows than coefficients, a group with a non-finite moment, and a group the
 * rank gate rejects (singular_x_tol; <= 0: no gate; solver as in pds_lr_params, PDS_SOLVER_SVD runs the pivoted QR as in
 * pds_lr_multi_*).  The gate depends on X alone: a group is null for every target or for none, so a NaN in ONE target nulls the group
 * (route 2 finds such a group by its coefficients: a gated group with a coefficient that is not finite is null).
 * Context option "grouped_multi_route": 1 = one kernel (grouped_multi.hip: one wave per group, X'X and all X't_c from one pass over
 * the group's rows, one L D L' factorisation, k substitutions; groups next to the gate go through the pivoted QR unless the solver
 * is PDS_SOLVER_CHOLESKEY), 2 = the fused kernel of pds_lr_grouped_* once per target on the one staged frame, 0 (default) = whichever
 * measured faster for the shape.  With singular_x_tol <= 0 every route runs the grouped Gram records and the pivoted QR per target.
 * Routes 0 / 2, the ungated form and the per-row outputs need offsets that are non-decreasing and inside the frame (a gated call
 * without per-row outputs falls back to route 1, which reads nothing of a bad group; otherwise PDS_ERR_INVALID).
 * "grouped_multi_waves": cap on the number of waves route 1 starts (<= 0: every wave slot); it changes no result bit.
 * Outputs, `space`-resident: coeffs [n_groups][n_targets][n_feat + add_bias] (bias last), is_null [n_groups]; optional pred / resid
 * [n_targets][n_rows] (target-major) and row_null [n_rows] (1 on the rows of null groups, whose pred / resid are NaN), in the frame's
 * own row order.
 * By key: int64 keys in any row order, groups returned in ascending key order; *n_groups receives the number of distinct keys, also
 * when it exceeds max_groups (PDS_ERR_INVALID, nothing fitted).  A caller that only wants the per-row outputs passes NULL for
 * out_keys, coeffs, is_null and n_groups (max_groups is then not looked at), as with pds_lr_by_key_pred_*.
 */
int pds_lr_multi_grouped_f64(pds_ctx* ctx, const double* const* cols, int n_targets, int n_feat, int64_t n_rows, const int64_t* group_offsets,
                             int64_t n_groups, pds_space space, int add_bias, double l2_reg, int solver, double singular_x_tol, double* coeffs,
                             uint8_t* is_null, double* pred, double* resid, uint8_t* row_null);
int pds_lr_multi_grouped_f32(pds_ctx* ctx, const float* const* cols, int n_targets, int n_feat, int64_t n_rows, const int64_t* group_offsets,
                             int64_t n_groups, pds_space space, int add_bias, float l2_reg, int solver, float singular_x_tol, float* coeffs,
                             uint8_t* is_null, float* pred, float* resid, uint8_t* row_null);
int pds_lr_multi_by_key_f64(pds_ctx* ctx, const double* const* cols, const int64_t* keys, int n_targets, int n_feat, int64_t n_rows, pds_space space,
                            int add_bias, double l2_reg, int solver, double singular_x_tol, int64_t max_groups, int64_t* out_keys, double* coeffs,
                            uint8_t* is_null, int64_t* n_groups, double* pred, double* resid, uint8_t* row_null);
int pds_lr_multi_by_key_f32(pds_ctx* ctx, const float* const* cols, const int64_t* keys, int n_targets, int n_feat, int64_t n_rows, pds_space space,
                            int add_bias, float l2_reg, int solver, float singular_x_tol, int64_t max_groups, int64_t* out_keys, float* coeffs,
                            uint8_t* is_null, int64_t* n_groups, float* pred, float* resid, uint8_t* row_null);
/*
 * pds_mixed_reml_grouped_* / pds_mixed_reml_by_key_* / pds_mixed_profile_grouped_*: the random-intercept linear mixed model
 * y = X beta + Z u + e, u ~ N(0, sigma_g^2 I), e ~ N(0, sigma_e^2 I), fitted by REML as fit_reml does (src/linear/mixed/mod.rs:173-272):
 * golden section over gamma = sigma_g^2 / sigma_e^2 in [0, 1e6] on the profiled deviance
 *   dev(gamma) = (n - p') ln(r' H^-1 r / (n - p')) + sum_g ln(1 + gamma n_g) + ln det(X' H^-1 X),   H = I + gamma Z Z',
 * bracket and update order as lines 195-219, stop at hi - lo < tol or after max_iter steps, gamma = (lo + hi) / 2.
 * cols = [y, x1..xp], 1 .. 16 feature columns (more: PDS_ERR_UNSUPPORTED); X = [1 | x1..xp], p' = p + 1, the intercept FIRST.  f32
 * frames are fitted in f64 arithmetic.  Groups: contiguous rows [group_offsets[g], group_offsets[g+1]) (`space`-resident, n_groups + 1
 * values, non-decreasing, inside the frame; empty groups are allowed and ignored), or int64 keys in any row order (ordered keys move
 * nothing; otherwise sort + gather).  The frame is streamed a fixed number of times (group means, the within-group scatter W, which
 * features vary inside a group: mixed.hip); an evaluation is then a reduction over the groups,
 *   [X y]' H^-1 [X y] = W + sum_g n_g / (1 + gamma n_g) [1, m_g] [1, m_g]',
 * one blocking copy of a 296-double record per evaluation, factored on the host.  Two calls give the same bits.
 * Outputs are doubles in HOST memory whatever `space` is: coeffs / std_errors / dfs [p'] (std_errors = sqrt(resid_variance
 * diag((X' H^-1 X)^-1)) at the optimum; dfs by containment, mod.rs:233-263: the intercept and every feature that is constant inside
 * every group get G - rank(those columns), the others n - rank([X | Z]), G = non-empty groups), *gamma, *resid_variance,
 * *n_groups_fit = G, *n_eval = deviance evaluations (two to start, one per step, one at the optimum).
 * Deliberate deviations: (1) the two ranks come from column-pivoted Cholesky factors of Gram matrices (rank([X | Z]) = G +
 * rank(W_xx)), a pivot counting above 1e-12 of the first; the reference's cutoff is 1e-9 on |R_ii| / |R_00| of a QR of the rows,
 * i.e. 1e-18 on a Gram pivot, which f64 cannot resolve -- this matters only for within-group column dependence between 1e-9 and 1e-6;
 * (2) the leading block counts as not positive definite when a Cholesky pivot falls below 1e-13 of its diagonal entry (an exactly
 * duplicated column would otherwise pass or fail by rounding).
 * pds_mixed_profile_grouped_*: the search-free form -- for each of n_gammas values (host array, finite, >= 0) deviance [k],
 * beta [k][p'] (the GLS coefficients at that gamma) and resid_variance [k], host arrays.
 * Errors: PDS_ERR_INVALID (null arguments, offsets that decrease or leave the frame, max_iter < 0, tol not finite);
 * PDS_ERR_TOO_FEW_ROWS "Not enough rows to fit a mixed model with this many fixed effects." (n <= p'); PDS_ERR_NUMERIC "X'HiX is not
 * positive definite; design may be rank-deficient." / "Residual variance estimate is non-positive." (NaN included).
 */
int pds_mixed_reml_grouped_f64(pds_ctx* ctx, const double* const* cols, int n_feat, int64_t n_rows, const int64_t* group_offsets,
                               int64_t n_groups, pds_space space, int max_iter, double tol, double* coeffs, double* std_errors, double* dfs,
                               double* gamma, double* resid_variance, int64_t* n_groups_fit, int32_t* n_eval);
int pds_mixed_reml_grouped_f32(pds_ctx* ctx, const float* const* cols, int n_feat, int64_t n_rows, const int64_t* group_offsets,
                               int64_t n_groups, pds_space space, int max_iter, double tol, double* coeffs, double* std_errors, double* dfs,
                               double* gamma, double* resid_variance, int64_t* n_groups_fit, int32_t* n_eval);
int pds_mixed_reml_by_key_f64(pds_ctx* ctx, const double* const* cols, const int64_t* keys, int n_feat, int64_t n_rows, pds_space space,
                              int max_iter, double tol, double* coeffs, double* std_errors, double* dfs, double* gamma,
                              double* resid_variance, int64_t* n_groups_fit, int32_t* n_eval);
int pds_mixed_reml_by_key_f32(pds_ctx* ctx, const float* const* cols, const int64_t* keys, int n_feat, int64_t n_rows, pds_space space,
                              int max_iter, double tol, double* coeffs, double* std_errors, double* dfs, double* gamma,
                              double* resid_variance, int64_t* n_groups_fit, int32_t* n_eval);
int pds_mixed_profile_grouped_f64(pds_ctx* ctx, const double* const* cols, int n_feat, int64_t n_rows, const int64_t* group_offsets,
                                  int64_t n_groups, pds_space space, const double* gammas, int n_gammas, double* deviance, double* beta,
                                  double* resid_variance);
int pds_mixed_profile_grouped_f32(pds_ctx* ctx, const float* const* cols, int n_feat, int64_t n_rows, const int64_t* group_offsets,
                                  int64_t n_groups, pds_space space, const double* gammas, int n_gammas, double* deviance, double* beta,
                                  double* resid_variance);
/*
 * pds_lin_reg_report_grouped_* / pds_lin_reg_report_by_key_*: `df.group_by(key).agg(pds.lin_reg_report(...))` in one call -- for
 * every group g what pds_lin_reg_report_* returns on g's rows alone (same se_type / add_bias, beta = (X'X)^-1 X'y through the
 * column-pivoted QR inverse, report_epilogue's formulas).  Deliberate deviations from a per-group pl_lin_reg_report call:
 *   1. a group with fewer rows than coefficients (or none) gets is_null = 1 and NaN outputs (the reference raises
 *      "#Data < #features" and aborts the whole query), as pds_lr_grouped_* does;
 *   2. var(y) per group is the target's sample variance (ddof = 1) from f64 sums of y - y_first on the device, unless the offsets
 *      form is given y_var (n_groups values, `space`-resident);
 *   3. p-values are computed on the device, within 2e-13 relative of pds_student_t_sf (the device's exp / log may differ from
 *      the host's in the last bit); the CI quantile is the host's student_t_ppf, once per distinct dof (bit-identical to the
 *      single report's).
 * Groups with n_g == p' (dof 0) or singular Gram matrices are not null (is_null = 0): a dof-0 group's beta is its exact-fit
 * solution and its se / hc1 standard errors (which divide by dof) are not finite; a singular group's values are whatever the
 * pivoted-QR inverse gives (not necessarily finite, nor equal to a single report's).  A group holding NaN / inf or a singular
 * design does not change any other group's outputs (bit for bit).
 * 1..64 features (more: PDS_ERR_UNSUPPORTED).  Output arrays are `space`-resident: beta .. ci_upper [n_groups][p'] row-major
 * (bias last), r2 / adj_r2 [n_groups], is_null [n_groups] bytes.  Context option "report_chunk_groups" sets how many groups one
 * pass works on (workspace bound; default from a 128 MiB record budget).
 */
typedef struct {
    double* beta;
    double* std_err;
    double* t;
    double* p;
    double* ci_lower;
    double* ci_upper;
    double* r2;
    double* adj_r2;
    uint8_t* is_null;
} pds_report_grouped_f64;
typedef struct {
    float* beta;
    float* std_err;
    float* t;
    float* p;
    float* ci_lower;
    float* ci_upper;
    float* r2;
    float* adj_r2;
    uint8_t* is_null;
} pds_report_grouped_f32;
int pds_lin_reg_report_grouped_f64(pds_ctx* ctx, const double* const* cols, int n_feat, int64_t n_rows, const int64_t* group_offsets,
                                   int64_t n_groups, pds_space space, int add_bias, int se_type, const double* y_var,
                                   pds_report_grouped_f64* out);
int pds_lin_reg_report_grouped_f32(pds_ctx* ctx, const float* const* cols, int n_feat, int64_t n_rows, const int64_t* group_offsets,
                                   int64_t n_groups, pds_space space, int add_bias, int se_type, const float* y_var,
                                   pds_report_grouped_f32* out);
/* keys: n_rows int64 values in any row order (`space`-resident); groups come back in ascending key order (out_keys, `space`);
 * max_groups: capacity of the outputs; n_groups: out (host).  Ordered keys move no data; others take the sorting route of
 * pds_lr_by_key_*.  var(y) is always derived per group. */
int pds_lin_reg_report_by_key_f64(pds_ctx* ctx, const double* const* cols, const int64_t* keys, int n_feat, int64_t n_rows,
                                  pds_space space, int add_bias, int se_type, int64_t max_groups, int64_t* out_keys,
                                  pds_report_grouped_f64* out, int64_t* n_groups);
int pds_lin_reg_report_by_key_f32(pds_ctx* ctx, const float* const* cols, const int64_t* keys, int n_feat, int64_t n_rows,
                                  pds_space space, int add_bias, int se_type, int64_t max_groups, int64_t* out_keys,
                                  pds_report_grouped_f32* out, int64_t* n_groups);
/*
 * pds_wls_report_grouped_* / pds_wls_report_by_key_*: the weighted form of the grouped report -- for every group g what
 * pds_lin_reg_report_* returns on g's rows with `weights` given (pl_wls_report, linear_regression.rs:982-1117): beta =
 * (X'WX)^-1 X'Wy through the column-pivoted QR inverse, mse = sum w e^2 / dof with dof = n_g - p', std_err_i = sqrt(mse inv_ii),
 * t / p / CI as in the unweighted grouped report, r2 = 1 - sum e^2 / (var(y) n_g) with the UNWEIGHTED sum e^2 and the unweighted
 * sample variance of the group's target (ddof = 1).  Plain standard error only (pl_wls_report knows no HC estimator).
 * weights: n_rows values, `space`-resident; NULL gives PDS_ERR_INVALID.  Weights enter X'WX as they are, whatever their sign (they
 * are never square-rooted and no scaled copy of the frame is made).  Zero weights are legal: such rows still count in n_g, in dof
 * and in the unweighted sum e^2.  Output struct, null rule (n_g < p': is_null = 1, NaN outputs), dof-0 and singular groups, the
 * isolation of groups, y_var (nullable, offsets form only), the 1..64 feature range, both memory spaces and the
 * "report_chunk_groups" option are those of pds_lin_reg_report_grouped_* / _by_key_* above.  By key, unordered keys take the
 * weights through the sort and the gather as one more column (fewer than 2^31 rows); ordered keys move nothing.  Repeated calls
 * give the same bits.
 */
int pds_wls_report_grouped_f64(pds_ctx* ctx, const double* const* cols, const double* weights, int n_feat, int64_t n_rows,
                               const int64_t* group_offsets, int64_t n_groups, pds_space space, int add_bias, const double* y_var,
                               pds_report_grouped_f64* out);
int pds_wls_report_grouped_f32(pds_ctx* ctx, const float* const* cols, const float* weights, int n_feat, int64_t n_rows,
                               const int64_t* group_offsets, int64_t n_groups, pds_space space, int add_bias, const float* y_var,
                               pds_report_grouped_f32* out);
int pds_wls_report_by_key_f64(pds_ctx* ctx, const double* const* cols, const double* weights, const int64_t* keys, int n_feat,
                              int64_t n_rows, pds_space space, int add_bias, int64_t max_groups, int64_t* out_keys,
                              pds_report_grouped_f64* out, int64_t* n_groups);
int pds_wls_report_by_key_f32(pds_ctx* ctx, const float* const* cols, const float* weights, const int64_t* keys, int n_feat,
                              int64_t n_rows, pds_space space, int add_bias, int64_t max_groups, int64_t* out_keys,
                              pds_report_grouped_f32* out, int64_t* n_groups);
/* TEST HOOK, not part of the supported interface: the grouped report's device Student-t survival function on host arrays
 * x[n], df[n] -> out[n], so that tests can hold it against pds_student_t_sf.  May change or go away without notice. */
int pds_student_t_sf_device(pds_ctx* ctx, const double* x, const double* df, int64_t n, double* out);

int pds_glm_irls_f32(pds_ctx* ctx, const float* const* cols, int n_feat, int64_t n_rows, pds_space space, int add_bias, int link,
                     int variance, float tol, int max_iter, float* coeffs, int* n_iter);

/* Fits straight from a ROW-MAJOR matrix -- the pyclass route (PyLR / PyElasticNet / PyOnlineLR, src/pymodels/py_lr.rs:21-224,
 * whose NumPy X the reference reads through a strided faer MatRef, src/pymodels/numpy_faer.rs:10-66).
 * X: n_rows x n_feat values, row stride ld (elements); y: n_rows values; both resident in `space`.
 * mode 0: LR::fit -- the pl_lr dispatch of `prm` (faer_solve_lr, lr_solvers.rs:65-73; pass singular_x_tol = 0 for the model class);
 * mode 1: ElasticNet::fit -- always faer_coordinate_descent with prm's l1_reg / l2_reg / tol / max_iter (lr_solvers.rs:139-164);
 * mode 2: OnlineLR::fit -- faer_qr_lr_with_inv (lr_online_solvers.rs:120-143): coeffs and inv = (X'X + lambda I)^-1 with
 *         lambda = prm->l2_reg on the feature diagonals, (n_feat + add_bias)^2 values column-major (inv required).
 * Up to 16 features the matrix core reads the rows as they lie (one pass, no transposition; host matrices as contiguous row
 * chunks); wider matrices are transposed once on the device.  coeffs: n_feat + add_bias values, bias last. */
int pds_lr_rowmajor_f64(pds_ctx* ctx, const double* X, int64_t ld, const double* y, int64_t n_rows, int n_feat, pds_space space,
                        const pds_lr_params* prm, int mode, double* coeffs, int* is_null, double* inv);
int pds_lr_rowmajor_f32(pds_ctx* ctx, const float* X, int64_t ld, const float* y, int64_t n_rows, int n_feat, pds_space space,
                        const pds_lr_params* prm, int mode, float* coeffs, int* is_null, float* inv);

/* Row-major matrix -> the contiguous column buffers every entry point takes (the pyclass route: the NumPy X of LR /
 * ElasticNet / OnlineLR, which the reference reads through a strided faer MatRef, src/pymodels/numpy_faer.rs:10-66).
 * X: n_rows x n_cols values with row stride ld (elements), resident in `space`.  out_cols: DEVICE buffer; column c is
 * written to out_cols + c * col_stride (col_stride >= n_rows).  Host matrices cross PCIe as contiguous row chunks. */
int pds_rows_to_cols_f64(pds_ctx* ctx, const double* X, int64_t ld, int64_t n_rows, int n_cols, pds_space space, double* out_cols,
                         int64_t col_stride);
int pds_rows_to_cols_f32(pds_ctx* ctx, const float* X, int64_t ld, int64_t n_rows, int n_cols, pds_space space, float* out_cols,
                         int64_t col_stride);

#ifdef __cplusplus
}
#endif
#endif /* PDS_LSTSQ_H */
