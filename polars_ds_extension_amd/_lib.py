"""
ctypes binding of libpds_lstsq_hip.so (the C ABI of include/pds_lstsq.h).

The library is built in-tree by `polars_ds_extension_amd._build.build()` (hipcc, gfx950).  There is NO
CPU fallback: if the shared object is missing or the device is not an MI355X-class gfx950 GPU every
entry point raises -- a silently different code path would void the parity claims.
"""
from __future__ import annotations

import ctypes as C
from pathlib import Path

_HERE = Path(__file__).resolve().parent
LIB_PATH = _HERE / "csrc" / "libpds_lstsq_hip.so"

PDS_HOST, PDS_DEVICE = 0, 1
SOLVERS = {"qr": 0, "svd": 1, "choleskey": 2}  # any other string -> qr (src/linear/lr/mod.rs:17-26)
SE_TYPES = {"se": 0, "hc0": 1, "hc1": 2, "hc2": 3, "hc3": 4}
WITHIN_SE_TYPES = {"se": 0, "cluster": 5, "cluster0": 6}  # pds_lin_reg_within_*: the clusters are the absorbed groups
CLUSTER_SE_TYPES = {"cluster": 5, "cluster0": 6}  # PDS_CLUSTER (CR1) / PDS_CLUSTER0 (CR0): pds_lin_reg_report_cluster_* only
GLM_ROBUST_SE_TYPES = {"hc0": 1, "hc1": 2, "hc2": 3, "hc3": 4, "cluster": 5, "cluster0": 6}  # pds_glm_report_robust_* / _cluster_*
PDS_REPORT_DERIVE_YVAR = 0x100  # include/pds_lstsq.h

EXPORTS = [
    "pds_last_error", "pds_version", "pds_ctx_create", "pds_ctx_destroy", "pds_ctx_set_stream",
    "pds_ctx_synchronize", "pds_ctx_num_cus", "pds_ctx_set_option", "pds_ctx_get_option", "pds_grouped_fused_split", "pds_set_host_staging", "pds_rows_to_cols_f64", "pds_rows_to_cols_f32", "pds_glm_irls_f64", "pds_glm_irls_f32", "pds_glm_irls_grouped_f64", "pds_glm_irls_grouped_f32", "pds_glm_irls_by_key_f64", "pds_glm_irls_by_key_f32",
    "pds_glm_irls_wo_f64", "pds_glm_irls_wo_f32", "pds_glm_irls_wo_grouped_f64", "pds_glm_irls_wo_grouped_f32", "pds_glm_irls_wo_by_key_f64", "pds_glm_irls_wo_by_key_f32",
    "pds_glm_enet_f64", "pds_glm_enet_f32", "pds_glm_enet_grouped_f64", "pds_glm_enet_grouped_f32", "pds_glm_enet_by_key_f64", "pds_glm_enet_by_key_f32",
    "pds_glm_report_wo_grouped_f64", "pds_glm_report_wo_grouped_f32", "pds_glm_report_wo_by_key_f64", "pds_glm_report_wo_by_key_f32",
    "pds_glm_report_grouped_f64", "pds_glm_report_grouped_f32", "pds_glm_report_by_key_f64", "pds_glm_report_by_key_f32",
    "pds_glm_report_robust_f64", "pds_glm_report_robust_f32", "pds_glm_report_cluster_grouped_f64", "pds_glm_report_cluster_grouped_f32",
    "pds_glm_report_cluster_by_key_f64", "pds_glm_report_cluster_by_key_f32",
    "pds_glm_within_grouped_f64", "pds_glm_within_grouped_f32", "pds_glm_within_by_key_f64", "pds_glm_within_by_key_f32",
    "pds_lr_rcond_grouped_f64", "pds_lr_rcond_grouped_f32", "pds_lr_rcond_by_key_f64", "pds_lr_rcond_by_key_f32",
    "pds_lr_multi_grouped_f64", "pds_lr_multi_grouped_f32", "pds_lr_multi_by_key_f64", "pds_lr_multi_by_key_f32",
    "pds_mixed_reml_grouped_f64", "pds_mixed_reml_grouped_f32", "pds_mixed_reml_by_key_f64", "pds_mixed_reml_by_key_f32",
    "pds_mixed_profile_grouped_f64", "pds_mixed_profile_grouped_f32",
    "pds_lr_rowmajor_f64", "pds_lr_rowmajor_f32", "pds_ctx_workspace_spills", "pds_ctx_workspace_bytes", "pds_ctx_set_timing", "pds_ctx_get_timing", "pds_ctx_get_timing_samples",
    "pds_lr_f64", "pds_lr_f32", "pds_lr_pred_f64", "pds_lr_pred_f32", "pds_lr_rcond_f64", "pds_lr_rcond_f32", "pds_elastic_net_f64", "pds_elastic_net_f32", "pds_lr_nullable_f64", "pds_lr_nullable_f32", "pds_lr_multi_f64", "pds_lr_multi_f32",
    "pds_lin_reg_report_f64", "pds_lin_reg_report_f32",
    "pds_lin_reg_report_grouped_f64", "pds_lin_reg_report_grouped_f32", "pds_lin_reg_report_by_key_f64", "pds_lin_reg_report_by_key_f32",
    "pds_lin_reg_report_cluster_grouped_f64", "pds_lin_reg_report_cluster_grouped_f32",
    "pds_lin_reg_report_cluster_by_key_f64", "pds_lin_reg_report_cluster_by_key_f32",
    "pds_lin_reg_within_grouped_f64", "pds_lin_reg_within_grouped_f32", "pds_lin_reg_within_by_key_f64", "pds_lin_reg_within_by_key_f32",
    "pds_lin_reg_within2_grouped_f64", "pds_lin_reg_within2_grouped_f32", "pds_lin_reg_within2_by_key_f64", "pds_lin_reg_within2_by_key_f32",
    "pds_lin_reg_within2_fx_grouped_f64", "pds_lin_reg_within2_fx_grouped_f32", "pds_lin_reg_within2_fx_by_key_f64", "pds_lin_reg_within2_fx_by_key_f32",
    "pds_absorb_components_i32",
    "pds_lin_reg_within_cl_grouped_f64", "pds_lin_reg_within_cl_grouped_f32", "pds_lin_reg_within_cl_by_key_f64", "pds_lin_reg_within_cl_by_key_f32",
    "pds_lin_reg_within2_cl_grouped_f64", "pds_lin_reg_within2_cl_grouped_f32", "pds_lin_reg_within2_cl_by_key_f64", "pds_lin_reg_within2_cl_by_key_f32",
    "pds_wls_report_grouped_f64", "pds_wls_report_grouped_f32", "pds_wls_report_by_key_f64", "pds_wls_report_by_key_f32",
    "pds_student_t_sf_device",
    "pds_report_fit_from_moments_f64", "pds_report_fit_from_moments_f32", "pds_report_partials_f64", "pds_report_partials_f32",
    "pds_report_finish_f64", "pds_report_finish_f32",
    "pds_lr_grouped_f64", "pds_lr_grouped_f32",
    "pds_rolling_lr_f64", "pds_rolling_lr_f32", "pds_recursive_lr_f64", "pds_recursive_lr_f32",
    "pds_recursive_lr_seeded_f64", "pds_recursive_lr_seeded_f32",
    "pds_rolling_lr_grouped_f64", "pds_rolling_lr_grouped_f32", "pds_recursive_lr_grouped_f64", "pds_recursive_lr_grouped_f32",
    "pds_rolling_lr_by_key_f64", "pds_rolling_lr_by_key_f32", "pds_recursive_lr_by_key_f64", "pds_recursive_lr_by_key_f32",
    "pds_lin_reg_report_nullable_f64", "pds_lin_reg_report_nullable_f32",
    "pds_lr_grouped_nullable_f64", "pds_lr_grouped_nullable_f32",
    "pds_lr_by_key_f64", "pds_lr_by_key_f32", "pds_lr_by_key_multi_f64", "pds_lr_by_key_multi_f32", "pds_lr_by_key_pred_multi_f64", "pds_lr_by_key_pred_multi_f32", "pds_host_alloc", "pds_host_free", "pds_device_count", "pds_device_alloc", "pds_device_free", "pds_ipc_export", "pds_ipc_open", "pds_ipc_close", "pds_signal_post", "pds_signal_wait", "pds_signal_wait_status", "pds_lr_grouped_pred_f64", "pds_lr_grouped_pred_f32", "pds_lr_by_key_pred_f64", "pds_lr_by_key_pred_f32", "pds_lr_grouped_weighted_f64", "pds_lr_grouped_weighted_f32",
    "pds_lr_with_inv_f64", "pds_lr_with_inv_f32",
    "pds_moments_f64", "pds_moments_f32", "pds_lr_from_moments_f64", "pds_lr_from_moments_f32",
    "pds_student_t_sf", "pds_student_t_ppf",
    "pds_allreduce_sum_f64", "pds_allreduce_sum_f32", "pds_scatter_rows_f64", "pds_scatter_rows_f32", "pds_gather_f64", "pds_gather_f32",
]


class LRParams(C.Structure):
    """pds_lr_params == the numeric fields of LRKwargs (src/num_ext/linear_regression.rs:27-45)."""

    _fields_ = [
        ("add_bias", C.c_int),
        ("l1_reg", C.c_double),
        ("l2_reg", C.c_double),
        ("tol", C.c_double),
        ("solver", C.c_int),
        ("positive", C.c_int),
        ("max_iter", C.c_int),
        ("singular_x_tol", C.c_double),
    ]


class ReportF64(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("beta", "std_err", "t", "p", "ci_lower", "ci_upper")] + [
        ("r2", C.c_double),
        ("adj_r2", C.c_double),
    ]


class ReportF32(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("beta", "std_err", "t", "p", "ci_lower", "ci_upper")] + [
        ("r2", C.c_float),
        ("adj_r2", C.c_float),
    ]


class ReportGrouped(C.Structure):
    """pds_report_grouped_f64 / _f32: pointers only, so one layout serves both precisions."""
    _fields_ = [(k, C.c_void_p) for k in ("beta", "std_err", "t", "p", "ci_lower", "ci_upper", "r2", "adj_r2", "is_null")]


class GlmReportOut(C.Structure):
    """pds_glm_report_out: nullable output pointers, one layout for both precisions."""
    _fields_ = [(k, C.c_void_p) for k in ("std_err", "z", "p", "ci_lower", "ci_upper", "cov", "deviance", "null_deviance", "pearson_chi2",
                                          "dispersion", "df_resid", "report_null")]


class WithinOut(C.Structure):
    """pds_within_out: nullable output pointers of the frame's type, one layout for both precisions."""
    _fields_ = [("alpha", C.c_void_p), ("pred", C.c_void_p), ("resid", C.c_void_p), ("r2_overall", C.c_double),
                ("n_groups_used", C.c_int64), ("df_resid", C.c_int64)]


class GlmWithinOut(C.Structure):
    """pds_glm_within_out: the fixed-effects GLM's report (host doubles for both precisions), its counts and the nullable alpha / pred
    outputs of the frame's type."""
    _fields_ = [(k, C.c_double * 16) for k in ("beta", "std_err", "z", "p", "ci_lower", "ci_upper")] + [
        ("cov", C.c_double * 256), ("deviance", C.c_double), ("pearson_chi2", C.c_double), ("dispersion", C.c_double),
        ("n_groups_used", C.c_int64), ("n_groups_dropped", C.c_int64), ("n_rows_used", C.c_int64), ("df_resid", C.c_int64),
        ("n_iter", C.c_int32), ("converged", C.c_int32), ("alpha", C.c_void_p), ("pred", C.c_void_p)]


class Within2Out(C.Structure):
    """pds_within2_out: the two-factor fixed-effects fit's nullable per-row outputs and its counts."""
    _fields_ = [("pred", C.c_void_p), ("resid", C.c_void_p), ("r2_overall", C.c_double), ("df_resid", C.c_int64),
                ("n_groups_used", C.c_int64), ("n_groups2_used", C.c_int64), ("n_components", C.c_int64), ("n_iter", C.c_int64)]


class Within2Effects(C.Structure):
    """pds_within2_effects: the estimated effects and components of the two-factor fit, nullable outputs in the frame's space."""
    _fields_ = [("effects1", C.c_void_p), ("effects2", C.c_void_p), ("component1", C.c_void_p), ("component2", C.c_void_p),
                ("keys1", C.c_void_p), ("cap1", C.c_int64), ("n_graph_rounds", C.c_int64)]


class ClusterKey(C.Structure):
    """pds_cluster_key: the cluster codes of pds_lin_reg_within_cl_* / pds_lin_reg_within2_cl_* and what the call reports about them."""
    _fields_ = [("codes", C.c_void_p), ("n_levels", C.c_int64), ("n_clusters", C.c_int64), ("nested1", C.c_int32), ("nested2", C.c_int32)]


class PdsError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"[pds {code}] {msg}")
        self.code = code
        self.msg = msg


_lib = None


def load() -> C.CDLL:
    """dlopen the HIP library; raises if it has not been built."""
    global _lib
    if _lib is None:
        if not LIB_PATH.exists():
            raise ImportError(
                f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950).  There is no CPU fallback."
            )
        # One HIP runtime per process: the PyTorch wheel bundles its own libamdhip64.  If this library
        # were loaded first it would bind /opt/rocm's copy, torch would then bring a second runtime and
        # whichever initialises HSA second sees "no ROCm-capable device".  Importing torch first makes the
        # loader resolve our DT_NEEDED libamdhip64.so.7 to the copy that is already mapped.
        try:
            import torch  # noqa: F401
        except Exception:  # torch-less host (e.g. a Rust plugin process): the system runtime is the only one
            pass
        lib = C.CDLL(str(LIB_PATH))
        lib.pds_last_error.restype = C.c_char_p
        lib.pds_version.restype = C.c_char_p
        lib.pds_student_t_sf.restype = C.c_double
        lib.pds_student_t_sf.argtypes = [C.c_double, C.c_double]
        lib.pds_student_t_ppf.restype = C.c_double
        lib.pds_student_t_ppf.argtypes = [C.c_double, C.c_double]
        lib.pds_ctx_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
        lib.pds_ctx_destroy.argtypes = [C.c_void_p]
        lib.pds_ctx_destroy.restype = None
        lib.pds_ctx_set_stream.argtypes = [C.c_void_p, C.c_void_p]
        lib.pds_ctx_synchronize.argtypes = [C.c_void_p]
        lib.pds_ctx_num_cus.argtypes = [C.c_void_p]
        lib.pds_ctx_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_longlong]
        if hasattr(lib, "pds_ctx_get_option"):  # (absent from older builds used in A/B runs)
            lib.pds_ctx_get_option.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_longlong)]
        if hasattr(lib, "pds_set_host_staging"):
            lib.pds_set_host_staging.argtypes = [C.c_double, C.c_double]
        if hasattr(lib, "pds_ctx_workspace_spills"):  # (absent from older builds used in A/B runs)
            lib.pds_ctx_workspace_spills.argtypes = [C.c_void_p]
            lib.pds_ctx_workspace_spills.restype = C.c_longlong
        for sfx, real in (("f64", C.c_double), ("f32", C.c_float)):  # (absent from older builds used in A/B runs)
            if hasattr(lib, "pds_lr_multi_grouped_" + sfx):
                # ctx, cols, n_targets, n_feat, n_rows, group_offsets, n_groups, space, add_bias, l2_reg, solver, singular_x_tol,
                # coeffs, is_null, pred, resid, row_null
                getattr(lib, "pds_lr_multi_grouped_" + sfx).argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_void_p,
                                                                      C.c_int64, C.c_int, C.c_int, real, C.c_int, real] + [C.c_void_p] * 5
                # ctx, cols, keys, n_targets, n_feat, n_rows, space, add_bias, l2_reg, solver, singular_x_tol, max_groups, out_keys,
                # coeffs, is_null, n_groups, pred, resid, row_null
                getattr(lib, "pds_lr_multi_by_key_" + sfx).argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_int,
                                                                     C.c_int, real, C.c_int, real, C.c_int64] + [C.c_void_p] * 7
            if hasattr(lib, "pds_lin_reg_within_grouped_" + sfx):
                # ctx, cols, n_feat, n_rows, group_offsets, n_groups, space, se_type, out, extra
                getattr(lib, "pds_lin_reg_within_grouped_" + sfx).argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_int64,
                                                                            C.c_int, C.c_int, C.c_void_p, C.c_void_p]
                # ctx, cols, keys, n_feat, n_rows, space, se_type, max_groups, out_keys, out, extra, n_groups
                getattr(lib, "pds_lin_reg_within_by_key_" + sfx).argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_int,
                                                                           C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
            if hasattr(lib, "pds_lin_reg_within2_grouped_" + sfx):
                # ctx, cols, n_feat, n_rows, group_offsets, n_groups, codes2, n_levels2, space, se_type, absorb_tol, absorb_max_iter, out, extra
                getattr(lib, "pds_lin_reg_within2_grouped_" + sfx).argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_int64,
                                                                             C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_double, C.c_int,
                                                                             C.c_void_p, C.c_void_p]
                # ctx, cols, keys, codes2, n_levels2, n_feat, n_rows, space, se_type, absorb_tol, absorb_max_iter, out, extra, n_groups
                getattr(lib, "pds_lin_reg_within2_by_key_" + sfx).argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int,
                                                                            C.c_int64, C.c_int, C.c_int, C.c_double, C.c_int, C.c_void_p,
                                                                            C.c_void_p, C.c_void_p]
            if hasattr(lib, "pds_lin_reg_within2_fx_grouped_" + sfx):  # the within2 lists plus a trailing pds_within2_effects*
                getattr(lib, "pds_lin_reg_within2_fx_grouped_" + sfx).argtypes = getattr(lib, "pds_lin_reg_within2_grouped_" + sfx).argtypes + [C.c_void_p]
                getattr(lib, "pds_lin_reg_within2_fx_by_key_" + sfx).argtypes = getattr(lib, "pds_lin_reg_within2_by_key_" + sfx).argtypes + [C.c_void_p]
            if hasattr(lib, "pds_lin_reg_within_cl_grouped_" + sfx):  # the within / within2_fx lists plus a trailing pds_cluster_key*
                for form in ("grouped_", "by_key_"):
                    getattr(lib, "pds_lin_reg_within_cl_" + form + sfx).argtypes = getattr(lib, "pds_lin_reg_within_" + form + sfx).argtypes + [C.c_void_p]
                    getattr(lib, "pds_lin_reg_within2_cl_" + form + sfx).argtypes = getattr(lib, "pds_lin_reg_within2_fx_" + form + sfx).argtypes + [C.c_void_p]
            if hasattr(lib, "pds_glm_within_grouped_" + sfx):
                # ctx, cols, weights, offset, n_feat, n_rows, group_offsets, n_groups, space, link, variance, tol, max_iter, se_type, out
                getattr(lib, "pds_glm_within_grouped_" + sfx).argtypes = [C.c_void_p] * 4 + [C.c_int, C.c_int64, C.c_void_p, C.c_int64, C.c_int,
                                                                                             C.c_int, C.c_int, real, C.c_int, C.c_int, C.c_void_p]
                # ctx, cols, weights, offset, keys, n_feat, n_rows, space, link, variance, tol, max_iter, se_type, max_groups, out_keys, out, n_groups
                getattr(lib, "pds_glm_within_by_key_" + sfx).argtypes = [C.c_void_p] * 5 + [C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int, real,
                                                                                            C.c_int, C.c_int, C.c_int64] + [C.c_void_p] * 3
        if hasattr(lib, "pds_absorb_components_i32"):
            # ctx, codes1, n_levels1, codes2, n_levels2, n_rows, space, component1, component2, n1, n2, n_components, n_rounds
            lib.pds_absorb_components_i32.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_int] + [C.c_void_p] * 6
        if hasattr(lib, "pds_debug_mark_state"):
            lib.pds_debug_mark_state.argtypes = [C.c_void_p, C.POINTER(C.c_uint)]
            lib.pds_debug_last_return_async.argtypes = [C.c_void_p]
        if hasattr(lib, "pds_ctx_workspace_bytes"):
            lib.pds_ctx_workspace_bytes.argtypes = [C.c_void_p, C.c_int]
            lib.pds_ctx_workspace_bytes.restype = C.c_longlong
        _lib = lib
    return _lib


def check(rc: int) -> None:
    if rc != 0:
        raise PdsError(rc, load().pds_last_error().decode("utf-8", "replace"))


def missing_exports() -> list[str]:
    lib = load()
    return [s for s in EXPORTS if not hasattr(lib, s)]
