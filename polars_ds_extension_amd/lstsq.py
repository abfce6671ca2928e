"""
Host-side mirror of the reference's least-squares expression interface on top of the C ABI.

Function names, keyword names, defaults and error behaviour follow
/root/reference/python/polars_ds/exprs/expr_linear.py (`lin_reg` :105-274, `lin_reg_report` :561-631,
`rolling_lin_reg` :482-558, `recursive_lin_reg` :413-479) and the Rust plugin functions they call
(src/num_ext/linear_regression.rs).  What differs is only the carrier: instead of a lazy `pl.Expr`
evaluated by Polars (not installable in this image) the functions take the column buffers directly --
numpy arrays (host memory, what an Arrow Float64/Float32 buffer is) or torch CUDA tensors (already in HBM).
All arithmetic happens in libpds_lstsq_hip.so; nothing here computes a regression on the CPU.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import threading
from typing import Sequence

import numpy as np

from . import _lib, config

__all__ = [
    "Context", "default_context", "lin_reg", "lin_reg_report", "lin_reg_by", "lin_reg_report_by", "lin_reg_report_by_key", "rolling_lin_reg", "rolling_lin_reg_by", "rolling_lin_reg_by_key", "recursive_lin_reg_by",
    "recursive_lin_reg_by_key", "glm_by", "glm_by_key", "glm_report_by", "glm_report_by_key", "logistic_reg", "mixed_reml", "mixed_reml_profile",
    "recursive_lin_reg", "lin_reg_w_rcond", "lin_reg_w_rcond_by", "lin_reg_w_rcond_by_key", "lin_reg_multi_by", "lin_reg_multi_by_key", "elastic_net_fit", "report_fit_from_moments", "report_partials", "report_finish", "gram_moments", "lin_reg_from_moments", "query_ar_coeffs",
]


def _is_torch(a) -> bool:
    return type(a).__module__.startswith("torch")


def _dtype():
    return np.float64 if config.LIN_REG_EXPR_F64 else np.float32


def _suffix() -> str:
    return "_f64" if config.LIN_REG_EXPR_F64 else "_f32"


class _Cols:
    """Column buffers (kept alive) + the void** array the C ABI wants, in the order [y, x1..xp]."""

    def __init__(self, y, xs: Sequence, weights=None):
        dt = _dtype()
        arrs = [y, *xs] + ([weights] if weights is not None else [])
        if any(_is_torch(a) for a in arrs):
            import torch

            tdt = torch.float64 if dt == np.float64 else torch.float32
            keep = []
            for a in arrs:
                if not _is_torch(a):
                    a = torch.as_tensor(np.asarray(a))
                if not a.is_cuda:
                    a = a.cuda()
                keep.append(a.to(tdt).contiguous())  # cast like series_to_slice_inner (src/utils/mod.rs:134-205)
            self.space = _lib.PDS_DEVICE
            ptrs = [int(a.data_ptr()) for a in keep]
            self.n_rows = int(keep[0].shape[0])
            self.device_index = keep[0].device.index or 0
            self.torch_device = keep[0].device
        else:
            keep = [np.ascontiguousarray(np.asarray(a), dtype=dt) for a in arrs]
            self.space = _lib.PDS_HOST
            ptrs = [int(a.ctypes.data) for a in keep]
            self.n_rows = int(keep[0].shape[0])
            self.device_index = None
        for a in keep:
            if a.ndim != 1 or int(a.shape[0]) != self.n_rows:
                raise ValueError("all columns must be 1-D and of equal length")
        self.keep = keep
        self.n_feat = len(xs)
        nb = 1 + self.n_feat
        self.cols = (C.c_void_p * nb)(*ptrs[:nb])
        self.weights = C.c_void_p(ptrs[nb]) if weights is not None else C.c_void_p(None)


class Context:
    """One pds_ctx: a device, a stream, HBM workspace.  Not thread-safe; use one per thread."""

    def __init__(self, device: int = 0, stream=None, follow_torch: bool = True):
        """follow_torch=False: the context stays on the stream it has (its private one unless `stream` / `set_stream` says otherwise)
        instead of moving to torch's current stream with every device-resident call; the caller then orders the inputs' producers
        and the results' consumers against that stream itself.  Calls on the private stream always block until the results are ready."""
        self._follow_torch = bool(follow_torch)
        self._lib = _lib.load()
        self._h = C.c_void_p()
        _lib.check(self._lib.pds_ctx_create(int(device), C.byref(self._h)))
        self.device = int(device)
        if stream is not None:
            self.set_stream(stream)

    def set_stream(self, stream) -> None:
        """stream: a torch.cuda.Stream, a raw hipStream_t integer, or None / 0 (HIP's default stream)."""
        raw = getattr(stream, "cuda_stream", stream)
        _lib.check(self._lib.pds_ctx_set_stream(self._h, C.c_void_p(int(raw) if raw else None)))
        self._stream_raw = int(raw) if raw else 0

    def follow_torch_stream(self, device) -> None:
        """
        Device-resident inputs are produced by work queued on torch's current stream: run on that stream
        so the kernels are ordered after the producers (and torch consumers after the kernels).
        """
        if not getattr(self, "_follow_torch", True):
            return
        import torch

        raw = int(torch.cuda.current_stream(device).cuda_stream)
        if getattr(self, "_stream_raw", -1) != raw:
            self.set_stream(raw)
            self._stream_raw = raw

    def synchronize(self) -> None:
        _lib.check(self._lib.pds_ctx_synchronize(self._h))

    def set_option(self, name: str, value) -> None:
        """Behaviour switches of the context (include/pds_lstsq.h, pds_ctx_set_option): "keyed_sort", "wide_f32_native", "report_chunk_groups",
        "glm_split_rows", "mixed_split_rows", "cluster_split_rows", "cluster_waves", "within_split_rows", "grouped_fused_waves", "grouped_fused_late_permille", "grouped_multi_route",
        "grouped_multi_waves", "within2_accel" (0: plain sweeps of the two-key fixed-effects calls, the default; 1: Irons-Tuck cycles),
        "rolling_waves" (cap on the waves a launch of the tiled rolling / expanding kernels starts; it changes no result bit),
        "blocking_return" (1: every call synchronises before it returns, also the device-resident `lin_reg_by` that otherwise leaves
        its work queued on the stream); the
        defaults came from PDS_KEYED_SORT / PDS_WIDE_F32_NATIVE when the context was created."""
        _lib.check(self._lib.pds_ctx_set_option(self._h, str(name).encode(), C.c_longlong(int(value))))

    def get_option(self, name: str) -> int:
        """The value the option has now (pds_ctx_get_option), whoever set it."""
        v = C.c_longlong(0)
        _lib.check(self._lib.pds_ctx_get_option(self._h, str(name).encode(), C.byref(v)))
        return int(v.value)

    def last_return_async(self) -> bool:
        """Whether the context's last `lin_reg_by` over device columns returned stream-ordered (its work still queued on the stream;
        include/pds_lstsq.h, "Synchronisation") instead of synchronising first.  Option "blocking_return" = 1 forces the latter."""
        return bool(self._lib.pds_debug_last_return_async(self._h))

    def mark_state(self) -> tuple:
        """(tests) Waits for the stream, then reads the hand-over words between the fused grouped kernel and its marked-group pass:
        (groups marked and not yet re-solved, fix-up blocks counted as gone).  Both rest at zero between calls."""
        w = (C.c_uint * 2)()
        _lib.check(self._lib.pds_debug_mark_state(self._h, w))
        return int(w[0]), int(w[1])

    @property
    def num_cus(self) -> int:
        return int(self._lib.pds_ctx_num_cus(self._h))

    def signal_post(self, word_addr: int, value: int) -> None:
        """Stream ordered: store `value` (system scope) into the 32-bit word at `word_addr` behind everything queued so far."""
        _lib.check(self._lib.pds_signal_post(self._h, C.c_void_p(int(word_addr)), C.c_uint(int(value) & 0xFFFFFFFF)))

    def signal_wait(self, words_addr: int, n_words: int, value: int, timeout_ms: int = 2000) -> None:
        """Stream ordered: what follows on the stream runs once the `n_words` words at `words_addr` are all >= `value`."""
        _lib.check(self._lib.pds_signal_wait(self._h, C.c_void_p(int(words_addr)), int(n_words), C.c_uint(int(value) & 0xFFFFFFFF), int(timeout_ms)))

    def signal_wait_timeouts(self) -> int:
        n = C.c_int(0)
        _lib.check(self._lib.pds_signal_wait_status(self._h, C.byref(n)))
        return int(n.value)

    WORKSPACES = ("scratch", "stage", "solve", "keyed", "wkeyed")

    def workspace_bytes(self, which: str = "keyed") -> int:
        """Bytes held in one of the context's grow-only HBM workspaces (pds_ctx_workspace_bytes)."""
        return int(self._lib.pds_ctx_workspace_bytes(self._h, self.WORKSPACES.index(which)))

    KINDS = ("moments", "grouped_moments", "solve", "pass2", "rolling", "iterative", "sweep_factor1", "sweep_factor2", "graph")

    def set_timing(self, enable: bool) -> None:
        _lib.check(self._lib.pds_ctx_set_timing(self._h, int(bool(enable))))

    def get_timing(self, reset: bool = True) -> dict:
        """Per kernel class: (summed ms, launches) measured with HIP events on the context's stream."""
        nk = len(self.KINDS)
        ms = (C.c_double * nk)()
        cnt = (C.c_longlong * nk)()
        _lib.check(self._lib.pds_ctx_get_timing(self._h, ms, cnt, nk, int(bool(reset))))
        return {k: (ms[i], int(cnt[i])) for i, k in enumerate(self.KINDS)}

    def get_timing_samples(self, kind: str, reset: bool = True) -> list:
        """The individual launch durations (ms) of one kernel class since the last reset, oldest first."""
        buf = (C.c_double * 4096)()
        n = int(self._lib.pds_ctx_get_timing_samples(self._h, self.KINDS.index(kind), buf, 4096, int(bool(reset))))
        if n < 0:
            raise ValueError(kind)
        return [float(buf[i]) for i in range(n)]

    def close(self) -> None:
        if getattr(self, "_h", None) and self._h.value:
            self._lib.pds_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def fn(self, name: str):
        return getattr(self._lib, name + _suffix())


_tls = threading.local()


def default_context() -> Context:
    """One context per calling thread (a pds_ctx is not thread-safe: stream, workspace and pinned staging are per call)."""
    ctx = getattr(_tls, "ctx", None)
    if ctx is None:
        ctx = _tls.ctx = Context(0)
    return ctx


def _follow(ctx: "Context", cols: "_Cols") -> None:
    if cols.space == _lib.PDS_DEVICE:
        ctx.follow_torch_stream(cols.torch_device)


def _params(add_bias, l1_reg, l2_reg, tol, solver, positive, max_iter, singular_x_tol) -> _lib.LRParams:
    if singular_x_tol is None:  # dtype-aware default, expr_linear.py:184-186
        singular_x_tol = 1e-12 if config.LIN_REG_EXPR_F64 else 1e-6
    return _lib.LRParams(int(bool(add_bias)), float(l1_reg), float(l2_reg), float(tol), _lib.SOLVERS.get(solver, 0),
                         int(bool(positive)), int(max_iter), float(singular_x_tol))


def _out_like(cols: _Cols, shape):
    """An output buffer in the same memory space as the inputs."""
    if cols.space == _lib.PDS_DEVICE:
        import torch

        tdt = torch.float64 if config.LIN_REG_EXPR_F64 else torch.float32
        t = torch.empty(shape, dtype=tdt, device=cols.keep[0].device)
        return t, C.c_void_p(int(t.data_ptr()))
    a = np.empty(shape, dtype=_dtype())
    return a, C.c_void_p(a.ctypes.data)


def _out_int(cols: _Cols, n, dtype: str):
    if cols.space == _lib.PDS_DEVICE:
        import torch

        t = torch.empty(n, dtype=getattr(torch, dtype), device=cols.keep[0].device)
        return t, C.c_void_p(int(t.data_ptr()))
    a = np.empty(n, dtype=dtype)
    return a, C.c_void_p(a.ctypes.data)


def _out_u8(cols: _Cols, n):
    return _out_int(cols, n, "uint8")


def parse_null_policy(value: str):
    """NullPolicy::try_from (src/linear/mod.rs:43-66): returns (policy code, fill value)."""
    v = str(value).lower()
    if v == "raise":
        return 0, 0.0
    if v == "skip":
        return 1, 0.0
    if v == "zero":
        return 2, 0.0
    if v == "one":
        return 2, 1.0
    if v == "ignore":
        return 3, 0.0
    try:
        return 2, float(value)
    except ValueError:
        raise ValueError("Invalid NullPolicy.") from None


def _is_arrow(a) -> bool:
    return type(a).__module__.startswith("pyarrow")


def _arrow_parts(a, dt):
    """(values ndarray, validity buffer address or 0, bit offset, keepalive) of a pyarrow (Chunked)Array."""
    import pyarrow as pa

    if isinstance(a, pa.ChunkedArray):
        a = a.combine_chunks() if a.num_chunks != 1 else a.chunk(0)  # like .rechunk()
    want = pa.float64() if dt == np.float64 else pa.float32()
    if a.type != want:
        a = a.cast(want)  # the Rust side casts non-matching inputs the same way (src/utils/mod.rs:134-205)
    vbuf, dbuf = a.buffers()
    vals = np.frombuffer(dbuf, dtype=dt)[a.offset : a.offset + len(a)]
    has_nulls = vbuf is not None and a.null_count > 0
    return vals, (vbuf.address if has_nulls else 0), a.offset, (a, vbuf, dbuf)


def _lin_reg_arrow(x, target, add_bias, return_pred, null_policy, prm, ctx):
    """pl_lr / pl_lr_pred on Arrow columns with validity bitmaps (host memory)."""
    dt = _dtype()
    parts = [_arrow_parts(c, dt) if _is_arrow(c) else (np.ascontiguousarray(np.asarray(c), dtype=dt), 0, 0, None)
             for c in (target, *x)]
    n = len(parts[0][0])
    if any(len(pt[0]) != n for pt in parts):
        raise ValueError("all columns must be 1-D and of equal length")
    nc = len(parts)
    cols = (C.c_void_p * nc)(*[pt[0].ctypes.data for pt in parts])
    vals = (C.c_void_p * nc)(*[pt[1] or None for pt in parts])
    offs = (C.c_int64 * nc)(*[pt[2] for pt in parts])
    code, fill = parse_null_policy(null_policy)
    pp = nc - 1 + int(bool(add_bias))
    coeffs = np.empty(pp, dtype=dt)
    is_null, n_used = C.c_int(0), C.c_int64(0)
    fillv = C.c_double(fill) if config.LIN_REG_EXPR_F64 else C.c_float(fill)
    if return_pred:
        pred, resid, valid = np.empty(n, dtype=dt), np.empty(n, dtype=dt), np.empty(n, dtype=np.uint8)
        pp_, rp_, vp_ = (C.c_void_p(a.ctypes.data) for a in (pred, resid, valid))
    else:
        pred = resid = valid = None
        pp_ = rp_ = vp_ = C.c_void_p(None)
    _lib.check(ctx.fn("pds_lr_nullable")(ctx._h, cols, vals, offs, nc - 1, C.c_int64(n), _lib.PDS_HOST, code, fillv, C.byref(prm),
                                         C.c_void_p(coeffs.ctypes.data), C.byref(is_null), pp_, rp_, vp_, C.byref(n_used)))
    if return_pred:
        if is_null.value:  # all-null {pred, resid} struct of the same length (linear_regression.rs:745-750)
            valid[:] = 0
            pred[:] = np.nan
            resid[:] = np.nan
        return pred, resid, valid.astype(bool)
    return None if is_null.value else coeffs


def lin_reg(*x, target, add_bias: bool = False, weights=None, return_pred: bool = False, l1_reg: float = 0.0,
            l2_reg: float = 0.0, tol: float = 1e-5, solver: str = "qr", max_iter: int = 200, positive: bool = False,
            singular_x_tol: float | None = None, null_policy: str = "skip", absorb=None, absorb_offsets=None,
            absorb_tol: float = 1e-8, absorb_max_iter: int = 10_000, absorb_accel: str | None = None, ctx: Context | None = None):
    """
    pds.lin_reg on null-free column buffers (pl_lr / pl_lr_pred).

    Returns the coefficient vector (bias last) or None when the rank gate fires (the reference returns
    a null list).  With return_pred=True returns (pred, resid) -- or None when gated (the reference
    returns an all-null struct).

    `absorb=key` / `absorb_offsets=off`: the fixed-effects fit with one intercept per group (see lin_reg_report); returns beta, or
    (beta, pred, resid) with return_pred=True.  OLS only: the penalties, `solver` and `positive` do not apply.  `absorb=[k1, k2]`: two
    absorbed keys (`absorb_tol`, `absorb_max_iter`, `absorb_accel`: see lin_reg_report; "irons_tuck" runs cycles of two sweeps and an
    extrapolation, and `absorb_max_iter` counts sweeps).
    """
    if absorb is not None or absorb_offsets is not None or absorb_accel is not None:
        rep = _lin_reg_within(x, target, add_bias, weights, None, None, absorb, absorb_offsets, None, False, return_pred, None, ctx, fit_only=True,
                              absorb_tol=absorb_tol, absorb_max_iter=absorb_max_iter, absorb_accel=absorb_accel)
        return (rep["beta"], rep["pred"], rep["resid"]) if return_pred else rep["beta"]
    if isinstance(target, (list, tuple)):  # multi-target: expr_linear.py:188-228
        if len(target) == 0:
            raise ValueError("If `target` is a list, it cannot be empty.")
        if len(target) == 1:
            return lin_reg(*x, target=target[0], add_bias=add_bias, weights=weights, return_pred=return_pred, l1_reg=l1_reg,
                           l2_reg=l2_reg, tol=tol, solver=solver, null_policy=null_policy, singular_x_tol=singular_x_tol, ctx=ctx)
        return _lin_reg_multi(x, list(target), add_bias, return_pred, l2_reg, solver, singular_x_tol, ctx or default_context())
    if max_iter <= 0:
        raise ValueError("Input `max_iter` must be a positive.")  # expr_linear.py:231-232
    ctx = ctx or default_context()
    if weights is None and any(_is_arrow(c) for c in (target, *x)):
        # Arrow columns may carry nulls: `null_policy` applies ("skip" is the reference's default, expr_linear.py:116);
        # with return_pred the result is (pred, resid, row_valid)
        prm = _params(add_bias, l1_reg, l2_reg, tol, solver, positive, max_iter, singular_x_tol)
        return _lin_reg_arrow(x, target, add_bias, return_pred, null_policy, prm, ctx)
    parse_null_policy(null_policy)  # validated even when no column can hold a null
    cols = _Cols(target, x, weights)
    _follow(ctx, cols)
    prm = _params(add_bias, l1_reg, l2_reg, tol, solver, positive, max_iter, singular_x_tol)
    pp = cols.n_feat + int(bool(add_bias))
    coeffs = np.empty(pp, dtype=_dtype())
    is_null = C.c_int(0)
    if return_pred:
        pred, pred_p = _out_like(cols, cols.n_rows)
        resid, resid_p = _out_like(cols, cols.n_rows)
        _lib.check(ctx.fn("pds_lr_pred")(ctx._h, cols.cols, cols.weights, cols.n_feat, C.c_int64(cols.n_rows), cols.space,
                                         C.byref(prm), C.c_void_p(coeffs.ctypes.data), C.byref(is_null), pred_p, resid_p))
        return None if is_null.value else (pred, resid)
    _lib.check(ctx.fn("pds_lr")(ctx._h, cols.cols, cols.weights, cols.n_feat, C.c_int64(cols.n_rows), cols.space,
                                C.byref(prm), C.c_void_p(coeffs.ctypes.data), C.byref(is_null)))
    return None if is_null.value else coeffs


def _lin_reg_multi(x, targets, add_bias, return_pred, l2_reg, solver, singular_x_tol, ctx):
    """pl_lr_multi / pl_lr_multi_pred: dict with the reference's struct field names (target_i[_pred|_resid])."""
    k = len(targets)
    cols = _Cols(targets[0], [*targets[1:], *x])  # C order: [t_0 .. t_{k-1}, x_1 .. x_p]
    _follow(ctx, cols)
    if singular_x_tol is None:
        singular_x_tol = 1e-12 if config.LIN_REG_EXPR_F64 else 1e-6
    p = len(x)
    pp = p + int(bool(add_bias))
    coeffs = np.empty((k, pp), dtype=_dtype())
    is_null = C.c_int(0)
    R = C.c_double if config.LIN_REG_EXPR_F64 else C.c_float
    if return_pred:
        pred, pr_p = _out_like(cols, (k, cols.n_rows))
        resid, rs_p = _out_like(cols, (k, cols.n_rows))
    else:
        pred = resid = None
        pr_p = rs_p = C.c_void_p(None)
    _lib.check(ctx.fn("pds_lr_multi")(ctx._h, cols.cols, k, p, C.c_int64(cols.n_rows), cols.space, int(bool(add_bias)),
                                      R(l2_reg), _lib.SOLVERS.get(solver, 0), R(singular_x_tol),
                                      C.c_void_p(coeffs.ctypes.data), C.byref(is_null), pr_p, rs_p))
    if return_pred:
        if is_null.value:
            return None
        out = {}
        for i in range(k):
            out[f"target_{i}_pred"] = pred[i]
            out[f"target_{i}_resid"] = resid[i]
        return out
    return {f"target_{i}": (None if is_null.value else coeffs[i]) for i in range(k)}


def query_ar_coeffs(x, lag: int, add_bias: bool = True, null_policy: str = "raise", ctx: Context | None = None):
    """
    Autoregressive coefficients of order `lag` (python/polars_ds/exprs/ts_features.py:419-461): `lin_reg` of x[t] on
    x[t-1] ... x[t-lag] over t = lag ... n-1, bias last.  The lagged features are *views* into the one series (the
    reference builds them with shift + slice): numpy / torch slices and pyarrow slices carry only a pointer and a bit
    offset, so no column is copied on the way to the Gram kernel, which reads element-aligned pointers.
    """
    if null_policy not in ("raise", "one", "zero"):
        import math

        try:
            z = float(null_policy)
            if not math.isfinite(z):
                raise ValueError
        except (TypeError, ValueError):
            raise ValueError("`null_polocy` must be 'raise', 'one', 'zero' or any finite numeric string for AR coefficients.") from None
    if lag <= 0:
        raise ValueError("`lag` must be > 0.")
    n = len(x)
    m = max(n - lag, 0)
    if _is_arrow(x):
        import pyarrow as pa

        if isinstance(x, pa.ChunkedArray):
            x = x.combine_chunks() if x.num_chunks != 1 else x.chunk(0)
        feats = [x.slice(lag - i, m) for i in range(1, lag + 1)]
        return lin_reg(*feats, target=x.slice(lag, m), add_bias=add_bias, null_policy=null_policy, ctx=ctx)
    feats = [x[lag - i : n - i] for i in range(1, lag + 1)]
    return lin_reg(*feats, target=x[lag:], add_bias=add_bias, null_policy=null_policy, ctx=ctx)


def lin_reg_w_rcond(*x, target, add_bias: bool = False, rcond: float = 0.0, l2_reg: float = 0.0, ctx: Context | None = None):
    """pds.lin_reg_w_rcond (pl_lr_w_rcond / pl_lr_w_rcond_f32): returns (coeffs, singular_values)."""
    ctx = ctx or default_context()
    cols = _Cols(target, x)
    _follow(ctx, cols)
    dt = _dtype()
    real = C.c_double if dt == np.float64 else C.c_float
    pp = cols.n_feat + int(bool(add_bias))
    # (kwargs.tol as T).max(T::EPSILON * max(nrows, p'))   linear_regression.rs:651-702, linear_regression_f32.rs:515-566
    rc = max(dt(rcond), np.finfo(dt).eps * dt(max(cols.n_rows, pp)))
    coeffs = np.empty(pp, dtype=dt)
    sv = np.empty(pp, dtype=dt)
    fn = ctx._lib.pds_lr_rcond_f64 if dt == np.float64 else ctx._lib.pds_lr_rcond_f32
    _lib.check(fn(ctx._h, cols.cols, cols.n_feat, C.c_int64(cols.n_rows), cols.space, int(bool(add_bias)), real(l2_reg), real(rc),
                  C.c_void_p(coeffs.ctypes.data), C.c_void_p(sv.ctypes.data)))
    return coeffs, sv


def _rcond_by_check(x, what):
    if len(x) < 1:
        raise ValueError(f"{what}: need at least one feature column")
    if len(x) > 16:
        raise NotImplementedError("grouped lin_reg_w_rcond: up to 16 feature columns")


def _real_args(*values):
    real = C.c_double if config.LIN_REG_EXPR_F64 else C.c_float
    return [real(float(v)) for v in values]


def lin_reg_w_rcond_by(*x, target, group_offsets, add_bias: bool = False, rcond: float = 0.0, l2_reg: float = 0.0,
                       ctx: Context | None = None):
    """
    `lin_reg_w_rcond` per group in one call: for every group g = rows [group_offsets[g], group_offsets[g+1]) what `lin_reg_w_rcond`
    computes on g's rows alone -- X'X (+ l2_reg) decomposed on chip, singular values below the cut dropped, the minimum-norm
    coefficients (`pds_lr_rcond_grouped_*`, one wave per group).  The cut of a group is max(rcond, eps * max(n_g, p')) with the
    group's own row count.  1 .. 16 feature columns.
    Returns (coeffs [G, p'] bias last, singular_values [G, p'] descending, is_null [G]) in the memory space of the inputs.  A group
    with fewer rows than coefficients, with NaN / inf in its rows, or whose coefficients do not end finite (the all-zero system) is
    null: is_null = 1, NaN coefficients and singular values.
    """
    _rcond_by_check(x, "lin_reg_w_rcond_by")
    ctx = ctx or default_context()
    cols = _Cols(target, x)
    _follow(ctx, cols)
    pp = cols.n_feat + int(bool(add_bias))
    off, off_p = _offsets_arg(cols, group_offsets)
    ng = int(off.shape[0]) - 1
    coeffs, co_p = _out_like(cols, (ng, pp))
    sv, sv_p = _out_like(cols, (ng, pp))
    nulls, nu_p = _out_u8(cols, ng)
    _lib.check(ctx.fn("pds_lr_rcond_grouped")(ctx._h, cols.cols, cols.n_feat, C.c_int64(cols.n_rows), off_p, C.c_int64(ng), cols.space,
                                              int(bool(add_bias)), *_real_args(l2_reg, rcond), co_p, sv_p, nu_p))
    return coeffs, sv, nulls


def lin_reg_w_rcond_by_key(*x, target, key, add_bias: bool = False, rcond: float = 0.0, l2_reg: float = 0.0,
                           max_groups: int | None = None, ctx: Context | None = None):
    """
    `lin_reg_w_rcond_by` for an integer key column in ANY row order (`pds_lr_rcond_by_key_*`): the frame is brought into key order on
    the device (nothing moves when the keys are already non-decreasing) and every group is fitted.
    Returns (keys [G] ascending, coeffs, singular_values, is_null).
    """
    _rcond_by_check(x, "lin_reg_w_rcond_by_key")
    ctx = ctx or default_context()
    cols = _Cols(target, x)
    _follow(ctx, cols)
    pp = cols.n_feat + int(bool(add_bias))
    k, k_p = _key_arg(cols, key)

    def call(cap, ok_p, ng_p):
        coeffs, co_p = _out_like(cols, (cap, pp))
        sv, sv_p = _out_like(cols, (cap, pp))
        nulls, nu_p = _out_u8(cols, cap)
        rc = ctx.fn("pds_lr_rcond_by_key")(ctx._h, cols.cols, k_p, cols.n_feat, C.c_int64(cols.n_rows), cols.space, int(bool(add_bias)),
                                           *_real_args(l2_reg, rcond), C.c_int64(cap), ok_p, co_p, sv_p, nu_p, ng_p)
        return rc, (coeffs, sv, nulls)

    keys, (coeffs, sv, nulls), g = _by_key_retry(cols, max_groups, call)
    return keys, coeffs[:g], sv[:g], nulls[:g]


MULTI_BY_LIMIT = "grouped multi-target lin_reg: up to 16 feature columns and 15 targets"


def _multi_by_check(x, targets, what):
    """Before a device is touched: the target list, the feature count, the limits of the grouped multi-target fit."""
    if not isinstance(targets, (list, tuple)):
        raise TypeError(f"{what}: `targets` is a list of target columns")
    if len(targets) == 0:
        raise ValueError("If `target` is a list, it cannot be empty.")
    if len(x) < 1:
        raise ValueError(f"{what}: need at least one feature column")
    if len(x) > 16 or len(targets) > 15:
        raise NotImplementedError(MULTI_BY_LIMIT)


def _multi_by_args(add_bias, l2_reg, solver, singular_x_tol):
    if singular_x_tol is None:  # dtype-aware default, expr_linear.py:184-186
        singular_x_tol = 1e-12 if config.LIN_REG_EXPR_F64 else 1e-6
    l2, tol = _real_args(l2_reg, singular_x_tol)
    return int(bool(add_bias)), l2, _lib.SOLVERS.get(solver, 0), tol


def _multi_pred_outs(cols, k, return_pred):
    if not return_pred:
        none = C.c_void_p(None)
        return (None, None, None), (none, none, none)
    pred, pr_p = _out_like(cols, (k, cols.n_rows))
    resid, rs_p = _out_like(cols, (k, cols.n_rows))
    rn, rn_p = _out_u8(cols, cols.n_rows)
    return (pred, resid, rn), (pr_p, rs_p, rn_p)


def lin_reg_multi_by(*x, targets, group_offsets, add_bias: bool = False, l2_reg: float = 0.0, solver: str = "qr",
                     singular_x_tol: float | None = None, return_pred: bool = False, ctx: Context | None = None):
    """
    `lin_reg(*x, target=[t_0 .. t_{k-1}])` per group in one call (`pds_lr_multi_grouped_*`): group g = rows [group_offsets[g],
    group_offsets[g+1]); the k targets share every group's design matrix, so the frame is staged once and a group's X'X is
    factorised once for all k right-hand sides.  OLS / ridge, 1 .. 16 feature columns, 1 .. 15 targets (beyond:
    NotImplementedError); torch CUDA tensors or NumPy arrays.
    Returns (coeffs [G, k, p'] bias last, is_null [G]) in the memory space of the inputs; the gate and the null rule are
    `lin_reg_by`'s, group for group, and a group is null for every target or for none (a NaN in one target nulls the group).
    `return_pred=True` adds (pred [k, n], resid [k, n], row_null [n]) in the frame's row order; the rows of a null group are NaN and
    flagged.  The context option "grouped_multi_route" picks the kernel (0 choose, 1 one kernel, 2 the fused kernel per target).
    """
    _multi_by_check(x, targets, "lin_reg_multi_by")
    ctx = ctx or default_context()
    k = len(targets)
    cols = _Cols(targets[0], [*targets[1:], *x])  # C order: [t_0 .. t_{k-1}, x_1 .. x_p]
    _follow(ctx, cols)
    p = len(x)
    bias, l2, sol, tol = _multi_by_args(add_bias, l2_reg, solver, singular_x_tol)
    off, off_p = _offsets_arg(cols, group_offsets)
    ng = int(off.shape[0]) - 1
    coeffs, co_p = _out_like(cols, (ng, k, p + bias))
    nulls, nu_p = _out_u8(cols, ng)
    rows, rows_p = _multi_pred_outs(cols, k, return_pred)
    _lib.check(ctx.fn("pds_lr_multi_grouped")(ctx._h, cols.cols, k, p, C.c_int64(cols.n_rows), off_p, C.c_int64(ng), cols.space, bias, l2, sol,
                                              tol, co_p, nu_p, *rows_p))
    return (coeffs, nulls, *rows) if return_pred else (coeffs, nulls)


def lin_reg_multi_by_key(*x, targets, key, add_bias: bool = False, l2_reg: float = 0.0, solver: str = "qr",
                         singular_x_tol: float | None = None, max_groups: int | None = None, return_pred: bool = False,
                         ctx: Context | None = None):
    """
    `lin_reg_multi_by` for an integer key column in ANY row order (`pds_lr_multi_by_key_*`): the keys are ordered once for all k
    targets (nothing moves when they are already non-decreasing) and every group is fitted.
    Returns (keys [G] ascending, coeffs [G, k, p'], is_null [G]), with `return_pred=True` followed by (pred [k, n], resid [k, n],
    row_null [n]) in the frame's own row order.
    """
    _multi_by_check(x, targets, "lin_reg_multi_by_key")
    ctx = ctx or default_context()
    k = len(targets)
    cols = _Cols(targets[0], [*targets[1:], *x])
    _follow(ctx, cols)
    p = len(x)
    bias, l2, sol, tol = _multi_by_args(add_bias, l2_reg, solver, singular_x_tol)
    ky, k_p = _key_arg(cols, key)

    def call(cap, ok_p, ng_p):
        coeffs, co_p = _out_like(cols, (cap, k, p + bias))
        nulls, nu_p = _out_u8(cols, cap)
        rows, rows_p = _multi_pred_outs(cols, k, return_pred)
        rc = ctx.fn("pds_lr_multi_by_key")(ctx._h, cols.cols, k_p, k, p, C.c_int64(cols.n_rows), cols.space, bias, l2, sol, tol, C.c_int64(cap),
                                           ok_p, co_p, nu_p, ng_p, *rows_p)
        return rc, (coeffs, nulls, rows)

    keys, (coeffs, nulls, rows), g = _by_key_retry(cols, max_groups, call)
    return (keys, coeffs[:g], nulls[:g], *rows) if return_pred else (keys, coeffs[:g], nulls[:g])


def elastic_net_fit(*x, target, l1_reg: float, l2_reg: float, add_bias: bool = False, tol: float = 1e-5, max_iter: int = 2000,
                    ctx: Context | None = None):
    """
    ElasticNet::fit_unchecked (src/linear/lr/lr_solvers.rs:139-164): always faer_coordinate_descent, also for l1_reg <= 0
    (pl_lr's dispatch would take the closed-form ridge there, which penalises with l2_reg where coordinate descent uses
    n_rows * l2_reg).  Returns the coefficients (bias last).
    """
    ctx = ctx or default_context()
    cols = _Cols(target, x)
    _follow(ctx, cols)
    dt = _dtype()
    prm = _lib.LRParams(int(bool(add_bias)), float(l1_reg), float(l2_reg), float(tol), 0, 0, int(max_iter), 0.0)
    pp = cols.n_feat + int(bool(add_bias))
    coeffs = np.empty(pp, dtype=dt)
    fn = ctx._lib.pds_elastic_net_f64 if dt == np.float64 else ctx._lib.pds_elastic_net_f32
    _lib.check(fn(ctx._h, cols.cols, cols.n_feat, C.c_int64(cols.n_rows), cols.space, C.byref(prm), C.c_void_p(coeffs.ctypes.data)))
    return coeffs


def lin_reg_report(*x, target, add_bias: bool = False, weights=None, std_err: str = "se", y_var: float | None = None,
                   feature_names: Sequence[str] | None = None, null_policy: str = "raise", cluster=None, cluster_offsets=None,
                   absorb=None, absorb_offsets=None, return_effects: bool = False, return_pred: bool = False,
                   absorb_tol: float = 1e-8, absorb_max_iter: int = 10_000, absorb_accel: str | None = None, cluster_key=None,
                   ctx: Context | None = None) -> dict:
    """
    pds.lin_reg_report (pl_lin_reg_report / pl_wls_report).  `y_var` is what Polars evaluates as
    `target.var()` (ddof=1) and hands to the plugin as input 0 (expr_linear.py:614-617); when omitted it
    is taken from the moment pass (sum y, sum y^2 are by-products of the Gram build).
    Returns the 9 report columns as a dict of arrays (r2 / adj_r2 broadcast like the reference's struct).
    pyarrow columns may carry nulls: `null_policy` then applies as in series_to_mat_for_lr (the reference's default for
    this expression is "raise", expr_linear.py:566); `y_var` must be given in that case (Polars computes it on the
    original target).

    `std_err="cluster"` (CR1) / `"cluster0"` (CR0): cluster-robust standard errors of the ONE model over the whole frame (Stata's
    vce(cluster id), statsmodels' cov_type="cluster").  The clusters are given either as `cluster`, an integer column in any row
    order, or as `cluster_offsets` (cluster g = rows [cluster_offsets[g], cluster_offsets[g+1]), contiguous) -- exactly one of the
    two, and neither with any other `std_err`.  The standard-error column is "cluster_se" / "cluster0_se", t / p / interval use
    G - 1 degrees of freedom, and the result gains "n_clusters" (G, the non-empty clusters).  1 .. 16 features, no weights, NumPy
    arrays or CUDA tensors (no pyarrow columns).

    `absorb=key` (an integer column in any row order) or `absorb_offsets=off` (group g = rows [off[g], off[g+1]), contiguous) --
    exactly one of the two: the fixed-effects regression y_i = alpha_g(i) + x_i' beta + e_i with one intercept per group, the within
    estimator (pds_lin_reg_within_*; include/pds_lstsq.h states the definitions).  No intercept column: `add_bias=True` is refused.
    `std_err` is "se" (n - G - p degrees of freedom), "cluster" or "cluster0" -- the clusters ARE the absorbed groups, so `cluster` /
    `cluster_offsets` are refused.  r2 / adj_r2 are the within values; the dict gains "r2_overall", "n_groups" (G, the non-empty
    groups) and "df_resid".  return_effects=True adds "effects" (alpha per group; NaN for an empty group of `absorb_offsets`) and
    "effect_keys" (the distinct keys, ascending; group indices with `absorb_offsets`); return_pred=True adds "pred" and "resid" in the
    frame's row order.  1 .. 16 features, no weights, NumPy arrays or CUDA tensors.

    `absorb=[k1, k2]` (a list or tuple of exactly two integer columns): TWO absorbed factors, y_i = alpha_k1(i) + gamma_k2(i) +
    x_i' beta + e_i -- firm and year effects, the two-way fixed-effects model (pds_lin_reg_within2_*; include/pds_lstsq.h states the
    definitions).  The columns are projected off both sets of dummies by alternating sweeps until the largest level mean subtracted
    in a sweep is `absorb_tol` (> 0; 1e-8) standard deviations of its column; `absorb_max_iter` sweeps without that raise PdsError
    (PDS_ERR_NUMERIC, "did not converge").  With A = G1 + G2 - (connected components of the cells), "se" has n - p - A degrees of
    freedom; "cluster" / "cluster0" cluster on the FIRST key.  The dict is the one-key dict plus "n_groups2" (G2), "n_components"
    and "n_iter" (sweeps used).  return_pred=True works as above; return_effects=True is refused with two keys (the effects
    need a normalisation: `fixed_effects` returns them under its own), and so are three or more keys; `absorb_offsets` cannot be combined with a second key.
    `absorb_accel` (two keys only, else ValueError): None -- what the context's option "within2_accel" says (plain sweeps unless it was
    set); "none" -- plain sweeps; "irons_tuck" -- the accelerated iteration.  A CYCLE is two sweeps, each exactly the plain sweep and
    each judged by its own delta, followed by one extrapolation of the table of factor-2 means along the last sweep's step (per
    column, c = <step2, step2 - step1> / |step2 - step1|^2; tables only, no read of the frame).  The call always ends on a sweep;
    "n_iter" and `absorb_max_iter` count SWEEPS, never extrapolations.  On frames whose plain sweeps converge slowly (few movers
    between the levels) the sweep count falls several times; it is never meant to rise.  A string sets the option for this call and
    puts the previous value back afterwards, also when the call raises.

    `cluster_key` (with `absorb=k`, `absorb_offsets=` or `absorb=[k1, k2]`, and std_err "cluster" or "cluster0" only): the standard
    errors are clustered on THIS key instead of the (first) absorbed one -- absorb firm and year and cluster on state, or cluster on
    the second absorbed key (pds_lin_reg_within_cl_* / pds_lin_reg_within2_cl_*; include/pds_lstsq.h states the definitions).  An
    integer column, NumPy array or CUDA tensor, in any row order; it is coded densely like the second absorbed key.  The fit itself
    is untouched: beta, r2, "n_iter", pred and resid are the bits of the call without `cluster_key`.  The dict gains "n_clusters" (Gc,
    the distinct keys) and "absorb_nested" (one bool per absorbed key: every level of it lies inside one cluster); "df_resid" is
    Gc - 1.  "cluster" scales by Gc / (Gc - 1) * (n - 1) / (n - K), where K counts p, the absorbed effects of every key that is NOT
    nested, and one intercept if some key is nested.  ValueError: without absorption, together with `cluster` / `cluster_offsets`,
    with std_err="se", or when the column is not an integer column.
    """
    if cluster_key is not None and absorb is None and absorb_offsets is None:
        raise ValueError("`cluster_key` goes with `absorb` or `absorb_offsets` only; without absorption the clusters are `cluster=`")
    if absorb is not None or absorb_offsets is not None or absorb_accel is not None:
        return _lin_reg_within(x, target, add_bias, weights, std_err, feature_names, absorb, absorb_offsets, (cluster, cluster_offsets),
                               return_effects, return_pred, None, ctx, absorb_tol=absorb_tol, absorb_max_iter=absorb_max_iter,
                               absorb_accel=absorb_accel, cluster_key=cluster_key)
    if return_effects or return_pred:
        raise ValueError("`return_effects` / `return_pred` go with `absorb` or `absorb_offsets` only")
    if std_err in _lib.CLUSTER_SE_TYPES:
        return _lin_reg_report_cluster(x, target, add_bias, weights, std_err, y_var, feature_names, cluster, cluster_offsets, ctx)
    if cluster is not None or cluster_offsets is not None:
        raise ValueError('`cluster` / `cluster_offsets` go with std_err="cluster" or "cluster0" only')
    ctx = ctx or default_context()
    arrow = weights is None and any(_is_arrow(c) for c in (target, *x))
    code, fill = parse_null_policy(null_policy)
    if arrow:
        if y_var is None:
            import pyarrow.compute as pc

            y_var = float(pc.variance(target, ddof=1).as_py())  # Polars' var() skips nulls the same way
        dt = _dtype()
        parts = [_arrow_parts(c, dt) if _is_arrow(c) else (np.ascontiguousarray(np.asarray(c), dtype=dt), 0, 0, None)
                 for c in (target, *x)]
        n = len(parts[0][0])
        if any(len(pt[0]) != n for pt in parts):
            raise ValueError("all columns must be 1-D and of equal length")
        nc = len(parts)
        n_feat = nc - 1
        pp = n_feat + int(bool(add_bias))
        outs = {k: np.empty(pp, dtype=dt) for k in ("beta", "std_err", "t", "p", "ci_lower", "ci_upper")}
        R = _lib.ReportF64 if config.LIN_REG_EXPR_F64 else _lib.ReportF32
        rep = R(*[C.c_void_p(outs[k].ctypes.data) for k in ("beta", "std_err", "t", "p", "ci_lower", "ci_upper")], 0.0, 0.0)
        cp = (C.c_void_p * nc)(*[pt[0].ctypes.data for pt in parts])
        vp = (C.c_void_p * nc)(*[pt[1] or None for pt in parts])
        op = (C.c_int64 * nc)(*[pt[2] for pt in parts])
        f = (C.c_double if config.LIN_REG_EXPR_F64 else C.c_float)
        n_used = C.c_int64(0)
        _lib.check(ctx.fn("pds_lin_reg_report_nullable")(ctx._h, cp, vp, op, n_feat, C.c_int64(n), _lib.PDS_HOST, code, f(fill),
                                                         int(bool(add_bias)), _lib.SE_TYPES.get(std_err, 0), f(y_var),
                                                         C.byref(rep), C.byref(n_used)))
        return _report_dict(outs, rep, n_feat, add_bias, std_err, False, feature_names, dt)
    cols = _Cols(target, x, weights)
    _follow(ctx, cols)
    pp = cols.n_feat + int(bool(add_bias))
    se_code = _lib.SE_TYPES.get(std_err, 0)
    if y_var is None:
        if weights is None:
            y_var = 0.0
            se_code |= _lib.PDS_REPORT_DERIVE_YVAR  # the library takes var(y) from its own pass over y (f64 sums)
        else:
            M = gram_moments(*x, target=target, ctx=ctx)
            q = cols.n_feat + 2
            n = float(cols.n_rows)
            sy, syy = float(M[q - 2, q - 1]), float(M[q - 1, q - 1])
            y_var = (syy - sy * sy / n) / (n - 1.0)
    dt = _dtype()
    outs = {k: np.empty(pp, dtype=dt) for k in ("beta", "std_err", "t", "p", "ci_lower", "ci_upper")}
    R = _lib.ReportF64 if config.LIN_REG_EXPR_F64 else _lib.ReportF32
    rep = R(*[C.c_void_p(outs[k].ctypes.data) for k in ("beta", "std_err", "t", "p", "ci_lower", "ci_upper")], 0.0, 0.0)
    yv = C.c_double(y_var) if config.LIN_REG_EXPR_F64 else C.c_float(y_var)
    _lib.check(ctx.fn("pds_lin_reg_report")(ctx._h, cols.cols, cols.weights, cols.n_feat, C.c_int64(cols.n_rows),
                                            cols.space, int(bool(add_bias)), se_code, yv,
                                            C.byref(rep)))
    return _report_dict(outs, rep, cols.n_feat, add_bias, std_err, weights is not None, feature_names, dt)


def _lin_reg_report_cluster(x, target, add_bias, weights, std_err, y_var, feature_names, cluster, cluster_offsets, ctx):
    """lin_reg_report(std_err="cluster" | "cluster0"): pds_lin_reg_report_cluster_by_key_* / _grouped_*."""
    if (cluster is None) == (cluster_offsets is None):
        raise ValueError(f'std_err="{std_err}": exactly one of `cluster` and `cluster_offsets` must be given')
    if weights is not None:
        raise _lib.PdsError(-5, "cluster-robust report: weights are not supported")  # PDS_ERR_UNSUPPORTED
    if any(_is_arrow(c) for c in (target, *x)) or (cluster is not None and _is_arrow(cluster)):
        raise NotImplementedError("cluster-robust report: pyarrow columns are not supported (NumPy arrays or CUDA tensors)")
    ctx = ctx or default_context()
    cols = _Cols(target, x)
    _follow(ctx, cols)
    pp = cols.n_feat + int(bool(add_bias))
    se_code = _lib.CLUSTER_SE_TYPES[std_err]
    if y_var is None:
        y_var = 0.0
        se_code |= _lib.PDS_REPORT_DERIVE_YVAR
    dt = _dtype()
    outs = {k: np.empty(pp, dtype=dt) for k in ("beta", "std_err", "t", "p", "ci_lower", "ci_upper")}
    R = _lib.ReportF64 if config.LIN_REG_EXPR_F64 else _lib.ReportF32
    rep = R(*[C.c_void_p(outs[k].ctypes.data) for k in ("beta", "std_err", "t", "p", "ci_lower", "ci_upper")], 0.0, 0.0)
    yv = C.c_double(y_var) if config.LIN_REG_EXPR_F64 else C.c_float(y_var)
    if cluster is not None:
        k, k_p = _key_arg(cols, cluster)
        ng = C.c_int64(0)
        _lib.check(ctx.fn("pds_lin_reg_report_cluster_by_key")(ctx._h, cols.cols, k_p, cols.n_feat, C.c_int64(cols.n_rows), cols.space,
                                                               int(bool(add_bias)), se_code, yv, C.byref(rep), C.byref(ng)))
        n_clusters = int(ng.value)
    else:
        off, off_p = _offsets_arg(cols, cluster_offsets)
        if off.ndim != 1 or int(off.shape[0]) < 2:
            raise ValueError("`cluster_offsets` must be 1-D with at least two entries")
        _lib.check(ctx.fn("pds_lin_reg_report_cluster_grouped")(ctx._h, cols.cols, cols.n_feat, C.c_int64(cols.n_rows), off_p,
                                                                C.c_int64(int(off.shape[0]) - 1), cols.space, int(bool(add_bias)), se_code,
                                                                yv, C.byref(rep)))
        n_clusters = int((off[1:] > off[:-1]).sum())  # the non-empty ones
    out = _report_dict(outs, rep, cols.n_feat, add_bias, std_err, False, feature_names, dt)
    out["n_clusters"] = n_clusters
    return out


# `absorb_accel` -> the context option "within2_accel"
ABSORB_ACCEL = {"none": 0, "irons_tuck": 1}


@contextlib.contextmanager
def _accel_option(ctx, absorb_accel):
    """`absorb_accel` for the library calls inside: the option is read from the context (pds_ctx_get_option), set, and the value read
    goes back whatever the calls do.  None leaves the context alone."""
    if absorb_accel is None:
        yield
        return
    before = ctx.get_option("within2_accel")
    ctx.set_option("within2_accel", ABSORB_ACCEL[absorb_accel])
    try:
        yield
    finally:
        ctx.set_option("within2_accel", before)


def _lin_reg_within(x, target, add_bias, weights, std_err, feature_names, absorb, absorb_offsets, clusters, return_effects, return_pred,
                    max_groups, ctx, fit_only: bool = False, absorb_tol: float = 1e-8, absorb_max_iter: int = 10_000, effects2: bool = False,
                    absorb_accel: str | None = None, cluster_key=None):
    """lin_reg / lin_reg_report(absorb= | absorb_offsets=): pds_lin_reg_within_by_key_* / _grouped_*; absorb=[k1, k2]: _within2_*;
    effects2 (fixed_effects): pds_lin_reg_within2_fx_by_key_*; cluster_key: the _cl_ forms of all of these."""
    if absorb_accel is not None:
        if absorb_accel not in ABSORB_ACCEL:
            raise ValueError('`absorb_accel` is None, "none" or "irons_tuck"')
        if not isinstance(absorb, (list, tuple)) or len(absorb) != 2 or absorb_offsets is not None:
            raise ValueError("`absorb_accel` goes with two absorbed keys, `absorb=[k1, k2]`, only")
    key2 = None
    if isinstance(absorb, (list, tuple)):
        if len(absorb) > 2:
            raise NotImplementedError("fixed-effects regression: three or more absorbed keys are not implemented")
        if len(absorb) != 2:
            raise ValueError("`absorb` is one integer column or a list of exactly two")
        if absorb_offsets is not None:
            raise ValueError("`absorb_offsets` together with a second absorbed key: give both keys as `absorb=[k1, k2]`")
        if return_effects:
            raise NotImplementedError("fixed-effects regression: `return_effects` with two absorbed keys is not implemented "
                                      "(the effects need a normalisation): lstsq.fixed_effects returns them under its own")
        if not float(absorb_tol) > 0.0:
            raise ValueError("`absorb_tol` must be > 0")
        if int(absorb_max_iter) < 1:
            raise ValueError("`absorb_max_iter` must be >= 1")
        absorb, key2 = absorb
    if (absorb is None) == (absorb_offsets is None):
        raise ValueError("exactly one of `absorb` and `absorb_offsets` must be given")
    if add_bias:
        raise ValueError("`add_bias=True` together with `absorb`: the intercept is absorbed by the group effects")
    if clusters is not None and (clusters[0] is not None or clusters[1] is not None):
        if cluster_key is not None:
            raise ValueError("`cluster_key` together with `cluster` / `cluster_offsets`: with absorption the clusters are `cluster_key` alone")
        raise ValueError('`cluster` / `cluster_offsets` together with `absorb`: std_err="cluster" means the absorbed key')
    if cluster_key is not None:
        if fit_only or std_err not in _lib.CLUSTER_SE_TYPES:
            raise ValueError('`cluster_key` goes with std_err="cluster" or "cluster0" only')
        if _is_arrow(cluster_key):
            raise NotImplementedError("fixed-effects regression: pyarrow columns are not supported (NumPy arrays or CUDA tensors)")
        if not _is_int_column(cluster_key):
            raise ValueError("`cluster_key` must be an integer column")
    if not fit_only and std_err not in _lib.WITHIN_SE_TYPES:
        if std_err in _lib.SE_TYPES:
            raise _lib.PdsError(-5, "fixed-effects regression: HC0 - HC3 standard errors are not available with absorption")  # PDS_ERR_UNSUPPORTED
        raise ValueError('`absorb`: std_err is "se", "cluster" or "cluster0"')
    if weights is not None:
        raise NotImplementedError("fixed-effects regression: weights are not implemented")
    if any(_is_arrow(c) for c in (target, *x)) or (absorb is not None and _is_arrow(absorb)) or (key2 is not None and _is_arrow(key2)):
        raise NotImplementedError("fixed-effects regression: pyarrow columns are not supported (NumPy arrays or CUDA tensors)")
    ctx = ctx or default_context()
    cols = _Cols(target, x)
    _follow(ctx, cols)
    p, n, dt = cols.n_feat, cols.n_rows, _dtype()
    keys = ("beta",) if fit_only else _REPORT_KEYS
    outs = {k: np.empty(p, dtype=dt) for k in keys}
    R = _lib.ReportF64 if config.LIN_REG_EXPR_F64 else _lib.ReportF32
    rep = R(*[C.c_void_p(outs[k].ctypes.data) if k in outs else C.c_void_p(None) for k in _REPORT_KEYS], 0.0, 0.0)
    se_code = _lib.WITHIN_SE_TYPES["se" if fit_only else std_err]
    pred = resid = None
    pred_p = resid_p = C.c_void_p(None)
    if return_pred:
        pred, pred_p = _out_like(cols, n)
        resid, resid_p = _out_like(cols, n)
    ck = None
    if cluster_key is not None:  # dense codes in the inputs' space, like the second absorbed key
        codes_c, codes_c_p, n_levels_c, _ = _dense_codes(cols, cluster_key)
        ck = _lib.ClusterKey(codes_c_p, n_levels_c, 0, 0, 0)
    cl_args = () if ck is None else (C.byref(ck),)
    if key2 is not None and effects2:
        k, k_p = _key_arg(cols, absorb)
        codes2, codes2_p, n_levels2, effect_keys2 = _dense_codes(cols, key2)
        alpha2, alpha2_p = _out_like(cols, n_levels2)
        comp2, comp2_p = _out_int(cols, n_levels2, "int32")

        def call(cap, keys_p, ng_p):
            alpha, alpha_p = _out_like(cols, cap)
            comp1, comp1_p = _out_int(cols, cap, "int32")
            extra = _lib.Within2Out(pred_p, resid_p, 0.0, 0, 0, 0, 0, 0)
            fx = _lib.Within2Effects(alpha_p, alpha2_p, comp1_p, comp2_p, keys_p, cap, 0)
            name = "pds_lin_reg_within2_fx_by_key" if ck is None else "pds_lin_reg_within2_cl_by_key"
            rc = ctx.fn(name)(ctx._h, cols.cols, k_p, codes2_p, C.c_int64(n_levels2), p, C.c_int64(n), cols.space, se_code,
                              C.c_double(float(absorb_tol)), int(absorb_max_iter), C.byref(rep), C.byref(extra), ng_p, C.byref(fx), *cl_args)
            return rc, (alpha, comp1, extra, fx)

        with _accel_option(ctx, absorb_accel):
            effect_keys, (alpha, comp1, extra, fx), g = _by_key_retry(cols, max_groups, call)
        alpha, comp1 = alpha[:g], comp1[:g]
    elif key2 is not None:
        k, k_p = _key_arg(cols, absorb)
        codes2, codes2_p, n_levels2, _ = _dense_codes(cols, key2)
        extra = _lib.Within2Out(pred_p, resid_p, 0.0, 0, 0, 0, 0, 0)
        ng = C.c_int64(0)
        with _accel_option(ctx, absorb_accel):
            if ck is None:
                _lib.check(ctx.fn("pds_lin_reg_within2_by_key")(ctx._h, cols.cols, k_p, codes2_p, C.c_int64(n_levels2), p, C.c_int64(n), cols.space,
                                                                se_code, C.c_double(float(absorb_tol)), int(absorb_max_iter), C.byref(rep),
                                                                C.byref(extra), C.byref(ng)))
            else:  # (no effects asked for: fx is NULL)
                _lib.check(ctx.fn("pds_lin_reg_within2_cl_by_key")(ctx._h, cols.cols, k_p, codes2_p, C.c_int64(n_levels2), p, C.c_int64(n), cols.space,
                                                                   se_code, C.c_double(float(absorb_tol)), int(absorb_max_iter), C.byref(rep),
                                                                   C.byref(extra), C.byref(ng), None, C.byref(ck)))
    else:
        form = "within" if ck is None else "within_cl"

        def by_key(k_p, cap, alpha_p, keys_p, ng_p):
            extra = _lib.WithinOut(alpha_p, pred_p, resid_p, 0.0, 0, 0)
            return ctx.fn(f"pds_lin_reg_{form}_by_key")(ctx._h, cols.cols, k_p, p, C.c_int64(n), cols.space, se_code, C.c_int64(cap), keys_p,
                                                        C.byref(rep), C.byref(extra), ng_p, *cl_args), extra

        def grouped(off_p, ng_all, alpha_p):
            extra = _lib.WithinOut(alpha_p, pred_p, resid_p, 0.0, 0, 0)
            return ctx.fn(f"pds_lin_reg_{form}_grouped")(ctx._h, cols.cols, p, C.c_int64(n), off_p, C.c_int64(ng_all), cols.space, se_code,
                                                         C.byref(rep), C.byref(extra), *cl_args), extra

        effect_keys, alpha, extra = _absorbed_call(cols, absorb, absorb_offsets, return_effects, max_groups, by_key, grouped)
    if fit_only:
        out = {"beta": outs["beta"]}
    else:
        out = _report_dict(outs, rep, p, False, std_err, False, feature_names, dt)
        out["r2_overall"] = float(extra.r2_overall)
        out["n_groups"] = int(extra.n_groups_used)
        out["df_resid"] = int(extra.df_resid)
        if key2 is not None:
            out["n_groups2"], out["n_components"], out["n_iter"] = int(extra.n_groups2_used), int(extra.n_components), int(extra.n_iter)
        if ck is not None:
            out["n_clusters"] = int(ck.n_clusters)
            out["absorb_nested"] = (bool(ck.nested1), bool(ck.nested2)) if key2 is not None else (bool(ck.nested1),)
    if return_effects or effects2:
        out["effects"], out["effect_keys"] = alpha, effect_keys
    if effects2:
        out["effects2"], out["effect_keys2"], out["component"], out["component2"] = alpha2, effect_keys2, comp1, comp2
        out["n_graph_rounds"] = int(fx.n_graph_rounds)
    if return_pred:
        out["pred"], out["resid"] = pred, resid
    return out


def _is_int_column(key) -> bool:
    """Whether a key column holds integers (asked before anything is copied or coded)."""
    if _is_torch(key):
        import torch

        return not (key.dtype.is_floating_point or key.dtype.is_complex or key.dtype == torch.bool)
    return np.asarray(key).dtype.kind in "iu"


def _codes_of(key, device, n_rows=None):
    """An integer key column as dense int32 codes per row (plumbing, not the hot path): (codes, address, the distinct keys ascending).
    `device`: the torch device the codes are wanted on, None for host memory."""
    if device is not None:
        import torch

        t = key if _is_torch(key) else torch.as_tensor(np.asarray(key))
        if t.dtype.is_floating_point or t.dtype == torch.bool:
            raise ValueError("an absorbed key must be an integer column")
        t = t.to(device=device)
        if t.ndim != 1 or (n_rows is not None and int(t.shape[0]) != n_rows):
            raise ValueError("`key` must have one entry per row")
        uniq, inv = torch.unique(t, return_inverse=True)
        codes = inv.to(torch.int32).contiguous()
        return codes, C.c_void_p(int(codes.data_ptr())), uniq
    a = key.detach().cpu().numpy() if _is_torch(key) else np.asarray(key)
    if a.dtype.kind not in "iu":
        raise ValueError("an absorbed key must be an integer column")
    if a.ndim != 1 or (n_rows is not None and int(a.shape[0]) != n_rows):
        raise ValueError("`key` must have one entry per row")
    uniq, inv = np.unique(a, return_inverse=True)
    codes = np.ascontiguousarray(inv.reshape(-1), dtype=np.int32)
    return codes, C.c_void_p(codes.ctypes.data), uniq


def _dense_codes(cols: "_Cols", key):
    """The second absorbed key as dense int32 codes per row in the inputs' space: (codes, address, levels, the distinct keys ascending)."""
    codes, codes_p, uniq = _codes_of(key, cols.keep[0].device if cols.space == _lib.PDS_DEVICE else None, cols.n_rows)
    return codes, codes_p, int(uniq.shape[0]), uniq


def fixed_effects(*x, target, absorb, std_err: str = "se", absorb_tol: float = 1e-8, absorb_max_iter: int = 10_000, return_pred: bool = False,
                  feature_names: Sequence[str] | None = None, add_bias: bool = False, weights=None, max_groups: int | None = None,
                  absorb_accel: str | None = None, cluster_key=None, ctx: Context | None = None) -> dict:
    """
    The two-way fixed-effects regression y_i = alpha_k1(i) + gamma_k2(i) + x_i' beta + e_i WITH its estimated effects
    (pds_lin_reg_within2_fx_by_key_*; include/pds_lstsq.h states the definitions).  `absorb=[k1, k2]`: exactly two integer columns.
    Every entry of lin_reg_report(absorb=[k1, k2]) with the same arguments, bit for bit, plus
        "effects" / "effect_keys"     alpha per distinct key of k1, ascending
        "effects2" / "effect_keys2"   gamma per distinct key of k2, ascending
        "component" / "component2"    the connected component of every level, as the index in "effect_keys" of its smallest level of k1
        "n_graph_rounds"              the rounds the component labelling took
    The effects are identified up to one constant per component.  The normalisation is a DEFINITION: in every component gamma is
    exactly 0.0 at the smallest key of k2 that occurs in it -- the coefficients of the regression on the features, a dummy per level
    of k1 and a dummy per level of k2 less that one per component.  NumPy arrays or CUDA tensors; a device frame gets device outputs.
    `max_groups`: a bound on the distinct keys of k1 (the outputs are sized for it), as in the other by-key calls.
    `absorb_accel`: None (the context's option "within2_accel"), "none" or "irons_tuck" -- cycles of two plain sweeps and one
    extrapolation of the factor-2 table, see lin_reg_report; "n_iter" counts sweeps.  The call ends on a sweep, so the effects and
    their normalisation are formed from the tables exactly as without acceleration.
    `cluster_key`: as in lin_reg_report -- the errors clustered on this key (std_err "cluster" / "cluster0"), "n_clusters" and
    "absorb_nested" added, "df_resid" = Gc - 1; every other entry, the effects included, as without it.
    """
    if not isinstance(absorb, (list, tuple)) or len(absorb) < 2:
        raise ValueError("fixed_effects: `absorb` is a list of exactly two integer columns; the effects of ONE absorbed key come from "
                         "lin_reg_report(absorb=k, return_effects=True)")
    return _lin_reg_within(x, target, add_bias, weights, std_err, feature_names, absorb, None, None, False, return_pred, max_groups, ctx,
                           absorb_tol=absorb_tol, absorb_max_iter=absorb_max_iter, effects2=True, absorb_accel=absorb_accel,
                           cluster_key=cluster_key)


def absorb_components(k1, k2, ctx: Context | None = None) -> dict:
    """
    The connected components of the bipartite graph whose edges are the (k1, k2) pairs that occur -- the "mobility groups" inside which
    the effects of a two-way fixed-effects model can be compared (pds_absorb_components_i32).  k1, k2: integer columns of equal length,
    NumPy arrays or CUDA tensors, rows in any order.  Returns "n_groups" / "n_groups2" (distinct keys), "n_components", "keys1" /
    "keys2" (the distinct keys, ascending), "component1" / "component2" (per distinct key, the index in "keys1" of the smallest key
    of k1 in its component) and "n_rounds" (rounds of the labelling).  Device columns get device outputs.
    """
    for k in (k1, k2):
        if _is_arrow(k):
            raise NotImplementedError("absorb_components: pyarrow columns are not supported (NumPy arrays or CUDA tensors)")
    device = next((k.device for k in (k1, k2) if _is_torch(k) and k.is_cuda), None)
    codes1, codes1_p, keys1 = _codes_of(k1, device)
    codes2, codes2_p, keys2 = _codes_of(k2, device, int(codes1.shape[0]))
    n = int(codes1.shape[0])
    if n == 0:
        raise ValueError("absorb_components: the key columns are empty")
    ctx = ctx or default_context()
    if device is not None:
        import torch

        ctx.follow_torch_stream(device)
        comp = [torch.empty(int(u.shape[0]), dtype=torch.int32, device=device) for u in (keys1, keys2)]
        comp_p = [C.c_void_p(int(c.data_ptr())) for c in comp]
    else:
        comp = [np.empty(int(u.shape[0]), dtype=np.int32) for u in (keys1, keys2)]
        comp_p = [C.c_void_p(c.ctypes.data) for c in comp]
    n1, n2, nc, rounds = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int(0)
    _lib.check(ctx._lib.pds_absorb_components_i32(ctx._h, codes1_p, C.c_int64(int(keys1.shape[0])), codes2_p, C.c_int64(int(keys2.shape[0])),
                                                  C.c_int64(n), _lib.PDS_DEVICE if device is not None else _lib.PDS_HOST, comp_p[0], comp_p[1],
                                                  C.byref(n1), C.byref(n2), C.byref(nc), C.byref(rounds)))
    return {"n_groups": int(n1.value), "n_groups2": int(n2.value), "n_components": int(nc.value), "keys1": keys1, "component1": comp[0],
            "keys2": keys2, "component2": comp[1], "n_rounds": int(rounds.value)}


# ---- the stages of lin_reg_report as separate calls (row-sharded multi-GPU form: parallel.lin_reg_report_row_sharded)
def report_fit_from_moments(moments, *, add_bias: bool = False, ctx: Context | None = None):
    """Stage 2: (all-reduced) moment matrix -> (beta [p'], inv [p' x p'] = (X'X)^-1 by column-pivoted QR).  Host arrays."""
    ctx = ctx or default_context()
    dt = _dtype()
    if _is_torch(moments):
        moments = moments.detach().cpu().numpy()
    m = np.asfortranarray(np.asarray(moments, dtype=dt))
    q = int(m.shape[0])
    p = q - 2
    pp = p + int(bool(add_bias))
    beta = np.empty(pp, dtype=dt)
    inv = np.empty((pp, pp), dtype=dt, order="F")
    _lib.check(ctx.fn("pds_report_fit_from_moments")(ctx._h, C.c_void_p(m.ctypes.data), p, int(bool(add_bias)),
                                                     C.c_void_p(beta.ctypes.data), C.c_void_p(inv.ctypes.data)))
    return beta, inv


def report_partials(*x, target, beta, inv, add_bias: bool = False, weights=None, std_err: str = "se", ctx: Context | None = None):
    """Stage 3 on this rank's rows: [sum e^2, sum w e^2, meat block ((p+2)^2)] as one float64 vector (the all-reduce payload)."""
    ctx = ctx or default_context()
    cols = _Cols(target, x, weights)
    _follow(ctx, cols)
    dt = _dtype()
    q = cols.n_feat + 2
    beta = np.ascontiguousarray(beta, dtype=dt)
    inv = np.asfortranarray(np.asarray(inv, dtype=dt))
    out = np.zeros(2 + q * q, dtype=np.float64)
    _lib.check(ctx.fn("pds_report_partials")(ctx._h, cols.cols, cols.weights, cols.n_feat, C.c_int64(cols.n_rows), cols.space,
                                             int(bool(add_bias)), _lib.SE_TYPES.get(std_err, 0), C.c_void_p(beta.ctypes.data),
                                             C.c_void_p(inv.ctypes.data), C.c_void_p(out.ctypes.data)))
    return out


def report_finish(beta, inv, partials, *, n_rows_total: int, y_var: float, add_bias: bool = False, weighted: bool = False,
                  std_err: str = "se", feature_names: Sequence[str] | None = None) -> dict:
    """Stage 4: the O(p'^2) epilogue on the summed partials (no device work)."""
    lib = _lib.load()
    dt = _dtype()
    beta = np.ascontiguousarray(beta, dtype=dt)
    inv = np.asfortranarray(np.asarray(inv, dtype=dt))
    partials = np.ascontiguousarray(partials, dtype=np.float64)
    pp = int(beta.shape[0])
    n_feat = pp - int(bool(add_bias))
    outs = {k: np.empty(pp, dtype=dt) for k in ("beta", "std_err", "t", "p", "ci_lower", "ci_upper")}
    R = _lib.ReportF64 if config.LIN_REG_EXPR_F64 else _lib.ReportF32
    rep = R(*[C.c_void_p(outs[k].ctypes.data) for k in ("beta", "std_err", "t", "p", "ci_lower", "ci_upper")], 0.0, 0.0)
    yv = C.c_double(y_var) if config.LIN_REG_EXPR_F64 else C.c_float(y_var)
    fn = getattr(lib, "pds_report_finish" + _suffix())
    _lib.check(fn(n_feat, int(bool(add_bias)), _lib.SE_TYPES.get(std_err, 0), int(bool(weighted)), C.c_int64(int(n_rows_total)), yv,
                  C.c_void_p(beta.ctypes.data), C.c_void_p(inv.ctypes.data), C.c_void_p(partials.ctypes.data), C.byref(rep)))
    return _report_dict(outs, rep, n_feat, add_bias, std_err, weighted, feature_names, dt)


def _report_dict(outs, rep, n_feat, add_bias, std_err, weighted, feature_names, dt):
    pp = n_feat + int(bool(add_bias))
    names = list(feature_names) if feature_names is not None else [f"x{i + 1}" for i in range(n_feat)]
    if add_bias:
        names.append("__bias__")  # linear_regression.rs:843-845
    se_name = {"se": "std_err", "hc0": "hc0_se", "hc1": "hc1_se", "hc2": "hc2_se", "hc3": "hc3_se", "cluster": "cluster_se",
               "cluster0": "cluster0_se"}.get(std_err, "std_err")
    if weighted:
        se_name = "std_err"
    return {
        "features": names, "beta": outs["beta"], se_name: outs["std_err"], "t": outs["t"], "p>|t|": outs["p"],
        "0.025": outs["ci_lower"], "0.975": outs["ci_upper"],
        "r2": np.full(pp, rep.r2, dtype=dt), "adj_r2": np.full(pp, rep.adj_r2, dtype=dt),
    }


_REPORT_KEYS = ("beta", "std_err", "t", "p", "ci_lower", "ci_upper")


def _report_grouped_outs(cols: _Cols, ng: int, pp: int):
    outs = {k: _out_like(cols, (ng, pp)) for k in _REPORT_KEYS}
    outs["r2"] = _out_like(cols, (ng,))
    outs["adj_r2"] = _out_like(cols, (ng,))
    outs["is_null"] = _out_u8(cols, ng)
    rep = _lib.ReportGrouped(*[outs[k][1] for k in (*_REPORT_KEYS, "r2", "adj_r2", "is_null")])
    return outs, rep


def _report_grouped_dict(outs, n_feat, add_bias, std_err, feature_names, g=None):
    names = list(feature_names) if feature_names is not None else [f"x{i + 1}" for i in range(n_feat)]
    if add_bias:
        names.append("__bias__")  # linear_regression.rs:843-845
    se_name = {"se": "std_err", "hc0": "hc0_se", "hc1": "hc1_se", "hc2": "hc2_se", "hc3": "hc3_se", "cluster": "cluster_se",
               "cluster0": "cluster0_se"}.get(std_err, "std_err")
    cut = (lambda a: a[:g]) if g is not None else (lambda a: a)
    return {
        "features": names, "beta": cut(outs["beta"][0]), se_name: cut(outs["std_err"][0]), "t": cut(outs["t"][0]),
        "p>|t|": cut(outs["p"][0]), "0.025": cut(outs["ci_lower"][0]), "0.975": cut(outs["ci_upper"][0]),
        "r2": cut(outs["r2"][0]), "adj_r2": cut(outs["adj_r2"][0]), "is_null": cut(outs["is_null"][0]),
    }


def _check_report_weights(x, target, weights) -> None:
    """Argument checks of the weighted grouped report that need no device: one weight per row, at most 64 features."""
    n = int(target.shape[0]) if hasattr(target, "shape") else len(target)
    nw = int(weights.shape[0]) if hasattr(weights, "shape") else len(weights)
    if nw != n:
        raise ValueError("`weights` must have one entry per row")
    if len(x) > 64:
        raise _lib.PdsError(-5, "grouped lin_reg_report: at most 64 features")  # PDS_ERR_UNSUPPORTED, as the C entry answers


def lin_reg_report_by(*x, target, group_offsets, add_bias: bool = False, std_err: str = "se", y_var=None,
                      feature_names: Sequence[str] | None = None, weights=None, ctx: Context | None = None) -> dict:
    """
    The grouped form of `lin_reg_report`: `df.group_by(key).agg(pds.lin_reg_report(...))` for a frame whose groups are contiguous
    row ranges (group g = rows [group_offsets[g], group_offsets[g+1])), in one call.  Every group's report equals the single
    report on its rows, except that a group with fewer rows than coefficients is null (`is_null`, NaN values) instead of an error.
    `y_var` (optional, one value per group): the target's variance per group; by default the sample variance (ddof=1) of each
    group's target is computed on the device.
    Returns a dict of [n_groups, p'] arrays ("beta", the standard-error column, "t", "p>|t|", "0.025", "0.975"), "r2" / "adj_r2" /
    "is_null" [n_groups] and "features", in the memory space of the inputs.
    `weights` (one per row, cast and placed like the columns): every group's report is the weighted one (`lin_reg_report(...,
    weights=w)` on its rows: pl_wls_report); the standard-error column is then "std_err" and `std_err` is ignored.
    """
    if weights is not None:
        _check_report_weights(x, target, weights)
        std_err = "se"
    ctx = ctx or default_context()
    cols = _Cols(target, x, weights)
    _follow(ctx, cols)
    pp = cols.n_feat + int(bool(add_bias))
    off, off_p = _offsets_arg(cols, group_offsets)
    ng = int(off.shape[0]) - 1
    outs, rep = _report_grouped_outs(cols, ng, pp)
    yv_p = C.c_void_p(None)
    if y_var is not None:
        if cols.space == _lib.PDS_DEVICE:
            import torch

            yv = y_var if _is_torch(y_var) else torch.as_tensor(np.asarray(y_var))
            yv = yv.to(device=cols.keep[0].device, dtype=cols.keep[0].dtype).contiguous()
            yv_p = C.c_void_p(int(yv.data_ptr()))
        else:
            yv = np.ascontiguousarray(np.asarray(y_var), dtype=_dtype())
            yv_p = C.c_void_p(yv.ctypes.data)
        if int(yv.shape[0]) != ng:
            raise ValueError("`y_var` must have one value per group")
    if weights is not None:
        _lib.check(ctx.fn("pds_wls_report_grouped")(ctx._h, cols.cols, cols.weights, cols.n_feat, C.c_int64(cols.n_rows), off_p,
                                                    C.c_int64(ng), cols.space, int(bool(add_bias)), yv_p, C.byref(rep)))
    else:
        _lib.check(ctx.fn("pds_lin_reg_report_grouped")(ctx._h, cols.cols, cols.n_feat, C.c_int64(cols.n_rows), off_p, C.c_int64(ng),
                                                        cols.space, int(bool(add_bias)), _lib.SE_TYPES.get(std_err, 0), yv_p,
                                                        C.byref(rep)))
    return _report_grouped_dict(outs, cols.n_feat, add_bias, std_err, feature_names)


def lin_reg_report_by_key(*x, target, key, add_bias: bool = False, std_err: str = "se", max_groups: int | None = None,
                          feature_names: Sequence[str] | None = None, weights=None, ctx: Context | None = None) -> dict:
    """
    `lin_reg_report_by` for an int64 key column in ANY row order (the frame is brought into key order on the device, as
    `lin_reg_by_key` does; nothing moves when the keys are already non-decreasing).  Returns the dict of `lin_reg_report_by`
    plus "keys" (ascending).  var(y) is always the per-group sample variance.  `weights`: as in `lin_reg_report_by` (with unordered
    keys they are reordered with the frame).
    """
    if weights is not None:
        _check_report_weights(x, target, weights)
        std_err = "se"
    ctx = ctx or default_context()
    cols = _Cols(target, x, weights)
    _follow(ctx, cols)
    pp = cols.n_feat + int(bool(add_bias))
    n_rows = cols.n_rows
    k, k_p = _key_arg(cols, key)

    def call(cap, ok_p, ng_p):
        outs, rep = _report_grouped_outs(cols, cap, pp)
        if weights is not None:
            rc = ctx.fn("pds_wls_report_by_key")(ctx._h, cols.cols, cols.weights, k_p, cols.n_feat, C.c_int64(n_rows), cols.space,
                                                 int(bool(add_bias)), C.c_int64(cap), ok_p, C.byref(rep), ng_p)
        else:
            rc = ctx.fn("pds_lin_reg_report_by_key")(ctx._h, cols.cols, k_p, cols.n_feat, C.c_int64(n_rows), cols.space,
                                                     int(bool(add_bias)), _lib.SE_TYPES.get(std_err, 0), C.c_int64(cap), ok_p,
                                                     C.byref(rep), ng_p)
        return rc, outs

    keys, outs, g = _by_key_retry(cols, max_groups, call)
    d = _report_grouped_dict(outs, cols.n_feat, add_bias, std_err, feature_names, g)
    d["keys"] = keys
    return d


def student_t_sf_device(x, df, ctx: Context | None = None):
    """The grouped report's device Student-t survival function on host arrays (tests: against pds_student_t_sf)."""
    ctx = ctx or default_context()
    xa = np.ascontiguousarray(np.asarray(x, dtype=np.float64))
    da = np.ascontiguousarray(np.broadcast_to(np.asarray(df, dtype=np.float64), xa.shape))
    out = np.empty_like(xa)
    _lib.check(_lib.load().pds_student_t_sf_device(ctx._h, C.c_void_p(xa.ctypes.data), C.c_void_p(da.ctypes.data),
                                                   C.c_int64(xa.size), C.c_void_p(out.ctypes.data)))
    return out


def lin_reg_by(*x, target, group_offsets, add_bias: bool = False, l1_reg: float = 0.0, l2_reg: float = 0.0,
               tol: float = 1e-5, solver: str = "qr", max_iter: int = 200, positive: bool = False,
               singular_x_tol: float | None = None, null_policy: str = "skip", weights=None, ctx: Context | None = None):
    """
    The key-aware batched form of `df.group_by(key).agg(pds.lin_reg(...))` (SURVEY.md 8b "pl_lr_by").
    Rows of a group are contiguous; group g = rows [group_offsets[g], group_offsets[g+1]).
    Returns (coeffs [n_groups, p'], is_null [n_groups]) in the memory space of the inputs.
    pyarrow columns may carry nulls; `null_policy` then applies inside every group, as it does when Polars calls pl_lr
    once per group.  `l1_reg` / `l2_reg` / `positive` select the method per group exactly as `lin_reg` does
    (lasso / elastic net / non-negative fits run the reference's coordinate descent on every group's Gram matrix).
    `weights`: per-group weighted least squares (faer_weighted_lr: no gate, no penalties, like `lin_reg(weights=...)`).
    """
    if max_iter <= 0:
        raise ValueError("Input `max_iter` must be a positive.")  # expr_linear.py:231-232
    ctx = ctx or default_context()
    if weights is not None:
        cols = _Cols(target, x, weights)
        _follow(ctx, cols)
        prm = _params(add_bias, 0.0, 0.0, tol, solver, False, max_iter, 0.0)
        pp = cols.n_feat + int(bool(add_bias))
        off, off_p = _offsets_arg(cols, group_offsets)
        ng = int(off.shape[0]) - 1
        coeffs, co_p = _out_like(cols, (ng, pp))
        nulls, nu_p = _out_u8(cols, ng)
        _lib.check(ctx.fn("pds_lr_grouped_weighted")(ctx._h, cols.cols, cols.weights, cols.n_feat, C.c_int64(cols.n_rows), off_p,
                                                     C.c_int64(ng), cols.space, C.byref(prm), co_p, nu_p))
        return coeffs, nulls
    code, fill = parse_null_policy(null_policy)
    if any(_is_arrow(c) for c in (target, *x)):
        dt = _dtype()
        parts = [_arrow_parts(c, dt) if _is_arrow(c) else (np.ascontiguousarray(np.asarray(c), dtype=dt), 0, 0, None)
                 for c in (target, *x)]
        n = len(parts[0][0])
        if any(len(pt[0]) != n for pt in parts):
            raise ValueError("all columns must be 1-D and of equal length")
        nc = len(parts)
        prm = _params(add_bias, l1_reg, l2_reg, tol, solver, positive, max_iter, singular_x_tol)
        pp = nc - 1 + int(bool(add_bias))
        off = np.ascontiguousarray(np.asarray(group_offsets), dtype=np.int64)
        ng = int(off.shape[0]) - 1
        coeffs = np.empty((ng, pp), dtype=dt)
        nulls = np.empty(ng, dtype=np.uint8)
        cp = (C.c_void_p * nc)(*[pt[0].ctypes.data for pt in parts])
        vp = (C.c_void_p * nc)(*[pt[1] or None for pt in parts])
        op = (C.c_int64 * nc)(*[pt[2] for pt in parts])
        f = (C.c_double if config.LIN_REG_EXPR_F64 else C.c_float)
        _lib.check(ctx.fn("pds_lr_grouped_nullable")(ctx._h, cp, vp, op, nc - 1, C.c_int64(n), C.c_void_p(off.ctypes.data),
                                                     C.c_int64(ng), _lib.PDS_HOST, code, f(fill), C.byref(prm),
                                                     C.c_void_p(coeffs.ctypes.data), C.c_void_p(nulls.ctypes.data)))
        return coeffs, nulls
    cols = _Cols(target, x)
    _follow(ctx, cols)
    prm = _params(add_bias, l1_reg, l2_reg, tol, solver, positive, max_iter, singular_x_tol)
    pp = cols.n_feat + int(bool(add_bias))
    off, off_p = _offsets_arg(cols, group_offsets)
    ng = int(off.shape[0]) - 1
    coeffs, co_p = _out_like(cols, (ng, pp))
    nulls, nu_p = _out_u8(cols, ng)
    _lib.check(ctx.fn("pds_lr_grouped")(ctx._h, cols.cols, cols.n_feat, C.c_int64(cols.n_rows), off_p, C.c_int64(ng),
                                        cols.space, C.byref(prm), co_p, nu_p))
    return coeffs, nulls


class DeviceBlock:
    """
    `bytes` of device memory that kernels of ANOTHER process can write (include/pds_lstsq.h: pds_device_alloc / pds_ipc_export /
    pds_ipc_open): the owner allocates and exports 64 opaque handle bytes; a peer maps them with `DeviceBlock.open(handle, device)`
    and uses `.addr` (+ byte offsets) as a raw output address.  `tensor(dtype, shape, byte_offset)` views the OWNER's block as a torch
    tensor (`__cuda_array_interface__`).  Freed / unmapped by `close()` (or at garbage collection).
    """

    def __init__(self, nbytes: int, device: int, fine_grained: bool = True):
        self._lib = _lib.load()
        self.device, self.nbytes, self.owner = int(device), int(nbytes), True
        p = C.c_void_p()
        # (fine grained: coherent across devices -- rows another device's kernel writes must not sit stale in this device's L2)
        _lib.check(self._lib.pds_device_alloc(self.device, C.c_size_t(self.nbytes), int(bool(fine_grained)), C.byref(p)))
        self.addr = int(p.value)

    @classmethod
    def open(cls, handle: bytes, device: int, nbytes: int = 0):
        self = cls.__new__(cls)
        self._lib = _lib.load()
        self.device, self.nbytes, self.owner = int(device), int(nbytes), False
        p = C.c_void_p()
        hb = (C.c_ubyte * 64).from_buffer_copy(bytes(handle))
        _lib.check(self._lib.pds_ipc_open(self.device, hb, C.byref(p)))
        self.addr = int(p.value)
        return self

    def handle(self) -> bytes:
        hb = (C.c_ubyte * 64)()
        _lib.check(self._lib.pds_ipc_export(self.device, C.c_void_p(self.addr), hb))
        return bytes(hb)

    def tensor(self, dtype, shape, byte_offset: int = 0):
        import torch

        class _View:  # (torch keeps the object alive as the tensor's base)
            pass

        v = _View()
        v.block = self
        typestr = {torch.float64: "<f8", torch.float32: "<f4", torch.uint8: "|u1", torch.int64: "<i8"}[dtype]
        v.__cuda_array_interface__ = {"shape": tuple(int(d) for d in shape), "typestr": typestr, "data": (self.addr + int(byte_offset), False),
                                      "version": 2, "strides": None}
        return torch.as_tensor(v, device=torch.device("cuda", self.device))

    def close(self) -> None:
        if getattr(self, "addr", 0):
            if self.owner:
                self._lib.pds_device_free(self.device, C.c_void_p(self.addr))
            else:
                self._lib.pds_ipc_close(self.device, C.c_void_p(self.addr))
            self.addr = 0

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class GroupedFit:
    """
    A prepared `lin_reg_by` over DEVICE-resident columns with contiguous groups: the column pointer table, the parameter block, the
    device offsets and the result buffers are set up once; `run()` is then one C call (`pds_lr_grouped_*`) and nothing else -- no
    allocation, no dtype / contiguity checks, no Python per column.  What a host engine that evaluates the same expression over a
    resident frame repeatedly (or one rank of the group-sharded step, parallel.GroupedShardPlan) holds on to.

    `out` / `out_null`: where the coefficients ([n_groups, p'] of the config dtype, contiguous) and the null flags ([n_groups] uint8)
    go -- e.g. rows of a larger gathered result, so that the fit writes them in place.  By default they are allocated here, once.
    Every `run()` recomputes and overwrites them; it returns the same two tensors.
    `out_addr` / `out_null_addr` (both or neither; instead of `out` / `out_null`): raw device addresses of such rows in memory that
    is not a torch tensor of this process -- the assembled result of ANOTHER rank, mapped with `DeviceBlock.open` (the direct gather of
    parallel.GroupedShardPlan): the kernel's stores cross the link.  `run()` then returns (None, None).
    """

    def __init__(self, *x, target, group_offsets, add_bias: bool = False, l1_reg: float = 0.0, l2_reg: float = 0.0, tol: float = 1e-5,
                 solver: str = "qr", max_iter: int = 200, positive: bool = False, singular_x_tol: float | None = None, out=None,
                 out_null=None, out_addr: int | None = None, out_null_addr: int | None = None, ctx: Context | None = None):
        if max_iter <= 0:
            raise ValueError("Input `max_iter` must be a positive.")  # expr_linear.py:231-232
        import torch

        self.ctx = ctx or default_context()
        cols = _Cols(target, x)
        if cols.space != _lib.PDS_DEVICE:
            raise ValueError("GroupedFit prepares device-resident frames (host frames: lin_reg_by)")
        self._cols = cols
        self._prm = _params(add_bias, l1_reg, l2_reg, tol, solver, positive, max_iter, singular_x_tol)
        self._off, off_p = _offsets_arg(cols, group_offsets)
        ng = int(self._off.shape[0]) - 1
        pp = cols.n_feat + int(bool(add_bias))
        tdt = torch.float64 if config.LIN_REG_EXPR_F64 else torch.float32
        dev = cols.keep[0].device
        if (out_addr is None) != (out_null_addr is None) or (out_addr is not None and (out is not None or out_null is not None)):
            raise ValueError("`out_addr` and `out_null_addr` come together, instead of `out` / `out_null`")
        if out_addr is not None:
            self.coeffs = self.is_null = None
            self.n_groups = ng
            self._fn = self.ctx.fn("pds_lr_grouped")
            self._args = (self.ctx._h, cols.cols, cols.n_feat, C.c_int64(cols.n_rows), off_p, C.c_int64(ng), cols.space, C.byref(self._prm),
                          C.c_void_p(int(out_addr)), C.c_void_p(int(out_null_addr)))
            self._dev = cols.torch_device
            return
        if out is None:
            out = torch.empty((ng, pp), dtype=tdt, device=dev)
        if out_null is None:
            out_null = torch.empty((ng,), dtype=torch.uint8, device=dev)
        if tuple(out.shape) != (ng, pp) or out.dtype != tdt or out.device != dev or not out.is_contiguous():
            raise ValueError(f"`out` must be a contiguous [{ng}, {pp}] {tdt} tensor on {dev}")
        if tuple(out_null.shape) != (ng,) or out_null.dtype != torch.uint8 or out_null.device != dev or not out_null.is_contiguous():
            raise ValueError(f"`out_null` must be a contiguous [{ng}] uint8 tensor on {dev}")
        self.coeffs, self.is_null = out, out_null
        self.n_groups = ng
        self._fn = self.ctx.fn("pds_lr_grouped")
        self._args = (self.ctx._h, cols.cols, cols.n_feat, C.c_int64(cols.n_rows), off_p, C.c_int64(ng), cols.space, C.byref(self._prm),
                      C.c_void_p(int(out.data_ptr())), C.c_void_p(int(out_null.data_ptr())))
        self._dev = cols.torch_device

    def run(self):
        if self.n_groups <= 0:
            return self.coeffs, self.is_null
        self.ctx.follow_torch_stream(self._dev)
        rc = self._fn(*self._args)
        if rc:
            _lib.check(rc)
        return self.coeffs, self.is_null  # ((None, None) with raw output addresses)


def lin_reg_by_key(*x, target, key, add_bias: bool = False, l1_reg: float = 0.0, l2_reg: float = 0.0, tol: float = 1e-5,
                   solver: str = "qr", max_iter: int = 200, positive: bool = False, singular_x_tol: float | None = None,
                   max_groups: int | None = None, ctx: Context | None = None):
    """
    `df.group_by(key).agg(pds.lin_reg(...))` for an integer key column in ANY row order: the frame is brought into key
    order on the device (radix sort of (key, row) pairs + column gather; nothing moves when the keys are already
    non-decreasing), then every group is fitted as in `lin_reg_by`.
    Returns (keys [n_groups] ascending, coeffs [n_groups, p'], is_null [n_groups]) in the memory space of the inputs.
    """
    if max_iter <= 0:
        raise ValueError("Input `max_iter` must be a positive.")  # expr_linear.py:231-232
    ctx = ctx or default_context()
    cols = _Cols(target, x)
    _follow(ctx, cols)
    prm = _params(add_bias, l1_reg, l2_reg, tol, solver, positive, max_iter, singular_x_tol)
    pp = cols.n_feat + int(bool(add_bias))
    n_rows = cols.n_rows
    k, k_p = _key_arg(cols, key)

    def call(cap, ok_p, ng_p):
        coeffs, co_p = _out_like(cols, (cap, pp))
        nulls, nu_p = _out_u8(cols, cap)
        rc = ctx.fn("pds_lr_by_key")(ctx._h, cols.cols, k_p, cols.n_feat, C.c_int64(n_rows), cols.space, C.byref(prm),
                                     C.c_int64(cap), ok_p, co_p, nu_p, ng_p)
        return rc, (coeffs, nulls)

    keys, (coeffs, nulls), g = _by_key_retry(cols, max_groups, call)
    return keys, coeffs[:g], nulls[:g]


def lin_reg_by_key_multi(*x, target, key, contexts, n_slices: int = 0, add_bias: bool = False, l1_reg: float = 0.0, l2_reg: float = 0.0,
                         tol: float = 1e-5, solver: str = "qr", max_iter: int = 200, positive: bool = False,
                         singular_x_tol: float | None = None, max_groups: int | None = None):
    """
    `lin_reg_by_key` for a HOST frame whose keys are in order, driven through several contexts from this one process
    (pds_lr_by_key_multi_*): the frame is cut into row slices at group boundaries and slice s is fitted by contexts[s mod n] on
    that context's device -- contexts on different devices pull their shards over their own PCIe links,
    several contexts on one device overlap a slice's transfer with the previous slice's fit.  Same results as `lin_reg_by_key`.
    Returns (keys, coeffs, is_null) as numpy arrays.
    """
    if max_iter <= 0:
        raise ValueError("Input `max_iter` must be a positive.")
    cols = _Cols(target, x)
    if cols.space != _lib.PDS_HOST:
        raise ValueError("lin_reg_by_key_multi takes host-resident columns (numpy)")
    prm = _params(add_bias, l1_reg, l2_reg, tol, solver, positive, max_iter, singular_x_tol)
    pp = cols.n_feat + int(bool(add_bias))
    n_rows = cols.n_rows
    k, k_p = _key_arg(cols, key)
    handles = (C.c_void_p * len(contexts))(*[c._h for c in contexts])
    fn = contexts[0].fn("pds_lr_by_key_multi")

    def call(cap, ok_p, ng_p):
        coeffs, co_p = _out_like(cols, (cap, pp))
        nulls, nu_p = _out_u8(cols, cap)
        rc = fn(handles, len(contexts), int(n_slices), cols.cols, k_p, cols.n_feat, C.c_int64(n_rows), C.byref(prm), C.c_int64(cap), ok_p,
                co_p, nu_p, ng_p)
        return rc, (coeffs, nulls)

    keys, (coeffs, nulls), g = _by_key_retry(cols, max_groups, call)
    return keys, coeffs[:g], nulls[:g]


# ---- the exchange steps of SURVEY.md 8(e) between the contexts of ONE process (include/pds_lstsq.h: pds_allreduce_sum_*,
# pds_scatter_rows_*, pds_gather_*): what a host without a collective library composes the multi-device paths from
def _exchange_suffix(t) -> str:
    import torch

    if t.dtype == torch.float64:
        return "_f64"
    if t.dtype == torch.float32:
        return "_f32"
    raise ValueError("exchange steps move float64 / float32 device tensors")


def allreduce_sum(contexts, tensors, prefix: bool = False) -> None:
    """tensors[c]: a contiguous CUDA tensor on contexts[c]'s device, all of one shape and dtype.  In place: every tensor becomes the
    element-wise sum (prefix=True: tensor c becomes the sum of tensors 0 .. c-1 -- the exclusive scan of the row-sharded expanding fit)."""
    n = len(contexts)
    if len(tensors) != n or n < 1:
        raise ValueError("one tensor per context")
    suf = _exchange_suffix(tensors[0])
    for x in tensors:
        if not (x.is_cuda and x.is_contiguous() and x.shape == tensors[0].shape and x.dtype == tensors[0].dtype):
            raise ValueError("contiguous CUDA tensors of one shape and dtype")
    h = (C.c_void_p * n)(*[c._h for c in contexts])
    b = (C.c_void_p * n)(*[x.data_ptr() for x in tensors])
    _lib.check(getattr(_lib.load(), "pds_allreduce_sum" + suf)(h, n, b, C.c_int64(tensors[0].numel()), 1 if prefix else 0))


def scatter_rows(contexts, cols, bounds):
    """cols: CUDA column tensors on contexts[0]'s device; rows [bounds[c], bounds[c+1]) of every column -> new tensors on contexts[c]'s
    device.  Returns a list (per context) of lists of column tensors; rank 0 gets views of the frame itself."""
    import torch

    n = len(contexts)
    suf = _exchange_suffix(cols[0])
    bounds = [int(v) for v in bounds]
    out = [[c[bounds[0]:bounds[1]] for c in cols]]
    for r in range(1, n):
        out.append([torch.empty(bounds[r + 1] - bounds[r], dtype=cols[0].dtype, device=torch.device("cuda", contexts[r].device)) for _ in cols])
    h = (C.c_void_p * n)(*[c._h for c in contexts])
    src = (C.c_void_p * len(cols))(*[c.data_ptr() for c in cols])
    tabs = [(C.c_void_p * len(cols))(*[x.data_ptr() for x in o]) for o in out]
    dst = (C.c_void_p * n)(*([None] + [C.cast(tb, C.c_void_p) for tb in tabs[1:]]))
    bd = (C.c_int64 * (n + 1))(*bounds)
    _lib.check(getattr(_lib.load(), "pds_scatter_rows" + suf)(h, n, src, len(cols), bd, dst))
    return out


def gather(contexts, blocks):
    """blocks[c]: a contiguous CUDA tensor on contexts[c]'s device -> one tensor on contexts[0]'s device, the blocks' elements back
    to back in rank order."""
    import torch

    n = len(contexts)
    suf = _exchange_suffix(blocks[0])
    counts = [int(b.numel()) for b in blocks]
    out = torch.empty(sum(counts), dtype=blocks[0].dtype, device=torch.device("cuda", contexts[0].device))
    h = (C.c_void_p * n)(*[c._h for c in contexts])
    src = (C.c_void_p * n)(*[b.data_ptr() for b in blocks])
    cn = (C.c_int64 * n)(*counts)
    _lib.check(getattr(_lib.load(), "pds_gather" + suf)(h, n, src, cn, C.c_void_p(out.data_ptr())))
    return out


def _offsets_arg(cols: "_Cols", group_offsets):
    if cols.space == _lib.PDS_DEVICE:
        import torch

        off = group_offsets if _is_torch(group_offsets) else torch.as_tensor(np.asarray(group_offsets))
        off = off.to(device=cols.keep[0].device, dtype=torch.int64).contiguous()
        return off, C.c_void_p(int(off.data_ptr()))
    off = np.ascontiguousarray(np.asarray(group_offsets), dtype=np.int64)
    return off, C.c_void_p(off.ctypes.data)


def _key_arg(cols: "_Cols", key):
    """The key column as int64 in the inputs' space (and its address): one entry per row."""
    k, k_p = _offsets_arg(cols, key)
    if int(k.shape[0]) != cols.n_rows:
        raise ValueError("`key` must have one entry per row")
    return k, k_p


def _by_key_retry(cols: "_Cols", max_groups, call):
    """
    The by-key entry points write at most `cap` groups and report the number of distinct keys.  `call(cap, keys_p, ng_p)` allocates
    the outputs for `cap` groups, makes the C call and returns (rc, outputs).  Outputs are sized for max_groups distinct keys;
    without a hint start from n_rows / 16 (at least 2^20) and repeat with the exact count when there are more -- sizing for one key
    per row would allocate p' x n_rows coefficients.  Returns (keys [g] ascending, the outputs of the call that fitted, g).
    """
    n_rows = cols.n_rows
    cap = int(max_groups) if max_groups is not None else (n_rows if n_rows <= (1 << 20) else max(1 << 20, n_rows // 16))
    ng = C.c_int64(0)
    while True:
        keys, keys_p = _out_int(cols, cap, "int64")
        rc, outs = call(cap, keys_p, C.byref(ng))
        if rc != 0 and max_groups is None and int(ng.value) > cap:
            cap = int(ng.value)  # more distinct keys than the first guess
            continue
        _lib.check(rc)
        g = int(ng.value)
        return keys[:g], outs, g


def _absorbed_call(cols: "_Cols", absorb, absorb_offsets, return_effects, max_groups, by_key, grouped):
    """
    The one-key absorbed call that may return effects, by `absorb` (a key column) or by `absorb_offsets`.
    `by_key(k_p, cap, alpha_p, keys_p, ng_p)` and `grouped(off_p, n_groups, alpha_p)` make the C call and return (rc, outputs); the
    effects' buffer and its size are chosen here: by key, room for `max_groups` groups with the retry of _by_key_retry when effects
    are wanted, else a single call with cap = n_rows; by offsets, one entry per group and effect_keys = the group indices.
    Returns (effect_keys, effects, the outputs of the call that fitted); both effects entries are None when none are wanted by key.
    """
    null = C.c_void_p(None)
    if absorb is None:
        off, off_p = _offsets_arg(cols, absorb_offsets)
        if off.ndim != 1 or int(off.shape[0]) < 2:
            raise ValueError("`absorb_offsets` must be 1-D with at least two entries")
        ng_all = int(off.shape[0]) - 1
        alpha, alpha_p = _out_like(cols, ng_all) if return_effects else (None, null)
        rc, outs = grouped(off_p, ng_all, alpha_p)
        _lib.check(rc)
        return np.arange(ng_all, dtype=np.int64), alpha, outs
    k, k_p = _key_arg(cols, absorb)

    def call(cap, keys_p, ng_p):
        alpha, alpha_p = _out_like(cols, cap) if return_effects else (None, null)
        rc, outs = by_key(k_p, cap, alpha_p, keys_p if return_effects else null, ng_p)
        return rc, (alpha, outs)

    if return_effects:
        effect_keys, (alpha, outs), g = _by_key_retry(cols, max_groups, call)
        return effect_keys, alpha[:g], outs
    ng = C.c_int64(0)
    rc, (_, outs) = call(cols.n_rows, None, C.byref(ng))
    _lib.check(rc)
    return None, None, outs


def lin_reg_by_pred(*x, target, group_offsets, add_bias: bool = False, l1_reg: float = 0.0, l2_reg: float = 0.0, tol: float = 1e-5,
                    solver: str = "qr", max_iter: int = 200, positive: bool = False, singular_x_tol: float | None = None,
                    weights=None, ctx: Context | None = None):
    """
    `df.group_by(key).agg(pds.lin_reg(..., return_pred=True))` / `pds.lin_reg(..., return_pred=True).over(key)` for contiguous
    groups (tests/test_linear_exprs.py:435-474): every group is fitted as `lin_reg_by` fits it, then one more pass writes
    pred = x . beta_group and resid = y - pred for every row.
    Returns (pred [n_rows], resid [n_rows], row_is_null [n_rows], coeffs [n_groups, p'], group_is_null [n_groups]); rows of a
    null group (gated, or fewer rows than coefficients) are NaN / flagged -- the reference returns an all-null struct there.
    """
    if max_iter <= 0:
        raise ValueError("Input `max_iter` must be a positive.")
    ctx = ctx or default_context()
    cols = _Cols(target, x, weights)
    _follow(ctx, cols)
    prm = (_params(add_bias, 0.0, 0.0, tol, solver, False, max_iter, 0.0) if weights is not None
           else _params(add_bias, l1_reg, l2_reg, tol, solver, positive, max_iter, singular_x_tol))
    pp = cols.n_feat + int(bool(add_bias))
    off, off_p = _offsets_arg(cols, group_offsets)
    ng = int(off.shape[0]) - 1
    coeffs, co_p = _out_like(cols, (ng, pp))
    nulls, nu_p = _out_u8(cols, ng)
    pred, pr_p = _out_like(cols, cols.n_rows)
    resid, re_p = _out_like(cols, cols.n_rows)
    rnull, rn_p = _out_u8(cols, cols.n_rows)
    _lib.check(ctx.fn("pds_lr_grouped_pred")(ctx._h, cols.cols, cols.weights, cols.n_feat, C.c_int64(cols.n_rows), off_p, C.c_int64(ng),
                                             cols.space, C.byref(prm), co_p, nu_p, pr_p, re_p, rn_p))
    return pred, resid, rnull, coeffs, nulls


def lin_reg_by_key_pred(*x, target, key, add_bias: bool = False, l1_reg: float = 0.0, l2_reg: float = 0.0, tol: float = 1e-5,
                        solver: str = "qr", max_iter: int = 200, positive: bool = False, singular_x_tol: float | None = None,
                        weights=None, ctx: Context | None = None):
    """
    The same for an integer key column in ANY row order: pred / resid come back in the FRAME's row order (the device orders the
    frame by key, fits, and sends every row's prediction back to where the row is).  Returns (pred, resid, row_is_null).
    """
    if max_iter <= 0:
        raise ValueError("Input `max_iter` must be a positive.")
    ctx = ctx or default_context()
    cols = _Cols(target, x, weights)
    _follow(ctx, cols)
    prm = (_params(add_bias, 0.0, 0.0, tol, solver, False, max_iter, 0.0) if weights is not None
           else _params(add_bias, l1_reg, l2_reg, tol, solver, positive, max_iter, singular_x_tol))
    n_rows = cols.n_rows
    k, k_p = _key_arg(cols, key)
    pred, pr_p = _out_like(cols, n_rows)
    resid, re_p = _out_like(cols, n_rows)
    rnull, rn_p = _out_u8(cols, n_rows)
    _lib.check(ctx.fn("pds_lr_by_key_pred")(ctx._h, cols.cols, cols.weights, k_p, cols.n_feat, C.c_int64(n_rows), cols.space,
                                            C.byref(prm), C.c_int64(n_rows), None, None, None, None, pr_p, re_p, rn_p))
    return pred, resid, rnull


def lin_reg_by_key_pred_multi(*x, target, key, contexts, n_slices: int = 0, add_bias: bool = False, l1_reg: float = 0.0, l2_reg: float = 0.0,
                              tol: float = 1e-5, solver: str = "qr", max_iter: int = 200, positive: bool = False,
                              singular_x_tol: float | None = None, weights=None):
    """
    `lin_reg_by_key_pred` for a HOST frame whose keys are in order, over several contexts of this one process
    (pds_lr_by_key_pred_multi_*): independent row slices cut at group boundaries, slice s on contexts[s mod n]; a slice's
    predictions travel back while the next slice's rows arrive.  Returns (pred, resid, row_is_null) as numpy arrays, frame order.
    """
    if max_iter <= 0:
        raise ValueError("Input `max_iter` must be a positive.")
    cols = _Cols(target, x, weights)
    if cols.space != _lib.PDS_HOST:
        raise ValueError("lin_reg_by_key_pred_multi takes host-resident columns (numpy)")
    prm = (_params(add_bias, 0.0, 0.0, tol, solver, False, max_iter, 0.0) if weights is not None
           else _params(add_bias, l1_reg, l2_reg, tol, solver, positive, max_iter, singular_x_tol))
    n_rows = cols.n_rows
    k, k_p = _key_arg(cols, key)
    pred, resid = np.empty(n_rows, dtype=_dtype()), np.empty(n_rows, dtype=_dtype())
    rnull = np.empty(n_rows, dtype=np.uint8)
    handles = (C.c_void_p * len(contexts))(*[c._h for c in contexts])
    _lib.check(contexts[0].fn("pds_lr_by_key_pred_multi")(handles, len(contexts), int(n_slices), cols.cols, cols.weights,
                                                          k_p, cols.n_feat, C.c_int64(n_rows), C.byref(prm),
                                                          C.c_void_p(pred.ctypes.data), C.c_void_p(resid.ctypes.data),
                                                          C.c_void_p(rnull.ctypes.data)))
    return pred, resid, rnull


def _windowed_outs(cols, add_bias, l2_reg):
    """coeffs [N, p'], pred [N], valid [N] in the inputs' space (+ their pointers) and the `lambda` argument of the windowed fits."""
    pp = cols.n_feat + int(bool(add_bias))
    coeffs, co_p = _out_like(cols, (cols.n_rows, pp))
    pred, pr_p = _out_like(cols, cols.n_rows)
    valid, va_p = _out_u8(cols, cols.n_rows)
    lam = C.c_double(abs(l2_reg)) if config.LIN_REG_EXPR_F64 else C.c_float(abs(l2_reg))  # `lambda`: abs(l2_reg) :546-552
    return (coeffs, pred, valid), (co_p, pr_p, va_p), lam


def _windowed(name, x, target, n, add_bias, l2_reg, min_size, ctx, seed_moments=None):
    ctx = ctx or default_context()
    cols = _Cols(target, x)
    _follow(ctx, cols)
    (coeffs, pred, valid), (co_p, pr_p, va_p), lam = _windowed_outs(cols, add_bias, l2_reg)
    if name == "pds_rolling_lr":
        _lib.check(ctx.fn(name)(ctx._h, cols.cols, cols.n_feat, C.c_int64(cols.n_rows), cols.space, int(bool(add_bias)),
                                C.c_int64(n), C.c_int64(min_size), lam, co_p, pr_p, va_p))
    elif seed_moments is not None:
        q = cols.n_feat + 2
        seed = np.asarray(seed_moments.cpu() if _is_torch(seed_moments) else seed_moments, dtype=_dtype())
        if seed.shape != (q, q):
            raise ValueError(f"seed_moments must be the ({q}, {q}) augmented moment matrix of the preceding rows")
        seed = np.asfortranarray(seed)
        _lib.check(ctx.fn("pds_recursive_lr_seeded")(ctx._h, cols.cols, cols.n_feat, C.c_int64(cols.n_rows), cols.space,
                                                     int(bool(add_bias)), C.c_int64(n), lam, C.c_void_p(seed.ctypes.data),
                                                     co_p, pr_p, va_p))
    else:
        _lib.check(ctx.fn(name)(ctx._h, cols.cols, cols.n_feat, C.c_int64(cols.n_rows), cols.space, int(bool(add_bias)),
                                C.c_int64(n), lam, co_p, pr_p, va_p))
    return coeffs, pred, valid


def rolling_lin_reg(*x, target, window_size: int, add_bias: bool = False, l2_reg: float = 0.0,
                    min_valid_rows: int | None = None, skip_non_finite: bool = False, ctx: Context | None = None):
    """
    pds.rolling_lin_reg (pl_rolling_lr).  Returns (coeffs [N, p'], pred [N], valid [N]); the first
    window_size-1 rows are invalid (null in the reference).  skip_non_finite=True selects the
    null_policy="skip" window algorithm (faer_rolling_skipping_lr) with min_valid_rows.
    """
    min_size = _check_rolling(len(x) + int(bool(add_bias)), window_size, min_valid_rows, skip_non_finite)
    return _windowed("pds_rolling_lr", x, target, window_size, add_bias, l2_reg, min_size, ctx)


def recursive_lin_reg(*x, target, start_with: int, add_bias: bool = False, l2_reg: float = 0.0, ctx: Context | None = None,
                      seed_moments=None):
    """
    pds.recursive_lin_reg (pl_recursive_lr): expanding-window fit from row start_with-1 on.
    seed_moments (the gram_moments matrix of rows that precede this frame) continues an earlier frame: the
    row-sharded multi-GPU form, see parallel.recursive_lin_reg_row_sharded.
    """
    _check_recursive(len(x) + int(bool(add_bias)), start_with)
    return _windowed("pds_recursive_lr", x, target, start_with, add_bias, l2_reg, 0, ctx, seed_moments=seed_moments)


def _check_rolling(n_features, window_size, min_valid_rows, skip_non_finite):
    if window_size < 2:
        raise ValueError("`window_size` must be >= 2.")  # expr_linear.py:524-526
    if n_features > window_size:
        raise ValueError("# features > window size. Linear regression is not well-defined.")  # :527-531
    min_size = 0
    if skip_non_finite:
        min_size = min(n_features, window_size) if min_valid_rows is None else int(min_valid_rows)  # :535-543
        if min_size < n_features or min_size > window_size:
            raise ValueError("`min_valid_rows` must be in [#features, window_size].")
    return min_size


def _check_recursive(n_features, start_with):
    if start_with < n_features:
        raise ValueError("# features > number of rows for the initial fit.")  # expr_linear.py:455-459


def _windowed_grouped(kind, form, x, target, groups, n, add_bias, l2_reg, min_size, ctx):
    """pds_{rolling,recursive}_lr_{grouped,by_key}_*: per-row outputs in frame order (coeffs [N, p'], pred [N], valid [N])."""
    ctx = ctx or default_context()
    cols = _Cols(target, x)
    _follow(ctx, cols)
    (coeffs, pred, valid), (co_p, pr_p, va_p), lam = _windowed_outs(cols, add_bias, l2_reg)
    g, g_p = _offsets_arg(cols, groups)  # (int64, in the inputs' space: offsets or keys)
    if form == "grouped":
        if g.ndim != 1 or g.shape[0] < 2:
            raise ValueError("group_offsets must hold n_groups + 1 >= 2 offsets")
        lead = (ctx._h, cols.cols, cols.n_feat, C.c_int64(cols.n_rows), g_p, C.c_int64(int(g.shape[0]) - 1), cols.space)
    else:
        if g.ndim != 1 or int(g.shape[0]) != cols.n_rows:
            raise ValueError("key must hold one value per row")
        lead = (ctx._h, cols.cols, g_p, cols.n_feat, C.c_int64(cols.n_rows), cols.space)
    wargs = (C.c_int64(n), C.c_int64(min_size)) if kind == "rolling" else (C.c_int64(n),)
    _lib.check(ctx.fn(f"pds_{kind}_lr_{form}")(*lead, int(bool(add_bias)), *wargs, lam, co_p, pr_p, va_p))
    return coeffs, pred, valid


def rolling_lin_reg_by(*x, target, group_offsets, window_size: int, add_bias: bool = False, l2_reg: float = 0.0,
                       min_valid_rows: int | None = None, skip_non_finite: bool = False, ctx: Context | None = None):
    """
    rolling_lin_reg on every group of contiguous rows (group g = rows [group_offsets[g], group_offsets[g+1])) in one call:
    what `pds.rolling_lin_reg(...).over(group)` gives.  Row r of group g is fitted on rows [max(s_g, r - w + 1), r] and is
    valid iff r - s_g >= w - 1.  Returns (coeffs [N, p'], pred [N], valid [N]) in frame order, on the inputs' device.
    """
    min_size = _check_rolling(len(x) + int(bool(add_bias)), window_size, min_valid_rows, skip_non_finite)
    return _windowed_grouped("rolling", "grouped", x, target, group_offsets, window_size, add_bias, l2_reg, min_size, ctx)


def rolling_lin_reg_by_key(*x, target, key, window_size: int, add_bias: bool = False, l2_reg: float = 0.0,
                           min_valid_rows: int | None = None, skip_non_finite: bool = False, ctx: Context | None = None):
    """rolling_lin_reg_by with int64 keys in any row order (rows of equal key form a group, in frame order)."""
    min_size = _check_rolling(len(x) + int(bool(add_bias)), window_size, min_valid_rows, skip_non_finite)
    return _windowed_grouped("rolling", "by_key", x, target, key, window_size, add_bias, l2_reg, min_size, ctx)


def recursive_lin_reg_by(*x, target, group_offsets, start_with: int, add_bias: bool = False, l2_reg: float = 0.0,
                         ctx: Context | None = None):
    """
    recursive_lin_reg on every group of contiguous rows in one call (`pds.recursive_lin_reg(...).over(group)`): row r of
    group g is fitted on rows [s_g, r] and is valid iff r - s_g >= start_with - 1.
    """
    _check_recursive(len(x) + int(bool(add_bias)), start_with)
    return _windowed_grouped("recursive", "grouped", x, target, group_offsets, start_with, add_bias, l2_reg, 0, ctx)


def recursive_lin_reg_by_key(*x, target, key, start_with: int, add_bias: bool = False, l2_reg: float = 0.0,
                             ctx: Context | None = None):
    """recursive_lin_reg_by with int64 keys in any row order."""
    _check_recursive(len(x) + int(bool(add_bias)), start_with)
    return _windowed_grouped("recursive", "by_key", x, target, key, start_with, add_bias, l2_reg, 0, ctx)


def gram_moments(*x, target, weights=None, ctx: Context | None = None, out_device: bool = False):
    """The augmented moment matrix A = Z'Z, Z = [x1..xp | 1 | y] ((p+2)^2), the measured Gram build."""
    ctx = ctx or default_context()
    cols = _Cols(target, x, weights)
    _follow(ctx, cols)
    q = cols.n_feat + 2
    if out_device:
        if cols.space != _lib.PDS_DEVICE:
            raise ValueError("out_device requires device-resident inputs")
        out, out_p = _out_like(cols, (q, q))
        _lib.check(ctx.fn("pds_moments")(ctx._h, cols.cols, cols.weights, cols.n_feat, C.c_int64(cols.n_rows), cols.space,
                                         out_p, _lib.PDS_DEVICE))
        return out.t()  # column-major -> logical (symmetric anyway)
    out = np.empty((q, q), dtype=_dtype())
    _lib.check(ctx.fn("pds_moments")(ctx._h, cols.cols, cols.weights, cols.n_feat, C.c_int64(cols.n_rows), cols.space,
                                     C.c_void_p(out.ctypes.data), _lib.PDS_HOST))
    return out.T


def lin_reg_from_moments(moments, *, add_bias: bool = False, l1_reg: float = 0.0, l2_reg: float = 0.0, tol: float = 1e-5,
                         solver: str = "qr", max_iter: int = 200, positive: bool = False,
                         singular_x_tol: float | None = None, ctx: Context | None = None):
    """Solve from an (all-reduced) moment matrix: the replicated tail of the multi-GPU single-OLS path."""
    ctx = ctx or default_context()
    prm = _params(add_bias, l1_reg, l2_reg, tol, solver, positive, max_iter, singular_x_tol)
    if _is_torch(moments):
        import torch

        tdt = torch.float64 if config.LIN_REG_EXPR_F64 else torch.float32
        m = moments.to(tdt).t().contiguous() if moments.is_cuda else None
        if m is None:
            moments = moments.numpy()
    if _is_torch(moments):
        q = int(m.shape[0])
        mp, space = C.c_void_p(int(m.data_ptr())), _lib.PDS_DEVICE
    else:
        m = np.asfortranarray(np.asarray(moments, dtype=_dtype()))
        q = int(m.shape[0])
        mp, space = C.c_void_p(m.ctypes.data), _lib.PDS_HOST
    p = q - 2
    pp = p + int(bool(add_bias))
    coeffs = np.empty(pp, dtype=_dtype())
    is_null = C.c_int(0)
    _lib.check(ctx.fn("pds_lr_from_moments")(ctx._h, mp, space, p, C.byref(prm), C.c_void_p(coeffs.ctypes.data),
                                             C.byref(is_null)))
    return None if is_null.value else coeffs


# ---------------------------------------------------------------------------------------------
# GLM per group (IRLS) and logistic_reg
# ---------------------------------------------------------------------------------------------
def _glm_family(family):
    from .linear_models import GLM_FAMILIES  # (linear_models imports this module)

    if family not in GLM_FAMILIES:
        raise NotImplementedError(f"GLM family {family!r}: one of {sorted(GLM_FAMILIES)}")  # as GLM.__init__
    return GLM_FAMILIES[family]


def _glm_check(x, max_iter, what):
    if max_iter < 1:
        raise ValueError("`max_iter` must be > 1.")  # GLM.__init__ (linear_models.py:756-757 of the reference)
    if len(x) < 1:
        raise ValueError(f"{what}: need at least one feature column")
    if len(x) > 16:
        raise NotImplementedError("grouped GLM (IRLS): up to 16 feature columns")


def _out_i32(cols: _Cols, n):
    return _out_int(cols, n, "int32")


def _tol_arg(tol):
    return C.c_double(abs(float(tol))) if config.LIN_REG_EXPR_F64 else C.c_float(abs(float(tol)))


def _pen_args(l1_reg, l2_reg):
    """() for an unpenalised fit (a penalty <= 0 means none, as in the reference), else the two arguments the `pds_glm_enet_*` entry
    points take after `variance`."""
    l1, l2 = max(float(l1_reg), 0.0), max(float(l2_reg), 0.0)
    if l1 == 0.0 and l2 == 0.0:
        return ()
    ct = C.c_double if config.LIN_REG_EXPR_F64 else C.c_float
    return (ct(l1), ct(l2))


def _glm_wo_cols(what, x, target, weights, offset, pen):
    """The frame of a GLM call with a prior-weight and / or an offset column: (cols, weights pointer, offset pointer).  The two
    columns are cast and placed like the frame's own (`_Cols`) and must have one entry per row; together with a penalty they are
    refused before a device is touched."""
    extra = [c for c in (weights, offset) if c is not None]
    if extra and pen:
        raise NotImplementedError(f"{what}: l1_reg / l2_reg together with weights= / offset= is not built")
    n = int(target.shape[0]) if hasattr(target, "shape") else len(target)
    for name, c in (("weights", weights), ("offset", offset)):
        if c is not None and (int(c.shape[0]) if hasattr(c, "shape") else len(c)) != n:
            raise ValueError(f"`{name}` must have one entry per row")
    cols = _Cols(target, x)
    if not extra:
        return cols, C.c_void_p(None), C.c_void_p(None)
    # the two columns: cast and placed like the frame's (a second _Cols whose "target" is the frame's, so that a device frame pulls
    # host columns onto the device and the reverse never happens), kept alive with it
    side = _Cols(cols.keep[0], extra)
    if side.space != cols.space:
        raise ValueError(f"{what}: weights / offset must live where the frame lives")
    cols.keep.extend(side.keep[1:])
    ptrs = [C.c_void_p(side.cols[1 + k]) for k in range(len(extra))]
    w_p = ptrs.pop(0) if weights is not None else C.c_void_p(None)
    o_p = ptrs.pop(0) if offset is not None else C.c_void_p(None)
    return cols, w_p, o_p


def glm_by(*x, target, group_offsets, family: str = "gaussian", add_bias: bool = False, tol: float = 1e-8, max_iter: int = 100,
           return_pred: bool = False, ctx: Context | None = None, l1_reg: float = 0.0, l2_reg: float = 0.0, weights=None, offset=None):
    """
    One GLM per group in one call: for every group g = rows [group_offsets[g], group_offsets[g+1]) what `GLM(family=...).fit` computes
    on g's rows alone (iteratively re-weighted least squares, the reference's faer_irls), every iteration of a group on chip
    (`pds_glm_irls_grouped_*`).  Families as `linear_models.GLM_FAMILIES`; 1 .. 16 feature columns.
    Returns (coeffs [G, p'] bias last, n_iter [G] int32, is_null [G]) in the memory space of the inputs, plus (pred [n_rows],
    row_null [n_rows]) with `return_pred`: the fitted mean g^-1(x . beta_group) of every row.  A group with fewer rows than
    coefficients, or whose fit does not end in finite coefficients (a separated binomial group, NaN / inf in its rows), is null:
    is_null = 1 (NaN pred, row_null = 1).
    `l1_reg` / `l2_reg` > 0 (`pds_glm_enet_grouped_*`): every group minimises
    (1/n) sum_i loss(y_i, eta_i) + (l2_reg / 2) sum_j beta_j^2 + l1_reg sum_j |beta_j| over its n rows, the loss being the family's
    unit-dispersion negative log-likelihood and the sums over j running over the features, never the bias.  Same iteration, each step
    the penalised weighted least squares problem (ridge: one solve; l1: coordinate descent in the wave, exact zeros).  A ridge term
    gives a separated binomial group a finite fit.
    `weights` / `offset` (one entry per row each, either alone or both; `pds_glm_irls_wo_grouped_*`): prior weights pw and an offset
    o per row, R's `glm(weights=, offset=)` -- eta = x . beta + o, working weight pw / (g'(mu)^2 V(mu)), start from the weighted mean
    of y.  A row of weight 0 contributes nothing and does not count as a row (its target may hold anything, its features and offset must be
    finite: they give the row's `pred`): a group with fewer rows of positive weight than
    coefficients, or with a weight that is negative or not finite, is null.  `pred` is g^-1(x . beta_group + o), rows of weight 0
    included.  Not together with `l1_reg` / `l2_reg` (NotImplementedError).  Without the two the call is the one it was.  Groups above the
    context option "glm_split_rows" take the full-device iteration (`pds_glm_irls_wo_*`) on their rows of the two columns.
    """
    _glm_check(x, max_iter, "glm_by")
    link, var = _glm_family(family)
    pen = _pen_args(l1_reg, l2_reg)
    wo = weights is not None or offset is not None
    cols, w_p, o_p = _glm_wo_cols("glm_by", x, target, weights, offset, pen)
    ctx = ctx or default_context()
    _follow(ctx, cols)
    pp = cols.n_feat + int(bool(add_bias))
    off, off_p = _offsets_arg(cols, group_offsets)
    ng = int(off.shape[0]) - 1
    coeffs, co_p = _out_like(cols, (ng, pp))
    iters, it_p = _out_i32(cols, ng)
    nulls, nu_p = _out_u8(cols, ng)
    pred = rnull = None
    pr_p = rn_p = None
    if return_pred:
        pred, pr_p = _out_like(cols, cols.n_rows)
        rnull, rn_p = _out_u8(cols, cols.n_rows)
    fn = ctx.fn("pds_glm_irls_wo_grouped" if wo else ("pds_glm_enet_grouped" if pen else "pds_glm_irls_grouped"))
    _lib.check(fn(ctx._h, cols.cols, *((w_p, o_p) if wo else ()), cols.n_feat, C.c_int64(cols.n_rows), off_p, C.c_int64(ng), cols.space,
                  int(bool(add_bias)), C.c_int(link), C.c_int(var), *pen, _tol_arg(tol), C.c_int(int(max_iter)), co_p, it_p, nu_p, pr_p,
                  rn_p))
    if return_pred:
        return coeffs, iters, nulls, pred, rnull
    return coeffs, iters, nulls


def glm_by_key(*x, target, key, family: str = "gaussian", add_bias: bool = False, tol: float = 1e-8, max_iter: int = 100,
               return_pred: bool = False, max_groups: int | None = None, ctx: Context | None = None, l1_reg: float = 0.0,
               l2_reg: float = 0.0, weights=None, offset=None):
    """
    `glm_by` for an integer key column in ANY row order (`pds_glm_irls_by_key_*`): the frame is brought into key order on the device
    (nothing moves when the keys are already non-decreasing), every group is fitted, per-row means come back at the rows' own
    positions.  Returns (keys [G] ascending, coeffs, n_iter, is_null), plus (pred, row_null) with `return_pred`.
    `l1_reg` / `l2_reg` > 0: the penalised fits of `glm_by` (`pds_glm_enet_by_key_*`).
    `weights` / `offset`: as in `glm_by` (`pds_glm_irls_wo_by_key_*`); the two columns travel with the frame into key order.
    """
    _glm_check(x, max_iter, "glm_by_key")
    link, var = _glm_family(family)
    pen = _pen_args(l1_reg, l2_reg)
    wo = weights is not None or offset is not None
    cols, w_p, o_p = _glm_wo_cols("glm_by_key", x, target, weights, offset, pen)
    ctx = ctx or default_context()
    _follow(ctx, cols)
    pp = cols.n_feat + int(bool(add_bias))
    n_rows = cols.n_rows
    k, k_p = _key_arg(cols, key)
    pred = rnull = None
    pr_p = rn_p = None
    if return_pred:
        pred, pr_p = _out_like(cols, n_rows)
        rnull, rn_p = _out_u8(cols, n_rows)

    def call(cap, ok_p, ng_p):
        coeffs, co_p = _out_like(cols, (cap, pp))
        iters, it_p = _out_i32(cols, cap)
        nulls, nu_p = _out_u8(cols, cap)
        fn = ctx.fn("pds_glm_irls_wo_by_key" if wo else ("pds_glm_enet_by_key" if pen else "pds_glm_irls_by_key"))
        rc = fn(ctx._h, cols.cols, *((w_p, o_p) if wo else ()), k_p, cols.n_feat, C.c_int64(n_rows), cols.space, int(bool(add_bias)),
                C.c_int(link), C.c_int(var), *pen, _tol_arg(tol), C.c_int(int(max_iter)), C.c_int64(cap), ok_p, co_p, it_p, nu_p, ng_p,
                pr_p, rn_p)
        return rc, (coeffs, iters, nulls)

    keys, (coeffs, iters, nulls), g = _by_key_retry(cols, max_groups, call)
    if return_pred:
        return keys, coeffs[:g], iters[:g], nulls[:g], pred, rnull
    return keys, coeffs[:g], iters[:g], nulls[:g]


_GLM_REPORT_COEF = ("std_err", "z", "p", "ci_lower", "ci_upper")
_GLM_REPORT_GROUP = ("deviance", "null_deviance", "pearson_chi2", "dispersion")


def _glm_report_outs(cols: _Cols, ng: int, pp: int, return_cov: bool):
    outs = {"beta": _out_like(cols, (ng, pp)), "n_iter": _out_i32(cols, ng), "is_null": _out_u8(cols, ng)}
    for k in _GLM_REPORT_COEF:
        outs[k] = _out_like(cols, (ng, pp))
    outs["cov"] = _out_like(cols, (ng, pp, pp)) if return_cov else (None, C.c_void_p(None))
    for k in _GLM_REPORT_GROUP:
        outs[k] = _out_like(cols, (ng,))
    outs["df_resid"] = _out_int(cols, ng, "int64")
    outs["report_null"] = _out_u8(cols, ng)
    rep = _lib.GlmReportOut(*[outs[k][1] for k in (*_GLM_REPORT_COEF, "cov", *_GLM_REPORT_GROUP, "df_resid", "report_null")])
    return outs, rep


def _glm_report_dict(outs, n_feat, add_bias, feature_names, return_cov, g=None):
    names = list(feature_names) if feature_names is not None else [f"x{i + 1}" for i in range(n_feat)]
    if add_bias:
        names.append("__bias__")
    cut = (lambda a: a[:g]) if g is not None else (lambda a: a)
    d = {"features": names, "beta": cut(outs["beta"][0]), "std_err": cut(outs["std_err"][0]), "z": cut(outs["z"][0]),
         "p>|z|": cut(outs["p"][0]), "0.025": cut(outs["ci_lower"][0]), "0.975": cut(outs["ci_upper"][0])}
    for k in (*_GLM_REPORT_GROUP, "df_resid", "n_iter", "is_null", "report_null"):
        d[k] = cut(outs[k][0])
    if return_cov:
        d["cov"] = cut(outs["cov"][0])
    return d


def _glm_report_check(x, max_iter, what, penalties):
    _glm_check(x, max_iter, what)
    if any(float(v) > 0.0 for v in penalties):
        raise NotImplementedError(f"{what}: penalised fits have no report")


def glm_report_by(*x, target, group_offsets, family: str = "gaussian", add_bias: bool = False, tol: float = 1e-8, max_iter: int = 100,
                  feature_names: Sequence[str] | None = None, return_cov: bool = False, ctx: Context | None = None, l1_reg: float = 0.0,
                  l2_reg: float = 0.0, weights=None, offset=None) -> dict:
    """
    The fit of `glm_by` and its report per group in one call (`pds_glm_report_grouped_*`): the GLM twin of `lin_reg_report_by`.
    "beta", "n_iter" and "is_null" are bit for bit what `glm_by` returns on the same frame; the report is formed on the device at
    those coefficients (for an f32 frame: the f32 values), in the unscaled convention of statsmodels' `GLM`: with mu = g^-1(x . beta),
    w = 1 / (g'(mu)^2 V(mu)) and I = sum w x x', cov = dispersion * I^-1, std_err = sqrt(diag cov), z = beta / std_err,
    p = erfc(|z| / sqrt 2) and the interval beta -+ 1.959963984540054 std_err -- the NORMAL distribution for every family
    (statsmodels' `use_t=False`), never Student's t.  dispersion is 1 for poisson / binomial and pearson_chi2 / df_resid for
    gaussian / gamma (NaN when df_resid = n - p' is 0, and the standard errors with it); deviance and null_deviance (the deviance at
    the group's mean with a bias, at g^-1(0) without: NaN for gamma) are the families' unit deviances summed over the group.
    Returns a dict in the memory space of the inputs: "beta", "std_err", "z", "p>|z|", "0.025", "0.975" [G, p'] (bias last);
    "deviance", "null_deviance", "pearson_chi2", "dispersion", "df_resid" (int64), "n_iter", "is_null", "report_null" [G];
    "features"; "cov" [G, p', p'] with `return_cov`.  report_null = 1 for a null fit and for a group whose I has no positive
    finite pivots (an all-zero column): its report fields are NaN, its coefficients stay what the fit returned.
    Penalised fits have no report: `l1_reg` / `l2_reg` > 0 raise NotImplementedError.
    `weights` / `offset` (`pds_glm_report_wo_grouped_*`): the fit of `glm_by(weights=, offset=)` and its report with prior weights pw
    and an offset o: mu = g^-1(x . beta + o), I = sum pw w x x', pearson_chi2 = sum pw (y - mu)^2 / V, deviance = sum pw d_i,
    df_resid = n+ - p' (n+: the rows of positive weight); null_deviance is the closed form with weighted sums, and NaN whenever an
    offset is given (the intercept-only model under an offset needs an iteration of its own).
    """
    _glm_report_check(x, max_iter, "glm_report_by", (l1_reg, l2_reg))
    link, var = _glm_family(family)
    wo = weights is not None or offset is not None
    cols, w_p, o_p = _glm_wo_cols("glm_report_by", x, target, weights, offset, ())
    ctx = ctx or default_context()
    _follow(ctx, cols)
    pp = cols.n_feat + int(bool(add_bias))
    off, off_p = _offsets_arg(cols, group_offsets)
    ng = int(off.shape[0]) - 1
    outs, rep = _glm_report_outs(cols, ng, pp, return_cov)
    fn = ctx.fn("pds_glm_report_wo_grouped" if wo else "pds_glm_report_grouped")
    _lib.check(fn(ctx._h, cols.cols, *((w_p, o_p) if wo else ()), cols.n_feat, C.c_int64(cols.n_rows), off_p, C.c_int64(ng), cols.space,
                  int(bool(add_bias)), C.c_int(link), C.c_int(var), _tol_arg(tol), C.c_int(int(max_iter)), outs["beta"][1],
                  outs["n_iter"][1], outs["is_null"][1], C.byref(rep)))
    return _glm_report_dict(outs, cols.n_feat, add_bias, feature_names, return_cov)


def glm_report_by_key(*x, target, key, family: str = "gaussian", add_bias: bool = False, tol: float = 1e-8, max_iter: int = 100,
                      feature_names: Sequence[str] | None = None, return_cov: bool = False, max_groups: int | None = None,
                      ctx: Context | None = None, l1_reg: float = 0.0, l2_reg: float = 0.0, weights=None, offset=None) -> dict:
    """
    `glm_report_by` for an integer key column in ANY row order (`pds_glm_report_by_key_*`): the frame is brought into key order on the
    device as `glm_by_key` does (nothing moves when the keys are already non-decreasing) and reported where it lies.  Returns the
    dict of `glm_report_by` plus "keys" (ascending).  The normal distribution is used for every family.
    `weights` / `offset`: as in `glm_report_by` (`pds_glm_report_wo_by_key_*`); the two columns travel with the frame into key order.
    """
    _glm_report_check(x, max_iter, "glm_report_by_key", (l1_reg, l2_reg))
    link, var = _glm_family(family)
    wo = weights is not None or offset is not None
    cols, w_p, o_p = _glm_wo_cols("glm_report_by_key", x, target, weights, offset, ())
    ctx = ctx or default_context()
    _follow(ctx, cols)
    pp = cols.n_feat + int(bool(add_bias))
    n_rows = cols.n_rows
    k, k_p = _key_arg(cols, key)

    def call(cap, ok_p, ng_p):
        outs, rep = _glm_report_outs(cols, cap, pp, return_cov)
        fn = ctx.fn("pds_glm_report_wo_by_key" if wo else "pds_glm_report_by_key")
        rc = fn(ctx._h, cols.cols, *((w_p, o_p) if wo else ()), k_p, cols.n_feat, C.c_int64(n_rows), cols.space, int(bool(add_bias)),
                C.c_int(link), C.c_int(var), _tol_arg(tol), C.c_int(int(max_iter)), C.c_int64(cap), ok_p, outs["beta"][1],
                outs["n_iter"][1], outs["is_null"][1], ng_p, C.byref(rep))
        return rc, outs

    keys, outs, g = _by_key_retry(cols, max_groups, call)
    d = _glm_report_dict(outs, cols.n_feat, add_bias, feature_names, return_cov, g)
    d["keys"] = keys
    return d


GLM_STD_ERR_TYPES = ("se", "hc0", "hc1", "cluster", "cluster0")


def _glm_std_err_check(what, std_err, cluster, cluster_offsets):
    """The argument rules of the robust GLM reports: which `std_err` exist, and that the clusters come with the cluster kinds alone."""
    if std_err in ("hc2", "hc3"):
        raise NotImplementedError(f'{what}: std_err="{std_err}" needs the leverages and is not built (one of {GLM_STD_ERR_TYPES})')
    if std_err not in GLM_STD_ERR_TYPES:
        raise ValueError(f"{what}: std_err={std_err!r} is not one of {GLM_STD_ERR_TYPES}")
    if std_err in _lib.CLUSTER_SE_TYPES:
        if (cluster is None) == (cluster_offsets is None):
            raise ValueError(f'{what}: std_err="{std_err}" takes exactly one of `cluster` and `cluster_offsets`')
    elif cluster is not None or cluster_offsets is not None:
        raise ValueError(f'{what}: `cluster` / `cluster_offsets` go with std_err="cluster" or "cluster0" only')


def glm_report(*x, target, family: str = "gaussian", add_bias: bool = False, tol: float = 1e-8, max_iter: int = 100, std_err: str = "se",
               cluster=None, cluster_offsets=None, weights=None, offset=None, return_cov: bool = False,
               feature_names: Sequence[str] | None = None, ctx: Context | None = None, absorb=None, absorb_offsets=None,
               return_effects: bool = False, return_pred: bool = False, max_groups: int | None = None) -> dict:
    """
    ONE GLM over the whole frame and its report: the one-model twin of `glm_report_by`.  Returns the dict of `glm_report_by` un-batched
    ("beta", "std_err", "z", "p>|z|", "0.025", "0.975" [p'] bias last; "deviance", "null_deviance", "pearson_chi2", "dispersion",
    "df_resid", "n_iter", "report_null" scalars; "features"; "cov" [p', p'] with `return_cov`) plus "n_clusters" and
    "std_err_type".  "is_null", the fit's own flag, comes with "se" only: the robust entry points return one flag, "report_null" (1
    for a null fit, an I without an inverse or a V with a bad diagonal: the report fields are then NaN, "beta" is what the fit gave).  The normal distribution is used for every family; "n_clusters" is there for a caller who wants t(G - 1).
    `std_err`:
      "se"        model-based errors, cov = dispersion I^-1: `glm_report_by` with the one group [0, n).
      "hc0"       robust: V = I^-1 M I^-1, M = sum_i r_i^2 x_i x_i', r_i = pw_i (y_i - mu_i) / (V(mu_i) g'(mu_i)) the score residual
      "hc1"       the same times n / (n - p') (n: the rows of positive weight)
      "cluster0"  cluster-robust: M = sum_g s_g s_g', s_g = sum_{i in g} r_i x_i
      "cluster"   the same times G / (G - 1) * (n - 1) / (n - p'), statsmodels' default (G: the clusters with a row of positive weight)
    (`pds_glm_report_robust_*` / `pds_glm_report_cluster_grouped_*` / `pds_glm_report_cluster_by_key_*`; include/pds_lstsq.h states
    the definitions).  The dispersion cancels in the sandwich.  The clusters are `cluster`, an integer column in any row order, or
    `cluster_offsets` (cluster g = rows [cluster_offsets[g], cluster_offsets[g+1]), contiguous, empty clusters allowed) -- exactly one
    of the two with the cluster kinds, neither with any other (ValueError).  "hc2" / "hc3" raise NotImplementedError.  The fit, the
    deviances, the dispersion and df_resid are bit for bit those of `glm_report_by(group_offsets=[0, n])` on the same frame.
    1 .. 16 features, `weights` / `offset` as in `glm_by`, no penalties.

    `absorb=key` (an integer column in any row order, NumPy or CUDA) or `absorb_offsets=off` (group g = rows [off[g], off[g+1]),
    contiguous): the FIXED-EFFECTS GLM, g(E y) = alpha_group + x . beta + o with one intercept per group absorbed -- a PPML gravity
    model with pair effects, a logit over a firm panel -- fitted by IRLS in which every step is a weighted within regression
    (`pds_glm_within_by_key_*` / `_grouped_*`; include/pds_lstsq.h states the definitions: what is dropped, the start, the stopping
    rule, the report).  `add_bias=True` is a ValueError (the intercept is absorbed).  `std_err` is "se" (cov = dispersion W_xx^-1),
    "cluster" or "cluster0" -- the clusters ARE the absorbed groups, so `cluster` / `cluster_offsets` are a ValueError; "hc0" .. "hc3"
    raise NotImplementedError.  A group without a row of positive weight, a poisson group whose counting y are all 0 and a binomial
    group whose counting y are all 0 or all 1 are dropped with their rows.  The dict holds the report fields above ("null_deviance" is
    NaN, "report_null" 0, "n_clusters" the kept groups with the cluster kinds) plus "n_groups" (kept), "n_groups_dropped",
    "n_rows_used", "df_resid" = n_rows_used - n_groups - p, "n_iter", "converged"; return_effects=True adds "effects" (alpha per group,
    NaN for a dropped or empty group) and "effect_keys" (the distinct keys ascending; group indices with `absorb_offsets`),
    return_pred=True adds "pred" (mu per row in frame order, NaN on the rows of dropped groups).  Refused: two absorbed keys, a
    cluster key other than the absorbed one, penalties, more than 16 features.  Without `absorb` / `absorb_offsets` nothing changes.
    """
    if absorb is not None or absorb_offsets is not None:
        return _glm_within(x, target, family, add_bias, tol, max_iter, std_err, cluster, cluster_offsets, weights, offset, return_cov,
                           feature_names, ctx, absorb, absorb_offsets, return_effects, return_pred, max_groups)
    if return_effects or return_pred:
        raise ValueError("`return_effects` / `return_pred` go with `absorb` or `absorb_offsets` only")
    _glm_std_err_check("glm_report", std_err, cluster, cluster_offsets)
    _glm_check(x, max_iter, "glm_report")
    if std_err == "se":
        n = int(target.shape[0]) if hasattr(target, "shape") else len(target)
        d = glm_report_by(*x, target=target, group_offsets=np.array([0, n], dtype=np.int64), family=family, add_bias=add_bias, tol=tol,
                          max_iter=max_iter, feature_names=feature_names, return_cov=return_cov, ctx=ctx, weights=weights, offset=offset)
        d = {k: (v if k == "features" else v[0]) for k, v in d.items()}
        d["n_clusters"] = 0
        d["std_err_type"] = std_err
        return d
    link, var = _glm_family(family)
    cols, w_p, o_p = _glm_wo_cols("glm_report", x, target, weights, offset, ())
    ctx = ctx or default_context()
    _follow(ctx, cols)
    pp = cols.n_feat + int(bool(add_bias))
    outs, rep = _glm_report_outs(cols, 1, pp, return_cov)
    se_code = C.c_int(_lib.GLM_ROBUST_SE_TYPES[std_err])
    ng = C.c_int64(0)
    head = (ctx._h, cols.cols, w_p, o_p)
    tail = (cols.space, int(bool(add_bias)), C.c_int(link), C.c_int(var), _tol_arg(tol), C.c_int(int(max_iter)), se_code, outs["beta"][1],
            outs["n_iter"][1], C.byref(rep), C.byref(ng))
    if cluster is not None:
        k, k_p = _key_arg(cols, cluster)
        _lib.check(ctx.fn("pds_glm_report_cluster_by_key")(*head, k_p, cols.n_feat, C.c_int64(cols.n_rows), *tail))
    elif cluster_offsets is not None:
        off, off_p = _offsets_arg(cols, cluster_offsets)
        if off.ndim != 1 or int(off.shape[0]) < 2:
            raise ValueError("`cluster_offsets` must be 1-D with at least two entries")
        _lib.check(ctx.fn("pds_glm_report_cluster_grouped")(*head, cols.n_feat, C.c_int64(cols.n_rows), off_p, C.c_int64(int(off.shape[0]) - 1),
                                                            *tail))
    else:
        _lib.check(ctx.fn("pds_glm_report_robust")(*head, cols.n_feat, C.c_int64(cols.n_rows), *tail))
    d = _glm_report_dict(outs, cols.n_feat, add_bias, feature_names, return_cov)
    d = {k: (v if k == "features" else v[0]) for k, v in d.items() if k != "is_null"}  # (the entry points return one flag: report_null)
    d["n_clusters"] = int(ng.value)
    d["std_err_type"] = std_err
    return d


def _glm_within(x, target, family, add_bias, tol, max_iter, std_err, cluster, cluster_offsets, weights, offset, return_cov, feature_names,
                ctx, absorb, absorb_offsets, return_effects, return_pred, max_groups):
    """glm_report(absorb= | absorb_offsets=): pds_glm_within_by_key_* / _grouped_*.  The report fields are host arrays of the
    frame's type; "effects" and "pred" live where the inputs live."""
    if isinstance(absorb, (list, tuple)):
        raise NotImplementedError("fixed-effects GLM: two or more absorbed keys are not implemented (`absorb` is one integer column)")
    if (absorb is None) == (absorb_offsets is None):
        raise ValueError("exactly one of `absorb` and `absorb_offsets` must be given")
    if add_bias:
        raise ValueError("`add_bias=True` together with `absorb`: the intercept is absorbed by the group effects")
    if cluster is not None or cluster_offsets is not None:
        raise ValueError('`cluster` / `cluster_offsets` together with `absorb`: std_err="cluster" means the absorbed key')
    if std_err in _lib.SE_TYPES and std_err != "se":
        raise NotImplementedError(f'fixed-effects GLM: std_err="{std_err}" is not available with absorption ("se", "cluster", "cluster0")')
    if std_err not in _lib.WITHIN_SE_TYPES:
        raise ValueError('`absorb`: std_err is "se", "cluster" or "cluster0"')
    if len(x) < 1:
        raise ValueError("glm_report: need at least one feature column")
    if max_iter < 1:
        raise ValueError("`max_iter` must be > 1.")
    link, var = _glm_family(family)
    if any(_is_arrow(c) for c in (target, *x)) or (absorb is not None and _is_arrow(absorb)):
        raise NotImplementedError("fixed-effects GLM: pyarrow columns are not supported (NumPy arrays or CUDA tensors)")
    if absorb is not None and not _is_int_column(absorb):
        raise ValueError("an absorbed key must be an integer column")
    cols, w_p, o_p = _glm_wo_cols("glm_report", x, target, weights, offset, ())
    ctx = ctx or default_context()
    _follow(ctx, cols)
    p, n, dt = cols.n_feat, cols.n_rows, _dtype()
    se_code = C.c_int(_lib.WITHIN_SE_TYPES[std_err])
    pred, pred_p = _out_like(cols, n) if return_pred else (None, C.c_void_p(None))
    tail = (C.c_int(link), C.c_int(var), _tol_arg(tol), C.c_int(int(max_iter)), se_code)

    def by_key(k_p, cap, alpha_p, keys_p, ng_p):
        rep = _lib.GlmWithinOut()
        rep.alpha, rep.pred = alpha_p, pred_p
        return ctx.fn("pds_glm_within_by_key")(ctx._h, cols.cols, w_p, o_p, k_p, p, C.c_int64(n), cols.space, *tail, C.c_int64(cap), keys_p,
                                               C.byref(rep), ng_p), rep

    def grouped(off_p, ng_all, alpha_p):
        rep = _lib.GlmWithinOut()
        rep.alpha, rep.pred = alpha_p, pred_p
        return ctx.fn("pds_glm_within_grouped")(ctx._h, cols.cols, w_p, o_p, p, C.c_int64(n), off_p, C.c_int64(ng_all), cols.space, *tail,
                                                C.byref(rep)), rep

    effect_keys, alpha, rep = _absorbed_call(cols, absorb, absorb_offsets, return_effects, max_groups, by_key, grouped)
    names =list(feature_names) if feature_names is not None else [f"x{i + 1}" for i in range(p)]
    vec = lambda field: np.array(field[:p], dtype=np.float64).astype(dt)  # noqa: E731
    d = {"features": names, "beta": vec(rep.beta), "std_err": vec(rep.std_err), "z": vec(rep.z), "p>|z|": vec(rep.p), "0.025": vec(rep.ci_lower),
         "0.975": vec(rep.ci_upper), "deviance": dt(rep.deviance), "null_deviance": dt(np.nan), "pearson_chi2": dt(rep.pearson_chi2),
         "dispersion": dt(rep.dispersion), "df_resid": int(rep.df_resid), "n_iter": int(rep.n_iter), "report_null": 0,
         "converged": bool(rep.converged), "n_groups": int(rep.n_groups_used), "n_groups_dropped": int(rep.n_groups_dropped),
         "n_rows_used": int(rep.n_rows_used), "n_clusters": int(rep.n_groups_used) if std_err != "se" else 0, "std_err_type": std_err}
    if return_cov:
        d["cov"] = np.array(rep.cov[:p * p], dtype=np.float64).reshape(p, p).astype(dt)
    if return_effects:
        d["effects"], d["effect_keys"] = alpha, effect_keys
    if return_pred:
        d["pred"] = pred
    return d


def logistic_reg(*x, target, add_bias: bool = True, l1_reg: float = 0.0, l2_reg: float = 0.0, tol: float = 1e-5, max_iter: int = 200,
                 return_pred: bool = False, ctx: Context | None = None):
    """
    `pds.logistic_reg` (expr_linear.py:277-353 of the reference): the reference's signature and defaults; returns the coefficients
    (bias last) as a NumPy vector whatever the inputs' memory space (one model: `pds_glm_irls_*` hands them to the host, as
    `GLM.fit` takes them), or with `return_pred` the fitted probabilities of every row in the inputs' memory space.
    Deliberate deviation: the reference minimises the mean log loss with L-BFGS from a seeded random start and stops at a gradient
    norm; this backend runs IRLS (binomial family, logit link, `pds_glm_irls_*` on the whole frame) to the same unpenalised
    maximum-likelihood point and stops when no coefficient moves by `tol`.  The two agree to the reference's own test tolerance, not
    bit for bit.  Penalised fits (`l1_reg` / `l2_reg` > 0) are not supported here and raise rather than return an unpenalised fit:
    `GLM(family="binomial", l1_reg=..., l2_reg=...)` and `glm_by` / `glm_by_key` fit them.
    """
    if l1_reg > 0.0 or l2_reg > 0.0:
        raise NotImplementedError("logistic_reg: l1_reg / l2_reg are not supported on this backend; use GLM(family='binomial', "
                                  "l2_reg=...) or glm_by / glm_by_key")
    if max_iter <= 0:
        raise ValueError("Input `max_iter` must be a positive.")  # expr_linear.py:231-232
    if len(x) < 1:
        raise ValueError("logistic_reg: need at least one feature column")
    ctx = ctx or default_context()
    cols = _Cols(target, x)
    _follow(ctx, cols)
    pp = cols.n_feat + int(bool(add_bias))
    co = np.empty(pp, dtype=_dtype())
    n_iter = C.c_int(0)
    _lib.check(ctx.fn("pds_glm_irls")(ctx._h, cols.cols, cols.n_feat, C.c_int64(cols.n_rows), cols.space, int(bool(add_bias)), C.c_int(2),
                                      C.c_int(2), _tol_arg(tol), C.c_int(int(max_iter)), C.c_void_p(co.ctypes.data), C.byref(n_iter)))
    if not return_pred:
        return co
    if cols.space == _lib.PDS_DEVICE:
        import torch

        b = torch.as_tensor(co, device=cols.keep[0].device)
        eta = torch.stack(cols.keep[1:1 + cols.n_feat], dim=1) @ b[:cols.n_feat]
        return torch.sigmoid(eta + b[-1] if add_bias else eta)
    eta = np.stack(cols.keep[1:1 + cols.n_feat], axis=1) @ co[:cols.n_feat] + (co[-1] if add_bias else 0.0)
    return 1.0 / (1.0 + np.exp(-eta))


# ---------------------------------------------------------------------------------------------
# random-intercept mixed model (REML)
# ---------------------------------------------------------------------------------------------
def _mixed_check(x, target, groups, what):
    """Lengths of the columns and of the group argument, before a context exists (fit_reml, mod.rs:184-186)."""
    if len(x) < 1:
        raise ValueError(f"{what}: need at least one feature column")
    n = len(target)
    if any(len(c) != n for c in x) or (groups is not None and len(groups) != n):
        raise ValueError("X, y, and group must have the same number of rows.")


def _f64_out(n):
    a = np.empty(n, dtype=np.float64)
    return a, C.c_void_p(a.ctypes.data)


def mixed_reml(*x, target, group_offsets=None, key=None, max_iter: int = 200, tol: float = 1e-10, ctx: Context | None = None):
    """
    The reference's `MixedModel` fit (fit_reml, src/linear/mixed/mod.rs:173-272): y = X beta + Z u + e with a random intercept per
    group, the variance ratio gamma = sigma_g^2 / sigma_e^2 found by the reference's golden section over the profiled REML deviance.
    X = [1 | x...] (the intercept FIRST), 1 .. 16 feature columns.  The groups are given either as `group_offsets` (group g = rows
    [group_offsets[g], group_offsets[g+1]), contiguous) or as `key`, an integer column in any row order -- exactly one of the two.
    The frame is streamed a fixed number of times (group means and the within-group scatter, `pds_mixed_reml_*`); every deviance
    evaluation is then a reduction over the groups.  Inputs: NumPy arrays or CUDA tensors.  Returns a dict of NumPy values:
    coeffs [p'], std_errors [p'], dfs [p'] (containment), gamma, resid_variance, n_groups (non-empty groups), n_eval (deviance
    evaluations).
    """
    if (group_offsets is None) == (key is None):
        raise ValueError("mixed_reml: exactly one of `group_offsets` and `key` must be given")
    if max_iter < 0:
        raise ValueError("`max_iter` must not be negative.")
    if not np.isfinite(tol):
        raise ValueError("`tol` must be finite.")
    _mixed_check(x, target, key, "mixed_reml")
    ctx = ctx or default_context()
    cols = _Cols(target, x)
    _follow(ctx, cols)
    pp = cols.n_feat + 1
    (co, co_p), (se, se_p), (df, df_p) = _f64_out(pp), _f64_out(pp), _f64_out(pp)
    gamma, rv, ng, ne = C.c_double(0.0), C.c_double(0.0), C.c_int64(0), C.c_int32(0)
    tail = (C.c_int(int(max_iter)), C.c_double(float(tol)), co_p, se_p, df_p, C.byref(gamma), C.byref(rv), C.byref(ng), C.byref(ne))
    if key is not None:
        k, k_p = _key_arg(cols, key)
        _lib.check(ctx.fn("pds_mixed_reml_by_key")(ctx._h, cols.cols, k_p, cols.n_feat, C.c_int64(cols.n_rows), cols.space, *tail))
    else:
        off, off_p = _offsets_arg(cols, group_offsets)
        _lib.check(ctx.fn("pds_mixed_reml_grouped")(ctx._h, cols.cols, cols.n_feat, C.c_int64(cols.n_rows), off_p,
                                                    C.c_int64(int(off.shape[0]) - 1), cols.space, *tail))
    return {"coeffs": co, "std_errors": se, "dfs": df, "gamma": float(gamma.value), "resid_variance": float(rv.value),
            "n_groups": int(ng.value), "n_eval": int(ne.value)}


def mixed_reml_profile(*x, target, group_offsets, gammas, ctx: Context | None = None):
    """
    The profiled REML deviance of `mixed_reml`'s model at given variance ratios, without the search (`pds_mixed_profile_grouped_*`):
    returns a dict of NumPy values deviance [k], beta [k, p'] (the GLS coefficients at that gamma, intercept first) and
    resid_variance [k].  For likelihood-ratio plots and for checking the evaluation on its own.
    """
    g = np.ascontiguousarray(np.atleast_1d(np.asarray(gammas, dtype=np.float64)))
    if g.ndim != 1 or not np.all(np.isfinite(g)) or np.any(g < 0.0):
        raise ValueError("`gammas` must be finite and not negative")
    _mixed_check(x, target, None, "mixed_reml_profile")
    ctx = ctx or default_context()
    cols = _Cols(target, x)
    _follow(ctx, cols)
    pp, k = cols.n_feat + 1, int(g.shape[0])
    (dev, dev_p), (beta, beta_p), (rv, rv_p) = _f64_out(k), _f64_out(k * pp), _f64_out(k)
    off, off_p = _offsets_arg(cols, group_offsets)
    _lib.check(ctx.fn("pds_mixed_profile_grouped")(ctx._h, cols.cols, cols.n_feat, C.c_int64(cols.n_rows), off_p,
                                                   C.c_int64(int(off.shape[0]) - 1), cols.space, C.c_void_p(g.ctypes.data), C.c_int(k), dev_p,
                                                   beta_p, rv_p))
    return {"deviance": dev, "beta": beta.reshape(k, pp), "resid_variance": rv}
