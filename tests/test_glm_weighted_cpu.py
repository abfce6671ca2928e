"""The weighted / offset grouped GLM fits without a GPU: the C ABI surface of pds_glm_irls_wo_grouped_* / _by_key_* (exports, header
declarations, the mock builder's view of them), the argument validation of lstsq.glm_by / glm_by_key that happens before a device is
touched, lstsq.glm_by / glm_by_key on the mock device with the new entry points bound to the restatement (which column lands in which
argument), and the identities of the restatement itself (tests/glm_weighted_reference.py), so that the yardstick of the device tests
is checked before the device is."""
import ctypes as C
import inspect
import re
import sys
import threading
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT))

import glm_cases as gc  # noqa: E402
import glm_weighted_cases as wc  # noqa: E402
import glm_weighted_reference as wr  # noqa: E402

NEW = ["pds_glm_report_wo_grouped_f64", "pds_glm_report_wo_grouped_f32", "pds_glm_report_wo_by_key_f64", "pds_glm_report_wo_by_key_f32",
       "pds_glm_irls_wo_f64", "pds_glm_irls_wo_f32", "pds_glm_irls_wo_grouped_f64", "pds_glm_irls_wo_grouped_f32", "pds_glm_irls_wo_by_key_f64", "pds_glm_irls_wo_by_key_f32"]
FAMILY_OF = {0: "gaussian", 1: "poisson", 2: "binomial", 3: "gamma"}


def _mock_build():
    sys.path.insert(0, str(ROOT / "tests" / "mock_device"))
    try:
        import build as mock_build
    finally:
        sys.path.pop(0)
    return mock_build


def test_exported_and_declared():
    from polars_ds_extension_amd import _lib

    assert all(n in _lib.EXPORTS for n in NEW)
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "pds_lstsq.h").read_text(), flags=re.S)
    for n in NEW:
        assert len(re.findall(rf"^int\s+{n}\s*\(", text, flags=re.M)) == 1, n


def test_argument_lists_are_the_twins_plus_two_columns():
    protos = {name: args for _, name, args in _mock_build().prototypes()}
    for sfx, real in (("f64", "double"), ("f32", "float")):
        for form in ("", "grouped_", "by_key_"):
            twin, new = protos[f"pds_glm_irls_{form}{sfx}"], protos[f"pds_glm_irls_wo_{form}{sfx}"]
            assert [a for _, a in new] == [a for _, a in twin[:2]] + ["weights", "offset"] + [a for _, a in twin[2:]]
            assert [t for t, _ in new[2:4]] == [f"const {real}*"] * 2
            assert [t for t, _ in new[:2]] + [t for t, _ in new[4:]] == [t for t, _ in twin]
        for form in ("grouped", "by_key"):
            twin, new = protos[f"pds_glm_report_{form}_{sfx}"], protos[f"pds_glm_report_wo_{form}_{sfx}"]
            assert [a for _, a in new] == [a for _, a in twin[:2]] + ["weights", "offset"] + [a for _, a in twin[2:]]


def test_validation_without_a_device():
    """Every one of these raises before a context is created (no GPU here: reaching the device would raise something else)."""
    import polars_ds_extension_amd as pds

    x = np.arange(12.0)
    y = (x > 5).astype(float)
    off = np.array([0, 6, 12])
    key = np.zeros(12, dtype=np.int64)
    w = np.ones(12)
    for pen in ({"l1_reg": 0.1}, {"l2_reg": 0.1}):
        for col in ({"weights": w}, {"offset": w}):
            with pytest.raises(NotImplementedError, match="weights= / offset="):
                pds.glm_by(x, target=y, group_offsets=off, family="binomial", **pen, **col)
            with pytest.raises(NotImplementedError, match="weights= / offset="):
                pds.glm_by_key(x, target=y, key=key, family="binomial", **pen, **col)
    with pytest.raises(ValueError, match="`weights` must have one entry per row"):
        pds.glm_by(x, target=y, group_offsets=off, weights=w[:5])
    with pytest.raises(ValueError, match="`offset` must have one entry per row"):
        pds.glm_by_key(x, target=y, key=key, offset=w[:5])
    with pytest.raises(NotImplementedError, match="up to 16 feature columns"):
        pds.glm_by(*[x] * 17, target=y, group_offsets=off, weights=w)
    for fn in (pds.glm_by, pds.glm_by_key):
        sig = inspect.signature(fn)
        assert sig.parameters["weights"].default is None and sig.parameters["offset"].default is None
        assert "offset" in fn.__doc__ and "weights" in fn.__doc__


# ------------------------------------------------------------------------------------------------- lstsq on the mock device
def bind_wo(lib, calls):
    """binds pds_glm_irls_wo_grouped_* / _by_key_* of the mock library `lib` to the restatement (host pointers); `calls` records which
    of the two column pointers each call received.  Returns the callbacks, which must outlive the library's use."""
    keep = []

    def view(ptr, n, dt):
        return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(np.ctypeslib.as_ctypes_type(dt))), shape=(n,))

    def frame(cols_p, w_p, o_p, n_feat, n, dt):
        ptrs = C.cast(cols_p, C.POINTER(C.c_void_p))
        cols = [view(ptrs[c], n, dt).astype(np.float64) for c in range(n_feat + 1)]
        pw = view(w_p, n, dt).astype(np.float64) if w_p else None
        o = view(o_p, n, dt).astype(np.float64) if o_p else None
        calls.append((pw is not None, o is not None))
        return np.stack(cols[1:], axis=1), cols[0], pw, o

    def fill(X, y, pw, o, off, bias, link, tol, max_iter, co_p, it_p, nu_p, pred, rnull, rows, dt):
        ng, p = len(off) - 1, X.shape[1]
        pp = p + int(bool(bias))
        co, it = wr.fit(X, y, off, pw, o, FAMILY_OF[link], bool(bias), tol, max_iter)
        nu = (~np.isfinite(co).all(axis=1)).astype(np.uint8)
        view(co_p, ng * pp, dt)[:] = co.reshape(-1)
        view(it_p, ng, np.int32)[:] = it
        view(nu_p, ng, np.uint8)[:] = nu
        gid = np.repeat(np.arange(ng), np.diff(off))
        eta = np.einsum("ij,ij->i", X, co[gid][:, :p]) + (co[gid][:, p] if bias else 0.0) + (0.0 if o is None else o)
        if pred is not None:
            pred[rows] = gc.inv_link(FAMILY_OF[link], eta)
        if rnull is not None:
            rnull[rows] = nu[gid]

    def make_grouped(dt, ct):
        def fn(ctx, cols_p, w_p, o_p, n_feat, n, off_p, ng, space, bias, link, var, tol, max_iter, co_p, it_p, nu_p, pr_p, rn_p):
            X, y, pw, o = frame(cols_p, w_p, o_p, n_feat, n, dt)
            fill(X, y, pw, o, view(off_p, ng + 1, np.int64).copy(), bias, link, tol, max_iter, co_p, it_p, nu_p,
                 view(pr_p, n, dt) if pr_p else None, view(rn_p, n, np.uint8) if rn_p else None, np.arange(n), dt)
            return 0

        return C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_int64, C.c_int,
                           C.c_int, C.c_int, C.c_int, ct, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)(fn)

    def make_by_key(dt, ct):
        def fn(ctx, cols_p, w_p, o_p, keys_p, n_feat, n, space, bias, link, var, tol, max_iter, max_groups, ok_p, co_p, it_p, nu_p, ng_p,
               pr_p, rn_p):
            keys = view(keys_p, n, np.int64)
            order = np.argsort(keys, kind="stable")
            uniq, counts = np.unique(keys[order], return_counts=True)
            C.c_int64.from_address(ng_p).value = len(uniq)
            if len(uniq) > max_groups:
                lib.mock_set_error(b"more distinct keys than max_groups")
                return -1
            X, y, pw, o = frame(cols_p, w_p, o_p, n_feat, n, dt)
            view(ok_p, len(uniq), np.int64)[:] = uniq
            fill(X[order], y[order], None if pw is None else pw[order], None if o is None else o[order], gc.offsets(counts), bias, link,
                 tol, max_iter, co_p, it_p, nu_p, view(pr_p, n, dt) if pr_p else None, view(rn_p, n, np.uint8) if rn_p else None, order, dt)
            return 0

        return C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_int,
                           C.c_int, C.c_int, ct, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                           C.c_void_p)(fn)

    # ---- the report entry points: the fit above, then the float64 restatement of the weighted report at its coefficients
    def fill_report(X, y, pw, o, off, bias, link, tol, max_iter, co_p, it_p, nu_p, out_p, dt):
        from polars_ds_extension_amd import _lib

        ng, pp = len(off) - 1, X.shape[1] + int(bool(bias))
        fill(X, y, pw, o, off, bias, link, tol, max_iter, co_p, it_p, nu_p, None, None, None, dt)
        co, nu = view(co_p, ng * pp, dt).reshape(ng, pp), view(nu_p, ng, np.uint8)
        out = C.cast(out_p, C.POINTER(_lib.GlmReportOut)).contents
        with np.errstate(all="ignore"):
            rep = wr.report_by(X, y, off, pw, o, co.astype(np.float64), FAMILY_OF[link], bool(bias), dtype=np.float64, skip=nu.astype(bool))
        for k, rk in (("std_err", "std_err"), ("z", "z"), ("p", "p"), ("ci_lower", "lo"), ("ci_upper", "hi")):
            if getattr(out, k):
                view(getattr(out, k), ng * pp, dt)[:] = rep[rk].reshape(-1)
        for k in ("deviance", "null_deviance", "pearson_chi2", "dispersion"):
            if getattr(out, k):
                view(getattr(out, k), ng, dt)[:] = rep[k]
        if out.df_resid:
            view(out.df_resid, ng, np.int64)[:] = rep["df_resid"]
        if out.report_null:
            view(out.report_null, ng, np.uint8)[:] = nu

    def make_report_grouped(dt, ct):
        def fn(ctx, cols_p, w_p, o_p, n_feat, n, off_p, ng, space, bias, link, var, tol, max_iter, co_p, it_p, nu_p, out_p):
            X, y, pw, o = frame(cols_p, w_p, o_p, n_feat, n, dt)
            fill_report(X, y, pw, o, view(off_p, ng + 1, np.int64).copy(), bias, link, tol, max_iter, co_p, it_p, nu_p, out_p, dt)
            return 0

        return C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_int64, C.c_int,
                           C.c_int, C.c_int, C.c_int, ct, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)(fn)

    def make_report_by_key(dt, ct):
        def fn(ctx, cols_p, w_p, o_p, keys_p, n_feat, n, space, bias, link, var, tol, max_iter, max_groups, ok_p, co_p, it_p, nu_p, ng_p,
               out_p):
            keys = view(keys_p, n, np.int64)
            order = np.argsort(keys, kind="stable")
            uniq, counts = np.unique(keys[order], return_counts=True)
            C.c_int64.from_address(ng_p).value = len(uniq)
            if len(uniq) > max_groups:
                lib.mock_set_error(b"more distinct keys than max_groups")
                return -1
            X, y, pw, o = frame(cols_p, w_p, o_p, n_feat, n, dt)
            view(ok_p, len(uniq), np.int64)[:] = uniq
            fill_report(X[order], y[order], None if pw is None else pw[order], None if o is None else o[order], gc.offsets(counts), bias,
                        link, tol, max_iter, co_p, it_p, nu_p, out_p, dt)
            return 0

        return C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_int,
                           C.c_int, C.c_int, ct, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                           C.c_void_p)(fn)

    for sfx, dt, ct in (("f64", np.float64, C.c_double), ("f32", np.float32, C.c_float)):
        for name, cb in ((f"pds_glm_report_wo_grouped_{sfx}", make_report_grouped(dt, ct)),
                         (f"pds_glm_report_wo_by_key_{sfx}", make_report_by_key(dt, ct))):
            keep.append(cb)
            getattr(lib, "mock_bind_" + name)(C.cast(cb, C.c_void_p))
    for sfx, dt, ct in (("f64", np.float64, C.c_double), ("f32", np.float32, C.c_float)):
        for name, cb in ((f"pds_glm_irls_wo_grouped_{sfx}", make_grouped(dt, ct)), (f"pds_glm_irls_wo_by_key_{sfx}", make_by_key(dt, ct))):
            keep.append(cb)
            getattr(lib, "mock_bind_" + name)(C.cast(cb, C.c_void_p))
    return keep


@pytest.fixture()
def mock_pds():
    """polars_ds_extension_amd on the mock device with the weighted / offset entry points bound (bind_wo)"""
    import torch
    from mock_device import device

    import polars_ds_extension_amd as m
    from polars_ds_extension_amd import _lib, lstsq

    lib = device.load_for_package()
    calls = []
    keep = bind_wo(lib, calls)
    saved_lib, saved_tls, saved_avail = _lib._lib, lstsq._tls, torch.cuda.is_available
    _lib._lib = lib
    lstsq._tls = threading.local()
    torch.cuda.is_available = lambda: False  # (the mock answers host pointers only)
    try:
        yield m, calls
    finally:
        torch.cuda.is_available = saved_avail
        _lib._lib, lstsq._tls = saved_lib, saved_tls
        m.config.LIN_REG_EXPR_F64 = True
        del keep[:]


@pytest.mark.parametrize("mode", ["both", "weights", "offset"])
def test_lstsq_hands_each_column_to_its_argument(mock_pds, mode):
    pds, calls = mock_pds
    X, y, off, pw, o = wc.frame("poisson", 3, "integer", with_offset=mode != "weights", n_groups=6)
    pw_arg, o_arg = (None if mode == "offset" else pw), (None if mode == "weights" else o)
    co_o, it_o = wr.fit(X, y, off, pw_arg, o_arg, "poisson", True, 1e-10, 100)
    cols = [np.ascontiguousarray(X[:, j]) for j in range(3)]
    co, it, nu, pred, rn = pds.glm_by(*cols, target=y, group_offsets=off, family="poisson", add_bias=True, tol=1e-10, max_iter=100,
                                      return_pred=True, weights=pw_arg, offset=o_arg)
    assert calls[-1] == (pw_arg is not None, o_arg is not None)
    assert np.array_equal(co, co_o) and np.array_equal(it, it_o) and not nu.any() and not rn.any()
    gid = np.repeat(np.arange(6), np.diff(off))
    want = np.exp(np.einsum("ij,ij->i", X, co[gid][:, :3]) + co[gid][:, 3] + (0.0 if o_arg is None else o_arg))
    assert np.allclose(pred, want, rtol=1e-14)
    # by key, shuffled rows: the same groups, pred at the rows' own positions
    perm = np.random.default_rng(1).permutation(len(y))
    key = (gid * 5 - 7).astype(np.int64)
    k, co2, it2, nu2, pred2, rn2 = pds.glm_by_key(*[c[perm] for c in cols], target=y[perm], key=key[perm], family="poisson", add_bias=True,
                                                  tol=1e-10, max_iter=100, return_pred=True,
                                                  weights=None if pw_arg is None else pw_arg[perm], offset=None if o_arg is None else o_arg[perm])
    assert calls[-1] == (pw_arg is not None, o_arg is not None)
    assert np.array_equal(k, np.arange(6) * 5 - 7) and np.array_equal(it2, it_o)
    assert np.allclose(co2, co_o, rtol=1e-9) and np.allclose(pred2, want[perm], rtol=1e-9)


def test_null_pointers_are_the_unweighted_fit_on_the_mock(mock_pds, orc):
    """the C entry point with both column pointers null, called as a C caller would: the unweighted fit of every group (the oracle's,
    at the device tests' bound) -- on the product library the same call is the twin's, bit for bit (tests/test_glm_weighted_gpu.py)"""
    from polars_ds_extension_amd import _lib

    pds, calls = mock_pds
    X, y, off, _, _ = wc.frame("poisson", 2, "real", with_offset=False, n_groups=5)
    lib, ctx = _lib.load(), pds.default_context()
    xs = [np.ascontiguousarray(X[:, j]) for j in range(2)]
    cols = (C.c_void_p * 3)(y.ctypes.data, xs[0].ctypes.data, xs[1].ctypes.data)
    co, it, nu = np.empty((5, 3)), np.empty(5, dtype=np.int32), np.empty(5, dtype=np.uint8)
    rc = lib.pds_glm_irls_wo_grouped_f64(ctx._h, cols, None, None, 2, C.c_int64(len(y)), C.c_void_p(off.ctypes.data), C.c_int64(5), _lib.PDS_HOST,
                                         1, 1, 1, C.c_double(1e-10), 100, C.c_void_p(co.ctypes.data), C.c_void_p(it.ctypes.data),
                                         C.c_void_p(nu.ctypes.data), None, None)
    assert rc == 0 and calls[-1] == (False, False) and not nu.any()
    co_o, it_o = gc.oracle_by(orc, X, y, off, "poisson", True, 1e-10, 100)
    assert (np.linalg.norm(co - co_o, axis=1) / np.linalg.norm(co_o, axis=1)).max() < 1e-9 and np.abs(it - it_o).max() <= 1


# ------------------------------------------------------------------------------------------------- the restatement's identities
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("family", gc.FAMILIES)
def test_unit_weights_and_zero_offset_are_the_oracle(orc, family, bias):
    """weights 1, offsets 0 (given or absent) = oracle.glm_irls on every group, at the device tests' bound"""
    X, y, off, _, _ = wc.frame(family, 4, "real", with_offset=False, n_groups=12)
    co_o, it_o = gc.oracle_by(orc, X, y, off, family, bias, 1e-10, 100)
    for pw, o in ((None, None), (np.ones(len(y)), np.zeros(len(y)))):
        co, it = wr.fit(X, y, off, pw, o, family, bias, 1e-10, 100)
        err = np.linalg.norm(co - co_o, axis=1) / np.linalg.norm(co_o, axis=1)
        assert err.max() < 1e-9 and np.abs(it - it_o).max() <= 1


@pytest.mark.parametrize("family", gc.FAMILIES)
def test_integer_weights_are_repeated_rows(family):
    X, y, off, pw, o = wc.frame(family, 3, "integer", n_groups=10)
    co, it = wr.fit(X, y, off, pw, o, family, True, 1e-10, 100)
    Xr, yr, offr, o_r = wc.replicate(X, y, off, pw, o)
    co_r, it_r = wr.fit(Xr, yr, offr, None, o_r, family, True, 1e-10, 100)
    err = np.linalg.norm(co - co_r, axis=1) / np.linalg.norm(co_r, axis=1)
    assert err.max() < 1e-9 and np.abs(it - it_r).max() <= 1


def test_constant_offset_moves_the_bias():
    X, y, off, pw, _ = wc.frame("poisson", 3, "real", with_offset=False, n_groups=10)
    c = np.linspace(-1.0, 1.0, 10)
    co0, it0 = wr.fit(X, y, off, pw, None, "poisson", True, 1e-10, 100)
    co, it = wr.fit(X, y, off, pw, np.repeat(c, np.diff(off)), "poisson", True, 1e-10, 100)
    co[:, 3] += c
    assert (np.linalg.norm(co - co0, axis=1) / np.linalg.norm(co0, axis=1)).max() < 1e-9 and np.abs(it - it0).max() <= 1


@pytest.mark.parametrize("kind", wc.KINDS)
def test_gaussian_is_weighted_least_squares_with_the_offset_taken_off_y(kind):
    X, y, off, pw, o = wc.frame("gaussian", 5, kind, n_groups=8)
    co, it = wr.fit(X, y, off, pw, o, "gaussian", True, 1e-10, 100)
    assert (it == 2).all()
    for g in range(8):
        a, b = off[g], off[g + 1]
        Z = np.column_stack([X[a:b], np.ones(b - a)])
        W = np.diag(pw[a:b])
        want = np.linalg.solve(Z.T @ W @ Z, Z.T @ W @ (y[a:b] - o[a:b]))
        assert np.linalg.norm(co[g] - want) < 1e-10 * np.linalg.norm(want)


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("family", gc.FAMILIES)
def test_the_fit_is_where_the_weighted_score_vanishes(family, bias):
    """solver-independent: X' diag(pw / (g' V)) (y - mu) = 0 at the returned coefficients, relative to the same sum of absolute terms"""
    X, y, off, pw, o = wc.frame(family, 8, "real", n_groups=10)
    co, it = wr.fit(X, y, off, pw, o, family, bias, 1e-12, 100)
    for g in range(10):
        a, b = off[g], off[g + 1]
        s = wr.score(X[a:b], y[a:b], pw[a:b], o[a:b], co[g], family, bias)
        Z = np.column_stack([X[a:b], np.ones(b - a)]) if bias else X[a:b]
        mu = wr.inv(family, Z @ co[g] + o[a:b])
        scale = np.abs(Z).T @ np.abs(pw[a:b] * (y[a:b] - mu) / (wr.deriv(family, mu) * wr.var(family, mu)))
        assert it[g] < 100 and (np.abs(s) <= 1e-9 * scale).all()


def test_null_rule():
    rng = np.random.default_rng(4)
    X, y = rng.normal(size=(30, 3)), rng.normal(size=30)
    pw = np.zeros(30)
    pw[:3] = 1.0
    assert wr.fit_group(X, y, pw, None, "gaussian", True)[1] == 0 and np.isnan(wr.fit_group(X, y, pw, None, "gaussian", True)[0]).all()
    b, it = wr.fit_group(X, y, pw, None, "gaussian", False)  # three live rows, three coefficients: the interpolation
    assert it == 2 and np.allclose(X[:3] @ b, y[:3], rtol=1e-10, atol=1e-12)
    for bad in (-1.0, np.nan, np.inf):
        pw2 = np.ones(30)
        pw2[11] = bad
        b, it = wr.fit_group(X, y, pw2, None, "gaussian", True)
        assert it == 0 and np.isnan(b).all()
    o = np.zeros(30)
    o[5] = np.nan
    b, it = wr.fit_group(X, y, None, o, "gaussian", True)
    assert it == 100 and not np.isfinite(b).all()  # (null by the coefficients, as the unweighted rule has it)
    # rows of weight 0 do not exist: whatever they hold
    y2, X2 = y.copy(), X.copy()
    pw3 = np.ones(30)
    pw3[7] = 0.0
    y2[7], X2[7, 1] = np.nan, np.inf
    b1, _ = wr.fit_group(X2, y2, pw3, None, "gaussian", True)
    b2, _ = wr.fit_group(np.delete(X, 7, axis=0), np.delete(y, 7), None, None, "gaussian", True)
    assert np.array_equal(b1, b2)
