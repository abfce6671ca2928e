"""Grouped GLM fits and logistic_reg without a GPU: the C ABI surface of pds_glm_irls_grouped_* / _by_key_* (exports, header
declarations, the mock builder's view of them) and the argument validation of lstsq.glm_by / glm_by_key / logistic_reg, which
happens before a device is touched."""
import re
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT))

NEW = ["pds_glm_irls_grouped_f64", "pds_glm_irls_grouped_f32", "pds_glm_irls_by_key_f64", "pds_glm_irls_by_key_f32"]


def test_exported_and_declared():
    from polars_ds_extension_amd import _lib

    assert all(n in _lib.EXPORTS for n in NEW)
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "pds_lstsq.h").read_text(), flags=re.S)
    for n in NEW:
        assert len(re.findall(rf"^int\s+{n}\s*\(", text, flags=re.M)) == 1, n


def _mock_build():
    sys.path.insert(0, str(ROOT / "tests" / "mock_device"))
    try:
        import build as mock_build
    finally:
        sys.path.pop(0)
    return mock_build


def test_mock_trampolines_parse():
    protos = {name: [a for _, a in args] for _, name, args in _mock_build().prototypes()}
    assert protos["pds_glm_irls_grouped_f64"] == ["ctx", "cols", "n_feat", "n_rows", "group_offsets", "n_groups", "space", "add_bias", "link",
                                                  "variance", "tol", "max_iter", "coeffs", "n_iter", "is_null", "pred", "row_null"]
    assert protos["pds_glm_irls_by_key_f32"] == ["ctx", "cols", "keys", "n_feat", "n_rows", "space", "add_bias", "link", "variance", "tol",
                                                 "max_iter", "max_groups", "out_keys", "coeffs", "n_iter", "is_null", "n_groups", "pred",
                                                 "row_null"]
    types = {name: [t for t, _ in args] for _, name, args in _mock_build().prototypes()}
    assert types["pds_glm_irls_grouped_f32"][10] == "float" and types["pds_glm_irls_grouped_f64"][10] == "double"


def test_source_lists_the_kernel():
    """The new kernel file is part of the library's build, and moments.hip takes the link functions from the shared header."""
    csrc = ROOT / "polars_ds_extension_amd" / "csrc"
    assert "grouped_irls.hip" in (csrc / "Makefile").read_text()
    assert '#include "glm_dev.hpp"' in (csrc / "moments.hip").read_text()
    assert "T glm_link(" not in (csrc / "moments.hip").read_text() and "T glm_link(" in (csrc / "glm_dev.hpp").read_text()
    assert '#include "glm_dev.hpp"' in (csrc / "grouped_irls.hip").read_text()


def test_public_names():
    import polars_ds_extension_amd as pds
    from polars_ds_extension_amd import lstsq

    for n in ("glm_by", "glm_by_key", "logistic_reg"):
        assert callable(getattr(pds, n)) and n in lstsq.__all__


def test_validation_without_a_device():
    """Every one of these raises before a context is created (no GPU here: reaching the device would raise something else)."""
    import inspect

    import polars_ds_extension_amd as pds

    x = np.arange(12.0)
    y = (x > 5).astype(float)
    off = np.array([0, 6, 12])
    with pytest.raises(NotImplementedError, match="logistic_reg: l1_reg / l2_reg are not supported on this backend"):
        pds.logistic_reg(x, target=y, l1_reg=0.1)
    with pytest.raises(NotImplementedError, match="logistic_reg: l1_reg / l2_reg are not supported on this backend"):
        pds.logistic_reg(x, target=y, l2_reg=0.1)
    with pytest.raises(ValueError, match="Input `max_iter` must be a positive."):
        pds.logistic_reg(x, target=y, max_iter=0)
    with pytest.raises(ValueError, match="`max_iter` must be > 1."):
        pds.glm_by(x, target=y, group_offsets=off, family="binomial", max_iter=0)
    with pytest.raises(NotImplementedError, match="family"):
        pds.glm_by(x, target=y, group_offsets=off, family="tweedie")
    with pytest.raises(NotImplementedError, match="family"):
        pds.glm_by_key(x, target=y, key=np.zeros(12, dtype=np.int64), family="tweedie")
    with pytest.raises(NotImplementedError, match=re.escape("grouped GLM (IRLS): up to 16 feature columns")):
        pds.glm_by(*[x] * 17, target=y, group_offsets=off)
    with pytest.raises(ValueError, match="at least one feature"):
        pds.glm_by(target=y, group_offsets=off)
    # the reference's signature and defaults (expr_linear.py:277-353)
    sig = inspect.signature(pds.logistic_reg)
    want = {"add_bias": True, "l1_reg": 0.0, "l2_reg": 0.0, "tol": 1e-5, "max_iter": 200, "return_pred": False}
    assert {k: sig.parameters[k].default for k in want} == want
    sig = inspect.signature(pds.glm_by)
    want = {"family": "gaussian", "add_bias": False, "tol": 1e-8, "max_iter": 100, "return_pred": False}
    assert {k: sig.parameters[k].default for k in want} == want
    assert "max_groups" in inspect.signature(pds.glm_by_key).parameters


# ------------------------------------------------------------------------------------------------- the plugin layer on the mock device
import ctypes as C  # noqa: E402

import glm_cases as gc  # noqa: E402

FAMILY_OF = {0: "gaussian", 1: "poisson", 2: "binomial", 3: "gamma"}
CALLS = []  # (entry point, n_rows, groups or max_groups) of every grouped GLM call the mock saw


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle

    oracle.build()
    return oracle


@pytest.fixture(scope="module")
def mock(orc):
    """The mock plugin library, its grouped GLM entry points bound to callbacks that loop oracle.glm_irls over the groups."""
    from mock_device import device

    lib = device.load()
    keep = []

    def view(ptr, n, dt):
        return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(np.ctypeslib.as_ctypes_type(dt))), shape=(n,))

    def frame(cols_p, n_feat, n, dt):
        ptrs = C.cast(cols_p, C.POINTER(C.c_void_p))
        cols = [view(ptrs[c], n, dt).copy() for c in range(n_feat + 1)]
        return np.stack(cols[1:], axis=1), cols[0]

    def fill(X, y, off, bias, link, tol, max_iter, co_p, it_p, nu_p, pred, rnull, rows, dt):
        """every group on its own rows; `rows`: where the rows of the group-ordered frame sit in pred / row_null"""
        ng = len(off) - 1
        pp = X.shape[1] + int(bool(bias))
        co, it, nu = view(co_p, ng * pp, dt).reshape(ng, pp), view(it_p, ng, np.int32), view(nu_p, ng, np.uint8)
        fam = FAMILY_OF[link]
        for g in range(ng):
            s, e = int(off[g]), int(off[g + 1])
            if e - s < pp:
                co[g], it[g], nu[g] = np.nan, 0, 1
                mu = np.full(e - s, np.nan)
            else:
                with np.errstate(all="ignore"):
                    b, k = orc.glm_irls(X[s:e].astype(np.float64), y[s:e].astype(np.float64), family=fam, add_bias=bool(bias), tol=float(tol),
                                        max_iter=int(max_iter))
                    co[g], it[g], nu[g] = b, k, int(not np.isfinite(b).all())
                    mu = gc.inv_link(fam, X[s:e].astype(np.float64) @ b[:X.shape[1]] + (b[-1] if bias else 0.0))
                if nu[g]:
                    mu = np.full(e - s, np.nan)
            if pred is not None:
                pred[rows[s:e]] = mu
            if rnull is not None:
                rnull[rows[s:e]] = nu[g]

    def make_grouped(dt, ct):
        def fn(ctx, cols_p, n_feat, n, off_p, ng, space, bias, link, var, tol, max_iter, co_p, it_p, nu_p, pred_p, rn_p):
            CALLS.append(("grouped", n, ng))
            X, y = frame(cols_p, n_feat, n, dt)
            fill(X, y, view(off_p, ng + 1, np.int64).copy(), bias, link, tol, max_iter, co_p, it_p, nu_p,
                 view(pred_p, n, dt) if pred_p else None, view(rn_p, n, np.uint8) if rn_p else None, np.arange(n), dt)
            return 0

        return C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, ct,
                           C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)(fn)

    def make_by_key(dt, ct):
        def fn(ctx, cols_p, keys_p, n_feat, n, space, bias, link, var, tol, max_iter, max_groups, ok_p, co_p, it_p, nu_p, ng_p, pred_p, rn_p):
            CALLS.append(("by_key", n, max_groups))
            keys = view(keys_p, n, np.int64)
            order = np.argsort(keys, kind="stable")
            uniq, counts = np.unique(keys[order], return_counts=True)
            C.c_int64.from_address(ng_p).value = len(uniq)
            if len(uniq) > max_groups:
                lib.mock_set_error(b"more distinct keys than max_groups")
                return -1
            X, y = frame(cols_p, n_feat, n, dt)
            view(ok_p, len(uniq), np.int64)[:] = uniq
            fill(X[order], y[order], np.concatenate([[0], np.cumsum(counts)]), bias, link, tol, max_iter, co_p, it_p, nu_p,
                 view(pred_p, n, dt) if pred_p else None, view(rn_p, n, np.uint8) if rn_p else None, order, dt)
            return 0

        return C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, ct, C.c_int,
                           C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)(fn)

    for sfx, dt, ct in (("f64", np.float64, C.c_double), ("f32", np.float32, C.c_float)):
        for name, cb in ((f"pds_glm_irls_grouped_{sfx}", make_grouped(dt, ct)), (f"pds_glm_irls_by_key_{sfx}", make_by_key(dt, ct))):
            keep.append(cb)
            getattr(lib, "mock_bind_" + name)(C.cast(cb, C.c_void_p))
    lib._glm_keep = keep
    return lib


def _glm_frame(rng, sizes, p, family="binomial", shuffle=True):
    """keys 7 g - 20 (ascending key order is not the order of first appearance), rows shuffled"""
    X, y, off = gc.family_frame(rng, family, sizes, p)
    key = np.repeat(np.arange(len(sizes), dtype=np.int64) * 7 - 20, sizes)
    if shuffle:
        perm = rng.permutation(len(y))
        key, X, y = key[perm], X[perm], y[perm]
    return key, X, y


def _inputs(key, X, y, key_name="k", dt=np.float64, key_mask=None, masks=None):
    import pyarrow as pa

    masks = masks or {}
    ins = [] if key is None else [(key_name, pa.array(key, type=pa.int64(), mask=key_mask))]
    ins.append(("y", pa.array(y.astype(dt), mask=masks.get(0))))
    ins += [(f"x{j + 1}", pa.array(X[:, j].astype(dt), mask=masks.get(j + 1))) for j in range(X.shape[1])]
    return ins


GKW = {"bias": True, "null_policy": "raise", "family": "binomial", "tol": 1e-10, "max_iter": 100}


def _check_groups(orc, out, key, X, y, bias, family, null_last=None, tol=1e-10):
    got_keys = out.field(0).to_pylist()
    uniq = sorted(set(int(k) for k in key if null_last is None or k != null_last))
    assert got_keys == uniq + ([None] if null_last is not None else [])  # ascending, the null key's group last
    co, it = out.field(1), out.field(2).to_pylist()
    pp = X.shape[1] + int(bias)
    for gi, k in enumerate(uniq + ([null_last] if null_last is not None else [])):
        rows = np.flatnonzero(key == k)
        if len(rows) < pp:
            assert not co[gi].is_valid and it[gi] == 0
            continue
        with np.errstate(all="ignore"):
            b, n_it = orc.glm_irls(X[rows], y[rows], family=family, add_bias=bias, tol=tol, max_iter=100)
        if not np.isfinite(b).all():  # (a fit that does not end in finite coefficients: a null group)
            assert not co[gi].is_valid and it[gi] == n_it
            continue
        assert co[gi].is_valid and it[gi] == n_it
        np.testing.assert_allclose(np.asarray(co[gi].as_py()), b, rtol=1e-12, atol=1e-12)


def test_plugin_glm_by(mock, orc):
    import pyarrow as pa
    from plugin_harness import call_plugin, output_field

    rng = np.random.default_rng(5)
    sizes = [60, 3, 45, 80, 50]  # group 1 (key -13): 3 rows < p' = 4 -> a null list
    key, X, y = _glm_frame(rng, sizes, 3)
    fld = output_field(mock, "pl_glm_by", [pa.field("k", pa.int64()), pa.field("y", pa.float64())])
    assert [f.name for f in fld.type] == ["k", "coeffs", "n_iter"]
    assert [f.type for f in fld.type] == [pa.int64(), pa.large_list(pa.float64()), pa.int32()]
    assert output_field(mock, "pl_glm_by_f32").type[1].type == pa.large_list(pa.float32())
    assert output_field(mock, "pl_glm_by_pred") == pa.field("pred", pa.float64())
    assert output_field(mock, "pl_glm_by_pred_f32") == pa.field("pred", pa.float32())
    CALLS.clear()
    field, out = call_plugin(mock, "pl_glm_by", _inputs(key, X, y), GKW)
    assert [f.name for f in out.type] == ["k", "coeffs", "n_iter"] and len(out) == len(sizes)
    assert CALLS == [("by_key", len(y), len(y))]  # one call, the whole frame
    _check_groups(orc, out, key, X, y, True, "binomial")
    # an unnamed key column: "key"; another family, no bias
    key2, X2, y2 = _glm_frame(rng, sizes, 3, "poisson")
    _, out2 = call_plugin(mock, "pl_glm_by", _inputs(key2, X2, y2, key_name=""), dict(GKW, family="poisson", bias=False))
    assert out2.type[0].name == "key"
    _check_groups(orc, out2, key2, X2, y2, False, "poisson")
    # per-row means at the rows' own positions, null for the rows of the short group
    fieldp, pred = call_plugin(mock, "pl_glm_by_pred", _inputs(key, X, y), GKW)
    assert fieldp.name == "pred" and pred.type == pa.float64() and len(pred) == len(y)
    pv = pred.to_numpy(zero_copy_only=False)
    for k in np.unique(key):
        rows = np.flatnonzero(key == k)
        if len(rows) < 4:
            assert pred.take(pa.array(rows)).null_count == len(rows)
            continue
        b, _ = orc.glm_irls(X[rows], y[rows], family="binomial", add_bias=True, tol=1e-10, max_iter=100)
        np.testing.assert_allclose(pv[rows], gc.inv_link("binomial", X[rows] @ b[:3] + b[3]), rtol=1e-12, atol=1e-12)
    assert pred.null_count == 3


def test_plugin_glm_by_null_keys_and_capacity_retry(mock, orc):
    from plugin_harness import call_plugin

    rng = np.random.default_rng(6)
    key, X, y = _glm_frame(rng, [50, 40, 45], 2)
    mask = key == -13  # the middle key's rows become the null group
    stand_in = int(key.max()) + 1
    _, out = call_plugin(mock, "pl_glm_by", _inputs(key, X, y, key_mask=mask), GKW)
    key_n = np.where(mask, stand_in, key)
    _check_groups(orc, out, key_n, X, y, True, "binomial", null_last=stand_in)
    # the capacity guess is too small: one retry with the device's count
    mock.pds_plugin_debug_glm_by_first_cap(C.c_longlong(2))
    try:
        CALLS.clear()
        _, out = call_plugin(mock, "pl_glm_by", _inputs(key, X, y), GKW)
        assert CALLS == [("by_key", len(y), 2), ("by_key", len(y), 3)]
        _check_groups(orc, out, key, X, y, True, "binomial")
    finally:
        mock.pds_plugin_debug_glm_by_first_cap(C.c_longlong(0))


@pytest.mark.parametrize("policy", ["skip", "zero", "0.5", "ignore"])
def test_plugin_glm_by_null_policies(mock, orc, policy):
    """Every policy against a frame prepared by hand: skip = rows with a null removed, fill = features filled and rows with a null
    target removed, ignore = the rows kept with NaN (that group's fit is not finite: a null group)."""
    import pyarrow as pa
    from plugin_harness import call_plugin

    rng = np.random.default_rng(7)
    key, X, y = _glm_frame(rng, [70, 60, 65], 2, "poisson")
    n = len(y)
    masks = {0: np.zeros(n, bool), 1: np.zeros(n, bool), 2: np.zeros(n, bool)}
    first = key == -20
    masks[0][np.flatnonzero(first)[:3]] = True      # nulls of the target, of x1 and of x2 in the first key's group only
    masks[1][np.flatnonzero(first)[5:9]] = True
    masks[2][np.flatnonzero(first)[7:11]] = True
    kw = dict(GKW, family="poisson", null_policy=policy)
    _, out = call_plugin(mock, "pl_glm_by", _inputs(key, X, y, masks=masks), kw)
    _, pred = call_plugin(mock, "pl_glm_by_pred", _inputs(key, X, y, masks=masks), kw)
    if policy == "ignore":
        assert out.field(0).to_pylist() == [-20, -13, -6]
        assert [c.is_valid for c in out.field(1)] == [False, True, True]
        assert pred.null_count == int(first.sum()) and pred.take(pa.array(np.flatnonzero(first))).null_count == int(first.sum())
        return
    if policy == "skip":
        keep = ~(masks[0] | masks[1] | masks[2])
        Xf = X
    else:
        keep = ~masks[0]
        Xf = X.copy()
        fillv = 0.0 if policy == "zero" else 0.5
        Xf[masks[1], 0] = fillv
        Xf[masks[2], 1] = fillv
    _check_groups(orc, out, key[keep], Xf[keep], y[keep], True, "poisson")
    _, pred_ref = call_plugin(mock, "pl_glm_by_pred", _inputs(key[keep], Xf[keep], y[keep]), dict(kw, null_policy="raise"))
    assert pred.null_count == int((~keep).sum())
    assert pred.take(pa.array(np.flatnonzero(~keep))).null_count == int((~keep).sum())
    np.testing.assert_array_equal(pred.to_numpy(zero_copy_only=False)[keep], pred_ref.to_numpy(zero_copy_only=False))
    with pytest.raises(Exception, match="Nulls found in data"):
        call_plugin(mock, "pl_glm_by", _inputs(key, X, y, masks=masks), dict(kw, null_policy="raise"))


def test_plugin_glm_by_kwargs_errors(mock):
    from plugin_harness import PluginFailure, call_plugin

    rng = np.random.default_rng(8)
    key, X, y = _glm_frame(rng, [30, 30], 2)
    with pytest.raises(PluginFailure, match="unknown GLM family 'tweedie'"):
        call_plugin(mock, "pl_glm_by", _inputs(key, X, y), dict(GKW, family="tweedie"))
    with pytest.raises(PluginFailure, match="`max_iter` must be > 1."):
        call_plugin(mock, "pl_glm_by", _inputs(key, X, y), dict(GKW, max_iter=0))
    with pytest.raises(PluginFailure, match="up to 16 feature columns"):
        call_plugin(mock, "pl_glm_by", _inputs(key, np.tile(X, (1, 9))[:, :17], y), GKW)
    LKW = {"bias": True, "null_policy": "raise", "l1_reg": 0.0, "l2_reg": 0.0, "solver": "qr", "tol": 1e-5, "max_iter": 200}
    for bad in ({"l1_reg": 0.1}, {"l2_reg": 0.1}):
        with pytest.raises(PluginFailure, match="logistic_reg: l1_reg / l2_reg are not supported on this backend"):
            call_plugin(mock, "pl_logistic_coeffs", _inputs(None, X, y), dict(LKW, **bad))
    with pytest.raises(PluginFailure, match="Input `max_iter` must be a positive."):
        call_plugin(mock, "pl_logistic_pred", _inputs(None, X, y), dict(LKW, max_iter=0))


@pytest.mark.parametrize("bias", [True, False])
def test_plugin_logistic(mock, orc, bias):
    import pyarrow as pa
    from plugin_harness import call_plugin, output_field

    LKW = {"bias": bias, "null_policy": "raise", "l1_reg": 0.0, "l2_reg": 0.0, "solver": "qr", "tol": 1e-8, "max_iter": 200}
    rng = np.random.default_rng(9)
    _, X, y = _glm_frame(rng, [400], 3)
    assert output_field(mock, "pl_logistic_coeffs") == pa.field("coeffs", pa.large_list(pa.field("item", pa.float64())))
    assert output_field(mock, "pl_logistic_pred") == pa.field("pred", pa.float64())
    CALLS.clear()
    field, out = call_plugin(mock, "pl_logistic_coeffs", _inputs(None, X, y), LKW)
    assert CALLS == [("grouped", 400, 1)] and field.name == "coeffs" and len(out) == 1
    b, _ = orc.glm_irls(X, y, family="binomial", add_bias=bias, tol=1e-8, max_iter=200)
    np.testing.assert_allclose(np.asarray(out[0].as_py()), b, rtol=1e-12, atol=1e-12)
    fieldp, pred = call_plugin(mock, "pl_logistic_pred", _inputs(None, X, y), LKW)
    assert fieldp.name == "pred" and pred.null_count == 0
    eta = X @ b[:3] + (b[3] if bias else 0.0)
    np.testing.assert_allclose(pred.to_numpy(), gc.inv_link("binomial", eta), rtol=1e-12, atol=1e-12)
    # nulls: "skip" fits on the rows without one, pred is null where the mask drops a row
    masks = {0: np.zeros(400, bool), 2: np.zeros(400, bool)}
    masks[0][[3, 50]] = True
    masks[2][[50, 77, 200]] = True
    keep = ~(masks[0] | masks[2])
    _, out_s = call_plugin(mock, "pl_logistic_coeffs", _inputs(None, X, y, masks=masks), dict(LKW, null_policy="skip"))
    bs, _ = orc.glm_irls(X[keep], y[keep], family="binomial", add_bias=bias, tol=1e-8, max_iter=200)
    np.testing.assert_allclose(np.asarray(out_s[0].as_py()), bs, rtol=1e-12, atol=1e-12)
    _, pred_s = call_plugin(mock, "pl_logistic_pred", _inputs(None, X, y, masks=masks), dict(LKW, null_policy="skip"))
    assert pred_s.null_count == 4 and pred_s.take(pa.array(np.flatnonzero(~keep))).null_count == 4
    eta = X[keep] @ bs[:3] + (bs[3] if bias else 0.0)
    np.testing.assert_allclose(pred_s.to_numpy(zero_copy_only=False)[keep], gc.inv_link("binomial", eta), rtol=1e-12, atol=1e-12)
    with pytest.raises(Exception, match="Nulls found in data"):
        call_plugin(mock, "pl_logistic_coeffs", _inputs(None, X, y, masks=masks), LKW)
