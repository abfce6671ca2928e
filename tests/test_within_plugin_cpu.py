"""The fixed-effects report's Polars layer without a GPU: the plugin symbol pl_lin_reg_report_within on the mock device with a callback
bound to the reference (within_reference.py) -- field names, the null key as its own group, each null policy, the kwargs that reach
the C ABI -- and the routing of polars_exprs.lin_reg_report(absorb=)."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT))

import within_cases as wc  # noqa: E402
import within_reference as wr  # noqa: E402

FIELDS = ["features", "beta", None, "t", "p>|t|", "0.025", "0.975", "r2", "adj_r2"]
SE_FIELD = {"se": "std_err", "cluster": "cluster_se", "cluster0": "cluster0_se"}
SE_CODE = {"se": 0, "cluster": 5, "cluster0": 6}
CALLS = []  # (entry point, n_rows, groups or None, se_type, extra is null, max_groups or None) of every call the mock saw


@pytest.fixture(scope="module")
def mock():
    """The mock plugin library, the within entry points bound to callbacks that run the reference in float64."""
    from mock_device import device
    from polars_ds_extension_amd import _lib

    lib = device.load()
    keep = []

    def view(ptr, n, dt):
        return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(np.ctypeslib.as_ctypes_type(dt))), shape=(n,))

    def frame(cols_p, n_feat, n, dt):
        ptrs = C.cast(cols_p, C.POINTER(C.c_void_p))
        cols = [view(ptrs[c], n, dt).copy() for c in range(n_feat + 1)]
        return np.stack(cols[1:], axis=1).astype(np.float64), cols[0].astype(np.float64)

    def answer(X, y, codes, se_type, out_p, R, dt):
        if X.shape[1] > 16:
            lib.mock_set_error(b"fixed-effects regression: up to 16 feature columns")
            return -5
        g = len(np.unique(codes))
        if se_type != 0 and g < 2:
            lib.mock_set_error(b"standard errors clustered on the absorbed key need at least two non-empty groups")
            return -1
        if len(y) - g - X.shape[1] <= 0:
            lib.mock_set_error(b"fixed-effects regression: #rows - #groups - #features <= 0. No conclusive result.")
            return -3
        r = wr.report(X, y, codes, {v: k for k, v in SE_CODE.items()}[se_type], np.float64)
        out = C.cast(out_p, C.POINTER(R)).contents
        for k, rk in (("beta", "beta"), ("std_err", "std_err"), ("t", "t"), ("p", "p"), ("ci_lower", "ci_lo"), ("ci_upper", "ci_hi")):
            view(getattr(out, k), X.shape[1], dt)[:] = r[rk]
        out.r2, out.adj_r2 = float(r["r2"]), float(r["adj_r2"])
        return 0

    def make_grouped(dt, R):
        def fn(ctx, cols_p, n_feat, n, off_p, ng, space, se_type, out_p, extra_p):
            CALLS.append(("grouped", n, ng, se_type, not extra_p, None))
            X, y = frame(cols_p, n_feat, n, dt)
            off = view(off_p, ng + 1, np.int64)
            return answer(X, y, np.repeat(np.arange(ng), np.diff(off)), se_type, out_p, R, dt)

        return C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p)(fn)

    def make_by_key(dt, R):
        def fn(ctx, cols_p, keys_p, n_feat, n, space, se_type, max_groups, out_keys_p, out_p, extra_p, ng_p):
            CALLS.append(("by_key", n, None, se_type, not extra_p, max_groups))
            keys = view(keys_p, n, np.int64).copy()
            C.c_int64.from_address(ng_p).value = len(np.unique(keys))
            X, y = frame(cols_p, n_feat, n, dt)
            return answer(X, y, keys, se_type, out_p, R, dt)

        return C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_void_p,
                           C.c_void_p, C.c_void_p)(fn)

    for sfx, dt, R in (("f64", np.float64, _lib.ReportF64), ("f32", np.float32, _lib.ReportF32)):
        for name, cb in ((f"pds_lin_reg_within_grouped_{sfx}", make_grouped(dt, R)), (f"pds_lin_reg_within_by_key_{sfx}", make_by_key(dt, R))):
            keep.append(cb)
            getattr(lib, "mock_bind_" + name)(C.cast(cb, C.c_void_p))
    lib._within_report_keep = keep
    return lib


def _frame(p=3, shuffle=True, seed=43):
    rng = np.random.default_rng(seed)
    F, y, off, codes = wc.equal_frame(7, p)
    key = codes.astype(np.int64) * 9 - 30  # negative, sparse
    F, y = np.array(F), np.array(y)
    if shuffle:
        perm = rng.permutation(len(y))
        key, F, y = key[perm], F[perm], y[perm]
    return key, F, y


def _inputs(key, X, y, key_name="firm", dt=np.float64, key_mask=None, masks=None):
    import pyarrow as pa

    masks = masks or {}
    ins = [(key_name, pa.array(key, type=pa.int64(), mask=key_mask)), ("y", pa.array(y.astype(dt), mask=masks.get(0)))]
    ins += [(f"x{j + 1}", pa.array(X[:, j].astype(dt), mask=masks.get(j + 1))) for j in range(X.shape[1])]
    return ins


KW = {"bias": False, "null_policy": "raise", "std_err": "se", "solver": "qr", "l1_reg": 0.0, "l2_reg": 0.0, "tol": 0.0}


def _check(out, key, X, y, se, rtol=1e-12):
    names = [f"x{j + 1}" for j in range(X.shape[1])]
    want = wr.report(X, y, key, se, np.float64)
    fields = [SE_FIELD[se] if f is None else f for f in FIELDS]
    assert [f.name for f in out.type] == fields and len(out) == len(names)
    assert out.field(0).to_pylist() == names
    for i, rk in ((1, "beta"), (2, "std_err"), (3, "t"), (4, "p"), (5, "ci_lo"), (6, "ci_hi")):
        np.testing.assert_allclose(np.asarray(out.field(i).to_pylist(), dtype=np.float64), np.asarray(want[rk], dtype=np.float64), rtol=rtol, atol=0)
    for i, rk in ((7, "r2"), (8, "adj_r2")):
        np.testing.assert_allclose(np.asarray(out.field(i).to_pylist(), dtype=np.float64), np.full(len(names), float(want[rk])), rtol=rtol)
    return want


def test_plugin_schema_and_values(mock):
    import pyarrow as pa
    from plugin_harness import call_plugin, output_field

    fld = output_field(mock, "pl_lin_reg_report_within", [pa.field("firm", pa.int64()), pa.field("y", pa.float64())])
    assert fld.name == "lin_reg_report" and [f.name for f in fld.type] == ["features", "beta", "std_err", "t", "p>|t|", "0.025", "0.975", "r2", "adj_r2"]
    assert fld.type[0].type == pa.large_string() and all(fld.type[i].type == pa.float64() for i in range(1, 9))
    assert all(output_field(mock, "pl_lin_reg_report_within_f32").type[i].type == pa.float32() for i in range(1, 9))
    key, X, y = _frame()
    for se in ("se", "cluster", "cluster0"):
        CALLS.clear()
        field, out = call_plugin(mock, "pl_lin_reg_report_within", _inputs(key, X, y), dict(KW, std_err=se))
        # keys in any row order go to the by-key entry as they are; no effects asked for, so no extra block and no bound on the groups
        assert CALLS == [("by_key", len(y), None, SE_CODE[se], True, len(y))]
        assert field.name == "lin_reg_report" and field.type == out.type
        want = _check(out, key, X, y, se)
        assert want["n_groups"] == 7
    k2, X2, y2 = _frame(shuffle=False)
    _, out2 = call_plugin(mock, "pl_lin_reg_report_within", _inputs(k2, X2, y2), KW)
    _check(out2, k2, X2, y2, "se")
    _, out32 = call_plugin(mock, "pl_lin_reg_report_within_f32", _inputs(key, X, y, dt=np.float32), dict(KW, std_err="cluster"))
    assert out32.field(2).type == pa.float32() and out32.type[2].name == "cluster_se"
    _check(out32, key, X.astype(np.float32).astype(np.float64), y.astype(np.float32).astype(np.float64), "cluster", rtol=2e-6)


def test_plugin_null_key_is_its_own_group(mock):
    from plugin_harness import call_plugin

    key, X, y = _frame()
    mask = key == -12  # (keys -30, -21, -12, ...: the third group becomes the null key's)
    assert mask.sum() == 5
    _, out = call_plugin(mock, "pl_lin_reg_report_within", _inputs(key, X, y, key_mask=mask), dict(KW, std_err="cluster"))
    want = _check(out, key, X, y, "cluster")  # the same groups, whatever value stands in for the null key
    assert want["n_groups"] == 7
    mask2 = key != -30  # all keys null but one group's: two groups
    _, out = call_plugin(mock, "pl_lin_reg_report_within", _inputs(key, X, y, key_mask=mask2), KW)
    _check(out, np.where(mask2, 0, 1), X, y, "se")


@pytest.mark.parametrize("policy", ["skip", "zero"])
def test_plugin_null_policies(mock, policy):
    """frames with nulls are prepared on the host (rows in key order, the policy row by row, a dropped row leaves with its key) and go
    to the offsets entry point"""
    from plugin_harness import call_plugin

    key, X, y = _frame()
    n = len(y)
    rng = np.random.default_rng(9)
    masks = {0: rng.uniform(size=n) < 0.1, 2: rng.uniform(size=n) < 0.15}
    assert masks[0].any() and masks[2].any()
    CALLS.clear()
    _, out = call_plugin(mock, "pl_lin_reg_report_within", _inputs(key, X, y, masks=masks), dict(KW, null_policy=policy, std_err="cluster0"))
    if policy == "skip":
        keep, Xf = ~(masks[0] | masks[2]), X
    else:
        keep, Xf = ~masks[0], X.copy()
        Xf[masks[2], 1] = 0.0
    assert CALLS == [("grouped", int(keep.sum()), 7, SE_CODE["cluster0"], True, None)]
    order = np.argsort(key[keep], kind="stable")
    _check(out, key[keep][order], Xf[keep][order], y[keep][order], "cluster0")
    with pytest.raises(Exception, match="Nulls found in data"):
        call_plugin(mock, "pl_lin_reg_report_within", _inputs(key, X, y, masks=masks), KW)


def test_plugin_refusals(mock):
    from plugin_harness import call_plugin

    key, X, y = _frame()
    with pytest.raises(Exception, match="at least two non-empty groups"):
        call_plugin(mock, "pl_lin_reg_report_within", _inputs(np.zeros_like(key), X, y), dict(KW, std_err="cluster"))
    with pytest.raises(Exception, match="up to 16 feature columns"):
        call_plugin(mock, "pl_lin_reg_report_within", _inputs(key, np.tile(X, (1, 6))[:, :17], y), KW)
    with pytest.raises(Exception, match='std_err is "se", "cluster" or "cluster0"'):
        call_plugin(mock, "pl_lin_reg_report_within", _inputs(key, X, y), dict(KW, std_err="hc1"))
    with pytest.raises(Exception, match="the intercept is absorbed"):
        call_plugin(mock, "pl_lin_reg_report_within", _inputs(key, X, y), dict(KW, bias=True))
    with pytest.raises(Exception, match="need a key, a target and at least one feature"):
        call_plugin(mock, "pl_lin_reg_report_within", _inputs(key, X, y)[:2], KW)
    with pytest.raises(Exception, match="input columns differ in length"):
        ins = _inputs(key, X, y)
        ins[2] = ("x1", ins[2][1][:-1])
        call_plugin(mock, "pl_lin_reg_report_within", ins, KW)
    with pytest.raises(Exception, match="Empty data"):
        call_plugin(mock, "pl_lin_reg_report_within", _inputs(key[:0], X[:0], y[:0]), KW)


def test_polars_exprs_routing(mock):
    """polars_exprs.lin_reg_report(absorb=...) through the engine (the real polars if importable, else tests/mini_polars) and the
    pickled kwargs into pl_lin_reg_report_within on the mock device; the refusals of the builder."""
    from test_polars_exprs import pl, px

    key, X, y = _frame()
    df = pl.DataFrame({"firm": key, "y": y, "x1": X[:, 0], "x2": X[:, 1], "x3": X[:, 2]})
    before = px.PLUGIN_PATH
    px.PLUGIN_PATH = str(mock._name)
    try:
        for se in ("se", "cluster", "cluster0"):
            CALLS.clear()
            rep = df.select(px.lin_reg_report("x1", "x2", "x3", target="y", std_err=se, absorb="firm")).unnest("lin_reg_report")
            assert CALLS == [("by_key", len(y), None, SE_CODE[se], True, len(y))]
            assert rep.columns == ["features", "beta", SE_FIELD[se], "t", "p>|t|", "0.025", "0.975", "r2", "adj_r2"]
            want = wr.report(X, y, key, se, np.float64)
            assert rep["features"].to_list() == ["x1", "x2", "x3"]
            np.testing.assert_allclose(rep["beta"].to_numpy(), np.asarray(want["beta"], dtype=np.float64), rtol=1e-12)
            np.testing.assert_allclose(rep[SE_FIELD[se]].to_numpy(), np.asarray(want["std_err"], dtype=np.float64), rtol=1e-12)
            np.testing.assert_allclose(rep["p>|t|"].to_numpy(), want["p"], rtol=1e-12)
        dfn = pl.DataFrame({"firm": key, "y": y, "x1": [None] + list(X[1:, 0])})
        with pytest.raises(Exception, match="Nulls found in data"):
            dfn.select(px.lin_reg_report("x1", target="y", absorb="firm"))
        CALLS.clear()
        dfn.select(px.lin_reg_report("x1", target="y", absorb="firm", null_policy="skip"))
        assert CALLS[0][:2] == ("grouped", len(y) - 1)
    finally:
        px.PLUGIN_PATH = before
    with pytest.raises(NotImplementedError, match="together with `by` or `weights`"):
        px.lin_reg_report("x1", target="y", absorb="firm", by="g")
    with pytest.raises(NotImplementedError, match="together with `by` or `weights`"):
        px.lin_reg_report("x1", target="y", absorb="firm", weights="w")
    with pytest.raises(ValueError, match="the intercept is absorbed"):
        px.lin_reg_report("x1", target="y", absorb="firm", add_bias=True)
    with pytest.raises(ValueError, match='std_err="cluster" means the absorbed key'):
        px.lin_reg_report("x1", target="y", absorb="firm", std_err="cluster", cluster="firm")
    with pytest.raises(ValueError, match='std_err is "se", "cluster" or "cluster0"'):
        px.lin_reg_report("x1", target="y", absorb="firm", std_err="hc1")
