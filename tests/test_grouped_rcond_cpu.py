"""Grouped lin_reg_w_rcond without a GPU: the conditions on the inputs of tests/test_grouped_rcond_gpu.py, the C ABI surface of
pds_lr_rcond_grouped_* / _by_key_* (exports, header declarations, the mock builder's view of them), the argument validation of
lstsq.lin_reg_w_rcond_by / _by_key (before a device is touched), the plugin layer (pl_lr_w_rcond_by) on the mock device with its
entry points answered per group by oracle.solve_lr_rcond, and the polars_exprs builders on the mini engine."""
import ctypes as C
import inspect
import re
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT))

import rcond_cases as rc  # noqa: E402

NEW = ["pds_lr_rcond_grouped_f64", "pds_lr_rcond_grouped_f32", "pds_lr_rcond_by_key_f64", "pds_lr_rcond_by_key_f32"]
F32_EPS = float(np.finfo(np.float32).eps)


# ------------------------------------------------------------------------------------------------- the inputs of the GPU tests
@pytest.mark.parametrize("p", rc.WIDTHS)
def test_input_conditions(p):
    """Every group of the frames the GPU tests use: kept eigenvalues >= 10 thr, cut ones <= thr / 10, ev_max / ev_min_kept <= 1e4
    (asserted inside frame_conditions, group by group); for the f32 widths again with the f32 cut on the f32-rounded data."""
    for bias in (False, True):
        f = rc.width_frame(p, bias)
        assert f.n_groups == 8 * 4 + 1 - (8 if p == 1 and not bias else 0)
        kept, cut, cond = rc.frame_conditions(f)
        assert kept >= 10.0 and cut <= 0.1 and cond <= 1e4
        if p in (1, 4, 8, 16):
            rc.frame_conditions(f, F32_EPS, np.float32)


def test_reference_agrees_with_numpy_on_the_inputs():
    """the f64 eigen formula (oracle.solve_lr_rcond with the group's cut) and np.linalg.lstsq(rcond=1e-6) on the same groups"""
    from oracle import oracle as orc

    orc.build()
    for p, bias in ((1, True), (2, False), (9, True), (16, True)):
        f = rc.width_frame(p, bias)
        co, _ = rc.oracle_by(orc, f)
        ref, _ = rc.lstsq_by(f)
        assert np.max(np.abs(co - ref)) < 1e-12


# ------------------------------------------------------------------------------------------------- the C ABI surface
def test_exported_and_declared():
    from polars_ds_extension_amd import _lib

    assert all(n in _lib.EXPORTS for n in NEW)
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "pds_lstsq.h").read_text(), flags=re.S)
    for n in NEW:
        assert len(re.findall(rf"^int\s+{n}\s*\(", text, flags=re.M)) == 1, n
    csrc = ROOT / "polars_ds_extension_amd" / "csrc"
    assert "grouped_rcond.hip" in (csrc / "Makefile").read_text()
    assert '#include "capi_rcond_grouped.hpp"' in (csrc / "capi.hip").read_text()
    assert '#include "wave_tile_dev.hpp"' in (csrc / "grouped_rcond.hip").read_text()


def _mock_build():
    sys.path.insert(0, str(ROOT / "tests" / "mock_device"))
    try:
        import build as mock_build
    finally:
        sys.path.pop(0)
    return mock_build


def test_mock_trampolines_parse():
    protos = {name: args for _, name, args in _mock_build().prototypes()}
    assert [a for _, a in protos["pds_lr_rcond_grouped_f64"]] == ["ctx", "cols", "n_feat", "n_rows", "group_offsets", "n_groups", "space",
                                                                 "add_bias", "l2_reg", "rcond", "coeffs", "singular_values", "is_null"]
    assert [a for _, a in protos["pds_lr_rcond_by_key_f32"]] == ["ctx", "cols", "keys", "n_feat", "n_rows", "space", "add_bias", "l2_reg",
                                                                "rcond", "max_groups", "out_keys", "coeffs", "singular_values", "is_null",
                                                                "n_groups"]
    assert [t for t, _ in protos["pds_lr_rcond_grouped_f32"]][8:10] == ["float", "float"]
    assert [t for t, _ in protos["pds_lr_rcond_by_key_f64"]][7:9] == ["double", "double"]


def test_signatures_and_validation_without_a_device():
    """Every one of these raises before a context is created (no GPU here: reaching the device would raise something else)."""
    import polars_ds_extension_amd as pds
    from polars_ds_extension_amd import lstsq

    for n in ("lin_reg_w_rcond_by", "lin_reg_w_rcond_by_key"):
        assert callable(getattr(pds, n)) and n in lstsq.__all__
    sig = inspect.signature(pds.lin_reg_w_rcond_by)
    want = {"add_bias": False, "rcond": 0.0, "l2_reg": 0.0, "ctx": None}
    assert {k: sig.parameters[k].default for k in want} == want
    assert sig.parameters["group_offsets"].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters["target"].kind is inspect.Parameter.KEYWORD_ONLY
    sig = inspect.signature(pds.lin_reg_w_rcond_by_key)
    want = {"add_bias": False, "rcond": 0.0, "l2_reg": 0.0, "max_groups": None, "ctx": None}
    assert {k: sig.parameters[k].default for k in want} == want
    x = np.arange(12.0)
    y = x + 1.0
    off = np.array([0, 6, 12])
    with pytest.raises(NotImplementedError, match=re.escape("grouped lin_reg_w_rcond: up to 16 feature columns")):
        pds.lin_reg_w_rcond_by(*[x] * 17, target=y, group_offsets=off)
    with pytest.raises(NotImplementedError, match=re.escape("grouped lin_reg_w_rcond: up to 16 feature columns")):
        pds.lin_reg_w_rcond_by_key(*[x] * 17, target=y, key=np.zeros(12, dtype=np.int64))
    with pytest.raises(ValueError, match="at least one feature"):
        pds.lin_reg_w_rcond_by(target=y, group_offsets=off)
    with pytest.raises(ValueError, match="at least one feature"):
        pds.lin_reg_w_rcond_by_key(target=y, key=np.zeros(12, dtype=np.int64))
    with pytest.raises(TypeError):
        pds.lin_reg_w_rcond_by(x, target=y)  # group_offsets is required


# ------------------------------------------------------------------------------------------------- the plugin layer on the mock device
CALLS = []  # (entry point, n_rows, groups or max_groups) of every grouped rcond call the mock saw


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle

    oracle.build()
    return oracle


@pytest.fixture(scope="module")
def mock(orc):
    """The mock plugin library, pds_lr_rcond_{grouped,by_key}_* bound to callbacks that run oracle.solve_lr_rcond on every group with
    the group's own cut max(rcond, eps_T max(n_g, p'))."""
    from mock_device import device

    lib = device.load()
    keep = []

    def view(ptr, n, dt):
        return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(np.ctypeslib.as_ctypes_type(dt))), shape=(n,))

    def frame(cols_p, n_feat, n, dt):
        ptrs = C.cast(cols_p, C.POINTER(C.c_void_p))
        cols = [view(ptrs[c], n, dt).copy() for c in range(n_feat + 1)]
        return np.stack(cols[1:], axis=1), cols[0]

    def fill(X, y, off, bias, l2, rcond, co_p, sv_p, nu_p, dt):
        ng = len(off) - 1
        pp = X.shape[1] + int(bool(bias))
        co, sv, nu = view(co_p, ng * pp, dt).reshape(ng, pp), view(sv_p, ng * pp, dt).reshape(ng, pp), view(nu_p, ng, np.uint8)
        for g in range(ng):
            s, e = int(off[g]), int(off[g + 1])
            A = rc.design(X[s:e].astype(np.float64), bias)
            ok = e - s >= pp and np.isfinite(A).all() and np.isfinite(y[s:e]).all()
            if ok:
                with np.errstate(all="ignore"):
                    b, sg = orc.solve_lr_rcond(A, y[s:e].astype(np.float64), float(l2), bool(bias),
                                               rc.rcond_g(e - s, pp, float(np.finfo(dt).eps), float(rcond)))
                ok = bool(np.isfinite(b).all())
            co[g], sv[g], nu[g] = (b, sg, 0) if ok else (np.nan, np.nan, 1)

    def make_grouped(dt, ct):
        def fn(ctx, cols_p, n_feat, n, off_p, ng, space, bias, l2, rcond, co_p, sv_p, nu_p):
            CALLS.append(("grouped", n, ng))
            X, y = frame(cols_p, n_feat, n, dt)
            fill(X, y, view(off_p, ng + 1, np.int64).copy(), bias, l2, rcond, co_p, sv_p, nu_p, dt)
            return 0

        return C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_int, ct, ct, C.c_void_p,
                           C.c_void_p, C.c_void_p)(fn)

    def make_by_key(dt, ct):
        def fn(ctx, cols_p, keys_p, n_feat, n, space, bias, l2, rcond, max_groups, ok_p, co_p, sv_p, nu_p, ng_p):
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
            fill(X[order], y[order], np.concatenate([[0], np.cumsum(counts)]), bias, l2, rcond, co_p, sv_p, nu_p, dt)
            return 0

        return C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_int, ct, ct, C.c_int64, C.c_void_p,
                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)(fn)

    for sfx, dt, ct in (("f64", np.float64, C.c_double), ("f32", np.float32, C.c_float)):
        for name, cb in ((f"pds_lr_rcond_grouped_{sfx}", make_grouped(dt, ct)), (f"pds_lr_rcond_by_key_{sfx}", make_by_key(dt, ct))):
            keep.append(cb)
            getattr(lib, "mock_bind_" + name)(C.cast(cb, C.c_void_p))
    lib._rcond_keep = keep
    return lib


KW = {"bias": True, "null_policy": "raise", "l1_reg": 0.0, "l2_reg": 0.0, "solver": "", "tol": rc.RCOND}  # what lin_reg_w_rcond sends
KINDS_OF = ("full", "dup", "const", "zero", "full")


def _keyed_frame(rng, sizes, p, bias=True, shuffle=True, dt=np.float64):
    """groups of the given sizes and kinds full / dup / const / zero / full ..., keys 7 g - 20 (ascending key order is not the order of
    first appearance), rows shuffled"""
    gs = [rc.group(rng, n, p, bias, KINDS_OF[k % len(KINDS_OF)]) for k, n in enumerate(sizes)]
    X = np.concatenate([g[0] for g in gs])
    y = np.concatenate([g[1] for g in gs])
    key = np.repeat(np.arange(len(sizes), dtype=np.int64) * 7 - 20, sizes)
    if shuffle:
        perm = rng.permutation(len(y))
        key, X, y = key[perm], X[perm], y[perm]
    return key, X, y


def _inputs(key, X, y, key_name="k", dt=np.float64, key_mask=None, masks=None):
    import pyarrow as pa

    masks = masks or {}
    ins = [(key_name, pa.array(key, type=pa.int64(), mask=key_mask))]
    ins.append(("y", pa.array(y.astype(dt), mask=masks.get(0))))
    ins += [(f"x{j + 1}", pa.array(X[:, j].astype(dt), mask=masks.get(j + 1))) for j in range(X.shape[1])]
    return ins


def _check_groups(orc, out, key, X, y, bias, null_last=None, l2=0.0, eps=np.finfo(np.float64).eps, tol=1e-12):
    got_keys = out.field(0).to_pylist()
    uniq = sorted(set(int(k) for k in key if null_last is None or k != null_last))
    assert got_keys == uniq + ([None] if null_last is not None else [])  # ascending, the null key's group last
    co, sv = out.field(1), out.field(2)
    pp = X.shape[1] + int(bias)
    for gi, k in enumerate(uniq + ([null_last] if null_last is not None else [])):
        rows = np.flatnonzero(key == k)
        A = rc.design(X[rows], bias)
        if len(rows) < pp or not (np.isfinite(A).all() and np.isfinite(y[rows]).all()):
            assert not co[gi].is_valid and not sv[gi].is_valid  # a null group: null lists
            continue
        b, s = orc.solve_lr_rcond(A, y[rows], l2, bool(bias), rc.rcond_g(len(rows), pp, eps))
        assert co[gi].is_valid and sv[gi].is_valid
        np.testing.assert_allclose(np.asarray(co[gi].as_py()), b, rtol=tol, atol=tol)
        np.testing.assert_allclose(np.asarray(sv[gi].as_py()), s, rtol=tol, atol=tol)


def test_plugin_rcond_by(mock, orc):
    import pyarrow as pa
    from plugin_harness import call_plugin, output_field

    rng = np.random.default_rng(5)
    sizes = [60, 3, 45, 80, 50]  # group 1 (key -13): 3 rows < p' = 4 -> null lists
    key, X, y = _keyed_frame(rng, sizes, 3)
    fld = output_field(mock, "pl_lr_w_rcond_by", [pa.field("k", pa.int64()), pa.field("y", pa.float64())])
    assert [f.name for f in fld.type] == ["k", "coeffs", "singular_values"]
    assert [f.type for f in fld.type] == [pa.int64(), pa.large_list(pa.float64()), pa.large_list(pa.float64())]
    assert output_field(mock, "pl_lr_w_rcond_by_f32").type[2].type == pa.large_list(pa.float32())
    CALLS.clear()
    field, out = call_plugin(mock, "pl_lr_w_rcond_by", _inputs(key, X, y), KW)
    assert [f.name for f in out.type] == ["k", "coeffs", "singular_values"] and len(out) == len(sizes)
    assert CALLS == [("by_key", len(y), len(y))]  # one call, the whole frame
    _check_groups(orc, out, key, X, y, True)
    assert [c.is_valid for c in out.field(1)] == [True, False, True, True, True]
    # an unnamed key column: "key"; no bias, a penalty
    _, out2 = call_plugin(mock, "pl_lr_w_rcond_by", _inputs(key, X, y, key_name=""), dict(KW, bias=False, l2_reg=0.5))
    assert out2.type[0].name == "key"
    _check_groups(orc, out2, key, X, y, False, l2=0.5)
    # the f32 twin: the cut uses f32's epsilon
    _, out3 = call_plugin(mock, "pl_lr_w_rcond_by_f32", _inputs(key, X, y, dt=np.float32), KW)
    assert out3.type[1].type == pa.large_list(pa.float32())
    _check_groups(orc, out3, key, X.astype(np.float32).astype(np.float64), y.astype(np.float32).astype(np.float64), True, eps=F32_EPS, tol=1e-5)


def test_plugin_rcond_by_null_keys_and_capacity_retry(mock, orc):
    from plugin_harness import call_plugin

    rng = np.random.default_rng(6)
    key, X, y = _keyed_frame(rng, [50, 40, 45], 2)
    mask = key == -13  # the middle key's rows become the null group
    stand_in = int(key.max()) + 1
    _, out = call_plugin(mock, "pl_lr_w_rcond_by", _inputs(key, X, y, key_mask=mask), KW)
    _check_groups(orc, out, np.where(mask, stand_in, key), X, y, True, null_last=stand_in)
    # the capacity guess is too small: one retry with the device's count
    mock.pds_plugin_debug_rcond_by_first_cap(C.c_longlong(2))
    try:
        CALLS.clear()
        _, out = call_plugin(mock, "pl_lr_w_rcond_by", _inputs(key, X, y), KW)
        assert CALLS == [("by_key", len(y), 2), ("by_key", len(y), 3)]
        _check_groups(orc, out, key, X, y, True)
    finally:
        mock.pds_plugin_debug_rcond_by_first_cap(C.c_longlong(0))


@pytest.mark.parametrize("policy", ["skip", "zero", "0.5", "ignore"])
def test_plugin_rcond_by_null_policies(mock, orc, policy):
    """Every policy against a frame prepared by hand: skip = rows with a null removed, fill = features filled and rows with a null
    target removed, ignore = the rows kept with NaN (that group is a null group); "raise" is the single call's error."""
    from plugin_harness import call_plugin

    rng = np.random.default_rng(7)
    key, X, y = _keyed_frame(rng, [70, 60, 65], 2)
    n = len(y)
    masks = {0: np.zeros(n, bool), 1: np.zeros(n, bool), 2: np.zeros(n, bool)}
    first = key == -20
    masks[0][np.flatnonzero(first)[:3]] = True  # nulls of the target, of x1 and of x2 in the first key's group only
    masks[1][np.flatnonzero(first)[5:9]] = True
    masks[2][np.flatnonzero(first)[7:11]] = True
    kw = dict(KW, null_policy=policy)
    CALLS.clear()
    _, out = call_plugin(mock, "pl_lr_w_rcond_by", _inputs(key, X, y, masks=masks), kw)
    assert [c[0] for c in CALLS] == ["grouped"]  # rows prepared on the host, the offsets entry point
    if policy == "ignore":
        assert out.field(0).to_pylist() == [-20, -13, -6]
        assert [c.is_valid for c in out.field(1)] == [False, True, True] and [c.is_valid for c in out.field(2)] == [False, True, True]
    else:
        if policy == "skip":
            keep = ~(masks[0] | masks[1] | masks[2])
            Xf = X
        else:
            keep = ~masks[0]
            Xf = X.copy()
            fillv = 0.0 if policy == "zero" else 0.5
            Xf[masks[1], 0] = fillv
            Xf[masks[2], 1] = fillv
        assert CALLS == [("grouped", int(keep.sum()), 3)]
        _check_groups(orc, out, key[keep], Xf[keep], y[keep], True)
    with pytest.raises(Exception, match="Nulls found in data"):
        call_plugin(mock, "pl_lr_w_rcond_by", _inputs(key, X, y, masks=masks), dict(kw, null_policy="raise"))


def test_plugin_rcond_by_argument_errors(mock):
    from plugin_harness import PluginFailure, call_plugin

    rng = np.random.default_rng(8)
    key, X, y = _keyed_frame(rng, [30, 30], 2)
    with pytest.raises(PluginFailure, match="up to 16 feature columns"):
        call_plugin(mock, "pl_lr_w_rcond_by", _inputs(key, np.tile(X, (1, 9))[:, :17], y), KW)
    with pytest.raises(PluginFailure, match="needs a key, a target and at least one feature"):
        call_plugin(mock, "pl_lr_w_rcond_by", _inputs(key, X, y)[:2], KW)


# ------------------------------------------------------------------------------------------------- polars_exprs on the mini engine
def test_polars_exprs_build_the_plugin_call(mock, orc):
    from test_polars_exprs import pl  # (the real polars if importable, else tests/mini_polars)

    from polars_ds_extension_amd import polars_exprs as px

    sig = inspect.signature(px.lin_reg_w_rcond)
    want = {"add_bias": False, "rcond": 0.0, "l2_reg": 0.0, "null_policy": "raise", "by": None}
    assert {k: sig.parameters[k].default for k in want} == want
    with pytest.raises(NotImplementedError, match="up to 16 feature columns"):
        px.lin_reg_w_rcond(*[f"x{j}" for j in range(17)], target="y", by="k")
    old = px.PLUGIN_PATH
    px.PLUGIN_PATH = Path(mock._name)
    try:
        rng = np.random.default_rng(12)
        sizes = [80, 2, 70, 90]  # (key -13: 2 rows < p' = 3 -> a null group)
        key, X, y = _keyed_frame(rng, sizes, 2)
        df = pl.DataFrame({"k": key, "y": y, "x1": X[:, 0], "x2": X[:, 1]})
        CALLS.clear()
        res = df.select(px.lin_reg_w_rcond("x1", "x2", target="y", add_bias=True, rcond=rc.RCOND, by="k")).unnest("rcond_by")
        assert CALLS == [("by_key", len(y), len(y))]
        assert res.columns == ["k", "coeffs", "singular_values"] and res["k"].to_list() == [-20, -13, -6, 1]
        for k, co, sv in zip(res["k"].to_list(), res["coeffs"].to_list(), res["singular_values"].to_list()):
            rows = key == k
            if rows.sum() < 3:
                assert co is None and sv is None
                continue
            b, s = orc.solve_lr_rcond(rc.design(X[rows], True), y[rows], 0.0, True, rc.rcond_g(int(rows.sum()), 3))
            np.testing.assert_allclose(co, b, rtol=1e-12, atol=1e-12)
            np.testing.assert_allclose(sv, s, rtol=1e-12, atol=1e-12)
        r1 = px.lin_reg_w_rcond_by_group(df, "k", "x1", "x2", target="y", add_bias=True, rcond=rc.RCOND)
        assert r1.columns == ["k", "coeffs", "singular_values"] and r1["k"].to_list() == [-20, -13, -6, 1]
        assert r1["coeffs"].to_list() == res["coeffs"].to_list()
        # keys of another dtype: order of first appearance, one row per distinct key
        names = np.array(["oak", "elm", "ash", "fir"])[(key + 20) // 7]
        d2 = pl.DataFrame({"tree": names.tolist(), "y": y, "x1": X[:, 0], "x2": X[:, 1]})
        r2 = px.lin_reg_w_rcond_by_group(d2, "tree", "x1", "x2", target="y", add_bias=True, rcond=rc.RCOND)
        assert r2.columns == ["tree", "coeffs", "singular_values"] and r2["tree"].to_list() == list(dict.fromkeys(names.tolist()))
        by_name = dict(zip(r2["tree"].to_list(), r2["coeffs"].to_list()))
        by_key = dict(zip(res["k"].to_list(), res["coeffs"].to_list()))
        for t, k in zip(("oak", "elm", "ash", "fir"), (-20, -13, -6, 1)):
            assert by_name[t] == by_key[k]
        # without `by` the function is the single call it was
        CALLS.clear()
        one = df.select(px.lin_reg_w_rcond("x1", "x2", target="y", add_bias=True, rcond=rc.RCOND))
        assert CALLS == [] and len(one) == 1
    finally:
        px.PLUGIN_PATH = old
