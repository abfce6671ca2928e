"""The grouped multi-target fit without a GPU: the conditions on the inputs of tests/test_grouped_multi_gpu.py (every group's gate
statistic, in NumPy, at least 1e3 away from 1 / singular_x_tol on its side), the C ABI surface of pds_lr_multi_grouped_* / _by_key_*
(exports, header declarations, the mock builder's view of them), the argument validation of lstsq.lin_reg_multi_by / _by_key (before a
device is touched), the plugin layer (pl_lr_multi_by / pl_lr_multi_by_pred) on the mock device with its entry points answered per
group and per target by oracle.solve_lr_gated, and the polars_exprs builders on the mini engine."""
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

import multi_cases as mc  # noqa: E402

NEW = ["pds_lr_multi_grouped_f64", "pds_lr_multi_grouped_f32", "pds_lr_multi_by_key_f64", "pds_lr_multi_by_key_f32"]
LIMIT = "grouped multi-target lin_reg: up to 16 feature columns and 15 targets"
SOLVER_NAMES = {0: "qr", 1: "svd", 2: "choleskey"}


# ------------------------------------------------------------------------------------------------- the inputs of the GPU tests
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("p,k", mc.PAIRS)
def test_input_conditions(p, k, bias):
    """Every full-rank group's pivot-ratio product lies at least 1e3 below 1 / tol and every degenerate group's at least 1e3 beyond it
    (or its factorisation breaks down): f64 frames, the ridge run (where no kind is degenerate any more) and the f32-rounded frames."""
    f = mc.pair_frame(p, k, bias)
    sizes = {f.n_of(g) for g in range(f.n_groups)}
    assert {0, 1, f.pp, f.pp + 1, 63, 64, 65, 128, 129, 200} <= sizes and set(f.kinds) == set(mc.KINDS)
    assert k == 1 or not f.T[:, k - 1].any()  # one target is identically zero
    for dtype, l2 in ((np.float64, 0.0), (np.float64, 0.1), (np.float32, 0.0)):
        fitted, gated = mc.frame_gate_margins(f, dtype, l2)
        assert fitted <= 1e-3 and gated >= 1e3, (dtype, l2, fitted, gated)
    assert any(f.expect_null(g) and f.n_of(g) >= f.pp for g in range(f.n_groups)) == (p >= 2 or bias)


def test_oracle_reference_nulls_by_construction():
    from oracle import oracle as orc

    orc.build()
    for p, k, bias in ((2, 2, True), (7, 3, False)):
        f = mc.pair_frame(p, k, bias)
        co, nu = mc.oracle_by(orc, f)
        assert np.array_equal(nu, [f.expect_null(g) for g in range(f.n_groups)])
        g = next(g for g in range(f.n_groups) if not nu[g] and f.n_of(g) == 200)
        ref = np.linalg.lstsq(mc.design(f.X[f.rows(g)], bias), f.T[f.rows(g)], rcond=None)[0].T
        assert np.max(np.abs(co[g] - ref)) < 1e-12


# ------------------------------------------------------------------------------------------------- the C ABI surface
def test_exported_and_declared():
    from polars_ds_extension_amd import _lib

    assert all(n in _lib.EXPORTS for n in NEW)
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "pds_lstsq.h").read_text(), flags=re.S)
    for n in NEW:
        assert len(re.findall(rf"^int\s+{n}\s*\(", text, flags=re.M)) == 1, n
    csrc = ROOT / "polars_ds_extension_amd" / "csrc"
    assert "grouped_multi.hip" in (csrc / "Makefile").read_text()
    assert '#include "capi_multi_grouped.hpp"' in (csrc / "capi.hip").read_text()
    assert '#include "wave_tile_dev.hpp"' in (csrc / "grouped_multi.hip").read_text()
    assert '#include "plugin_multi_by.hpp"' in (csrc / "plugin.cpp").read_text()
    assert LIMIT in (csrc / "capi_multi_grouped.hpp").read_text()


def _mock_build():
    sys.path.insert(0, str(ROOT / "tests" / "mock_device"))
    try:
        import build as mock_build
    finally:
        sys.path.pop(0)
    return mock_build


def test_mock_trampolines_parse():
    protos = {name: args for _, name, args in _mock_build().prototypes()}
    grouped = ["ctx", "cols", "n_targets", "n_feat", "n_rows", "group_offsets", "n_groups", "space", "add_bias", "l2_reg", "solver",
               "singular_x_tol", "coeffs", "is_null", "pred", "resid", "row_null"]
    by_key = ["ctx", "cols", "keys", "n_targets", "n_feat", "n_rows", "space", "add_bias", "l2_reg", "solver", "singular_x_tol", "max_groups",
              "out_keys", "coeffs", "is_null", "n_groups", "pred", "resid", "row_null"]
    for sfx, real in (("f64", "double"), ("f32", "float")):
        assert [a for _, a in protos[f"pds_lr_multi_grouped_{sfx}"]] == grouped
        assert [a for _, a in protos[f"pds_lr_multi_by_key_{sfx}"]] == by_key
        tg = [t for t, _ in protos[f"pds_lr_multi_grouped_{sfx}"]]
        assert (tg[9], tg[10], tg[11]) == (real, "int", real) and tg[12] == f"{real}*" and tg[13] == "uint8_t*"
        tk = [t for t, _ in protos[f"pds_lr_multi_by_key_{sfx}"]]
        assert (tk[8], tk[9], tk[10], tk[11]) == (real, "int", real, "int64_t") and tk[15] == "int64_t*"


def test_signatures_and_validation_without_a_device():
    """Every one of these raises before a context is created (no GPU here: reaching the device would raise something else)."""
    import polars_ds_extension_amd as pds
    from polars_ds_extension_amd import lstsq

    for n in ("lin_reg_multi_by", "lin_reg_multi_by_key"):
        assert callable(getattr(pds, n)) and n in lstsq.__all__
    sig = inspect.signature(pds.lin_reg_multi_by)
    want = {"add_bias": False, "l2_reg": 0.0, "solver": "qr", "singular_x_tol": None, "return_pred": False, "ctx": None}
    assert {k: sig.parameters[k].default for k in want} == want
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("targets", "group_offsets"))
    assert "l1_reg" not in sig.parameters and "positive" not in sig.parameters  # not part of the multi-target call, as in the reference
    sig = inspect.signature(pds.lin_reg_multi_by_key)
    want["max_groups"] = None
    assert {k: sig.parameters[k].default for k in want} == want
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("targets", "key"))
    x = np.arange(12.0)
    off = np.array([0, 6, 12])
    key = np.zeros(12, dtype=np.int64)
    for call in (lambda *a, **kw: pds.lin_reg_multi_by(*a, group_offsets=off, **kw), lambda *a, **kw: pds.lin_reg_multi_by_key(*a, key=key, **kw)):
        with pytest.raises(NotImplementedError, match=re.escape(LIMIT)):
            call(*[x] * 17, targets=[x, x])
        with pytest.raises(NotImplementedError, match=re.escape(LIMIT)):
            call(x, targets=[x] * 16)
        with pytest.raises(ValueError, match="cannot be empty"):
            call(x, targets=[])
        with pytest.raises(ValueError, match="at least one feature"):
            call(targets=[x, x])
        with pytest.raises(TypeError):
            call(x, targets=x)
    with pytest.raises(TypeError):
        pds.lin_reg_multi_by(x, targets=[x, x])  # group_offsets is required


# ------------------------------------------------------------------------------------------------- the plugin layer on the mock device
CALLS = []  # (entry point, n_rows, n_targets, n_feat, groups or max_groups) of every grouped multi-target call the mock saw


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle

    oracle.build()
    return oracle


def _fit_group(orc, X, T, bias, l2=0.0, solver="qr", tol=1e-12):
    """coefficients [k, p'] of one group by the oracle, None for a null group"""
    pp = X.shape[1] + int(bool(bias))
    A = mc.design(X.astype(np.float64), bias)
    if len(A) < pp or not (np.isfinite(A).all() and np.isfinite(T).all()):
        return None
    b = orc.solve_lr_gated(A, T.astype(np.float64), float(l2), bool(bias), solver, float(tol))
    return None if b is None else np.asarray(b).reshape(pp, T.shape[1]).T


@pytest.fixture(scope="module")
def mock(orc):
    """The mock plugin library, pds_lr_multi_{grouped,by_key}_* bound to callbacks that answer per group and per target with
    oracle.solve_lr_gated."""
    from mock_device import device

    lib = device.load()
    keep = []

    def view(ptr, n, dt):
        return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(np.ctypeslib.as_ctypes_type(dt))), shape=(n,))

    def frame(cols_p, k, p, n, dt):
        ptrs = C.cast(cols_p, C.POINTER(C.c_void_p))
        cols = [view(ptrs[c], n, dt).copy() for c in range(k + p)]
        return np.stack(cols[k:], axis=1), np.stack(cols[:k], axis=1)

    def fill(X, T, off, bias, l2, solver, tol, co_p, nu_p, pr_p, rs_p, rn_p, rows_of, dt):
        """rows_of[i]: the caller's row of row i of the ordered frame"""
        ng, k, n = len(off) - 1, T.shape[1], len(X)
        pp = X.shape[1] + int(bool(bias))
        co = view(co_p, ng * k * pp, dt).reshape(ng, k, pp) if co_p else None
        nu = view(nu_p, ng, np.uint8) if nu_p else None
        pred = view(pr_p, k * n, dt).reshape(k, n) if pr_p else None
        resid = view(rs_p, k * n, dt).reshape(k, n) if rs_p else None
        rn = view(rn_p, n, np.uint8) if rn_p else None
        for g in range(ng):
            s, e = int(off[g]), int(off[g + 1])
            b = _fit_group(orc, X[s:e], T[s:e], bias, l2, SOLVER_NAMES[solver], tol)
            if co is not None:
                co[g] = np.nan if b is None else b
                nu[g] = b is None
            rows = rows_of[s:e]
            fitted = np.nan if b is None else mc.design(X[s:e].astype(np.float64), bias) @ b.T  # [n_g, k]
            for arr, val in ((pred, fitted), (resid, T[s:e] - fitted)):
                if arr is not None:
                    arr[:, rows] = np.broadcast_to(val, (e - s, k)).T
            if rn is not None:
                rn[rows] = b is None

    def make_grouped(dt, ct):
        def fn(ctx, cols_p, k, p, n, off_p, ng, space, bias, l2, solver, tol, co_p, nu_p, pr_p, rs_p, rn_p):
            CALLS.append(("grouped", n, k, p, ng))
            X, T = frame(cols_p, k, p, n, dt)
            fill(X, T, view(off_p, ng + 1, np.int64).copy(), bias, l2, solver, tol, co_p, nu_p, pr_p, rs_p, rn_p, np.arange(n), dt)
            return 0

        return C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_int, ct, C.c_int, ct,
                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)(fn)

    def make_by_key(dt, ct):
        def fn(ctx, cols_p, keys_p, k, p, n, space, bias, l2, solver, tol, max_groups, ok_p, co_p, nu_p, ng_p, pr_p, rs_p, rn_p):
            CALLS.append(("by_key", n, k, p, max_groups))
            keys = view(keys_p, n, np.int64)
            order = np.argsort(keys, kind="stable")
            uniq, counts = np.unique(keys[order], return_counts=True)
            if ng_p:
                C.c_int64.from_address(ng_p).value = len(uniq)
            if len(uniq) > max_groups:
                lib.mock_set_error(b"more distinct keys than max_groups")
                return -1
            X, T = frame(cols_p, k, p, n, dt)
            if ok_p:
                view(ok_p, len(uniq), np.int64)[:] = uniq
            fill(X[order], T[order], np.concatenate([[0], np.cumsum(counts)]), bias, l2, solver, tol, co_p, nu_p, pr_p, rs_p, rn_p, order, dt)
            return 0

        return C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_int, C.c_int, ct, C.c_int, ct, C.c_int64,
                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)(fn)

    for sfx, dt, ct in (("f64", np.float64, C.c_double), ("f32", np.float32, C.c_float)):
        for name, cb in ((f"pds_lr_multi_grouped_{sfx}", make_grouped(dt, ct)), (f"pds_lr_multi_by_key_{sfx}", make_by_key(dt, ct))):
            keep.append(cb)
            getattr(lib, "mock_bind_" + name)(C.cast(cb, C.c_void_p))
    lib._multi_keep = keep
    return lib


def _kw(k, **over):  # what lin_reg(target=[..]) sends
    return dict({"bias": True, "null_policy": "raise", "solver": "qr", "last_target_idx": k, "l2_reg": 0.0, "singular_x_tol": 1e-12}, **over)


KINDS_OF = ("full", "dup", "full", "full", "const")


def _keyed_frame(rng, sizes, p, k, bias=True, shuffle=True):
    """groups of the given sizes and kinds full / dup / full / full / const ..., keys 7 g - 20, rows shuffled"""
    gs = [mc.group(rng, n, p, k, bias, KINDS_OF[i % len(KINDS_OF)]) for i, n in enumerate(sizes)]
    X = np.concatenate([g[0] for g in gs])
    T = np.concatenate([g[1] for g in gs])
    key = np.repeat(np.arange(len(sizes), dtype=np.int64) * 7 - 20, sizes)
    if shuffle:
        perm = rng.permutation(len(key))
        key, X, T = key[perm], X[perm], T[perm]
    return key, X, T


def _inputs(key, X, T, names=("ta", "tb", "tc"), key_name="k", dt=np.float64, key_mask=None, masks=None):
    import pyarrow as pa

    masks = masks or {}
    k = T.shape[1]
    ins = [(key_name, pa.array(key, type=pa.int64(), mask=key_mask))]
    ins += [(names[t], pa.array(T[:, t].astype(dt), mask=masks.get(t))) for t in range(k)]
    ins += [(f"x{j + 1}", pa.array(X[:, j].astype(dt), mask=masks.get(k + j))) for j in range(X.shape[1])]
    return ins


def _check_groups(orc, out, key, X, T, bias, names, null_last=None, l2=0.0, tol=1e-12, gate=1e-12):
    got_keys = out.field(0).to_pylist()
    uniq = sorted(set(int(v) for v in key if null_last is None or v != null_last))
    assert got_keys == uniq + ([None] if null_last is not None else [])  # ascending, the null key's group last
    assert [f.name for f in out.type][1:] == list(names[:T.shape[1]])
    nulls = []
    for gi, kv in enumerate(uniq + ([null_last] if null_last is not None else [])):
        rows = np.flatnonzero(key == kv)
        b = _fit_group(orc, X[rows], T[rows], bias, l2, "qr", gate)
        nulls.append(b is None)
        for t in range(T.shape[1]):
            cell = out.field(1 + t)[gi]
            assert cell.is_valid == (b is not None)  # a null group: a null list in EVERY target field
            if b is not None:
                np.testing.assert_allclose(np.asarray(cell.as_py()), b[t], rtol=tol, atol=tol)
    return nulls


def test_plugin_multi_by(mock, orc):
    import pyarrow as pa
    from plugin_harness import call_plugin, output_field

    rng = np.random.default_rng(5)
    sizes = [60, 50, 3, 45, 80]  # key -13: a duplicated column (gated); key -6: 3 rows < p' = 4; key 8: a constant column beside the bias
    key, X, T = _keyed_frame(rng, sizes, 3, 2)
    fld = output_field(mock, "pl_lr_multi_by", [pa.field("k", pa.int64()), pa.field("ta", pa.float64())])
    assert fld.type[0].name == "k" and fld.type[0].type == pa.int64()
    assert output_field(mock, "pl_lr_multi_by_f32", [pa.field("k", pa.int64())]).type[1].type == pa.large_list(pa.float32())
    assert [f.name for f in output_field(mock, "pl_lr_multi_by_pred").type] == ["pred", "resid"]
    CALLS.clear()
    _, out = call_plugin(mock, "pl_lr_multi_by", _inputs(key, X, T), _kw(2))
    assert [f.name for f in out.type] == ["k", "ta", "tb"] and len(out) == len(sizes)
    assert [f.type for f in out.type] == [pa.int64(), pa.large_list(pa.float64()), pa.large_list(pa.float64())]
    assert CALLS == [("by_key", len(key), 2, 3, len(key))]  # ONE call: the whole frame, both targets
    assert _check_groups(orc, out, key, X, T, True, ("ta", "tb")) == [False, True, True, False, True]
    # an unnamed key column: "key"; no bias, a penalty (the duplicated column is then regular), three targets
    key3, X3, T3 = _keyed_frame(rng, sizes, 3, 3)
    _, out2 = call_plugin(mock, "pl_lr_multi_by", _inputs(key3, X3, T3, key_name=""), _kw(3, bias=False, l2_reg=0.5))
    assert out2.type[0].name == "key"
    assert _check_groups(orc, out2, key3, X3, T3, False, ("ta", "tb", "tc"), l2=0.5) == [False] * 5
    # the f32 twin
    _, out3 = call_plugin(mock, "pl_lr_multi_by_f32", _inputs(key, X, T, dt=np.float32), _kw(2, singular_x_tol=1e-6))
    assert out3.type[1].type == pa.large_list(pa.float32())
    r32 = lambda a: a.astype(np.float32).astype(np.float64)  # noqa: E731
    _check_groups(orc, out3, key, r32(X), r32(T), True, ("ta", "tb"), tol=1e-5, gate=1e-6)


def test_plugin_multi_by_null_keys_and_capacity_retry(mock, orc):
    from plugin_harness import call_plugin

    rng = np.random.default_rng(6)
    key, X, T = _keyed_frame(rng, [50, 40, 45], 2, 2)
    mask = key == -13  # the middle key's rows become the null group
    stand_in = int(key.max()) + 1
    _, out = call_plugin(mock, "pl_lr_multi_by", _inputs(key, X, T, key_mask=mask), _kw(2))
    _check_groups(orc, out, np.where(mask, stand_in, key), X, T, True, ("ta", "tb"), null_last=stand_in)
    # the capacity guess is too small: one retry with the device's count
    mock.pds_plugin_debug_multi_by_first_cap(C.c_longlong(2))
    try:
        CALLS.clear()
        _, out = call_plugin(mock, "pl_lr_multi_by", _inputs(key, X, T), _kw(2))
        assert CALLS == [("by_key", len(key), 2, 2, 2), ("by_key", len(key), 2, 2, 3)]
        _check_groups(orc, out, key, X, T, True, ("ta", "tb"))
    finally:
        mock.pds_plugin_debug_multi_by_first_cap(C.c_longlong(0))


def test_plugin_multi_by_null_policies(mock, orc):
    """series_to_mat_for_multi_lr's three outcomes: "raise" on any null; a numeric fill fills the features (and refuses a null in a
    target); every other policy is not supported by the multi-target fit."""
    from plugin_harness import PluginFailure, call_plugin

    rng = np.random.default_rng(7)
    key, X, T = _keyed_frame(rng, [70, 60, 65], 2, 2)
    n = len(key)
    feat_masks = {2: np.zeros(n, bool), 3: np.zeros(n, bool)}
    feat_masks[2][np.flatnonzero(key == -20)[5:9]] = True
    feat_masks[3][np.flatnonzero(key == -13)[7:11]] = True
    with pytest.raises(PluginFailure, match="Nulls found in data"):
        call_plugin(mock, "pl_lr_multi_by", _inputs(key, X, T, masks=feat_masks), _kw(2))
    for policy in ("skip", "ignore", "skip_window"):
        with pytest.raises(PluginFailure, match="not supported by multi-target"):
            call_plugin(mock, "pl_lr_multi_by", _inputs(key, X, T, masks=feat_masks), _kw(2, null_policy=policy))
    CALLS.clear()
    _, out = call_plugin(mock, "pl_lr_multi_by", _inputs(key, X, T, masks=feat_masks), _kw(2, null_policy="0.5"))
    assert CALLS == [("by_key", n, 2, 2, n)]  # every row stays: the fill applies to the features only
    Xf = X.copy()
    Xf[feat_masks[2], 0] = 0.5
    Xf[feat_masks[3], 1] = 0.5
    _check_groups(orc, out, key, Xf, T, True, ("ta", "tb"))
    target_mask = dict(feat_masks)
    target_mask[1] = np.zeros(n, bool)
    target_mask[1][3] = True
    with pytest.raises(PluginFailure, match="Filling null doesn't work for multi-target lstsq"):
        call_plugin(mock, "pl_lr_multi_by", _inputs(key, X, T, masks=target_mask), _kw(2, null_policy="0.5"))
    for sym in ("pl_lr_multi_by", "pl_lr_multi_by_pred"):  # the same rules in front of the per-row form
        with pytest.raises(PluginFailure, match="not supported by multi-target"):
            call_plugin(mock, sym, _inputs(key, X, T, masks=feat_masks), _kw(2, null_policy="skip"))


def test_plugin_multi_by_pred_rows_in_frame_order(mock, orc):
    import pyarrow as pa
    from plugin_harness import call_plugin

    rng = np.random.default_rng(8)
    sizes = [40, 30, 2, 35]  # key -13: gated (duplicated column); key -6: 2 rows < p' = 3
    key, X, T = _keyed_frame(rng, sizes, 2, 2)
    CALLS.clear()
    _, out = call_plugin(mock, "pl_lr_multi_by_pred", _inputs(key, X, T), _kw(2))
    assert CALLS == [("by_key", len(key), 2, 2, len(key))]
    assert [f.name for f in out.type] == ["ta_pred", "ta_resid", "tb_pred", "tb_resid"] and len(out) == len(key)
    assert all(f.type == pa.float64() for f in out.type)
    null_rows = np.isin(key, [-13, -6])
    for t in range(2):
        pred = np.array(out.field(2 * t).to_pylist(), dtype=np.float64)
        resid = np.array(out.field(2 * t + 1).to_pylist(), dtype=np.float64)
        assert np.array_equal(np.isnan(pred), null_rows) and np.array_equal(np.isnan(resid), null_rows)  # (None -> NaN)
        assert out.field(2 * t).null_count == int(null_rows.sum())
        for kv in (-20, 1):
            rows = np.flatnonzero(key == kv)  # the rows of the group wherever the shuffle put them
            b = _fit_group(orc, X[rows], T[rows], True)
            want = mc.design(X[rows], True) @ b[t]
            np.testing.assert_allclose(pred[rows], want, rtol=1e-12, atol=1e-12)
            np.testing.assert_allclose(resid[rows], T[rows, t] - want, rtol=1e-12, atol=1e-12)


def test_plugin_multi_by_argument_errors(mock):
    from plugin_harness import PluginFailure, call_plugin

    rng = np.random.default_rng(9)
    key, X, T = _keyed_frame(rng, [30, 30], 2, 2)
    with pytest.raises(PluginFailure, match=re.escape(LIMIT)):
        call_plugin(mock, "pl_lr_multi_by", _inputs(key, np.tile(X, (1, 9))[:, :17], T), _kw(2))
    with pytest.raises(PluginFailure, match="needs a key, targets and at least one feature"):
        call_plugin(mock, "pl_lr_multi_by", _inputs(key, X, T)[:3], _kw(2))


def test_mock_offsets_entry_point_is_bound(mock, orc):
    """pds_lr_multi_grouped_* through its trampoline: the argument order of the header reaches the callback"""
    rng = np.random.default_rng(10)
    key, X, T = _keyed_frame(rng, [20, 25], 2, 2, shuffle=False)
    cols = [np.ascontiguousarray(c) for c in (T[:, 0], T[:, 1], X[:, 0], X[:, 1])]
    ptrs = (C.c_void_p * 4)(*[c.ctypes.data for c in cols])
    off = np.array([0, 20, 45], dtype=np.int64)
    co, nu = np.empty((2, 2, 3)), np.empty(2, dtype=np.uint8)
    CALLS.clear()
    fn = mock.pds_lr_multi_grouped_f64
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_double, C.c_int, C.c_double] + \
        [C.c_void_p] * 5
    assert fn(None, ptrs, 2, 2, 45, off.ctypes.data, 2, 0, 1, 0.0, 0, 1e-12, co.ctypes.data, nu.ctypes.data, None, None, None) == 0
    assert CALLS == [("grouped", 45, 2, 2, 2)] and nu.tolist() == [0, 1]  # (the second group has a duplicated column)
    np.testing.assert_allclose(co[0], _fit_group(orc, X[:20], T[:20], True), rtol=1e-12, atol=1e-12)
    assert np.isnan(co[1]).all()


# ------------------------------------------------------------------------------------------------- polars_exprs on the mini engine
def test_by_is_not_dropped_for_a_list_target():
    """the builder alone, no library behind it: `by` used to be ignored for a list target (the ungrouped pl_lr_multi was built)"""
    from test_polars_exprs import pl  # noqa: F401

    from polars_ds_extension_amd import polars_exprs as px

    e = px.lin_reg("x1", "x2", target=["a", "b"], by="k")
    inner = getattr(e, "e", None)
    if inner is not None and hasattr(inner, "fn"):  # the mini engine keeps the call open to inspection
        assert inner.fn == "pl_lr_multi_by" and inner.kwargs["last_target_idx"] == 2
    else:  # a real Polars expression prints the plugin function it calls
        assert "pl_lr_multi_by" in str(e)


def test_lin_reg_with_a_list_target_and_by_builds_the_grouped_symbol(mock):
    """lin_reg(target=[a, b], by="k") builds pl_lr_multi_by with last_target_idx == 2 (it used to drop `by` and build pl_lr_multi)"""
    from test_polars_exprs import pl  # noqa: F401  (the real polars if importable, else tests/mini_polars)

    from polars_ds_extension_amd import polars_exprs as px

    with pytest.raises(NotImplementedError, match=re.escape(LIMIT)):
        px.lin_reg(*[f"x{j}" for j in range(17)], target=["a", "b"], by="k")
    with pytest.raises(NotImplementedError, match=re.escape(LIMIT)):
        px.lin_reg("x1", target=[f"t{j}" for j in range(16)], by="k")
    old = px.PLUGIN_PATH
    px.PLUGIN_PATH = Path(mock._name)
    try:
        e = px.lin_reg("x1", "x2", target=["a", "b"], add_bias=True, by="k")
        inner = getattr(e, "e", None)
        if inner is not None and hasattr(inner, "fn"):  # (the mini engine keeps the call open to inspection)
            assert inner.fn == "pl_lr_multi_by" and inner.kwargs["last_target_idx"] == 2 and inner.changes_length
            assert len(inner.args) == 1 + 2 + 2
            ep = px.lin_reg("x1", "x2", target=["a", "b"], add_bias=True, by="k", return_pred=True)
            assert ep.e.fn == "pl_lr_multi_by_pred" and ep.e.kwargs["last_target_idx"] == 2
            one = px.lin_reg("x1", "x2", target=["a"], add_bias=True, by="k")  # a one-element list: the single-target call, with `by`
            assert one.e.fn == "pl_lr_by"
            assert px.lin_reg("x1", "x2", target=["a", "b"], add_bias=True).e.fn == "pl_lr_multi"  # without `by`: what it was
        rng = np.random.default_rng(12)
        key, X, T = _keyed_frame(rng, [80, 70, 2, 90], 2, 2)
        df = pl.DataFrame({"k": key, "a": T[:, 0], "b": T[:, 1], "x1": X[:, 0], "x2": X[:, 1]})
        CALLS.clear()
        res = df.select(e).unnest("coeffs_by")
        assert CALLS == [("by_key", len(key), 2, 2, len(key))]  # last_target_idx == 2 reached the device call as n_targets
        assert res.columns == ["k", "target_0", "target_1"] and res["k"].to_list() == [-20, -13, -6, 1]
    finally:
        px.PLUGIN_PATH = old


def test_lin_reg_by_group_with_a_list_target(mock, orc):
    """one list column per target, null lists for a null group; lin_reg_over joins them back onto the frame; keys of another dtype"""
    from test_polars_exprs import pl

    from polars_ds_extension_amd import polars_exprs as px

    old = px.PLUGIN_PATH
    px.PLUGIN_PATH = Path(mock._name)
    try:
        rng = np.random.default_rng(13)
        sizes = [80, 70, 2, 90]  # key -13: gated (duplicated column); key -6: 2 rows < p' = 3
        key, X, T = _keyed_frame(rng, sizes, 2, 2)
        df = pl.DataFrame({"k": key, "a": T[:, 0], "b": T[:, 1], "x1": X[:, 0], "x2": X[:, 1]})
        CALLS.clear()
        r = px.lin_reg_by_group(df, "k", "x1", "x2", target=["a", "b"], add_bias=True)
        assert CALLS == [("by_key", len(key), 2, 2, len(key))]
        assert r.columns == ["k", "target_0", "target_1"] and r["k"].to_list() == [-20, -13, -6, 1]
        for kv, c0, c1 in zip(r["k"].to_list(), r["target_0"].to_list(), r["target_1"].to_list()):
            b = _fit_group(orc, X[key == kv], T[key == kv], True)
            if b is None:
                assert kv in (-13, -6) and c0 is None and c1 is None
                continue
            np.testing.assert_allclose(c0, b[0], rtol=1e-12, atol=1e-12)
            np.testing.assert_allclose(c1, b[1], rtol=1e-12, atol=1e-12)
        over = px.lin_reg_over(df, "k", "x1", "x2", target=["a", "b"], add_bias=True)
        assert over.columns == ["k", "a", "b", "x1", "x2", "target_0", "target_1"] and len(over) == len(key)
        by_key = dict(zip(r["k"].to_list(), r["target_1"].to_list()))
        assert all(c == by_key[kv] for kv, c in zip(over["k"].to_list(), over["target_1"].to_list()))
        pr = px.lin_reg_by_group(df, "k", "x1", "x2", target=["a", "b"], add_bias=True, return_pred=True)
        assert pr.columns == ["k", "a", "b", "x1", "x2", "target_0_pred", "target_0_resid", "target_1_pred", "target_1_resid"]
        rows = key == 1
        want = mc.design(X[rows], True) @ _fit_group(orc, X[rows], T[rows], True)[1]
        np.testing.assert_allclose(np.array(pr["target_1_pred"].to_list(), dtype=np.float64)[rows], want, rtol=1e-12, atol=1e-12)
        names = np.array(["oak", "elm", "ash", "fir"])[(key + 20) // 7]
        d2 = pl.DataFrame({"tree": names.tolist(), "a": T[:, 0], "b": T[:, 1], "x1": X[:, 0], "x2": X[:, 1]})
        r2 = px.lin_reg_by_group(d2, "tree", "x1", "x2", target=["a", "b"], add_bias=True)
        assert r2.columns == ["tree", "target_0", "target_1"] and r2["tree"].to_list() == list(dict.fromkeys(names.tolist()))
        by_name = dict(zip(r2["tree"].to_list(), r2["target_0"].to_list()))
        by_k = dict(zip(r["k"].to_list(), r["target_0"].to_list()))
        for t, kv in zip(("oak", "elm", "ash", "fir"), (-20, -13, -6, 1)):
            assert by_name[t] == by_k[kv]
    finally:
        px.PLUGIN_PATH = old
