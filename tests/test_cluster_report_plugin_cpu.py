"""The cluster-robust report without a GPU: the C ABI surface (exports, header declarations, the mock builder's view of them), the
plugin symbol pl_lin_reg_report_cluster on the mock device with a callback bound to the reference (cluster_reference.py), and the
routing and kwargs of polars_exprs.lin_reg_report(cluster=)."""
import ctypes as C
import re
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT))

import cluster_cases as cc  # noqa: E402
import cluster_reference as cr  # noqa: E402

NEW = ["pds_lin_reg_report_cluster_grouped_f64", "pds_lin_reg_report_cluster_grouped_f32", "pds_lin_reg_report_cluster_by_key_f64",
       "pds_lin_reg_report_cluster_by_key_f32"]
FIELDS = ["features", "beta", None, "t", "p>|t|", "0.025", "0.975", "r2", "adj_r2"]
CALLS = []  # (entry point, n_rows, clusters or None, se_type, y_var) of every call the mock saw
PDS_CLUSTER, PDS_CLUSTER0, DERIVE = 5, 6, 0x100


def test_exported_and_declared():
    from polars_ds_extension_amd import _lib

    assert all(n in _lib.EXPORTS for n in NEW)
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "pds_lstsq.h").read_text(), flags=re.S)
    for n in NEW:
        assert len(re.findall(rf"^int\s+{n}\s*\(", text, flags=re.M)) == 1, n
    enum = re.search(r"typedef enum \{([^}]*)\} pds_se_type;", text, flags=re.S).group(1)
    assert re.findall(r"(PDS_\w+)\s*=\s*(\d+)", enum) == [("PDS_SE", "0"), ("PDS_HC0", "1"), ("PDS_HC1", "2"), ("PDS_HC2", "3"), ("PDS_HC3", "4"),
                                                          ("PDS_CLUSTER", "5"), ("PDS_CLUSTER0", "6")]
    assert _lib.CLUSTER_SE_TYPES == {"cluster": PDS_CLUSTER, "cluster0": PDS_CLUSTER0} and _lib.PDS_REPORT_DERIVE_YVAR == DERIVE


def test_mock_trampolines_parse():
    sys.path.insert(0, str(ROOT / "tests" / "mock_device"))
    try:
        import build as mock_build
    finally:
        sys.path.pop(0)
    protos = {name: args for _, name, args in mock_build.prototypes()}
    assert [a for _, a in protos["pds_lin_reg_report_cluster_grouped_f64"]] == ["ctx", "cols", "n_feat", "n_rows", "cluster_offsets", "n_clusters",
                                                                               "space", "add_bias", "se_type", "y_var", "out"]
    assert [a for _, a in protos["pds_lin_reg_report_cluster_by_key_f32"]] == ["ctx", "cols", "keys", "n_feat", "n_rows", "space", "add_bias",
                                                                              "se_type", "y_var", "out", "n_clusters"]
    assert protos["pds_lin_reg_report_cluster_grouped_f32"][9][0] == "float" and protos["pds_lin_reg_report_cluster_by_key_f64"][8][0] == "double"
    assert protos["pds_lin_reg_report_cluster_by_key_f64"][9][0] == "pds_report_f64*"


def test_source_lists_the_kernel():
    csrc = ROOT / "polars_ds_extension_amd" / "csrc"
    assert "cluster_meat.hip" in (csrc / "Makefile").read_text()
    assert '#include "capi_report_cluster.hpp"' in (csrc / "capi.hip").read_text()
    assert '#include "plugin_cluster.hpp"' in (csrc / "plugin.cpp").read_text()
    # the score / meat idiom is score_meat_dev.hpp's (shared with within_pass.hip), which builds on the wave tile
    text, shared = (csrc / "cluster_meat.hip").read_text(), (csrc / "score_meat_dev.hpp").read_text()
    assert '#include "score_meat_dev.hpp"' in text and '#include "wave_tile_dev.hpp"' in shared
    assert "__builtin_amdgcn_mfma_f64_16x16x4f64" in shared
    assert "score_rows4<P>" in text and "ScoreMeat<true>" in text and "score_long_meat_kernel<true, int>" in text  # (with a bias entry)
    assert "launch_sum_records(" in text and "compensated=*/true" in text
    # no atomics in any sum: the pass, the shared idiom, the record sum (mixed.hip, whose one integer atomicOr is the flag word's)
    atomics = r"atomic(Add|Or|Max|Min|CAS|Exch)"
    assert not re.search(atomics, text) and not re.search(atomics, shared)
    mixed = (csrc / "mixed.hip").read_text()
    sum_text = mixed[mixed.index("template <bool COMPENSATED>"):mixed.index("template <int P>\n__global__ __launch_bounds__(64) void mixed_profile_kernel")]
    sum_text += mixed[mixed.index("int launch_sum_records("):mixed.index("int mixed_stats_blocks(")]
    assert "sum_records_kernel(" in sum_text and "two_sum(s, c, v)" in sum_text and "hipLaunchKernelGGL" in sum_text
    assert not re.search(atomics, sum_text)


# ------------------------------------------------------------------------------------------------- the plugin layer on the mock device
def _reference(X, y, codes, bias, se, y_var):
    """what the mock answers: the float64 mode of the reference"""
    Z = np.column_stack([X, np.ones(len(y))]) if bias else X
    return cr.report(Z, y, codes, se, np.float64, y_var=y_var)


@pytest.fixture(scope="module")
def mock():
    """The mock plugin library, the cluster report's entry points bound to callbacks that run the reference."""
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

    def answer(X, y, codes, bias, se_type, y_var, out_p, R, dt):
        if X.shape[1] > 16:
            lib.mock_set_error(b"cluster-robust report: up to 16 feature columns")
            return -5
        if len(np.unique(codes)) < 2:
            lib.mock_set_error(b"cluster-robust standard errors need at least two non-empty clusters")
            return -1
        derive = bool(se_type & DERIVE)
        se = {PDS_CLUSTER: "cluster", PDS_CLUSTER0: "cluster0"}[se_type & ~DERIVE]
        r = _reference(X, y, codes, bool(bias), se, None if derive else float(y_var))
        out = C.cast(out_p, C.POINTER(R)).contents
        pp = X.shape[1] + int(bool(bias))
        for k, rk in (("beta", "beta"), ("std_err", "std_err"), ("t", "t"), ("p", "p"), ("ci_lower", "ci_lo"), ("ci_upper", "ci_hi")):
            view(getattr(out, k), pp, dt)[:] = r[rk]
        out.r2, out.adj_r2 = float(r["r2"]), float(r["adj_r2"])
        return 0

    def make_grouped(dt, ct, R):
        def fn(ctx, cols_p, n_feat, n, off_p, ng, space, bias, se_type, y_var, out_p):
            CALLS.append(("grouped", n, ng, se_type, float(y_var)))
            X, y = frame(cols_p, n_feat, n, dt)
            off = view(off_p, ng + 1, np.int64)
            return answer(X, y, np.repeat(np.arange(ng), np.diff(off)), bias, se_type, y_var, out_p, R, dt)

        return C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, ct, C.c_void_p)(fn)

    def make_by_key(dt, ct, R):
        def fn(ctx, cols_p, keys_p, n_feat, n, space, bias, se_type, y_var, out_p, ng_p):
            CALLS.append(("by_key", n, None, se_type, float(y_var)))
            keys = view(keys_p, n, np.int64).copy()
            C.c_int64.from_address(ng_p).value = len(np.unique(keys))
            X, y = frame(cols_p, n_feat, n, dt)
            return answer(X, y, keys, bias, se_type, y_var, out_p, R, dt)

        return C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int, ct, C.c_void_p, C.c_void_p)(fn)

    for sfx, dt, ct, R in (("f64", np.float64, C.c_double, _lib.ReportF64), ("f32", np.float32, C.c_float, _lib.ReportF32)):
        for name, cb in ((f"pds_lin_reg_report_cluster_grouped_{sfx}", make_grouped(dt, ct, R)),
                         (f"pds_lin_reg_report_cluster_by_key_{sfx}", make_by_key(dt, ct, R))):
            keep.append(cb)
            getattr(lib, "mock_bind_" + name)(C.cast(cb, C.c_void_p))
    lib._cluster_report_keep = keep
    return lib


def _frame(p=3, shuffle=True, seed=41):
    rng = np.random.default_rng(seed)
    F, y, off, codes = cc.equal_frame(7, p)
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


KW = {"bias": True, "null_policy": "raise", "std_err": "cluster", "solver": "qr", "l1_reg": 0.0, "l2_reg": 0.0, "tol": 0.0}


def _check(out, key, X, y, bias, se, y_var=None, rtol=1e-12):
    names = [f"x{j + 1}" for j in range(X.shape[1])] + (["__bias__"] if bias else [])
    want = _reference(X, y, key, bias, se, y_var)
    fields = [se + "_se" if f is None else f for f in FIELDS]
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

    fld = output_field(mock, "pl_lin_reg_report_cluster", [pa.field("firm", pa.int64()), pa.field("y", pa.float64())])
    assert fld.name == "lin_reg_report" and [f.name for f in fld.type] == ["features", "beta", "cluster_se", "t", "p>|t|", "0.025", "0.975", "r2",
                                                                         "adj_r2"]
    assert fld.type[0].type == pa.large_string() and all(fld.type[i].type == pa.float64() for i in range(1, 9))
    assert all(output_field(mock, "pl_lin_reg_report_cluster_f32").type[i].type == pa.float32() for i in range(1, 9))
    key, X, y = _frame()
    for se in ("cluster", "cluster0"):
        for bias in (True, False):
            CALLS.clear()
            field, out = call_plugin(mock, "pl_lin_reg_report_cluster", _inputs(key, X, y), dict(KW, std_err=se, bias=bias))
            # keys in any row order go to the by-key entry as they are; var(y) is left to the library
            assert CALLS == [("by_key", len(y), None, (PDS_CLUSTER if se == "cluster" else PDS_CLUSTER0) | DERIVE, 0.0)]
            assert field.name == "lin_reg_report" and field.type == out.type
            want = _check(out, key, X, y, bias, se)
            assert want["n_clusters"] == 7
    # the standard-error column is not the plain report's: the parent commit answered this request with "std_err"
    assert "std_err" not in [f.name for f in out.type]
    # ordered keys give the same answer as shuffled ones (the reference does not care; the entry is the same)
    k2, X2, y2 = _frame(shuffle=False)
    _, out2 = call_plugin(mock, "pl_lin_reg_report_cluster", _inputs(k2, X2, y2), KW)
    _check(out2, k2, X2, y2, True, "cluster")
    # f32
    _, out32 = call_plugin(mock, "pl_lin_reg_report_cluster_f32", _inputs(key, X, y, dt=np.float32), KW)
    assert out32.field(2).type == pa.float32()
    _check(out32, key, X.astype(np.float32).astype(np.float64), y.astype(np.float32).astype(np.float64), True, "cluster", rtol=2e-6)


def test_plugin_null_key_is_its_own_cluster(mock):
    from plugin_harness import call_plugin

    key, X, y = _frame()
    mask = key == -12  # (keys -30, -21, -12, ...: the third cluster becomes the null key's)
    assert mask.sum() == 5
    _, out = call_plugin(mock, "pl_lin_reg_report_cluster", _inputs(key, X, y, key_mask=mask), KW)
    want = _check(out, key, X, y, True, "cluster")  # the same clusters, whatever value stands in for the null key
    assert want["n_clusters"] == 7
    # all keys null but one cluster's: two clusters
    mask2 = key != -30
    _, out = call_plugin(mock, "pl_lin_reg_report_cluster", _inputs(key, X, y, key_mask=mask2), KW)
    _check(out, np.where(mask2, 0, 1), X, y, True, "cluster")


@pytest.mark.parametrize("policy", ["skip", "zero"])
def test_plugin_null_policies(mock, policy):
    """frames with nulls are prepared on the host (rows in key order, the policy row by row, a dropped row leaves with its key) and
    go to the offsets entry point with var(y) of the original non-null target"""
    from plugin_harness import call_plugin

    key, X, y = _frame()
    n = len(y)
    rng = np.random.default_rng(8)
    masks = {0: rng.uniform(size=n) < 0.1, 2: rng.uniform(size=n) < 0.15}
    assert masks[0].any() and masks[2].any()
    CALLS.clear()
    _, out = call_plugin(mock, "pl_lin_reg_report_cluster", _inputs(key, X, y, masks=masks), dict(KW, null_policy=policy))
    if policy == "skip":
        keep, Xf = ~(masks[0] | masks[2]), X
    else:
        keep, Xf = ~masks[0], X.copy()
        Xf[masks[2], 1] = 0.0
    y_var = float(np.var(y[~masks[0]], ddof=1))
    assert len(CALLS) == 1 and CALLS[0][:4] == ("grouped", int(keep.sum()), 7, PDS_CLUSTER)
    assert abs(CALLS[0][4] - y_var) <= 1e-14 * y_var
    order = np.argsort(key[keep], kind="stable")
    _check(out, key[keep][order], Xf[keep][order], y[keep][order], True, "cluster", y_var=CALLS[0][4])
    with pytest.raises(Exception, match="Nulls found in data"):
        call_plugin(mock, "pl_lin_reg_report_cluster", _inputs(key, X, y, masks=masks), KW)


def test_plugin_refusals(mock):
    from plugin_harness import call_plugin

    key, X, y = _frame()
    with pytest.raises(Exception, match="at least two non-empty clusters"):
        call_plugin(mock, "pl_lin_reg_report_cluster", _inputs(np.zeros_like(key), X, y), KW)
    with pytest.raises(Exception, match="up to 16 feature columns"):
        call_plugin(mock, "pl_lin_reg_report_cluster", _inputs(key, np.tile(X, (1, 6))[:, :17], y), KW)
    with pytest.raises(Exception, match='std_err is "cluster" or "cluster0"'):
        call_plugin(mock, "pl_lin_reg_report_cluster", _inputs(key, X, y), dict(KW, std_err="hc1"))
    with pytest.raises(Exception, match="need a key, a target and at least one feature"):
        call_plugin(mock, "pl_lin_reg_report_cluster", _inputs(key, X, y)[:2], KW)
    with pytest.raises(Exception, match="input columns differ in length"):
        ins = _inputs(key, X, y)
        ins[2] = ("x1", ins[2][1][:-1])
        call_plugin(mock, "pl_lin_reg_report_cluster", ins, KW)
    with pytest.raises(Exception, match="Empty data"):
        call_plugin(mock, "pl_lin_reg_report_cluster", _inputs(key[:0], X[:0], y[:0]), KW)


def test_polars_exprs_round_trip(mock):
    """polars_exprs.lin_reg_report(std_err="cluster", cluster=...) through the engine (the real polars if importable, else
    tests/mini_polars) and the pickled kwargs into pl_lin_reg_report_cluster on the mock device; the refusals of the builder."""
    from test_polars_exprs import pl, px

    key, X, y = _frame()
    df = pl.DataFrame({"firm": key, "y": y, "x1": X[:, 0], "x2": X[:, 1], "x3": X[:, 2]})
    before = px.PLUGIN_PATH
    px.PLUGIN_PATH = str(mock._name)
    try:
        for se, bias in (("cluster", True), ("cluster0", False)):
            CALLS.clear()
            rep = df.select(px.lin_reg_report("x1", "x2", "x3", target="y", add_bias=bias, std_err=se, cluster="firm")).unnest("lin_reg_report")
            assert CALLS == [("by_key", len(y), None, (PDS_CLUSTER if se == "cluster" else PDS_CLUSTER0) | DERIVE, 0.0)]
            assert rep.columns == ["features", "beta", se + "_se", "t", "p>|t|", "0.025", "0.975", "r2", "adj_r2"]
            want = _reference(X, y, key, bias, se, None)
            assert rep["features"].to_list() == ["x1", "x2", "x3"] + (["__bias__"] if bias else [])
            np.testing.assert_allclose(rep["beta"].to_numpy(), np.asarray(want["beta"], dtype=np.float64), rtol=1e-12)
            np.testing.assert_allclose(rep[se + "_se"].to_numpy(), np.asarray(want["std_err"], dtype=np.float64), rtol=1e-12)
            np.testing.assert_allclose(rep["p>|t|"].to_numpy(), want["p"], rtol=1e-12)
        # the null policy travels in the kwargs: a null with "raise" fails, with "skip" the frame is prepared on the host
        dfn = pl.DataFrame({"firm": key, "y": y, "x1": [None] + list(X[1:, 0])})
        with pytest.raises(Exception, match="Nulls found in data"):
            dfn.select(px.lin_reg_report("x1", target="y", std_err="cluster", cluster="firm"))
        CALLS.clear()
        dfn.select(px.lin_reg_report("x1", target="y", std_err="cluster", cluster="firm", null_policy="skip"))
        assert CALLS[0][:2] == ("grouped", len(y) - 1)
    finally:
        px.PLUGIN_PATH = before
    with pytest.raises(NotImplementedError, match="together with `by` or `weights`"):
        px.lin_reg_report("x1", target="y", std_err="cluster", cluster="firm", by="g")
    with pytest.raises(NotImplementedError, match="together with `by` or `weights`"):
        px.lin_reg_report("x1", target="y", std_err="cluster", cluster="firm", weights="w")
    with pytest.raises(ValueError, match="needs `cluster`"):
        px.lin_reg_report("x1", target="y", std_err="cluster")
    with pytest.raises(ValueError, match="goes with std_err"):
        px.lin_reg_report("x1", target="y", std_err="hc0", cluster="firm")
