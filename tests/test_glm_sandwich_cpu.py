"""The robust / cluster-robust one-model GLM report without a GPU: the C ABI surface (exports, header declarations, the mock builder's
view of them), the reference (tests/glm_sandwich_reference.py) against an independent restatement, the plugin symbol
pl_glm_report_robust on the mock device with callbacks bound to the reference, and the routing and argument errors of
lstsq.glm_report, GLM.fit and polars_exprs.glm_report."""
import ctypes as C
import re
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT))

import cluster_reference as cr  # noqa: E402
import glm_sandwich_cases as sc  # noqa: E402
import glm_sandwich_reference as sr  # noqa: E402
import glm_weighted_reference as wr  # noqa: E402

NEW = [f"pds_glm_report_{form}_{sfx}" for form in ("robust", "cluster_grouped", "cluster_by_key") for sfx in ("f64", "f32")]
FIELDS = ["features", "beta", "std_err", "z", "p>|z|", "0.025", "0.975", "deviance", "null_deviance", "dispersion", "n_iter", "n_clusters"]
SE_CODE = {"hc0": 1, "hc1": 2, "cluster": 5, "cluster0": 6}
SE_NAME = {v: k for k, v in SE_CODE.items()}
FAMILY = {0: "gaussian", 1: "poisson", 2: "binomial", 3: "gamma"}
CALLS = []  # (entry point, n_rows, clusters or None, se_type, has weights, has offset) of every call the mock saw


# ------------------------------------------------------------------------------------------------- the surface
def test_exported_and_declared():
    from polars_ds_extension_amd import _lib

    assert all(n in _lib.EXPORTS for n in NEW)
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "pds_lstsq.h").read_text(), flags=re.S)
    for n in NEW:
        assert len(re.findall(rf"^int\s+{n}\s*\(", text, flags=re.M)) == 1, n
    assert _lib.GLM_ROBUST_SE_TYPES == {"hc0": 1, "hc1": 2, "hc2": 3, "hc3": 4, "cluster": 5, "cluster0": 6}


def test_mock_trampolines_parse():
    sys.path.insert(0, str(ROOT / "tests" / "mock_device"))
    try:
        import build as mock_build
    finally:
        sys.path.pop(0)
    protos = {name: args for _, name, args in mock_build.prototypes()}
    tail = ["space", "add_bias", "link", "variance", "tol", "max_iter", "se_type", "coeffs", "n_iter", "out", "n_clusters"]
    head = ["ctx", "cols", "weights", "offset"]
    assert [a for _, a in protos["pds_glm_report_robust_f64"]] == head + ["n_feat", "n_rows"] + tail
    assert [a for _, a in protos["pds_glm_report_cluster_grouped_f32"]] == head + ["n_feat", "n_rows", "cluster_offsets", "n_offsets"] + tail
    assert [a for _, a in protos["pds_glm_report_cluster_by_key_f64"]] == head + ["keys", "n_feat", "n_rows"] + tail
    by_name = {a: t for t, a in protos["pds_glm_report_cluster_by_key_f32"]}
    assert by_name["tol"] == "float" and by_name["out"] == "const pds_glm_report_out*" and by_name["n_clusters"] == "int64_t*"
    assert {a: t for t, a in protos["pds_glm_report_robust_f64"]}["tol"] == "double"


def test_source_lists_the_kernel():
    csrc = ROOT / "polars_ds_extension_amd" / "csrc"
    assert "glm_meat.hip" in (csrc / "Makefile").read_text()
    assert '#include "capi_glm_sandwich.hpp"' in (csrc / "capi.hip").read_text()
    assert '#include "plugin_glm_sandwich.hpp"' in (csrc / "plugin.cpp").read_text()
    text = (csrc / "glm_meat.hip").read_text()
    assert '#include "score_meat_dev.hpp"' in text and '#include "glm_dev.hpp"' in text
    assert "score_rows4<P>" in text and "ScoreMeat<true>" in text and "score_long_meat_kernel<true, int>" in text and "park_d(" in text
    assert "wave_tile_gram<P>" in text and "CompSq" in text
    assert "launch_sum_records(" in text and "compensated=*/true" in text
    assert not re.search(r"atomic(Add|Or|Max|Min|CAS|Exch)|__hip_atomic|unsafeAtomic", text)  # no atomic of any kind, floating-point or not


# ------------------------------------------------------------------------------------------------- the reference
@pytest.mark.parametrize("p", sc.WIDTHS)
def test_reference_is_the_linear_report_for_the_gaussian_family(p):
    """identity link, unit variance: r = y - x . beta and I = X'X, so every kind is cluster_reference's (an independent restatement)"""
    X, y, off, codes, _, _ = sc.ragged("gaussian", p, weighted=False)
    Z = np.concatenate([X, np.ones((len(X), 1))], axis=1)
    lin = cr.report(Z, y, codes, "cluster")
    for kind in sc.KINDS:
        r = sr.report(X, y, lin["beta"], "gaussian", True, kind, codes=codes)
        assert cr.rel(r["std_err"], lin["se_all"][kind]) < 1e-17, kind
        assert r["n_clusters"] == (10 if kind in sr.CLUSTER_KINDS else 0) and r["n"] == len(y) and r["df_resid"] == len(y) - p - 1
    # float64 is the same code in the narrower format: near the longdouble result, not equal to it
    lo = sr.report(X, y, lin["beta"], "gaussian", True, "cluster", codes=codes, dtype=np.float64)
    assert lo["std_err"].dtype == np.float64 and 0 < cr.rel(lo["std_err"], lin["se_all"]["cluster"]) < 1e-12


def test_reference_weights():
    """integer weights are replication for the cluster sums; a row of weight 0 reaches nothing, whatever it holds; G and n count the
    rows of positive weight"""
    import glm_weighted_cases as wc

    X, y, off, codes, pw, o = sc.ragged("gamma", 16)
    assert pw[0] == 0  # (the one-row cluster: G = 9)
    beta = wr.fit(X, y, np.array([0, len(y)]), pw, o, "gamma", True, 1e-12, 100)[0][0]
    a = sr.report(X, y, beta, "gamma", True, "cluster0", codes=codes, pw=pw, o=o)
    assert a["n_clusters"] == 9 and a["n"] == int((pw > 0).sum())
    Xr, yr, offr, orep = wc.replicate(X, y, off, pw, o)
    b = sr.report(Xr, yr, beta, "gamma", True, "cluster0", codes=sc.codes_of(offr), o=orep)
    assert cr.rel(a["std_err"], b["std_err"]) < 1e-16
    y2 = y.copy()
    y2[pw == 0] = np.nan
    c = sr.report(X, y2, beta, "gamma", True, "cluster0", codes=codes, pw=pw, o=o)
    assert np.array_equal(a["std_err"], c["std_err"])
    for kind, c_want in (("hc1", a["n"] / (a["n"] - 17)), ("cluster", 9 / 8 * (a["n"] - 1) / (a["n"] - 17))):
        base = "hc0" if kind == "hc1" else "cluster0"
        r1, r0 = (sr.report(X, y, beta, "gamma", True, k, codes=codes, pw=pw, o=o) for k in (kind, base))
        assert cr.rel(r1["cov"], r0["cov"] * np.longdouble(c_want)) < 1e-15  # (c_want is a float64 quotient: a few 1e-16)


def test_budget_rule():
    assert sr.budget(1e-14) == 64e-14 and sr.budget(1e-17) == 8 * np.finfo(np.float64).eps
    assert sr.budget(1e-6, np.float32) == 64e-6 and sr.budget(1e-9, np.float32) == 8 * float(np.finfo(np.float32).eps)


# ------------------------------------------------------------------------------------------------- the plugin layer on the mock device
def _reference(X, y, family, bias, kind, codes=None, pw=None, o=None):
    """what the mock answers: a float64 fit (glm_weighted_reference) and the float64 mode of the reference at it"""
    co, it = wr.fit(X, y, np.array([0, len(y)]), pw, o, family, bias, 1e-10, 100)
    r = sr.report(X, y, co[0], family, bias, kind, codes=codes, pw=pw, o=o, dtype=np.float64)
    r["beta"], r["n_iter"] = co[0], int(it[0])
    return r


@pytest.fixture(scope="module")
def mock():
    """The mock plugin library, the robust GLM report's entry points bound to callbacks that run the reference."""
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

    def answer(name, cols_p, w_p, o_p, n_feat, n, codes, bias, link, se_type, co_p, it_p, out_p, ng_p, dt):
        CALLS.append((name, n, None if codes is None else len(np.unique(codes)), se_type, bool(w_p), bool(o_p)))
        if n_feat > 16:
            lib.mock_set_error(b"robust GLM report: up to 16 feature columns")
            return -5
        if codes is not None and len(np.unique(codes)) < 2:
            lib.mock_set_error(b"cluster-robust standard errors need at least two non-empty clusters")
            return -1
        X, y = frame(cols_p, n_feat, n, dt)
        pw = view(w_p, n, dt).astype(np.float64) if w_p else None
        o = view(o_p, n, dt).astype(np.float64) if o_p else None
        r = _reference(X, y, FAMILY[link], bool(bias), SE_NAME[se_type], codes, pw, o)
        pp = n_feat + int(bool(bias))
        view(co_p, pp, dt)[:] = r["beta"]
        C.c_int32.from_address(it_p).value = r["n_iter"]
        C.c_int64.from_address(ng_p).value = r["n_clusters"]
        out = C.cast(out_p, C.POINTER(_lib.GlmReportOut)).contents
        for k, rk in (("std_err", "std_err"), ("z", "z"), ("p", "p"), ("ci_lower", "lo"), ("ci_upper", "hi")):
            view(getattr(out, k), pp, dt)[:] = r[rk]
        view(out.deviance, 1, dt)[0], view(out.null_deviance, 1, dt)[0], view(out.dispersion, 1, dt)[0] = 11.0, 22.0, 1.0
        C.c_uint8.from_address(out.report_null).value = 0
        assert not out.cov and not out.df_resid  # (the plugin asks for neither)
        return 0

    P, I, L = C.c_void_p, C.c_int, C.c_int64

    def make(form, dt, ct):
        tail = [I, I, I, I, ct, I, I, P, P, P, P]  # space, add_bias, link, variance, tol, max_iter, se_type, coeffs, n_iter, out, n_clusters
        if form == "robust":
            def fn(ctx, cols_p, w_p, o_p, n_feat, n, space, bias, link, var, tol, mi, se, co_p, it_p, out_p, ng_p):
                return answer(form, cols_p, w_p, o_p, n_feat, n, None, bias, link, se, co_p, it_p, out_p, ng_p, dt)
            return C.CFUNCTYPE(I, P, P, P, P, I, L, *tail)(fn)
        if form == "cluster_grouped":
            def fn(ctx, cols_p, w_p, o_p, n_feat, n, off_p, ng, space, bias, link, var, tol, mi, se, co_p, it_p, out_p, ng_p):
                off = view(off_p, ng + 1, np.int64)
                return answer(form, cols_p, w_p, o_p, n_feat, n, np.repeat(np.arange(ng), np.diff(off)), bias, link, se, co_p, it_p, out_p, ng_p, dt)
            return C.CFUNCTYPE(I, P, P, P, P, I, L, P, L, *tail)(fn)

        def fn(ctx, cols_p, w_p, o_p, keys_p, n_feat, n, space, bias, link, var, tol, mi, se, co_p, it_p, out_p, ng_p):
            return answer(form, cols_p, w_p, o_p, n_feat, n, view(keys_p, n, np.int64).copy(), bias, link, se, co_p, it_p, out_p, ng_p, dt)
        return C.CFUNCTYPE(I, P, P, P, P, P, I, L, *tail)(fn)

    for sfx, dt, ct in (("f64", np.float64, C.c_double), ("f32", np.float32, C.c_float)):
        for form in ("robust", "cluster_grouped", "cluster_by_key"):
            cb = make(form, dt, ct)
            keep.append(cb)
            getattr(lib, f"mock_bind_pds_glm_report_{form}_{sfx}")(C.cast(cb, C.c_void_p))
    lib._glm_sandwich_keep = keep
    return lib


def _frame(p=3, shuffle=True, weighted=False):
    rng = np.random.default_rng(61)
    sizes = [6, 9, 12, 7, 16]
    X, y, pw, o = sc.one_model_frame(rng, "poisson", sum(sizes), p, weighted=True, with_offset=True)
    if not weighted:
        X, y = sc.plain_frame(np.random.default_rng(62), "poisson", sum(sizes), p)
        pw = o = None
    key = sc.codes_of(np.concatenate([[0], np.cumsum(sizes)])) * 9 - 30  # negative, sparse
    if shuffle:
        perm = rng.permutation(len(y))
        key, X, y = key[perm], X[perm], y[perm]
        pw, o = (None, None) if pw is None else (pw[perm], o[perm])
    return key, X, y, pw, o


def _inputs(key, X, y, pw=None, o=None, dt=np.float64, key_mask=None, masks=None):
    import pyarrow as pa

    masks = masks or {}
    ins = [] if key is None else [("firm", pa.array(key, type=pa.int64(), mask=key_mask))]
    ins += [(nm, pa.array(c.astype(dt), mask=masks.get(nm))) for nm, c in (("w", pw), ("o", o)) if c is not None]
    ins.append(("y", pa.array(y.astype(dt), mask=masks.get(0))))
    return ins + [(f"x{j + 1}", pa.array(X[:, j].astype(dt), mask=masks.get(j + 1))) for j in range(X.shape[1])]


def _kw(kind, key=None, pw=None, o=None, **more):
    return dict({"bias": True, "null_policy": "raise", "family": "poisson", "tol": 1e-10, "max_iter": 100, "std_err": kind,
                 "has_cluster": key is not None, "has_weights": pw is not None, "has_offset": o is not None}, **more)


def _check(out, X, y, bias, kind, codes=None, pw=None, o=None, rtol=1e-12):
    names = [f"x{j + 1}" for j in range(X.shape[1])] + (["__bias__"] if bias else [])
    want = _reference(X, y, "poisson", bias, kind, codes, pw, o)
    assert [f.name for f in out.type] == FIELDS and len(out) == len(names)
    assert out.field(0).to_pylist() == names
    for i, rk in ((1, "beta"), (2, "std_err"), (3, "z"), (4, "p"), (5, "lo"), (6, "hi")):
        np.testing.assert_allclose(np.asarray(out.field(i).to_pylist(), dtype=np.float64), np.asarray(want[rk], dtype=np.float64), rtol=rtol, atol=0)
    for i, v in ((7, 11.0), (8, 22.0), (9, 1.0), (10, want["n_iter"]), (11, want["n_clusters"])):
        assert out.field(i).to_pylist() == [v] * len(names)
    return want


def test_plugin_schema_and_values(mock):
    import pyarrow as pa
    from plugin_harness import call_plugin, output_field

    fld = output_field(mock, "pl_glm_report_robust", [pa.field("y", pa.float64())])
    assert fld.name == "glm_report" and [f.name for f in fld.type] == FIELDS
    assert fld.type[0].type == pa.large_string() and all(fld.type[i].type == pa.float64() for i in range(1, 10))
    assert fld.type[10].type == pa.int32() and fld.type[11].type == pa.int64()
    f32 = output_field(mock, "pl_glm_report_robust_f32")
    assert all(f32.type[i].type == pa.float32() for i in range(1, 10)) and f32.type[11].type == pa.int64()
    key, X, y, _, _ = _frame()
    for kind in sc.KINDS:
        k = key if kind in sr.CLUSTER_KINDS else None
        for bias in (True, False):
            CALLS.clear()
            field, out = call_plugin(mock, "pl_glm_report_robust", _inputs(k, X, y), _kw(kind, k, bias=bias))
            # keys in any row order go to the by-key entry as they are
            assert CALLS == [("robust" if k is None else "cluster_by_key", len(y), None if k is None else 5, SE_CODE[kind], False, False)]
            assert field.name == "glm_report" and field.type == out.type
            want = _check(out, X, y, bias, kind, k)
            assert want["n_clusters"] == (5 if k is not None else 0)
    # weights and offset travel as the leading inputs the kwargs name, either alone or both
    key, X, y, pw, o = _frame(weighted=True)
    for w_, o_ in ((pw, o), (pw, None), (None, o)):
        for kind, k in (("cluster", key), ("hc1", None)):
            CALLS.clear()
            _, out = call_plugin(mock, "pl_glm_report_robust", _inputs(k, X, y, w_, o_), _kw(kind, k, w_, o_))
            assert CALLS[0][4:] == (w_ is not None, o_ is not None)
            _check(out, X, y, True, kind, k, w_, o_)
    # f32
    key, X, y, _, _ = _frame()
    _, out32 = call_plugin(mock, "pl_glm_report_robust_f32", _inputs(key, X, y, dt=np.float32), _kw("cluster", key))
    assert out32.field(2).type == pa.float32()
    _check(out32, X.astype(np.float32).astype(np.float64), y, True, "cluster", key, rtol=2e-6)


def test_plugin_null_key_is_its_own_cluster(mock):
    from plugin_harness import call_plugin

    key, X, y, _, _ = _frame()
    mask = key == -12  # (keys -30, -21, -12, ...: the third cluster becomes the null key's)
    assert mask.sum() == 12
    _, out = call_plugin(mock, "pl_glm_report_robust", _inputs(key, X, y, key_mask=mask), _kw("cluster", key))
    want = _check(out, X, y, True, "cluster", key)  # the same clusters, whatever value stands in for the null key
    assert want["n_clusters"] == 5
    mask2 = key != -30  # all keys null but one cluster's: two clusters
    _, out = call_plugin(mock, "pl_glm_report_robust", _inputs(key, X, y, key_mask=mask2), _kw("cluster", key))
    assert _check(out, X, y, True, "cluster", np.where(mask2, 0, 1))["n_clusters"] == 2


@pytest.mark.parametrize("policy", ["skip", "zero"])
def test_plugin_null_policies(mock, policy):
    """frames with nulls are prepared on the host: with a key rows in key order, the policy row by row, to the offsets entry point;
    without a key the surviving rows to the robust entry point.  Weights ride with their rows."""
    from plugin_harness import call_plugin

    key, X, y, pw, o = _frame(weighted=True)
    n = len(y)
    rng = np.random.default_rng(8)
    masks = {0: rng.uniform(size=n) < 0.1, 2: rng.uniform(size=n) < 0.15}
    assert masks[0].any() and masks[2].any()
    if policy == "skip":
        keep, Xf = ~(masks[0] | masks[2]), X
    else:
        keep, Xf = ~masks[0], X.copy()
        Xf[masks[2], 1] = 0.0
    CALLS.clear()
    _, out = call_plugin(mock, "pl_glm_report_robust", _inputs(key, X, y, pw, None, masks=masks), _kw("cluster", key, pw, null_policy=policy))
    assert CALLS == [("cluster_grouped", int(keep.sum()), 5, SE_CODE["cluster"], True, False)]
    order = np.argsort(key[keep], kind="stable")
    _check(out, Xf[keep][order], y[keep][order], True, "cluster", key[keep][order], pw[keep][order])
    CALLS.clear()
    _, out = call_plugin(mock, "pl_glm_report_robust", _inputs(None, X, y, None, o, masks=masks), _kw("hc0", None, None, o, null_policy=policy))
    assert CALLS == [("robust", int(keep.sum()), None, SE_CODE["hc0"], False, True)]
    _check(out, Xf[keep], y[keep], True, "hc0", None, None, o[keep])
    with pytest.raises(Exception, match="Nulls found in data"):
        call_plugin(mock, "pl_glm_report_robust", _inputs(key, X, y, masks=masks), _kw("cluster", key))
    # a null in the weights / the offset is an error whatever the policy
    for nm, w_, o_ in (("w", pw, None), ("o", None, o)):
        with pytest.raises(Exception, match="nulls in the weights or the offset"):
            call_plugin(mock, "pl_glm_report_robust", _inputs(key, X, y, w_, o_, masks={nm: masks[0]}), _kw("cluster", key, w_, o_, null_policy=policy))


def test_plugin_refusals(mock):
    from plugin_harness import call_plugin

    key, X, y, _, _ = _frame()
    sym = "pl_glm_report_robust"
    with pytest.raises(Exception, match="at least two non-empty clusters"):
        call_plugin(mock, sym, _inputs(np.zeros_like(key), X, y), _kw("cluster", key))
    with pytest.raises(Exception, match="up to 16 feature columns"):
        call_plugin(mock, sym, _inputs(None, np.tile(X, (1, 6))[:, :17], y), _kw("hc0"))
    with pytest.raises(Exception, match="hc2 / hc3 need the leverages"):
        call_plugin(mock, sym, _inputs(None, X, y), _kw("hc3"))
    with pytest.raises(Exception, match='std_err is "hc0", "hc1", "cluster" or "cluster0"'):
        call_plugin(mock, sym, _inputs(None, X, y), _kw("se"))
    with pytest.raises(Exception, match="a cluster key goes with"):
        call_plugin(mock, sym, _inputs(key, X, y), _kw("hc1", key))
    with pytest.raises(Exception, match="a cluster key goes with"):
        call_plugin(mock, sym, _inputs(None, X, y), _kw("cluster"))
    with pytest.raises(Exception, match="needs a target and at least one feature"):
        call_plugin(mock, sym, _inputs(key, X, y)[:2], _kw("cluster", key))
    with pytest.raises(Exception, match="input columns differ in length"):
        ins = _inputs(key, X, y)
        ins[2] = ("x1", ins[2][1][:-1])
        call_plugin(mock, sym, ins, _kw("cluster", key))
    with pytest.raises(Exception, match="Empty data"):
        call_plugin(mock, sym, _inputs(key[:0], X[:0], y[:0]), _kw("cluster", key))
    with pytest.raises(Exception, match="Empty data"):
        call_plugin(mock, sym, _inputs(None, X[:0], y[:0]), _kw("hc0"))
    with pytest.raises(Exception, match="max_iter"):
        call_plugin(mock, sym, _inputs(None, X, y), _kw("hc0", max_iter=0))


def test_polars_exprs_round_trip(mock):
    """polars_exprs.glm_report(by=None, std_err=..., cluster=...) through the engine (the real polars if importable, else
    tests/mini_polars) and the pickled kwargs into pl_glm_report_robust on the mock device; the refusals of the builder."""
    from test_polars_exprs import pl, px

    key, X, y, pw, o = _frame(weighted=True)
    df = pl.DataFrame({"firm": key, "y": y, "x1": X[:, 0], "x2": X[:, 1], "x3": X[:, 2], "w": pw, "o": o})
    before = px.PLUGIN_PATH
    px.PLUGIN_PATH = str(mock._name)
    try:
        for kind, bias in (("cluster", True), ("cluster0", False), ("hc0", True), ("hc1", False)):
            cl = "firm" if kind in sr.CLUSTER_KINDS else None
            CALLS.clear()
            rep = df.select(px.glm_report("x1", "x2", "x3", target="y", family="poisson", add_bias=bias, tol=1e-10, std_err=kind, cluster=cl,
                                          weights="w", offset="o")).unnest("glm_report")
            assert CALLS == [("robust" if cl is None else "cluster_by_key", len(y), None if cl is None else 5, SE_CODE[kind], True, True)]
            assert rep.columns == FIELDS
            want = _reference(X, y, "poisson", bias, kind, key if cl else None, pw, o)
            assert rep["features"].to_list() == ["x1", "x2", "x3"] + (["__bias__"] if bias else [])
            np.testing.assert_allclose(rep["beta"].to_numpy(), np.asarray(want["beta"], dtype=np.float64), rtol=1e-12)
            np.testing.assert_allclose(rep["std_err"].to_numpy(), np.asarray(want["std_err"], dtype=np.float64), rtol=1e-12)
            np.testing.assert_allclose(rep["p>|z|"].to_numpy(), want["p"], rtol=1e-12)
            assert rep["n_clusters"].to_list() == [want["n_clusters"]] * len(rep["beta"].to_list())
        dfn = pl.DataFrame({"firm": key, "y": y, "x1": [None] + list(X[1:, 0])})
        with pytest.raises(Exception, match="Nulls found in data"):
            dfn.select(px.glm_report("x1", target="y", family="poisson", std_err="cluster", cluster="firm"))
        CALLS.clear()
        dfn.select(px.glm_report("x1", target="y", family="poisson", std_err="cluster", cluster="firm", null_policy="skip"))
        assert CALLS[0][:2] == ("cluster_grouped", len(y) - 1)
    finally:
        px.PLUGIN_PATH = before


# ------------------------------------------------------------------------------------------------- routing and argument errors
def test_polars_exprs_argument_errors():
    from test_polars_exprs import px

    with pytest.raises(NotImplementedError, match="per-group reports"):
        px.glm_report("x1", target="y", by="g", std_err="hc1")
    with pytest.raises(NotImplementedError, match="per-group reports"):
        px.glm_report("x1", target="y", by="g", std_err="cluster", cluster="firm")
    with pytest.raises(ValueError, match=r"GLM.fit\(report=True\) or lstsq.glm_report"):
        px.glm_report("x1", target="y")
    with pytest.raises(ValueError, match="exactly one of"):
        px.glm_report("x1", target="y", std_err="cluster")
    with pytest.raises(ValueError, match="go with std_err"):
        px.glm_report("x1", target="y", std_err="hc0", cluster="firm")
    with pytest.raises(ValueError, match="go with std_err"):
        px.glm_report("x1", target="y", by="g", cluster="firm")
    with pytest.raises(NotImplementedError, match="leverages"):
        px.glm_report("x1", target="y", std_err="hc2")
    with pytest.raises(ValueError, match="not one of"):
        px.glm_report("x1", target="y", std_err="robust")
    with pytest.raises(NotImplementedError, match="GLM family"):
        px.glm_report("x1", target="y", std_err="hc0", family="tweedie")


def test_lstsq_glm_report_argument_errors():
    """every refusal that needs no device comes before one is touched"""
    from polars_ds_extension_amd import lstsq

    x, y, k = np.arange(6.0), np.arange(6.0), np.arange(6)
    with pytest.raises(ValueError, match="exactly one of"):
        lstsq.glm_report(x, target=y, std_err="cluster")
    with pytest.raises(ValueError, match="exactly one of"):
        lstsq.glm_report(x, target=y, std_err="cluster0", cluster=k, cluster_offsets=[0, 3, 6])
    for kind in ("se", "hc0", "hc1"):
        with pytest.raises(ValueError, match="go with std_err"):
            lstsq.glm_report(x, target=y, std_err=kind, cluster=k)
        with pytest.raises(ValueError, match="go with std_err"):
            lstsq.glm_report(x, target=y, std_err=kind, cluster_offsets=[0, 3, 6])
    with pytest.raises(NotImplementedError, match="leverages"):
        lstsq.glm_report(x, target=y, std_err="hc2")
    with pytest.raises(ValueError, match="not one of"):
        lstsq.glm_report(x, target=y, std_err="HC1")
    with pytest.raises(NotImplementedError, match="16 feature"):
        lstsq.glm_report(*[x] * 17, target=y, std_err="hc0")
    with pytest.raises(ValueError, match="max_iter"):
        lstsq.glm_report(x, target=y, std_err="hc0", max_iter=0)
    with pytest.raises(NotImplementedError, match="GLM family"):
        lstsq.glm_report(x, target=y, std_err="hc0", family="tweedie")
    with pytest.raises(ValueError, match="one entry per row"):
        lstsq.glm_report(x, target=y, std_err="hc0", weights=np.ones(5))
    import polars_ds_extension_amd as pds

    assert pds.glm_report is lstsq.glm_report


def test_glm_fit_argument_errors():
    from polars_ds_extension_amd.linear_models import GLM

    X, y, k = np.arange(12.0).reshape(6, 2), np.arange(6.0), np.arange(6)
    with pytest.raises(ValueError, match="go with `report=True`"):
        GLM(family="poisson").fit(X, y, std_err="hc1")
    with pytest.raises(ValueError, match="go with `report=True`"):
        GLM(family="poisson").fit(X, y, std_err="cluster", cluster=k)
    with pytest.raises(NotImplementedError, match="penalised"):
        GLM(family="poisson", l2_reg=0.1).fit(X, y, report=True, std_err="hc1")
    with pytest.raises(ValueError, match="exactly one of"):
        GLM(family="poisson").fit(X, y, report=True, std_err="cluster")
    with pytest.raises(ValueError, match="go with std_err"):
        GLM(family="poisson").fit(X, y, report=True, cluster=k)
    with pytest.raises(NotImplementedError, match="leverages"):
        GLM(family="poisson").fit(X, y, report=True, std_err="hc3")
