"""
Prior weights and an offset through the Polars layer: `pl_glm_by` / `pl_glm_by_pred` with the kwargs `has_weights` / `has_offset`
(inputs [key, weights?, offset?, y, x1..xp]) and `polars_exprs.glm_by_group` / `logistic_reg(by=)` with `weights=` / `offset=`,
against the NumPy restatement of tests/glm_weighted_reference.py on every group's rows (1e-9, +-1 iteration: the device tests'
bound).  CPU: the mock device behind the same plugin.cpp, its weighted / offset entry points bound to the restatement
(tests/test_glm_weighted_cpu.py's bind_wo).  GPU: the product library, and there also against lstsq.glm_by_key on the same frame.
tests/mini_polars stands in for the Polars engine where no real one is importable (tests/test_polars_exprs.py's arrangement).
"""
import ctypes as C
import inspect
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import glm_cases as gc  # noqa: E402
import glm_weighted_cases as wc  # noqa: E402
import glm_weighted_reference as wr  # noqa: E402
from test_glm_weighted_cpu import bind_wo  # noqa: E402
from test_polars_exprs import ENGINE, pl  # noqa: E402  (the real polars if importable, else tests/mini_polars)

from polars_ds_extension_amd import polars_exprs as px  # noqa: E402

CALLS = []


@pytest.fixture(scope="module")
def wmock():
    from mock_device import device

    lib = device.load()
    lib._glm_wo_keep = bind_wo(lib, CALLS)
    return lib


def _keyed(family, p, kind, sizes, seed):
    """(key, X, y, pw, o) in shuffled row order, keys 7 g - 20"""
    rng = np.random.default_rng(seed)
    X, y, off, pw, o = wc.frame_for_sizes(rng, family, np.array(sizes), p, kind)
    key = np.repeat(np.arange(len(sizes), dtype=np.int64) * 7 - 20, sizes)
    perm = rng.permutation(len(y))
    return key[perm], X[perm], y[perm], pw[perm], o[perm]


def _inputs(key, X, y, pw=None, o=None, masks=None):
    import pyarrow as pa

    masks = masks or {}
    ins = [("k", pa.array(key, type=pa.int64()))]
    if pw is not None:
        ins.append(("w", pa.array(pw, mask=masks.get("w"))))
    if o is not None:
        ins.append(("o", pa.array(o, mask=masks.get("o"))))
    ins.append(("y", pa.array(y, mask=masks.get(0))))
    ins += [(f"x{j + 1}", pa.array(np.ascontiguousarray(X[:, j]), mask=masks.get(j + 1))) for j in range(X.shape[1])]
    return ins


def _check_groups(keys, coeffs, iters, key, X, y, pw, o, family, bias):
    """coeffs / iters: one entry per ascending key (None for a null group)"""
    assert list(keys) == sorted(set(key.tolist()))
    for k, co, it in zip(keys, coeffs, iters):
        r = key == k
        b, n_it = wr.fit_group(X[r], y[r], None if pw is None else pw[r], None if o is None else o[r], family, bias, 1e-10, 100)
        if not np.isfinite(b).all():
            assert co is None
            continue
        assert co is not None and abs(it - n_it) <= 1
        assert np.linalg.norm(np.asarray(co) - b) < 1e-9 * np.linalg.norm(b)


def t_plugin_symbols(lib):
    import pyarrow as pa
    from plugin_harness import PluginFailure, call_plugin

    key, X, y, pw, o = _keyed("poisson", 3, "integer", [60, 45, 80, 50], 21)
    kw = {"bias": True, "null_policy": "raise", "family": "poisson", "tol": 1e-10, "max_iter": 100}
    for use_w, use_o in ((True, True), (True, False), (False, True)):
        kw2 = dict(kw, **({"has_weights": True} if use_w else {}), **({"has_offset": True} if use_o else {}))
        a_w, a_o = (pw if use_w else None), (o if use_o else None)
        CALLS.clear()
        _, out = call_plugin(lib, "pl_glm_by", _inputs(key, X, y, a_w, a_o), kw2)
        if CALLS:  # (the mock records which pointers arrived: one call, the whole frame)
            assert CALLS == [(use_w, use_o)]
        assert [f.name for f in out.type] == ["k", "coeffs", "n_iter"]
        _check_groups(out.field(0).to_pylist(), out.field(1).to_pylist(), out.field(2).to_pylist(), key, X, y, a_w, a_o, "poisson", True)
        _, pred = call_plugin(lib, "pl_glm_by_pred", _inputs(key, X, y, a_w, a_o), kw2)
        pv = pred.to_numpy(zero_copy_only=False)
        assert pred.null_count == 0 and len(pv) == len(y)
        for k in np.unique(key):
            r = key == k
            b, _ = wr.fit_group(X[r], y[r], None if a_w is None else a_w[r], None if a_o is None else a_o[r], "poisson", True, 1e-10, 100)
            np.testing.assert_allclose(pv[r], np.exp(X[r] @ b[:3] + b[3] + (0.0 if a_o is None else a_o[r])), rtol=1e-9)
    # the f32 symbols take the same inputs
    f = np.float32
    _, out32 = call_plugin(lib, "pl_glm_by_f32", _inputs(key, X.astype(f), y.astype(f), pw.astype(f), o.astype(f)),
                           dict(kw, has_weights=True, has_offset=True, tol=1e-6))
    assert out32.type[1].type == pa.large_list(pa.float32()) and out32.field(1).null_count == 0
    # a null in the weights or the offset: an error whatever the null policy, and the message says so
    wmask = np.zeros(len(y), bool)
    wmask[4] = True
    for policy in ("skip", "zero", "ignore"):
        for m in ({"w": wmask}, {"o": wmask}):
            with pytest.raises(PluginFailure, match="nulls in the weights or the offset"):
                call_plugin(lib, "pl_glm_by", _inputs(key, X, y, pw, o, masks=m), dict(kw, has_weights=True, has_offset=True, null_policy=policy))
    with pytest.raises(PluginFailure, match="Nulls found in data"):
        call_plugin(lib, "pl_glm_by", _inputs(key, X, y, pw, o, masks={"w": wmask}), dict(kw, has_weights=True, has_offset=True))
    # nulls elsewhere under "skip": the rows go, with their weights and offsets
    masks = {0: np.zeros(len(y), bool), 2: np.zeros(len(y), bool)}
    masks[0][[3, 50, 51]] = True
    masks[2][[7, 90]] = True
    keep = ~(masks[0] | masks[2])
    kws = dict(kw, has_weights=True, has_offset=True, null_policy="skip")
    _, out = call_plugin(lib, "pl_glm_by", _inputs(key, X, y, pw, o, masks=masks), kws)
    _check_groups(out.field(0).to_pylist(), out.field(1).to_pylist(), out.field(2).to_pylist(), key[keep], X[keep], y[keep], pw[keep], o[keep],
                  "poisson", True)
    _, pred = call_plugin(lib, "pl_glm_by_pred", _inputs(key, X, y, pw, o, masks=masks), kws)
    assert pred.null_count == int((~keep).sum())
    # refused: a penalty with either column
    with pytest.raises(PluginFailure, match="together with weights / offset is not built"):
        call_plugin(lib, "pl_glm_by", _inputs(key, X, y, pw), dict(kw, has_weights=True, l2_reg=0.1))


def _df(key, X, y, pw, o, key_name="k"):
    data = {key_name: key, "w": pw, "o": o, "y": y}
    data.update({f"x{j + 1}": X[:, j] for j in range(X.shape[1])})
    return pl.DataFrame(data)


def t_exprs(path):
    px.PLUGIN_PATH = path
    key, X, y, pw, o = _keyed("poisson", 2, "real", [80, 70, 90], 22)
    df = _df(key, X, y, pw, o)
    res = px.glm_by_group(df, "k", "x1", "x2", target="y", family="poisson", add_bias=True, tol=1e-10, weights="w", offset="o")
    assert res.columns == ["k", "coeffs", "n_iter"]
    _check_groups(res["k"].to_list(), res["coeffs"].to_list(), res["n_iter"].to_list(), key, X, y, pw, o, "poisson", True)
    pr = px.glm_by_group(df, "k", "x1", "x2", target="y", family="poisson", add_bias=True, tol=1e-10, offset="o", return_pred=True)
    assert pr.columns == ["k", "w", "o", "y", "x1", "x2", "glm_pred"] and len(pr) == len(y)
    r = key == -13
    b, _ = wr.fit_group(X[r], y[r], None, o[r], "poisson", True, 1e-10, 100)
    np.testing.assert_allclose(pr["glm_pred"].to_numpy()[r], np.exp(X[r] @ b[:2] + b[2] + o[r]), rtol=1e-9)
    # keys of another dtype
    names = np.array(["oak", "elm", "ash"])[(key + 20) // 7]
    d2 = _df(names.tolist(), X, y, pw, o, key_name="tree")
    r2 = px.glm_by_group(d2, "tree", "x1", "x2", target="y", family="poisson", add_bias=True, tol=1e-10, weights="w")
    assert r2["tree"].to_list() == list(dict.fromkeys(names.tolist()))
    for t, co in zip(r2["tree"].to_list(), r2["coeffs"].to_list()):
        rr = names == t
        b, _ = wr.fit_group(X[rr], y[rr], pw[rr], None, "poisson", True, 1e-10, 100)
        assert np.linalg.norm(np.asarray(co) - b) < 1e-9 * np.linalg.norm(b)
    # logistic_reg(by=, weights=): success proportions with their trial counts = the Bernoulli frame with every trial a row
    rng = np.random.default_rng(23)
    sizes = [60, 75]
    Xb, _, off = gc.family_frame(rng, "binomial", np.array(sizes), 2)
    trials = rng.integers(1, 6, size=len(Xb)).astype(np.float64)
    gid = np.repeat(np.arange(2), sizes)
    eta = Xb @ np.array([0.6, -0.4]) + 0.2
    succ = rng.binomial(trials.astype(np.int64), 1.0 / (1.0 + np.exp(-eta))).astype(np.float64)
    kb = (gid * 3 + 1).astype(np.int64)
    db = _df(kb, Xb, succ / trials, trials, np.zeros(len(Xb)))
    rb = db.select(px.logistic_reg("x1", "x2", target="y", by="k", weights="w", tol=1e-10, max_iter=100)).unnest("glm_by")
    for k, co in zip(rb["k"].to_list(), rb["coeffs"].to_list()):
        rows = np.flatnonzero(kb == k)
        rep = np.repeat(rows, trials[rows].astype(np.int64))
        yb = np.concatenate([np.r_[np.ones(int(succ[i])), np.zeros(int(trials[i] - succ[i]))] for i in rows])
        b, _ = wr.fit_group(Xb[rep], yb, None, None, "binomial", True, 1e-10, 100)
        assert np.linalg.norm(np.asarray(co) - b) < 1e-9 * np.linalg.norm(b)


def t_report_symbol(lib):
    """pl_glm_report_by with has_weights / has_offset: the long format against the restatement on every group's rows"""
    from plugin_harness import PluginFailure, call_plugin

    key, X, y, pw, o = _keyed("poisson", 3, "integer", [60, 45, 80, 50], 41)
    kw = {"bias": True, "null_policy": "raise", "family": "poisson", "tol": 1e-10, "max_iter": 100}
    for use_w, use_o in ((True, True), (True, False), (False, True)):
        kw2 = dict(kw, **({"has_weights": True} if use_w else {}), **({"has_offset": True} if use_o else {}))
        a_w, a_o = (pw if use_w else None), (o if use_o else None)
        _, out = call_plugin(lib, "pl_glm_report_by", _inputs(key, X, y, a_w, a_o), kw2)
        names = [f.name for f in out.type]
        assert names[:3] == ["k", "features", "beta"] and out.field(1).to_pylist() == ["x1", "x2", "x3", "__bias__"] * 4
        col = lambda n: np.asarray(out.field(names.index(n)).to_numpy(zero_copy_only=False), dtype=np.float64).reshape(4, 4)  # noqa: E731
        for gi, k in enumerate(sorted(set(key.tolist()))):
            r = key == k
            b, _ = wr.fit_group(X[r], y[r], None if a_w is None else a_w[r], None if a_o is None else a_o[r], "poisson", True, 1e-10, 100)
            ref = wr.report_group(X[r], y[r], None if a_w is None else a_w[r], None if a_o is None else a_o[r], b, "poisson", True, np.float64)
            assert np.allclose(col("beta")[gi], b, rtol=1e-9) and np.allclose(col("std_err")[gi], ref["std_err"], rtol=1e-8)
            assert np.allclose(col("deviance")[gi], float(ref["deviance"]), rtol=1e-8)
            assert np.isnan(col("null_deviance")[gi]).all() == use_o
    wmask = np.zeros(len(y), bool)
    wmask[1] = True
    with pytest.raises(PluginFailure, match="nulls in the weights or the offset"):
        call_plugin(lib, "pl_glm_report_by", _inputs(key, X, y, pw, o, masks={"o": wmask}),
                    dict(kw, has_weights=True, has_offset=True, null_policy="skip"))


def test_report_symbol_against_the_mock_device(wmock):
    t_report_symbol(wmock)


@pytest.mark.gpu
def test_report_symbol_against_the_hip_library():
    t_report_symbol(_hip_lib())


def test_plugin_symbols_against_the_mock_device(wmock):
    t_plugin_symbols(wmock)


def test_exprs_against_the_mock_device(wmock):
    t_exprs(Path(wmock._name))


def test_builders_validate():
    with pytest.raises(NotImplementedError, match="weights= / offset= need by="):
        px.logistic_reg("x1", target="y", weights="w")
    with pytest.raises(NotImplementedError, match="together with weights= / offset="):
        px._glm_by(("x1",), "y", "k", "poisson", True, 1e-8, 100, "raise", False, 0.0, 0.1, "w", None)
    for fn in (px.glm_by_group, px.logistic_reg):
        sig = inspect.signature(fn)
        assert sig.parameters["weights"].default is None and sig.parameters["offset"].default is None
    # the reference's signature of logistic_reg stands in front of the additions
    assert list(inspect.signature(px.logistic_reg).parameters)[:10] == ["x", "target", "add_bias", "l1_reg", "l2_reg", "tol", "max_iter",
                                                                      "null_policy", "return_pred", "by"]
    assert ENGINE in ("mini", "real")


# ---- GPU: the product library -----------------------------------------------------------------------------------------------
def _hip_lib():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from polars_ds_extension_amd import _lib

    _lib.load()
    return C.CDLL(str(_lib.LIB_PATH))


@pytest.mark.gpu
def test_plugin_symbols_against_the_hip_library():
    CALLS.clear()
    t_plugin_symbols(_hip_lib())


@pytest.mark.gpu
def test_exprs_against_the_hip_library():
    from polars_ds_extension_amd import _lib

    _hip_lib()
    t_exprs(_lib.LIB_PATH)


@pytest.mark.gpu
@pytest.mark.parametrize("family,bias,p,kind", [("binomial", True, 8, "integer"), ("gamma", False, 4, "real"), ("poisson", True, 16, "real")])
def test_plugin_glm_by_against_lstsq(family, bias, p, kind):
    """pl_glm_by(_pred) with the two columns on host Arrow frames = lstsq.glm_by_key(weights=, offset=) on the same frame, bit for bit
    (no nulls: the plugin makes the same single pds_glm_irls_wo_by_key_* call), ordered keys and shuffled rows alike."""
    import pyarrow as pa
    from plugin_harness import call_plugin

    import polars_ds_extension_amd as pds

    lib = _hip_lib()
    X, y, off, pw, o = wc.frame(family, p, kind)
    key = np.repeat(np.arange(wc.G, dtype=np.int64) * 3 - 100, np.diff(off))
    kw = {"bias": bias, "null_policy": "raise", "family": family, "tol": 1e-10, "max_iter": 100, "has_weights": True, "has_offset": True}
    for perm in (np.arange(len(y)), np.random.default_rng(3).permutation(len(y))):
        Xq, yq, kq, wq, oq = X[perm], y[perm], key[perm], pw[perm], o[perm]
        ins = _inputs(kq, Xq, yq, wq, oq)
        _, out = call_plugin(lib, "pl_glm_by", ins, kw)
        _, pred = call_plugin(lib, "pl_glm_by_pred", ins, kw)
        ks, co, it, nu, pr, rn = pds.glm_by_key(*[np.ascontiguousarray(Xq[:, j]) for j in range(p)], target=yq, key=kq, family=family,
                                                add_bias=bias, tol=1e-10, max_iter=100, return_pred=True, weights=wq, offset=oq)
        assert out.field(0).to_pylist() == ks.tolist() and out.field(2).to_pylist() == it.tolist()
        assert [c.is_valid for c in out.field(1)] == [not v for v in nu.astype(bool)]
        got = np.array([c.as_py() for c in out.field(1) if c.is_valid])
        assert np.array_equal(got.view(np.uint8), np.ascontiguousarray(co[nu == 0]).view(np.uint8))
        assert pred.null_count == int(rn.sum())
        live = rn == 0
        assert np.array_equal(pred.to_numpy(zero_copy_only=False)[live].view(np.uint8), pr[live].view(np.uint8))


@pytest.mark.gpu
@pytest.mark.parametrize("use_o", [False, True])
def test_plugin_and_exprs_glm_report_by_against_lstsq(use_o):
    """pl_glm_report_by with has_weights (/ has_offset), called directly and through polars_exprs.glm_report / glm_report_by_group, =
    lstsq.glm_report_by_key(weights=, offset=) on the same frame: the long format, p' rows per group, keys ascending; shuffled rows;
    a null in the weights is an error whatever the null policy; null_deviance is NaN exactly under an offset."""
    from plugin_harness import PluginFailure, call_plugin

    import polars_ds_extension_amd as pds
    from polars_ds_extension_amd import _lib

    lib = _hip_lib()
    key, X, y, pw, o = _keyed("poisson", 3, "integer", [60, 45, 80, 50], 31)
    a_o = o if use_o else None
    kw = {"bias": True, "null_policy": "raise", "family": "poisson", "tol": 1e-10, "max_iter": 100, "has_weights": True}
    if use_o:
        kw["has_offset"] = True
    _, out = call_plugin(lib, "pl_glm_report_by", _inputs(key, X, y, pw, a_o), kw)
    ref = pds.glm_report_by_key(*[np.ascontiguousarray(X[:, j]) for j in range(3)], target=y, key=key, family="poisson", add_bias=True,
                                tol=1e-10, max_iter=100, weights=pw, offset=a_o)
    names = [f.name for f in out.type]
    assert names == ["k", "features", "beta", "std_err", "z", "p>|z|", "0.025", "0.975", "deviance", "null_deviance", "dispersion", "n_iter"]
    assert out.field(0).to_pylist() == np.repeat(ref["keys"], 4).tolist()
    assert out.field(1).to_pylist() == ["x1", "x2", "x3", "__bias__"] * 4
    for k in ("beta", "std_err", "z", "p>|z|", "0.025", "0.975"):
        got = np.asarray(out.field(names.index(k)).to_pylist(), dtype=np.float64).reshape(4, 4)
        assert np.array_equal(got.view(np.uint8), np.ascontiguousarray(ref[k]).view(np.uint8)), k
    dev_ = np.asarray(out.field(names.index("deviance")).to_pylist(), dtype=np.float64).reshape(4, 4)[:, 0]
    assert np.array_equal(dev_, ref["deviance"])
    nd = np.asarray(out.field(names.index("null_deviance")).to_numpy(zero_copy_only=False), dtype=np.float64)
    assert np.isnan(nd).all() == use_o and np.isnan(ref["null_deviance"]).all() == use_o and (use_o or np.isfinite(nd).all())
    wmask = np.zeros(len(y), bool)
    wmask[2] = True
    with pytest.raises(PluginFailure, match="nulls in the weights or the offset"):
        call_plugin(lib, "pl_glm_report_by", _inputs(key, X, y, pw, a_o, masks={"w": wmask}), dict(kw, null_policy="skip"))
    # the expressions
    px.PLUGIN_PATH = _lib.LIB_PATH
    df = _df(key, X, y, pw, o)
    res = df.select(px.glm_report("x1", "x2", "x3", target="y", by="k", family="poisson", add_bias=True, tol=1e-10, weights="w",
                                  offset="o" if use_o else None)).unnest("glm_report")
    assert np.allclose(np.asarray(res["std_err"].to_list()).reshape(4, 4), ref["std_err"], rtol=1e-12)
    res2 = px.glm_report_by_group(df, "k", "x1", "x2", "x3", target="y", family="poisson", add_bias=True, tol=1e-10, weights="w",
                                  offset="o" if use_o else None)
    assert np.allclose(np.asarray(res2["beta"].to_list()).reshape(4, 4), ref["beta"], rtol=1e-12)
