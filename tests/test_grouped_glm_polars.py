"""
`polars_exprs.logistic_reg`, `logistic_reg(by=)` and `glm_by_group`: expression -> plugin call -> `_polars_plugin_*` symbol -> Arrow
result, with tests/mini_polars standing in for the Polars engine where no real one is importable (tests/test_polars_exprs.py's
arrangement).  CPU: the mock device behind the same plugin.cpp, its grouped GLM entry points bound to the oracle
(tests/test_grouped_glm_cpu.py's fixture).  GPU: the product library; there also the reference's own test of logistic_reg against
scikit-learn (tests/test_linear_exprs.py:18-58 of the reference) restated through pl_logistic_coeffs / pl_logistic_pred, and
pl_glm_by(_pred) on host Arrow frames against lstsq.glm_by_key.
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
from test_grouped_glm_cpu import mock, orc  # noqa: E402,F401  (fixtures: the mock library with the GLM entry points bound)
from test_polars_exprs import ENGINE, pl  # noqa: E402  (the real polars if importable, else tests/mini_polars)

from polars_ds_extension_amd import polars_exprs as px  # noqa: E402


def _df(key, X, y, key_name="k"):
    data = {key_name: key, "y": y}
    data.update({f"x{j + 1}": X[:, j] for j in range(X.shape[1])})
    return pl.DataFrame(data)


def _frame(rng, sizes, p, family):
    X, y, off = gc.family_frame(rng, family, sizes, p)
    key = np.repeat(np.arange(len(sizes), dtype=np.int64) * 7 - 20, sizes)
    perm = rng.permutation(len(y))
    return key[perm], X[perm], y[perm]


def t_logistic_reg(path, orc):  # noqa: F811
    px.PLUGIN_PATH = path
    rng = np.random.default_rng(11)
    _, X, y = _frame(rng, [600], 3, "binomial")
    df = _df(np.zeros(600, dtype=np.int64), X, y)
    out = df.select(px.logistic_reg("x1", "x2", "x3", target="y", tol=1e-9))
    assert out.columns == ["__coeffs__"]
    b, _ = orc.glm_irls(X, y, family="binomial", add_bias=True, tol=1e-9, max_iter=200)
    np.testing.assert_allclose(out["__coeffs__"].to_list()[0], b, rtol=1e-9, atol=1e-11)
    out = df.select(px.logistic_reg("x1", "x2", "x3", target="y", add_bias=False, tol=1e-9, return_pred=True))
    assert out.columns == ["__pred__"]
    b0, _ = orc.glm_irls(X, y, family="binomial", add_bias=False, tol=1e-9, max_iter=200)
    np.testing.assert_allclose(out["__pred__"].to_numpy(), gc.inv_link("binomial", X @ b0), rtol=1e-9, atol=1e-11)


def t_logistic_by_and_glm_by_group(path, orc):  # noqa: F811
    px.PLUGIN_PATH = path
    rng = np.random.default_rng(12)
    sizes = [80, 2, 70, 90]  # (key -13: 2 rows < p' = 3 -> a null group)
    key, X, y = _frame(rng, sizes, 2, "binomial")
    df = _df(key, X, y)
    res = df.select(px.logistic_reg("x1", "x2", target="y", by="k", tol=1e-10, max_iter=100)).unnest("glm_by")
    assert res.columns == ["k", "coeffs", "n_iter"] and res["k"].to_list() == [-20, -13, -6, 1]
    for k, co, it in zip(res["k"].to_list(), res["coeffs"].to_list(), res["n_iter"].to_list()):
        rows = key == k
        if rows.sum() < 3:
            assert co is None and it == 0
            continue
        b, n_it = orc.glm_irls(X[rows], y[rows], family="binomial", add_bias=True, tol=1e-10, max_iter=100)
        np.testing.assert_allclose(co, b, rtol=1e-9, atol=1e-11)
        assert abs(it - n_it) <= 1
    pr = df.with_columns(px.logistic_reg("x1", "x2", target="y", by="k", tol=1e-10, max_iter=100, return_pred=True))
    assert pr.columns == ["k", "y", "x1", "x2", "glm_pred"] and len(pr) == len(y)
    rows = key == -6
    b, _ = orc.glm_irls(X[rows], y[rows], family="binomial", add_bias=True, tol=1e-10, max_iter=100)
    np.testing.assert_allclose(pr["glm_pred"].to_numpy()[rows], gc.inv_link("binomial", X[rows] @ b[:2] + b[2]), rtol=1e-9, atol=1e-11)
    assert sum(v is None for v in pr["glm_pred"].to_list()) == 2
    # keys of another dtype: order of first appearance, one row per distinct key
    kp, Xp, yp = _frame(rng, sizes, 2, "poisson")
    names = np.array(["oak", "elm", "ash", "fir"])[(kp + 20) // 7]
    d2 = _df(names.tolist(), Xp, yp, key_name="tree")
    r2 = px.glm_by_group(d2, "tree", "x1", "x2", target="y", family="poisson", add_bias=True, tol=1e-10)
    assert r2.columns == ["tree", "coeffs", "n_iter"] and len(r2) == 4
    first = list(dict.fromkeys(names.tolist()))
    assert r2["tree"].to_list() == first
    for t, co in zip(r2["tree"].to_list(), r2["coeffs"].to_list()):
        rows = names == t
        if rows.sum() < 3:
            assert co is None
            continue
        b, _ = orc.glm_irls(Xp[rows], yp[rows], family="poisson", add_bias=True, tol=1e-10, max_iter=100)
        np.testing.assert_allclose(co, b, rtol=1e-9, atol=1e-11)
    p2 = px.glm_by_group(d2, "tree", "x1", "x2", target="y", family="poisson", add_bias=True, tol=1e-10, return_pred=True)
    assert p2.columns == ["tree", "y", "x1", "x2", "glm_pred"] and len(p2) == len(yp)


T_FUNCS = [t_logistic_reg, t_logistic_by_and_glm_by_group]


@pytest.mark.parametrize("fn", T_FUNCS, ids=lambda f: f.__name__)
def test_exprs_against_the_mock_device(fn, mock, orc):  # noqa: F811
    fn(Path(mock._name), orc)


def test_builders_validate_and_keep_the_reference_signature():
    with pytest.raises(NotImplementedError, match="logistic_reg: l1_reg / l2_reg are not supported on this backend"):
        px.logistic_reg("x1", target="y", l1_reg=0.5)
    with pytest.raises(ValueError, match="Input `max_iter` must be a positive."):
        px.logistic_reg("x1", target="y", max_iter=0)
    with pytest.raises(NotImplementedError, match="family"):
        px._glm_by(("x1",), "y", "k", "tweedie", True, 1e-8, 100, "raise", False)
    sig = inspect.signature(px.logistic_reg)
    want = {"add_bias": True, "l1_reg": 0.0, "l2_reg": 0.0, "tol": 1e-5, "max_iter": 200, "null_policy": "skip", "return_pred": False,
            "by": None}
    assert {k: sig.parameters[k].default for k in want} == want
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
@pytest.mark.parametrize("fn", T_FUNCS, ids=lambda f: f.__name__)
def test_exprs_against_the_hip_library(fn, orc):  # noqa: F811
    from polars_ds_extension_amd import _lib

    _hip_lib()
    fn(_lib.LIB_PATH, orc)


@pytest.mark.gpu
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("n_feat", [5, 10])
def test_logistic_reg_against_sklearn(n_feat, bias):
    """The reference's test_logistic_reg_against_sklearn restated: |coeffs - sklearn| < 1e-5 and |pred - predict_proba| < 1e-5 against
    LogisticRegression(penalty=None, tol=1e-6, max_iter=400) -- with abs, which the reference omits; lbfgs owns that slack, so also
    < 1e-9 against solver="newton-cholesky", tol=1e-12."""
    import pyarrow as pa
    from plugin_harness import call_plugin
    from sklearn.datasets import make_classification
    from sklearn.linear_model import LogisticRegression

    lib = _hip_lib()
    # the reference's frame (tests/test_linear_exprs.py:26-33): no redundant column -- with make_classification's default two
    # redundant columns the design is collinear and the coefficients are not identified (only pred is) -- and its tol / max_iter
    X, y = make_classification(n_samples=10_000, n_features=n_feat, n_redundant=0, n_informative=n_feat - 1, random_state=1,
                               n_clusters_per_class=1)
    ins = [("y", pa.array(y.astype(np.float64)))] + [(f"x{j + 1}", pa.array(np.ascontiguousarray(X[:, j]))) for j in range(n_feat)]
    kw = {"bias": bias, "null_policy": "skip", "l1_reg": 0.0, "l2_reg": 0.0, "solver": "", "tol": 1e-6, "max_iter": 400}
    _, co = call_plugin(lib, "pl_logistic_coeffs", ins, kw)
    _, pred = call_plugin(lib, "pl_logistic_pred", ins, kw)
    co = np.asarray(co[0].as_py())
    pred = pred.to_numpy()
    for solver, tol, bound in (("lbfgs", 1e-6, 1e-5), ("newton-cholesky", 1e-12, 1e-9)):
        sk = LogisticRegression(penalty=None, tol=tol, max_iter=400, fit_intercept=bias, solver=solver).fit(X, y)
        want = np.r_[sk.coef_.ravel(), sk.intercept_] if bias else sk.coef_.ravel()
        dc = np.abs(co - want).max()
        dp = np.abs(pred - sk.predict_proba(X)[:, 1]).max()
        print(f"n={n_feat} bias={bias} {solver}: coefficients {dc:.3e}, pred {dp:.3e}")
        assert dc < bound and dp < bound


@pytest.mark.gpu
@pytest.mark.parametrize("family,bias,p", [("binomial", True, 8), ("gamma", False, 4)])
def test_plugin_glm_by_against_lstsq(family, bias, p):
    """pl_glm_by(_pred) on host Arrow frames = lstsq.glm_by_key on the same frame: bit for bit where the plugin makes the same single
    call (no nulls: one pds_glm_irls_by_key_* call on the whole frame), ordered keys and shuffled rows alike."""
    import pyarrow as pa
    from plugin_harness import call_plugin

    import polars_ds_extension_amd as pds

    lib = _hip_lib()
    rng = np.random.default_rng(123)
    sizes = gc.ragged_sizes(rng, 200, p)
    X, y, off = gc.family_frame(rng, family, sizes, p)
    key = np.repeat(np.arange(200, dtype=np.int64) * 3 - 100, sizes)
    kw = {"bias": bias, "null_policy": "raise", "family": family, "tol": 1e-10, "max_iter": 100}
    for perm in (np.arange(len(y)), rng.permutation(len(y))):
        Xq, yq, kq = X[perm], y[perm], key[perm]
        ins = [("k", pa.array(kq)), ("y", pa.array(yq))] + [(f"x{j + 1}", pa.array(np.ascontiguousarray(Xq[:, j]))) for j in range(p)]
        _, out = call_plugin(lib, "pl_glm_by", ins, kw)
        _, pred = call_plugin(lib, "pl_glm_by_pred", ins, kw)
        ks, co, it, nu, pr, rn = pds.glm_by_key(*[np.ascontiguousarray(Xq[:, j]) for j in range(p)], target=yq, key=kq, family=family,
                                                add_bias=bias, tol=1e-10, max_iter=100, return_pred=True)
        assert out.field(0).to_pylist() == ks.tolist() and out.field(2).to_pylist() == it.tolist()
        assert [c.is_valid for c in out.field(1)] == [not v for v in nu.astype(bool)]
        got = np.array([c.as_py() for c in out.field(1) if c.is_valid])
        assert np.array_equal(got.view(np.uint8), np.ascontiguousarray(co[nu == 0]).view(np.uint8))
        assert pred.null_count == int(rn.sum())
        live = rn == 0
        assert np.array_equal(pred.to_numpy(zero_copy_only=False)[live].view(np.uint8), pr[live].view(np.uint8))
