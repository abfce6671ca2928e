"""pl_glm_report_robust on the product library and GLM.fit(report=True, std_err=...): the struct and the model's attributes hold the
bits of the lstsq.glm_report call on the same frame (keys with a null cluster included), and a null policy gives what lstsq gives on
the rows that survive it (tests/test_cluster_report_polars_gpu.py's arrangement: the plugin symbol through tests/plugin_harness.py,
Arrow in and out)."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT))

import glm_sandwich_cases as sc  # noqa: E402
import glm_sandwich_reference as sr  # noqa: E402

P = 4
NAMES = ["beta", "std_err", "z", "p>|z|", "0.025", "0.975", "deviance", "null_deviance", "dispersion", "n_iter", "n_clusters"]


@pytest.fixture(scope="module")
def pds():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import polars_ds_extension_amd as m

    return m


@pytest.fixture(scope="module")
def lib(pds):
    from polars_ds_extension_amd import _lib

    return C.CDLL(str(_lib.LIB_PATH))


@pytest.fixture(scope="module")
def frame():
    rng = np.random.default_rng(909)
    sizes = [5, 70, 9, 130, 3, 40]
    X, y, pw, o = sc.one_model_frame(rng, "poisson", sum(sizes), P)
    key = sc.codes_of(np.concatenate([[0], np.cumsum(sizes)])) * 7 - 20
    perm = rng.permutation(len(y))
    return key[perm], X[perm], y[perm], pw[perm], o[perm]


def _cols(X):
    return [np.ascontiguousarray(X[:, j]) for j in range(X.shape[1])]


def _kw(kind, key, pw, o, **more):
    return dict({"bias": True, "null_policy": "raise", "family": "poisson", "tol": 1e-10, "max_iter": 100, "std_err": kind,
                 "has_cluster": key is not None, "has_weights": pw is not None, "has_offset": o is not None}, **more)


def _inputs(key, X, y, pw, o, key_mask=None, masks=None):
    import pyarrow as pa

    masks = masks or {}
    ins = [] if key is None else [("firm", pa.array(key, type=pa.int64(), mask=key_mask))]
    ins += [(nm, pa.array(c)) for nm, c in (("w", pw), ("o", o)) if c is not None]
    ins.append(("y", pa.array(y, mask=masks.get(0))))
    return ins + [(f"x{j + 1}", pa.array(np.ascontiguousarray(X[:, j]), mask=masks.get(j + 1))) for j in range(X.shape[1])]


def _same_bits(out, r):
    assert [f.name for f in out.type] == ["features", *NAMES] and len(out) == P + 1
    assert out.field(0).to_pylist() == [f"x{j + 1}" for j in range(P)] + ["__bias__"]
    for i, name in enumerate(NAMES):
        got = out.field(1 + i).to_numpy(zero_copy_only=False)
        want = np.broadcast_to(np.asarray(r[name]), (P + 1,))
        assert np.array_equal(got, want.astype(got.dtype), equal_nan=True), name


def _lstsq(pds, kind, key, X, y, pw, o):
    return pds.glm_report(*_cols(X), target=y, family="poisson", add_bias=True, tol=1e-10, max_iter=100, std_err=kind,
                          cluster=key if kind in sr.CLUSTER_KINDS else None, weights=pw, offset=o)


@pytest.mark.parametrize("kind", sc.KINDS)
def test_plugin_holds_the_lstsq_bits(pds, lib, frame, kind):
    from plugin_harness import call_plugin

    key, X, y, pw, o = frame
    k = key if kind in sr.CLUSTER_KINDS else None
    field, out = call_plugin(lib, "pl_glm_report_robust", _inputs(k, X, y, pw, o), _kw(kind, k, pw, o))
    assert field.name == "glm_report" and field.type == out.type
    r = _lstsq(pds, kind, key, X, y, pw, o)
    assert r["n_clusters"] == (6 if k is not None else 0) and r["report_null"] == 0
    _same_bits(out, r)
    if k is not None:  # a null key is one cluster: the same clusters, whatever value stands in for it
        _, out2 = call_plugin(lib, "pl_glm_report_robust", _inputs(k, X, y, pw, o, key_mask=key == key.max()), _kw(kind, k, pw, o))
        _same_bits(out2, r)


@pytest.mark.parametrize("kind", ["cluster", "hc1"])
def test_plugin_null_policy_is_lstsq_on_the_surviving_rows(pds, lib, frame, kind):
    from plugin_harness import call_plugin

    key, X, y, pw, o = frame
    k = key if kind == "cluster" else None
    rng = np.random.default_rng(3)
    masks = {0: rng.uniform(size=len(y)) < 0.05, 2: rng.uniform(size=len(y)) < 0.1}
    keep = ~(masks[0] | masks[2])
    _, out = call_plugin(lib, "pl_glm_report_robust", _inputs(k, X, y, pw, o, masks=masks), _kw(kind, k, pw, o, null_policy="skip"))
    order = np.argsort(key[keep], kind="stable") if k is not None else np.arange(int(keep.sum()))  # (the plugin's host preparation)
    sel = np.flatnonzero(keep)[order]
    _same_bits(out, _lstsq(pds, kind, key[sel], X[sel], y[sel], pw[sel], o[sel]))


@pytest.mark.parametrize("kind", sc.KINDS)
def test_glm_fit_fills_its_attributes_from_the_same_numbers(pds, frame, kind):
    from polars_ds_extension_amd.linear_models import GLM

    key, X, y, pw, o = frame
    k = key if kind in sr.CLUSTER_KINDS else None
    m = GLM(family="poisson", add_bias=True, tol=1e-10).fit(X, y, report=True, std_err=kind, cluster=k, sample_weight=pw, offset=o)
    r = pds.glm_report(*_cols(X), target=y, family="poisson", add_bias=True, tol=1e-10, max_iter=100, std_err=kind, cluster=k, weights=pw,
                       offset=o, return_cov=True)
    assert np.array_equal(np.append(m.coeffs(), m.bias()), r["beta"]) and m.n_iter_ == int(r["n_iter"])
    for attr, name in (("std_errors_", "std_err"), ("z_", "z"), ("p_values_", "p>|z|"), ("ci_lower_", "0.025"), ("ci_upper_", "0.975"),
                       ("cov_", "cov")):
        assert np.array_equal(getattr(m, attr), r[name]), attr
    assert (m.deviance_, m.dispersion_, m.df_resid_, m.n_clusters_) == (float(r["deviance"]), float(r["dispersion"]), int(r["df_resid"]),
                                                                        r["n_clusters"])
    assert m.n_clusters_ == (6 if k is not None else 0) and m.std_err_type_ == kind
    rep = m.report_dict()
    assert np.array_equal(rep["std_err"], r["std_err"]) and rep["features"][-1] == "__bias__"
    # the default call is untouched: model-based errors, no robust attributes
    d = GLM(family="poisson", add_bias=True, tol=1e-10).fit(X, y, report=True, sample_weight=pw, offset=o)
    if k is None:  # (the same fit to the bit; a shuffled key column fits the frame in key order: the same sums in another order)
        assert np.array_equal(d.coeffs(), m.coeffs())
    np.testing.assert_allclose(d.coeffs(), m.coeffs(), rtol=1e-9)
    assert not np.array_equal(d.std_errors_, m.std_errors_) and not hasattr(d, "n_clusters_")


def test_polars_expression_on_the_product_library(pds, frame):
    """polars_exprs.glm_report(std_err=, cluster=) through the engine (the real polars if importable, else tests/mini_polars)"""
    from test_polars_exprs import pl, px

    key, X, y, pw, o = frame
    df = pl.DataFrame({"firm": key, "y": y, **{f"x{j + 1}": X[:, j] for j in range(P)}, "w": pw, "o": o})
    for kind in ("cluster", "hc0"):
        rep = df.select(px.glm_report(*[f"x{j + 1}" for j in range(P)], target="y", family="poisson", add_bias=True, tol=1e-10, std_err=kind,
                                      cluster="firm" if kind == "cluster" else None, weights="w", offset="o")).unnest("glm_report")
        r = _lstsq(pds, kind, key, X, y, pw, o)
        assert rep.columns == ["features", *NAMES]
        for name in ("beta", "std_err", "z", "p>|z|", "0.025", "0.975"):
            assert np.array_equal(rep[name].to_numpy(), r[name]), name
        assert rep["n_clusters"].to_list() == [r["n_clusters"]] * (P + 1)
