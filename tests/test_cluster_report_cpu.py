"""The cluster-robust reference (cluster_reference.py) against closed forms, and the Python front door's argument checks that need
no device.  Nothing here touches a GPU."""
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT))

import cluster_cases as cc  # noqa: E402
import cluster_reference as cr  # noqa: E402
import report_reference as rr  # noqa: E402


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("p", [1, 4, 16])
def test_singletons_are_hc(p, bias):
    """Every row its own cluster: s_g = x_i e_i, so M is the HC0 meat; CR1's factor is n / (n - p'): HC1."""
    F, y, off, codes = cc.singleton_frame(p, n=500)
    X = cc.design(F, bias)
    want = rr.report(X, y, "hc0")
    for se, hc in (("cluster0", "hc0"), ("cluster", "hc1")):
        got = cr.report(X, y, codes, se)
        assert cr.rel(got["std_err"], want["se_all"][hc]) < 1e-15  # (report_reference rounds its results to float64)
        assert cr.rel(got["beta"], want["beta"]) < 1e-15
        assert abs(float(got["r2"]) - want["r2"]) < 1e-15
        assert got["n_clusters"] == 500 and got["t_dof"] == 499
        # the same code in float64 agrees with itself in long double to rounding
        assert cr.rel(cr.report(X, y, codes, se, np.float64)["std_err"], got["std_err"]) < 1e-12


@pytest.mark.parametrize("k", [2, 3])
def test_duplicated_rows_scale_the_meat(k):
    """Every cluster's rows repeated k times: beta and the residuals stay, every score and so M scales by k (M by k^2)."""
    F, y, off, codes = cc.ragged_frame(4)
    X = cc.design(F, True)
    one = cr.report(X, y, codes, "cluster0")
    rep = cr.report(np.tile(X, (k, 1)), np.tile(y, k), np.tile(codes, k), "cluster0")
    assert rep["n_clusters"] == one["n_clusters"]
    assert cr.rel(rep["beta"], one["beta"]) < 1e-15
    assert cr.rel(rep["meat"], one["meat"] * k * k) < 1e-14
    # inv scales by 1 / k: V = inv M inv is unchanged
    assert cr.rel(rep["std_err"], one["std_err"]) < 1e-14


def test_codes_in_any_order():
    F, y, off, codes = cc.ragged_frame(8)
    X = cc.design(F, True)
    base = cr.report(X, y, codes, "cluster")
    perm = np.random.default_rng(1).permutation(len(y))
    got = cr.report(X[perm], y[perm], (codes * 5 - 77)[perm], "cluster")
    assert got["n_clusters"] == base["n_clusters"] == len(off) - 1
    assert cr.rel(got["std_err"], base["std_err"]) < 1e-15
    assert cr.rel(got["p"], base["p"]) < 1e-12


def test_estimator_matters_on_the_ragged_frames():
    """What the GPU tests rely on: on every ragged frame the cluster and the HC1 errors differ by more than 20 % somewhere."""
    for p in cc.WIDTHS:
        for bias in (True, False):
            w = cc.ref("ragged", p, bias, "cluster")
            ratio = np.asarray(w["se_all"]["cluster"] / w["se_all"]["hc1"], dtype=np.float64)
            assert np.max(np.abs(ratio - 1.0)) > 0.2, (p, bias, ratio)


def test_small_sample_factor():
    F, y, off, codes = cc.equal_frame(5, 4)
    X = cc.design(F, True)
    a, b = cr.report(X, y, codes, "cluster"), cr.report(X, y, codes, "cluster0")
    n, pp, g = len(y), 5, 5
    c = g / (g - 1) * (n - 1) / (n - pp)
    assert cr.rel(a["std_err"], b["std_err"] * np.sqrt(np.longdouble(c))) < 1e-15
    from scipy import stats as st

    assert np.allclose(a["p"], 2 * st.t.sf(np.abs(np.asarray(a["t"], dtype=np.float64)), g - 1), rtol=1e-14)


def test_argument_checks_need_no_device():
    """Both or neither of `cluster` / `cluster_offsets`, a cluster argument with another estimator, weights: refused before any
    context exists."""
    from polars_ds_extension_amd import _lib, lstsq

    F, y, off, codes = cc.equal_frame(4, 2)
    cols = cc.columns(F)
    with pytest.raises(ValueError, match="exactly one of"):
        lstsq.lin_reg_report(*cols, target=y, std_err="cluster")
    with pytest.raises(ValueError, match="exactly one of"):
        lstsq.lin_reg_report(*cols, target=y, std_err="cluster0", cluster=codes, cluster_offsets=off)
    with pytest.raises(ValueError, match="go with std_err"):
        lstsq.lin_reg_report(*cols, target=y, std_err="hc0", cluster_offsets=off)
    with pytest.raises(_lib.PdsError, match="weights are not supported") as e:
        lstsq.lin_reg_report(*cols, target=y, std_err="cluster", cluster=codes, weights=np.ones(len(y)))
    assert e.value.code == -5
    assert _lib.CLUSTER_SE_TYPES == {"cluster": 5, "cluster0": 6} and not set(_lib.CLUSTER_SE_TYPES) & set(_lib.SE_TYPES)
