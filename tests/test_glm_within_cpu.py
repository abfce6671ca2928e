"""The fixed-effects GLM without a GPU: the C ABI surface, the reference (tests/glm_within_reference.py) -- its two routes, the
definition and the dummy-column maximum-likelihood fit, agree on every case frame, every frame converges before max_iter in float64,
the drop counts are what tests/glm_within_cases.py states and every frame keeps df_resid > 0 -- and the argument rules of
lstsq.glm_report(absorb=...) that are decided before the library is asked."""
import re
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT))

import glm_report_reference as rr  # noqa: E402
import glm_within_cases as wc  # noqa: E402
import glm_within_reference as wr  # noqa: E402

NEW = [f"pds_glm_within_{form}_{sfx}" for form in ("grouped", "by_key") for sfx in ("f64", "f32")]
CASES = [(fam, p) for fam in wc.FAMILIES for p in wc.WIDTHS]


def test_exported_declared_and_listed():
    from polars_ds_extension_amd import _lib

    assert all(n in _lib.EXPORTS for n in NEW)
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "pds_lstsq.h").read_text(), flags=re.S)
    for n in NEW:
        assert len(re.findall(rf"^int\s+{n}\s*\(", text, flags=re.M)) == 1, n
    csrc = ROOT / "polars_ds_extension_amd" / "csrc"
    assert "glm_within.hip" in (csrc / "Makefile").read_text()
    assert '#include "capi_glm_within.hpp"' in (csrc / "capi.hip").read_text()
    # the struct the binding mirrors: six coefficient rows, cov, three doubles, four int64, two int32, two pointers
    import ctypes as C

    assert C.sizeof(_lib.GlmWithinOut) == 8 * (6 * 16 + 256 + 3) + 4 * 8 + 2 * 4 + 2 * C.sizeof(C.c_void_p)


@pytest.mark.parametrize("family,p", CASES)
def test_reference_routes_agree(family, p):
    """the definition (weighted within regressions) run to a fixed point in longdouble == the dummy-column MLE in longdouble"""
    f = wc.frame(family, p)
    hi = wr.fit(f["X"], f["y"], f["codes"], family, f["pw"], f["o"], tol=1e-17, max_iter=60)
    ml = wr.dummy_mle(f["X"], f["y"], f["codes"], family, f["pw"], f["o"])
    eb, ea = rr.rel_err(hi["beta"], ml["beta"]), rr.rel_err(hi["alpha"], ml["alpha"])
    print(f"{family} p={p}: definition vs dummy MLE, beta {eb:.2g} alpha {ea:.2g} ({hi['n_iter']} iterations)")
    # two longdouble computations of one fixed point by different algebra: 1e4 longdouble ulps (1e-15), far below every f64 budget
    assert eb < 1e-15 and ea < 1e-13  # (alpha: relative to entries that may be 100 times smaller than the largest)
    assert np.array_equal(np.isnan(hi["alpha"].astype(np.float64)), ml["drop"])


@pytest.mark.parametrize("family,p", CASES)
def test_cases_converge_drop_and_keep_df(family, p):
    f = wc.frame(family, p)
    lo = wr.fit(f["X"], f["y"], f["codes"], family, f["pw"], f["o"], tol=1e-10, max_iter=100, dtype=np.float64)
    assert lo["converged"] and 2 <= lo["n_iter"] <= 8, lo["n_iter"]
    assert lo["n_groups_dropped"] == wc.DROPPED[(family, p)]
    assert lo["n_groups"] + lo["n_groups_dropped"] == len(wc.SIZES)
    assert lo["df_resid"] > 0
    l32 = wr.fit(f["X"], f["y"], f["codes"], family, f["pw"], f["o"], tol=1e-5, max_iter=100, dtype=np.float32)
    assert l32["converged"] and l32["n_iter"] <= 6


def test_report_reference_is_the_definition_at_a_fixed_point():
    """report_at at the longdouble fit: the group-wise score residuals vanish (the optimality the device is tested for) and the
    unweighted gaussian report is the linear within report (s2 W_xx^-1)"""
    f = wc.frame("poisson", 7)
    hi = wr.fit(f["X"], f["y"], f["codes"], "poisson", f["pw"], f["o"], tol=1e-17, max_iter=60)
    rep = wr.report_at(f["X"], f["y"], f["codes"], "poisson", hi["beta"], hi["alpha"], "cluster", f["pw"], f["o"])
    r, g = rep["score_r"], rep["g_used"]
    assert float(np.max(np.abs(np.bincount(g, r.astype(np.float64))))) < 1e-12 * float(np.abs(r).sum())
    assert float(np.max(np.abs(rep["score_x"].sum(axis=0)))) < 1e-12 * float(np.abs(rep["score_x"]).sum())
    assert np.isnan(rep["pred"].astype(np.float64)).sum() == 0 and rep["df_resid"] == hi["df_resid"]
    f = wc.frame("gaussian", 7)
    hi = wr.fit(f["X"], f["y"], f["codes"], "gaussian", tol=1e-17, max_iter=60)
    rep = wr.report_at(f["X"], f["y"], f["codes"], "gaussian", hi["beta"], hi["alpha"], "se")
    X, y, c = f["X"].astype(np.longdouble), f["y"].astype(np.longdouble), f["codes"]
    G = len(wc.SIZES)
    cnt = np.bincount(c).astype(np.longdouble)
    mx = np.stack([np.bincount(c, X[:, j].astype(np.float64)) for j in range(7)], axis=1) / cnt[:, None]
    Xc = X - mx[c]
    yc = y - (np.bincount(c, f["y"]) / cnt)[c]
    b = np.linalg.solve((Xc.T @ Xc).astype(np.float64), (Xc.T @ yc).astype(np.float64))
    e = yc - Xc @ b
    s2 = float(e @ e) / (len(y) - G - 7)
    se = np.sqrt(s2 * np.diag(np.linalg.inv((Xc.T @ Xc).astype(np.float64))))
    np.testing.assert_allclose(hi["beta"].astype(np.float64), b, rtol=1e-11)
    np.testing.assert_allclose(rep["std_err"].astype(np.float64), se, rtol=1e-11)


# ------------------------------------------------------------------------------------------------- lstsq.glm_report(absorb=...)
def _args():
    f = wc.frame("poisson", 1)
    return [f["X"][:, 0]], f["y"], f["codes"], f["off"]


def test_argument_rules_before_the_library():
    from polars_ds_extension_amd import lstsq

    x, y, key, off = _args()
    with pytest.raises(ValueError, match="the intercept is absorbed"):
        lstsq.glm_report(*x, target=y, family="poisson", absorb=key, add_bias=True)
    with pytest.raises(ValueError, match="exactly one of `absorb` and `absorb_offsets`"):
        lstsq.glm_report(*x, target=y, family="poisson", absorb=key, absorb_offsets=off)
    for kw in ({"cluster": key}, {"cluster_offsets": off}):
        with pytest.raises(ValueError, match='std_err="cluster" means the absorbed key'):
            lstsq.glm_report(*x, target=y, family="poisson", absorb=key, std_err="cluster", **kw)
    for kind in ("hc0", "hc1", "hc2", "hc3"):
        with pytest.raises(NotImplementedError, match="not available with absorption"):
            lstsq.glm_report(*x, target=y, family="poisson", absorb=key, std_err=kind)
    with pytest.raises(ValueError, match='std_err is "se", "cluster" or "cluster0"'):
        lstsq.glm_report(*x, target=y, family="poisson", absorb=key, std_err="robust")
    with pytest.raises(NotImplementedError, match="two or more absorbed keys"):
        lstsq.glm_report(*x, target=y, family="poisson", absorb=[key, key])
    with pytest.raises(ValueError, match="an absorbed key must be an integer column"):
        lstsq.glm_report(*x, target=y, family="poisson", absorb=key.astype(np.float64))
    with pytest.raises(NotImplementedError, match="GLM family"):
        lstsq.glm_report(*x, target=y, family="tweedie", absorb=key)
    with pytest.raises(ValueError, match="max_iter"):
        lstsq.glm_report(*x, target=y, family="poisson", absorb=key, max_iter=0)
    with pytest.raises(ValueError, match="one entry per row"):
        lstsq.glm_report(*x, target=y, family="poisson", absorb=key, weights=np.ones(3))
    with pytest.raises(ValueError, match="go with `absorb` or `absorb_offsets` only"):
        lstsq.glm_report(*x, target=y, family="poisson", return_pred=True)
    with pytest.raises(ValueError, match="go with `absorb` or `absorb_offsets` only"):
        lstsq.glm_report(*x, target=y, family="poisson", return_effects=True)
