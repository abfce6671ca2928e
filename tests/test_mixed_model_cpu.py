"""MixedModel without a GPU: the NumPy reference helper against dense algebra, the moment identity the device form rests on, the
public surface (names, defaults, exported C symbols, header declarations) and every validation error that is raised before a
context exists."""
import inspect
import re
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT))

import mixed_cases as mc  # noqa: E402
import mixed_reference as mr  # noqa: E402

NEW = ["pds_mixed_reml_grouped_f64", "pds_mixed_reml_grouped_f32", "pds_mixed_reml_by_key_f64", "pds_mixed_reml_by_key_f32",
       "pds_mixed_profile_grouped_f64", "pds_mixed_profile_grouped_f32"]


def _small_frame(seed=11, p=3):
    rng = np.random.default_rng(seed)
    sizes = np.array([1, 2, 5, 17, 40, 3, 64, 29, 70, 31])
    codes = np.repeat(np.arange(len(sizes)), sizes)
    n = int(sizes.sum())  # 262 rows
    F = rng.normal(size=(n, p)) + 3.0
    F[:, p - 1] = (rng.normal(size=len(sizes)) + 3.0)[codes]
    y = 0.5 + F @ rng.normal(size=p) + 0.7 * rng.normal(size=len(sizes))[codes] + rng.normal(size=n)
    return F, y, codes, len(sizes)


@pytest.mark.parametrize("dtype", [np.float64, np.longdouble])
def test_helper_against_dense_algebra(dtype):
    """V = I + gamma Z Z' built explicitly (n = 262): GLS beta, r' V^-1 r and both log-determinants at five gammas."""
    F, y, codes, G = _small_frame()
    X = mr.design(F)
    n, p = X.shape
    Z = np.zeros((n, G))
    Z[np.arange(n), codes] = 1.0
    for gamma in mc.GAMMAS:
        V = np.eye(n) + gamma * Z @ Z.T
        Vi = np.linalg.inv(V)
        xvx = X.T @ Vi @ X
        beta = np.linalg.solve(xvx, X.T @ Vi @ y)
        r = y - X @ beta
        rvr = r @ Vi @ r
        got = mr.profile(mr.design(F, dtype), y, codes, G, gamma, dtype)
        # dense f64 algebra on a 262 x 262 inverse is the weaker side: 1e-9 covers cond(V) <= 1 + 70 gamma at gamma = 1e3
        np.testing.assert_allclose(got["beta"].astype(np.float64), beta, rtol=1e-9, atol=1e-9)
        assert abs(float(got["rhr"]) - rvr) <= 1e-9 * rvr
        assert abs(float(got["logdet_h"]) - np.linalg.slogdet(V)[1]) <= 1e-9 * max(1.0, np.linalg.slogdet(V)[1])
        assert abs(float(got["logdet_xhx"]) - np.linalg.slogdet(xvx)[1]) <= 1e-9 * abs(np.linalg.slogdet(xvx)[1]) + 1e-9
        dev = (n - p) * np.log(rvr / (n - p)) + np.linalg.slogdet(V)[1] + np.linalg.slogdet(xvx)[1]
        assert abs(float(got["deviance"]) - dev) <= 1e-9 * abs(dev)


def test_moment_identity():
    """[X y]' H^-1 [X y] = W + sum_g c_g m_g m_g' (c_g = n_g / (1 + gamma n_g)), and beta / r' H^-1 r / ln det(X' H^-1 X) read off
    its Cholesky factor with y ordered last, against the helper's Woodbury form in long double."""
    ld = np.longdouble
    F, y, codes, G = _small_frame(seed=12, p=4)
    X = mr.design(F, ld)
    n = len(y)
    counts = mr.group_counts(codes, G, ld)
    for gamma in mc.GAMMAS:
        z = np.concatenate([X, np.asarray(y, dtype=ld)[:, None]], axis=1)
        direct = z.T @ mr.apply_hi(z, codes, counts, ld(gamma))
        m = mr.moment_form(X, y, codes, G, gamma, ld)
        assert mc.rel(m, direct) < 1e-16
        assert np.all(m[0, :] == m[:, 0])  # W's intercept row and column are zero: row 0 is sum_g c_g m_g alone
        want = mr.profile(X, y, codes, G, gamma, ld)
        beta, rhr, logdet, dev = mr.solve_moment_form(m, n, want["logdet_h"])
        assert mc.rel(beta, want["beta"]) < 1e-14
        assert mc.rel(rhr, want["rhr"]) < 1e-14
        assert mc.rel(logdet, want["logdet_xhx"]) < 1e-15
        assert mc.rel(dev, want["deviance"]) < 1e-15
    # the between column: exactly constant inside every group, so its centred values vanish
    assert mr.between_columns(np.asarray(X, dtype=np.float64), codes) == [0, 4]


def test_helper_search_and_errors():
    F, y, codes, G = _small_frame()
    fit = mr.fit_reml(mr.design(F), y, codes, G)
    assert fit["n_eval"] == 80 and 0.0 < float(fit["gamma"]) < 1e6  # 2 + 77 steps (1e6 phi^77 < 1e-10) + the final evaluation
    assert list(fit["dfs"]) == [G - 2.0, 262.0 - G - 2.0, 262.0 - G - 2.0, G - 2.0]
    assert mr.fit_reml(mr.design(F), y, codes, G, max_iter=0)["n_eval"] == 3
    with pytest.raises(ValueError, match="Not enough rows"):
        mr.fit_reml(mr.design(F[:4]), y[:4], codes[:4], 3)
    with pytest.raises(ValueError, match="non-positive"):
        mr.profile(mr.design(F), np.where(np.arange(len(y)) == 5, np.nan, y), codes, G, 0.5)


def test_exported_and_declared():
    from polars_ds_extension_amd import _lib

    assert all(n in _lib.EXPORTS for n in NEW)
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "pds_lstsq.h").read_text(), flags=re.S)
    for n in NEW:
        assert len(re.findall(rf"^int\s+{n}\s*\(", text, flags=re.M)) == 1, n
    so = _lib.load()
    assert all(hasattr(so, n) for n in NEW)
    csrc = ROOT / "polars_ds_extension_amd" / "csrc"
    assert "mixed.hip" in (csrc / "Makefile").read_text()
    assert '#include "capi_mixed.hpp"' in (csrc / "capi.hip").read_text()


def test_public_names_and_defaults():
    import polars_ds_extension_amd as pds
    from polars_ds_extension_amd import linear_models, lstsq

    for n in ("mixed_reml", "mixed_reml_profile"):
        assert callable(getattr(pds, n)) and n in lstsq.__all__
    assert "MixedModel" in linear_models.__all__
    sig = inspect.signature(pds.mixed_reml)
    want = {"group_offsets": None, "key": None, "max_iter": 200, "tol": 1e-10, "ctx": None}
    assert {k: sig.parameters[k].default for k in want} == want
    assert list(inspect.signature(pds.mixed_reml_profile).parameters)[1:] == ["target", "group_offsets", "gammas", "ctx"]
    mm = linear_models.MixedModel
    for meth, want in (("fit_df", {"null_policy": "skip", "max_iter": 200, "tol": 1e-10}),
                       ("fit", {"null_policy": "ignore", "max_iter": 200, "tol": 1e-10})):
        sig = inspect.signature(getattr(mm, meth))
        assert {k: sig.parameters[k].default for k in want} == want
    assert list(inspect.signature(mm.fit_df).parameters)[1:5] == ["df", "features", "target", "group"]
    m = mm()
    assert not m.is_fit() and repr(m) == "MixedModel (not fitted yet)"
    for call in (m.report, m.report_dict):
        with pytest.raises(ValueError, match="Model is not fit yet."):
            call()


def test_validation_without_a_device():
    """Every one of these raises before a context is created (no GPU here: reaching the device would raise PdsError)."""
    import polars_ds_extension_amd as pds
    from polars_ds_extension_amd.linear_models import MixedModel

    x, y = np.arange(12.0), np.arange(12.0) ** 2
    off, key = np.array([0, 6, 12]), np.repeat([0, 1], 6)
    with pytest.raises(ValueError, match="exactly one of `group_offsets` and `key`"):
        pds.mixed_reml(x, target=y)
    with pytest.raises(ValueError, match="exactly one of `group_offsets` and `key`"):
        pds.mixed_reml(x, target=y, group_offsets=off, key=key)
    with pytest.raises(ValueError, match="max_iter"):
        pds.mixed_reml(x, target=y, group_offsets=off, max_iter=-1)
    for bad in (np.nan, np.inf):
        with pytest.raises(ValueError, match="tol"):
            pds.mixed_reml(x, target=y, group_offsets=off, tol=bad)
    with pytest.raises(ValueError, match="at least one feature"):
        pds.mixed_reml(target=y, group_offsets=off)
    with pytest.raises(ValueError, match="X, y, and group must have the same number of rows."):
        pds.mixed_reml(x[:11], target=y, group_offsets=off)
    with pytest.raises(ValueError, match="X, y, and group must have the same number of rows."):
        pds.mixed_reml(x, target=y, key=key[:11])
    with pytest.raises(ValueError, match="X, y, and group must have the same number of rows."):
        pds.mixed_reml_profile(x, target=y[:5], group_offsets=off, gammas=[0.5])
    for bad in ([-1.0], [np.nan], [[0.5, 1.0]]):
        with pytest.raises(ValueError, match="gammas"):
            pds.mixed_reml_profile(x, target=y, group_offsets=off, gammas=bad)
    with pytest.raises(ValueError, match="X, y, and group must have the same number of rows."):
        MixedModel().fit(x.reshape(-1, 1), y, key[:7])
    with pytest.raises(ValueError, match="2D"):
        MixedModel().fit(x, y, key)


def test_no_cpu_fallback_without_device():
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    import polars_ds_extension_amd as pds
    from polars_ds_extension_amd import _lib
    from polars_ds_extension_amd.linear_models import MixedModel

    F, y, codes, G = _small_frame()
    off = np.concatenate([[0], np.cumsum(np.bincount(codes))])
    for call in (lambda: pds.mixed_reml(*mc.columns(F), target=y, group_offsets=off),
                 lambda: pds.mixed_reml(*mc.columns(F), target=y, key=codes),
                 lambda: pds.mixed_reml_profile(*mc.columns(F), target=y, group_offsets=off, gammas=[0.5]),
                 lambda: MixedModel().fit(F, y, codes)):
        with pytest.raises(_lib.PdsError) as e:
            call()
        assert e.value.code == -4  # PDS_ERR_HIP: nothing is computed on the CPU
