"""MixedModel on the MI355X against the NumPy helper (mixed_reference.py) in long double.

Frames (mixed_cases.ragged_frame): seeded, 60 ragged groups -- 1, 2, 63, 64, 65, 127, 128, 129, 300 and 1 000 rows plus 50 sizes
in 3 .. 200 -- features standard normal plus a constant 3, the last feature constant within groups, y = X beta + 0.7 u_g + e;
widths 1, 4, 8, 15 and 16; each run as is and with "mixed_split_rows" = 128, which cuts the 129-, 300- and 1 000-row groups.

Budgets.  The device may be at most 10 x as far from the long double helper as the helper's own float64 arithmetic is (8 ulp where
that distance is 0).  The distances are measured on the CPU inside the tests, before anything is asserted on the device result;
distance = |a - b| / |b| for a scalar, max |a - b| / max |b| for a vector.  Measured on these frames:

  fixed gamma (worst over the five widths and gamma in {0, 1e-3, 0.5, 10, 1e3}), helper float64 vs long double:
      deviance 3.1e-12    beta 2.5e-9    residual variance 3.3e-16
  the NumPy restatement of the device's form in float64 (moments of y - [1, x] . beta0) against long double:
      deviance 1.4e-14    beta 1.1e-13   residual variance 6.8e-16
  (taken of y itself, without the first solution beta0, the same form is 4.5e-14 off on the residual variance: outside the budget)
  full fit, helper float64 vs long double per width 1 / 4 / 8 / 15 / 16 (search noise, not arithmetic):
      gamma            1.2e-7  9.0e-8  5.8e-8  1.6e-7  1.7e-7
      coefficients     2.0e-10 8.4e-10 2.2e-10 2.4e-9  2.2e-9
      standard errors  5.7e-8  4.0e-8  2.5e-8  6.5e-8  6.8e-8
      residual var.    1.0e-9  7.6e-10 4.6e-10 1.3e-9  1.2e-9
  both helper searches take 80 evaluations (2 to start, 77 steps, 1 at the optimum).
  the device (MI355X), worst over widths, gammas and both split settings:
      fixed gamma: deviance 2.5e-14   beta 1.2e-13   residual variance 5.4e-16
      full fit:    gamma 7.7e-8   coefficients 7.2e-10   standard errors 3.5e-8   residual variance 6.5e-10   80 evaluations
"""
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT))

import mixed_cases as mc  # noqa: E402
import mixed_reference as mr  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pds():
    import polars_ds_extension_amd as pds

    return pds


@pytest.fixture(scope="module")
def contexts(pds):
    """(the default context, one whose split threshold cuts every group above 128 rows)"""
    cut = pds.Context(0)
    cut.set_option("mixed_split_rows", 128)
    yield {"whole": pds.default_context(), "cut": cut}
    cut.close()


def _fit(pds, p, ctx=None, **kw):
    F, y, off, codes = mc.ragged_frame(p)
    return pds.mixed_reml(*mc.columns(F), target=y, group_offsets=off, ctx=ctx, **kw)


def _same_bits(a, b):
    for k in ("coeffs", "std_errors", "dfs"):
        assert np.array_equal(a[k], b[k]), k
    for k in ("gamma", "resid_variance", "n_groups", "n_eval"):
        assert a[k] == b[k], k


def _check_fit(got, p, what):
    """test 2's budgets: 10 x the spread of the helper's own search on that frame"""
    want, spread = mc.ref_fit(p, "longdouble"), mc.fit_spread(p)
    dist = {k: mc.rel(got[k], want[k]) for k in mc.FIT_FIELDS}
    print(f"{what} p={p}: device vs long double {dist}; helper f64 vs long double {spread}; n_eval {got['n_eval']} / {want['n_eval']}")
    for k in mc.FIT_FIELDS:
        assert dist[k] <= mc.budget(spread[k]), (k, dist[k], spread[k])
    assert abs(got["n_eval"] - want["n_eval"]) <= 2
    assert np.array_equal(got["dfs"], want["dfs"])
    assert got["n_groups"] == want["n_groups"]


@pytest.mark.parametrize("split", ["whole", "cut"])
@pytest.mark.parametrize("p", mc.WIDTHS)
def test_fixed_gamma(pds, contexts, p, split):
    """The sharp test: the evaluation on its own, at gamma in {0, 1e-3, 0.5, 10, 1e3}."""
    assert np.finfo(np.longdouble).eps < 1e-18  # the reference has to be wider than the arithmetic under test
    spread = mc.profile_spread()  # measured first, on the CPU, over every frame and gamma
    d_ld, b_ld, v_ld = mc.ref_profile(p, "longdouble")
    F, y, off, codes = mc.ragged_frame(p)
    got = pds.mixed_reml_profile(*mc.columns(F), target=y, group_offsets=off, gammas=mc.GAMMAS, ctx=contexts[split])
    assert got["beta"].shape == (len(mc.GAMMAS), p + 1)
    for k, gamma in enumerate(mc.GAMMAS):
        dist = {"deviance": mc.rel(got["deviance"][k], d_ld[k]), "beta": mc.rel(got["beta"][k], b_ld[k]),
                "resid_var": mc.rel(got["resid_variance"][k], v_ld[k])}
        print(f"p={p} {split} gamma={gamma}: device vs long double {dist}; helper f64 vs long double {spread}")
        for q in dist:
            assert dist[q] <= mc.budget(spread[q]), (q, gamma, dist[q], spread[q])


@pytest.mark.parametrize("split", ["whole", "cut"])
@pytest.mark.parametrize("p", mc.WIDTHS)
def test_full_fit(pds, contexts, p, split):
    _check_fit(_fit(pds, p, ctx=contexts[split]), p, split)


def test_reference_own_test(pds):
    """tests/test_linear_models.py:276-311 of the reference, through MixedModel.fit and report_dict (its frame: 40 groups x 25 rows
    from RandomState(42); the reference's algorithm in NumPy ends at gamma = 3.75223 on it)."""
    from polars_ds_extension_amd.linear_models import MixedModel

    rng = np.random.RandomState(42)
    n_groups, per_group = 40, 25
    n = n_groups * per_group
    beta0_true, beta1_true = 1.5, 2.0
    sigma_g, sigma_e = 1.0, 0.5
    group = np.repeat(np.arange(n_groups), per_group)
    u = rng.normal(0.0, sigma_g, n_groups)[group]
    x = rng.normal(0.0, 1.0, n)
    noise_col = rng.normal(0.0, 1.0, n)
    e = rng.normal(0.0, sigma_e, n)
    y = beta0_true + beta1_true * x + u + e
    mm = MixedModel().fit(np.column_stack([x, noise_col]), y, group)
    mm.feature_names_in_ = ["x", "noise"]
    assert mm.is_fit()
    report = mm.report_dict()
    assert report["effect"] == ["Intercept", "x", "noise"]
    beta0_hat, beta1_hat, beta_noise_hat = report["estimate"]
    assert abs(beta0_hat - beta0_true) < 0.5
    assert abs(beta1_hat - beta1_true) < 0.2
    p_x, p_noise = report["p_value"][1], report["p_value"][2]
    assert p_x < 1e-6
    assert p_noise > 0.05
    assert mm.gamma_ is not None and mm.gamma_ > 0.0
    assert np.all(mm.dfs_ > 0)
    print(f"gamma {mm.gamma_}")
    assert list(mm.dfs_) == [39.0, 958.0, 958.0]
    assert set(report) == {"effect", "estimate", "std_err", "df", "t", "p_value"}
    assert np.array_equal(report["t"], mm.coeffs_ / mm.std_errors_)
    assert repr(mm).startswith("MixedModel(Random Intercept, REML)\nGroup: None\nVariance ratio (group / residual): 3.75")
    # string labels are coded densely on the host: the same groups, the same fit
    labels = np.array([f"school-{g:02d}" for g in group])
    _same_bits(MixedModel().fit(np.column_stack([x, noise_col]), y, labels)._fit, mm._fit)


def test_boundary(pds):
    """y without any group effect: the search has to run into gamma = 0."""
    F, y, off, codes = mc.boundary_frame()
    for dtype in (np.float64, np.longdouble):  # checked on the CPU first
        assert float(mr.fit_reml(mr.design(F, dtype), y, codes, len(off) - 1, dtype=dtype)["gamma"]) <= 1e-9
    got = pds.mixed_reml(*mc.columns(F), target=y, group_offsets=off)
    print(f"boundary gamma {got['gamma']}")
    assert 0.0 <= got["gamma"] <= 1e-9
    assert np.all(np.isfinite(got["std_errors"])) and np.all(got["std_errors"] > 0)


@pytest.mark.parametrize("p", [4, 16])
def test_forms_agree(pds, p):
    import torch

    F, y, off, codes = mc.ragged_frame(p)
    cols = mc.columns(F)
    base = pds.mixed_reml(*cols, target=y, group_offsets=off)
    _same_bits(pds.mixed_reml(*cols, target=y, group_offsets=off), base)  # two identical calls
    _same_bits(pds.mixed_reml(*cols, target=y, key=codes * 3 - 50), base)  # ordered keys: nothing moves
    dev = torch.device("cuda", 0)
    tcols = [torch.from_numpy(c).to(dev) for c in cols]
    ty = torch.from_numpy(np.ascontiguousarray(y)).to(dev)
    _same_bits(pds.mixed_reml(*tcols, target=ty, group_offsets=torch.from_numpy(off).to(dev)), base)
    _same_bits(pds.mixed_reml(*tcols, target=ty, key=torch.from_numpy(codes * 3 - 50).to(dev)), base)
    # rows shuffled: unordered keys, the sort + gather route
    perm = np.random.default_rng(5).permutation(len(y))
    shuffled = pds.mixed_reml(*[c[perm] for c in cols], target=y[perm], key=(codes * 3 - 50)[perm])
    _check_fit(shuffled, p, "shuffled")


@pytest.mark.parametrize("p", [4, 16])
def test_f32_frame(pds, p):
    """An f32 frame against the f64 fit of the same rounded values: the arithmetic is f64 either way."""
    F, y, off, codes = mc.ragged_frame(p)
    F32, y32 = F.astype(np.float32), y.astype(np.float32)
    want = pds.mixed_reml(*mc.columns(F32.astype(np.float64)), target=y32.astype(np.float64), group_offsets=off)
    pds.config.LIN_REG_EXPR_F64 = False
    try:
        got = pds.mixed_reml(*mc.columns(F32), target=y32, group_offsets=off)
        prof = pds.mixed_reml_profile(*mc.columns(F32), target=y32, group_offsets=off, gammas=[0.5])
    finally:
        pds.config.LIN_REG_EXPR_F64 = True
    spread = mc.fit_spread(p)
    dist = {k: mc.rel(got[k], want[k]) for k in mc.FIT_FIELDS}
    print(f"f32 p={p}: {dist}; budgets from {spread}")
    for k in mc.FIT_FIELDS:
        assert dist[k] <= mc.budget(spread[k]), (k, dist[k], spread[k])
    assert np.array_equal(got["dfs"], want["dfs"]) and abs(got["n_eval"] - want["n_eval"]) <= 2
    assert np.isfinite(prof["deviance"][0])


def test_empty_groups(pds, contexts):
    """Empty groups in the offsets change no output bit and are not counted, with whole groups and with the long ones cut into chunks
    (a host frame, empty groups and chunks in one call)."""
    F, y, off, codes = mc.ragged_frame(4)
    cols = mc.columns(F)
    padded = np.concatenate([[0, 0], off[:20], [off[19], off[19]], off[20:], [off[-1]]])
    for ctx in contexts.values():
        base = pds.mixed_reml(*cols, target=y, group_offsets=off, ctx=ctx)
        got = pds.mixed_reml(*cols, target=y, group_offsets=padded, ctx=ctx)
        assert got["n_groups"] == len(off) - 1 == base["n_groups"]
        _same_bits(got, base)
        a = pds.mixed_reml_profile(*cols, target=y, group_offsets=off, gammas=mc.GAMMAS, ctx=ctx)
        b = pds.mixed_reml_profile(*cols, target=y, group_offsets=padded, gammas=mc.GAMMAS, ctx=ctx)
        for k in a:
            assert np.array_equal(a[k], b[k]), k


def test_all_singletons(pds):
    """Every group one row: H = (1 + gamma) I, the deviance does not depend on gamma and the helper's search wanders without an error
    (it ends wherever the rounding noise sends it).  Pinned: the device returns too; its coefficients are the OLS solution, which no
    gamma changes; every column counts as between, so every df is n - p'."""
    rng = np.random.default_rng(3)
    n = 50
    F = rng.normal(size=(n, 2)) + 3.0
    y = 1.0 + F @ np.array([1.0, -2.0]) + rng.normal(size=n)
    codes = np.arange(n)
    f64 = mr.fit_reml(mr.design(F), y, codes, n)
    fld = mr.fit_reml(mr.design(F, np.longdouble), y, codes, n, dtype=np.longdouble)
    got = pds.mixed_reml(*mc.columns(F), target=y, group_offsets=np.arange(n + 1))
    spread = mc.rel(f64["coeffs"], fld["coeffs"])
    print(f"singletons: device gamma {got['gamma']}, coeffs off by {mc.rel(got['coeffs'], fld['coeffs'])}; helper f64 vs long double {spread}")
    assert 0.0 <= got["gamma"] <= 1e6 and got["n_groups"] == n
    assert mc.rel(got["coeffs"], fld["coeffs"]) <= mc.budget(spread)
    assert list(got["dfs"]) == list(fld["dfs"]) == [47.0, 47.0, 47.0]
    assert np.all(np.isfinite(got["std_errors"]))


def test_errors(pds):
    from polars_ds_extension_amd._lib import PdsError

    F, y, off, codes = mc.ragged_frame(4)
    cols = mc.columns(F)
    with pytest.raises(PdsError, match="X'HiX is not positive definite; design may be rank-deficient.") as e:
        pds.mixed_reml(*cols, cols[1], target=y, group_offsets=off)  # a duplicated feature column
    assert e.value.code == -6
    ynan = y.copy()
    ynan[777] = np.nan
    with pytest.raises(PdsError, match="Residual variance estimate is non-positive.") as e:
        pds.mixed_reml(*cols, target=ynan, group_offsets=off)
    assert e.value.code == -6
    with pytest.raises(PdsError, match="up to 16 feature columns") as e:
        pds.mixed_reml(*[cols[0]] * 17, target=y, group_offsets=off)
    assert e.value.code == -5  # PDS_ERR_UNSUPPORTED
    with pytest.raises(PdsError, match="Not enough rows to fit a mixed model with this many fixed effects.") as e:
        pds.mixed_reml(*[c[:5] for c in cols], target=y[:5], group_offsets=np.array([0, 2, 5]))  # n = p' = 5
    assert e.value.code == -3  # PDS_ERR_TOO_FEW_ROWS
    with pytest.raises(PdsError, match="group offsets must be non-decreasing and inside the frame") as e:
        pds.mixed_reml(*cols, target=y, group_offsets=np.array([0, 50, 40, len(y)]))
    assert e.value.code == -1
    # a failed call leaves the context usable
    assert pds.mixed_reml(*cols, target=y, group_offsets=off)["n_eval"] == mc.ref_fit(4, "longdouble")["n_eval"]
