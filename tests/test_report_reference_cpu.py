"""The high-precision per-group report (tests/report_reference.py) held against the oracle and against mpmath (no GPU needed)."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import report_reference as rr  # noqa: E402


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("p", [1, 4, 17])
def test_against_oracle(orc, p, bias):
    """Well-conditioned groups: every output within 1e-12 of the oracle's f64 report, for all five standard errors."""
    rng = np.random.default_rng(40 + p + bias)
    for n in (4 * (p + int(bias)), 150, 700):  # (leverages well below 1: HC2 / HC3 of n ~ p' amplify f64 rounding)
        X = rng.normal(size=(n, p))
        y = X @ rng.normal(size=p) + 0.5 + 0.3 * rng.normal(size=n) * (1 + np.abs(X[:, 0]))
        Xb = np.c_[X, np.ones(n)] if bias else X
        for se in rr.SE_TYPES:
            ref = rr.report(Xb, y, std_err=se)
            ro = orc.lin_reg_report(Xb, y, std_err=se)
            assert ref["dof"] == n - Xb.shape[1]
            for k in ("beta", "std_err"):
                assert rr.nrel(ref[k], ro[k]) <= 1e-12, (n, se, k)
            # t and the CI limits may cancel to near zero: measured on the scale of their terms
            bn, hw = np.linalg.norm(ro["beta"]), 0.5 * (ro["ci_hi"] - ro["ci_lo"])
            assert np.all(np.abs(ref["t"] - ro["t"]) <= 1e-12 * (bn / ro["std_err"] + np.abs(ro["t"]))), (n, se)
            for k in ("ci_lo", "ci_hi"):
                assert np.all(np.abs(ref[k] - ro[k]) <= 1e-12 * (bn + hw)), (n, se, k)
            assert np.all(np.abs(ref["p"] - ro["p"]) <= 1e-12 * np.maximum(ro["p"], 1e-3)), (n, se)
            for k in ("r2", "adj_r2"):
                assert abs(ref[k] - ro[k]) <= 1e-12 * max(1.0, abs(ro[k])), (n, se, k)
            assert np.allclose(ref["se_all"][se], ref["std_err"], rtol=0, atol=0)


def _mp_truth(X, y, digits=50):
    """beta, se and hc0..hc3 from mpmath's own LU solve / inverse (independent of the helper's elimination)."""
    import mpmath

    with mpmath.workdps(digits):
        Xm = mpmath.matrix(X.tolist())
        ym = mpmath.matrix(y.tolist())
        n, pp = X.shape
        G = Xm.T * Xm
        inv = G ** -1
        beta = mpmath.lu_solve(G, Xm.T * ym)
        e = ym - Xm * beta
        ssr = sum(e[i] ** 2 for i in range(n))
        out = {"beta": [beta[i] for i in range(pp)], "se": [mpmath.sqrt(inv[i, i] * ssr / (n - pp)) for i in range(pp)]}
        h = [sum(Xm[r, a] * inv[a, b] * Xm[r, b] for a in range(pp) for b in range(pp)) for r in range(n)]
        for name in ("hc0", "hc1", "hc2", "hc3"):
            s = [e[r] ** 2 / ((1 - h[r]) ** {"hc0": 0, "hc1": 0, "hc2": 1, "hc3": 2}[name]) for r in range(n)]
            meat = mpmath.matrix(pp, pp)
            for a in range(pp):
                for b in range(pp):
                    meat[a, b] = sum(s[r] * Xm[r, a] * Xm[r, b] for r in range(n))
            cov = inv * meat * inv
            f = mpmath.mpf(n) / (n - pp) if name == "hc1" else 1
            out[name] = [mpmath.sqrt(cov[i, i] * f) for i in range(pp)]
        return {k: np.array([float(v) for v in vals]) for k, vals in out.items()}


@pytest.mark.parametrize("digits", [None, 40])
def test_against_mpmath_ill_conditioned(orc, digits):
    """One small group with kappa(X'X) ~ 1e10: the helper (long double, and its mpmath fallback) stays within 1e-11 of a 50-digit
    computation (measured: 3e-13 in long double), where f64 arithmetic (the oracle) is ~1e-9 away."""
    rng = np.random.default_rng(3)
    n = 40
    x0 = rng.normal(size=n)
    X = np.c_[x0, x0 + 1e-3 * rng.normal(size=n), rng.normal(size=n) + 50.0, np.ones(n)]
    kappa = np.linalg.cond(X.T @ X)
    assert 3e9 <= kappa <= 1e11, kappa
    y = X[:, :3] @ np.array([1.0, -2.0, 0.01]) + 0.1 * rng.normal(size=n)
    truth = _mp_truth(X, y)
    worst_orc = 0.0
    for se in rr.SE_TYPES:
        ref = rr.report(X, y, std_err=se, digits=digits)
        assert rr.nrel(ref["beta"], truth["beta"]) <= 1e-11, se
        assert rr.nrel(ref["std_err"], truth[se]) <= 1e-11, se
        worst_orc = max(worst_orc, rr.nrel(orc.lin_reg_report(X, y, std_err=se)["beta"], truth["beta"]))
    # the case is hard enough for f64 to show it (otherwise the 1e-11 above says nothing)
    assert worst_orc >= 1e-10
