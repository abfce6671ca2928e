"""The grouped GLM report restated in NumPy (tests/test_glm_report_cpu.py, tests/test_glm_report_gpu.py): the definitions of
DESIGN.md 4.7a for one group at GIVEN coefficients, in np.longdouble (the inverse of I: a float64 inverse refined by Newton-Schulz
steps in longdouble) or, with dtype=np.float64, the same code in plain float64 (the inverse: np.linalg.inv).  The distance between
the two is the rounding a float64 evaluation of these formulas carries on a frame: the budget of the device tests is a multiple of
it.  Also an independent longdouble Newton (IRLS) fit, for the test that the report at the device's coefficients is the report at
the maximum-likelihood estimate."""
import math

import numpy as np

Z975 = 1.959963984540054
FAMILY_ID = {"gaussian": 0, "normal": 0, "poisson": 1, "binomial": 2, "logistic": 2, "gamma": 3}
_erfc = np.vectorize(math.erfc, otypes=[np.float64])


def _inv_link(fam, eta):
    if fam == 1:
        return np.exp(eta)
    if fam == 2:
        return 1 / (1 + np.exp(-eta))
    if fam == 3:
        return 1 / eta
    return eta


def _link(fam, mu):
    if fam == 1:
        return np.log(mu)
    if fam == 2:
        return np.log(mu / (1 - mu))
    if fam == 3:
        return 1 / mu
    return mu


def _dlink(fam, mu):  # g'(mu)
    if fam == 1:
        return 1 / mu
    if fam == 2:
        return 1 / (mu * (1 - mu))
    if fam == 3:
        return -1 / (mu * mu)
    return np.ones_like(mu)


def _var(fam, mu):
    if fam == 1:
        return mu
    if fam == 2:
        return mu * (1 - mu)
    if fam == 3:
        return mu * mu
    return np.ones_like(mu)


def _xlogy(a, b):
    """a ln b with 0 ln 0 = 0"""
    out = np.zeros_like(a)
    m = a > 0
    out[m] = a[m] * np.log(b[m])
    return out


def unit_deviance(fam, y, mu):
    if fam == 1:
        return 2 * (_xlogy(y, y / mu) - (y - mu))
    if fam == 2:
        return 2 * (_xlogy(y, y / mu) + _xlogy(1 - y, (1 - y) / (1 - mu)))
    if fam == 3:
        return 2 * (-np.log(y / mu) + (y - mu) / mu)
    return (y - mu) ** 2


def _design(X, bias, dtype):
    Z = np.asarray(X).astype(dtype)
    if bias:
        Z = np.concatenate([Z, np.ones((Z.shape[0], 1), dtype=dtype)], axis=1)
    return Z


def spd_inverse(A, dtype):
    """A^-1: np.linalg.inv in float64; for longdouble three Newton-Schulz steps X <- X (2 - A X) on top of it (each squares the
    residual: from cond * 1e-16 to far below the longdouble rounding for the condition numbers of the tests)."""
    A64 = A.astype(np.float64)
    try:
        if not np.isfinite(A64).all():
            raise np.linalg.LinAlgError
        Xk = np.linalg.inv(A64).astype(dtype)
    except np.linalg.LinAlgError:  # (singular or not finite: no inverse, NaN fields)
        return np.full(A.shape, np.nan, dtype=dtype)
    if dtype is np.float64 or dtype == np.float64:
        return Xk
    eye2 = 2 * np.eye(A.shape[0], dtype=dtype)
    for _ in range(3):
        Xk = Xk @ (eye2 - A @ Xk)
    return (Xk + Xk.T) / 2


def _cond(A):
    A64 = A.astype(np.float64)
    return float(np.linalg.cond(A64)) if np.isfinite(A64).all() else float("nan")


def report_group(X, y, beta, family, bias, dtype=np.longdouble):
    """The report of one group's rows X [n, p], y [n] at the coefficients beta [p'] (bias last).  Returns a dict of `dtype` values:
    std_err, z, p, lo, hi [p'], cov [p', p'], deviance, null_deviance, pearson_chi2, dispersion, and df_resid, cond (float64
    condition number of I)."""
    fam = FAMILY_ID[family]
    Z = _design(X, bias, dtype)
    yv = np.asarray(y).astype(dtype)
    b = np.asarray(beta).astype(dtype)
    n, pp = Z.shape
    eta = Z @ b
    mu = _inv_link(fam, eta)
    v = _var(fam, mu)
    w = 1 / (_dlink(fam, mu) ** 2 * v)
    info = Z.T @ (Z * w[:, None])
    pearson = np.sum((yv - mu) ** 2 / v)
    df = n - pp
    nan = dtype(np.nan)
    phi = dtype(1) if fam in (1, 2) else (pearson / df if df > 0 else nan)
    cov = phi * spd_inverse(info, dtype)
    with np.errstate(invalid="ignore"):
        se = np.sqrt(np.diag(cov))
        z = b / se
    p = _erfc(np.abs(z.astype(np.float64)) / math.sqrt(2.0))
    if bias:
        mu0 = np.full(n, np.sum(yv) / n, dtype=dtype)
    else:
        mu0 = np.full(n, {0: 0.0, 1: 1.0, 2: 0.5, 3: np.nan}[fam], dtype=dtype)
    with np.errstate(invalid="ignore"):
        null_dev = np.sum(unit_deviance(fam, yv, mu0))
    return {"std_err": se, "z": z, "p": p, "lo": b - dtype(Z975) * se, "hi": b + dtype(Z975) * se, "cov": cov,
            "deviance": np.sum(unit_deviance(fam, yv, mu)), "null_deviance": null_dev, "pearson_chi2": pearson, "dispersion": phi,
            "df_resid": df, "cond": _cond(info)}


_COEF = ("std_err", "z", "p", "lo", "hi")
_GROUP = ("deviance", "null_deviance", "pearson_chi2", "dispersion")


def report_by(X, y, off, beta, family, bias, dtype=np.longdouble, skip=None):
    """report_group over the groups of a frame: a dict of [G, p'] / [G, p', p'] / [G] arrays of `dtype` (NaN rows for the groups in
    `skip`, a boolean [G] mask, and for groups with fewer rows than coefficients)."""
    G, pp = len(off) - 1, X.shape[1] + int(bias)
    out = {k: np.full((G, pp), np.nan, dtype=dtype) for k in _COEF}
    out["cov"] = np.full((G, pp, pp), np.nan, dtype=dtype)
    out.update({k: np.full(G, np.nan, dtype=dtype) for k in _GROUP})
    out["df_resid"] = np.zeros(G, dtype=np.int64)
    out["cond"] = np.full(G, np.nan)
    for g in range(G):
        a, e = int(off[g]), int(off[g + 1])
        out["df_resid"][g] = e - a - pp
        if e - a < pp or (skip is not None and skip[g]):
            continue
        r = report_group(X[a:e], y[a:e], beta[g], family, bias, dtype)
        for k in (*_COEF, "cov", *_GROUP, "cond"):
            out[k][g] = r[k]
    return out


def newton_fit(X, y, family, bias, tol=1e-15, max_iter=60):
    """The maximum-likelihood coefficients of one group by Newton's method in longdouble (the links are canonical: the IRLS step
    beta <- I^-1 X'W (eta + g'(mu) (y - mu)) is the Newton step), from the start the library documents (mu0 = (y + 0.5) / 2 for
    the binomial family, (y + mean y) / 2 otherwise), until the largest move is below tol * (1 + max |beta|)."""
    dtype = np.longdouble
    fam = FAMILY_ID[family]
    Z = _design(X, bias, dtype)
    yv = np.asarray(y).astype(dtype)
    mu = (yv + dtype(0.5)) / 2 if fam == 2 else (yv + np.mean(yv)) / 2
    eta = _link(fam, mu)
    b = np.zeros(Z.shape[1], dtype=dtype)
    for _ in range(max_iter):
        d = _dlink(fam, mu)
        w = 1 / (d * d * _var(fam, mu))
        info = Z.T @ (Z * w[:, None])
        rhs = Z.T @ (w * (eta + d * (yv - mu)))
        nb = spd_inverse(info, dtype) @ rhs
        nb = nb + spd_inverse(info, dtype) @ (rhs - info @ nb)  # (one step of iterative refinement)
        move = np.max(np.abs(nb - b))
        b = nb
        eta = Z @ b
        mu = _inv_link(fam, eta)
        if move < tol * (1 + np.max(np.abs(b))):
            break
    return b


def rel_err(a, ref):
    """max |a - ref| / max(|ref|, tiny) over the finite entries of ref (float64)"""
    a = np.asarray(a).astype(np.longdouble)
    ref = np.asarray(ref).astype(np.longdouble)
    m = np.isfinite(ref)
    if not m.any():
        return 0.0
    return float(np.max(np.abs(a[m] - ref[m]) / np.maximum(np.abs(ref[m]), np.longdouble(1e-300))))


def cov_err(a, ref):
    """The error of covariance matrices [G, p', p'] on the correlation scale: max over the groups with a finite reference of
    |a_ij - ref_ij| / sqrt(ref_ii ref_jj) (an off-diagonal entry may be arbitrarily close to 0: an error relative to itself has no
    bound)."""
    a = np.asarray(a).astype(np.longdouble)
    ref = np.asarray(ref).astype(np.longdouble)
    worst = 0.0
    for g in range(ref.shape[0]):
        if not np.isfinite(ref[g]).all():
            continue
        s = np.sqrt(np.diag(ref[g]))
        worst = max(worst, float(np.max(np.abs(a[g] - ref[g]) / np.outer(s, s))))
    return worst
