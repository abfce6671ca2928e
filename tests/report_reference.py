"""
A high-precision restatement of one lin_reg_report (test infrastructure): the report of a single group's rows in np.longdouble
(80-bit extended on x86-64: a 64-bit significand), or with mpmath at `digits` decimal digits where the platform's long double is
narrower (40 digits) or when a caller asks for it.  It is the "truth" the grouped report's accuracy tests measure the device and
the oracle against; nothing in it follows either one's operation order.

    report(X, y, std_err="se", y_var=None, digits=None) -> dict
        X: [n, p'] with the bias column already appended (as the oracle takes it); y: [n]
        beta, std_err (the requested type), se_all (all five types), t, p, ci_lo, ci_hi, r2, adj_r2, dof, h (leverages)
    beta(X, y, digits=None) -> the coefficients alone, formed the same way (tests/partition_cases.py)

Gram X'X and X'y in extended precision, the inverse by Gauss-Jordan elimination with complete pivoting, beta = inv X'y plus one
step of iterative refinement, residuals, leverages h_i = x_i' inv x_i, the sandwich inv (X' diag(s) X) inv, and var(y)
(ddof = 1) from the centred target.  Where dof = n - p' is 0, se and hc1 (which divide by dof) are NaN.  p-values and the CI
quantile come from scipy.stats.t in f64 at the report's own t.
"""
from __future__ import annotations

import contextlib

import numpy as np

SE_TYPES = ("se", "hc0", "hc1", "hc2", "hc3")
EXTENDED = np.finfo(np.longdouble).nmant >= 63


class _Ld:
    ctx = contextlib.nullcontext

    @staticmethod
    def arr(a):
        return np.asarray(a, np.float64).astype(np.longdouble)

    @staticmethod
    def sqrt(a):
        with np.errstate(invalid="ignore"):
            return np.sqrt(a)

    @staticmethod
    def eye(n):
        return np.eye(n, dtype=np.longdouble)


class _Mp:
    def __init__(self, digits):
        import mpmath

        self.mp = mpmath
        self.digits = digits

    def ctx(self):
        return self.mp.workdps(self.digits)

    def arr(self, a):
        return np.vectorize(lambda v: self.mp.mpf(float(v)), otypes=[object])(np.asarray(a, np.float64))

    def sqrt(self, a):
        return np.vectorize(lambda v: self.mp.sqrt(v) if v >= 0 else self.mp.mpf("nan"), otypes=[object])(a)

    def eye(self, n):
        return self.arr(np.eye(n))


def _f64(a):
    a = np.asarray(a)
    return a.astype(np.float64)


def inverse(G, ops):
    """Gauss-Jordan elimination with complete pivoting on [G | I]."""
    n = G.shape[0]
    A = G.copy()
    E = ops.eye(n)
    cols = np.arange(n)
    for k in range(n):
        sub = np.abs(_f64(A[k:, k:]))
        i, j = np.unravel_index(int(np.argmax(sub)), sub.shape)
        i, j = int(i) + k, int(j) + k
        A[[k, i]], E[[k, i]] = A[[i, k]], E[[i, k]]
        A[:, [k, j]] = A[:, [j, k]]
        cols[[k, j]] = cols[[j, k]]
        piv = A[k, k]
        A[k] = A[k] / piv
        E[k] = E[k] / piv
        f = A[:, k].copy()
        f[k] = 0 * f[k]
        A -= np.outer(f, A[k])
        E -= np.outer(f, E[k])
    # E G P = I (row operations E, column permutation P: (G P)[:, k] = G[:, cols[k]]) -> G^-1 = P E
    out = E.copy()
    out[cols] = E
    return out


def report(X, y, std_err="se", y_var=None, digits=None) -> dict:
    from scipy import stats as st

    ops = _Ld() if digits is None and EXTENDED else _Mp(digits or 40)
    X = np.asarray(X, np.float64)
    y = np.asarray(y, np.float64)
    n, pp = X.shape
    dof = n - pp
    nan = np.full(pp, np.nan)
    with ops.ctx():
        Xl, yl = ops.arr(X), ops.arr(y)
        G = Xl.T @ Xl
        xty = Xl.T @ yl
        inv = inverse(G, ops)
        beta = inv @ xty
        beta = beta + inv @ (xty - G @ beta)  # one refinement step
        e = yl - Xl @ beta
        e2 = e * e
        ssr = e2.sum()
        h = ((Xl @ inv) * Xl).sum(axis=1)
        se_all = {"se": _f64(ops.sqrt(np.diag(inv) * (ssr / dof))) if dof > 0 else nan}
        for name, s in (("hc0", e2), ("hc1", e2), ("hc2", e2 / (1 - h)), ("hc3", e2 / ((1 - h) * (1 - h)))):
            v = np.diag(inv @ ((Xl * s[:, None]).T @ Xl) @ inv)
            if name == "hc1":
                v = v * n / dof if dof > 0 else None
            se_all[name] = _f64(ops.sqrt(v)) if v is not None else nan
        yc = yl - yl.sum() / n
        yv = (yc * yc).sum() / (n - 1) if y_var is None else ops.arr([y_var])[0]
        ratio = ssr / (yv * n)
        r2 = float(1 - ratio)
        adj = float(1 - ratio * (n - 1) / (dof - 1)) if dof != 1 else -np.inf
        b, h = _f64(beta), _f64(h)
    se_v = se_all[std_err]
    with np.errstate(divide="ignore", invalid="ignore"):
        t = b / se_v
        p = 2.0 * st.t.sf(np.abs(t), dof) if dof > 0 else nan
        tc = st.t.ppf(0.975, dof) if dof > 0 else np.nan
    return {"beta": b, "std_err": se_v, "se_all": se_all, "t": t, "p": p, "ci_lo": b - tc * se_v, "ci_hi": b + tc * se_v,
            "r2": r2, "adj_r2": adj, "dof": dof, "h": h}


def beta(X, y, digits=None) -> np.ndarray:
    """The coefficients alone, the way report() forms them: extended-precision normal equations, `inverse`, one refinement step."""
    ops = _Ld() if digits is None and EXTENDED else _Mp(digits or 40)
    with ops.ctx():
        Xl, yl = ops.arr(X), ops.arr(y)
        G = Xl.T @ Xl
        xty = Xl.T @ yl
        inv = inverse(G, ops)
        b = inv @ xty
        b = b + inv @ (xty - G @ b)
        return _f64(b)


def nrel(a, truth) -> float:
    """Normwise relative distance ||a - truth|| / ||truth||, in f64."""
    a, truth = np.asarray(a, np.float64), np.asarray(truth, np.float64)
    return float(np.linalg.norm(a - truth) / max(np.linalg.norm(truth), 1e-300))
