"""
A high-precision restatement of lin_reg_report with cluster-robust standard errors (TEST INFRASTRUCTURE ONLY): one model over the
whole frame, V = c inv M inv with M = sum_g s_g s_g', s_g = X_g' e_g the score of cluster g; CR1: c = G / (G - 1) (n - 1) / (n - p'),
CR0: c = 1; t, p and the 95 % interval from the Student t with G - 1 degrees of freedom (Stata's vce(cluster), statsmodels'
cov_type="cluster" with use_t=True, R's vcovCL).  G counts the clusters that have rows.

    report(X, y, codes, std_err="cluster", dtype=np.longdouble, y_var=None) -> dict
        X: [n, p'] with the bias column already appended (as report_reference takes it); y: [n]; codes: [n] integers in any order
        beta, std_err, se_all ("cluster", "cluster0", "hc0", "hc1"), meat, t, p, ci_lo, ci_hi, r2, adj_r2, n_clusters

On top of report_reference.py: its `inverse` (Gauss-Jordan with complete pivoting) and its beta with one refinement step.  The scores
are summed per cluster, in the frame's arithmetic; nothing follows the device's operation order.  `dtype` is the arithmetic of the
whole computation: np.longdouble is the truth the tests measure against, np.float64 (and np.float32) the same code in the narrower
format, whose distance from the long double result is what a budget is made of.
"""
from __future__ import annotations

import numpy as np

import report_reference as rr

SE_TYPES = ("cluster", "cluster0")
FIELDS = ("beta", "std_err", "t", "r2", "adj_r2")  # the fields a budget is measured for


class _Ops:
    def __init__(self, dtype):
        self.dtype = dtype

    def eye(self, n):
        return np.eye(n, dtype=self.dtype)


def scores(X, e, codes):
    """S [G, p']: row g = X_g' e_g, the clusters in ascending order of their code."""
    order = np.argsort(codes, kind="stable")
    c = np.asarray(codes)[order]
    starts = np.flatnonzero(np.concatenate([[True], c[1:] != c[:-1]]))
    return np.add.reduceat((X * e[:, None])[order], starts, axis=0)


def report(X, y, codes, std_err="cluster", dtype=np.longdouble, y_var=None) -> dict:
    from scipy import stats as st

    assert std_err in SE_TYPES
    ops = _Ops(dtype)
    Xl, yl = np.asarray(X).astype(dtype), np.asarray(y).astype(dtype)
    n, pp = Xl.shape
    dof = n - pp
    G = Xl.T @ Xl
    xty = Xl.T @ yl
    inv = rr.inverse(G, ops)
    beta = inv @ xty
    beta = beta + inv @ (xty - G @ beta)  # one refinement step
    e = yl - Xl @ beta
    e2 = e * e
    ssr = e2.sum()
    S = scores(Xl, e, codes)
    g = S.shape[0]
    meat = S.T @ S
    v0 = np.diag(inv @ meat @ inv)
    one = dtype(1)
    c1 = (dtype(g) / dtype(g - 1)) * (dtype(n - 1) / dtype(n - pp))
    hc0 = np.diag(inv @ ((Xl * e2[:, None]).T @ Xl) @ inv)
    se_all = {"cluster0": np.sqrt(v0), "cluster": np.sqrt(v0 * c1), "hc0": np.sqrt(hc0), "hc1": np.sqrt(hc0 * dtype(n) / dtype(dof))}
    yc = yl - yl.sum() / dtype(n)
    yv = (yc * yc).sum() / dtype(n - 1) if y_var is None else dtype(y_var)
    ratio = ssr / (yv * dtype(n))
    se_v = se_all[std_err]
    t = beta / se_v
    t64 = t.astype(np.float64)
    b64, s64 = beta.astype(np.float64), se_v.astype(np.float64)
    tc = st.t.ppf(0.975, g - 1)
    return {"beta": beta, "std_err": se_v, "se_all": se_all, "meat": meat, "t": t, "p": 2.0 * st.t.sf(np.abs(t64), g - 1),
            "ci_lo": b64 - tc * s64, "ci_hi": b64 + tc * s64, "r2": one - ratio, "adj_r2": one - ratio * dtype(n - 1) / dtype(dof - 1),
            "n_clusters": g, "t_dof": g - 1, "t_crit": float(tc)}


def rel(a, b) -> float:
    """Distance of a from the reference b relative to b's size: max |a - b| / max |b|."""
    a = np.atleast_1d(np.asarray(a)).astype(np.longdouble)
    b = np.atleast_1d(np.asarray(b)).astype(np.longdouble)
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


def budget(spread: float, dtype=np.float64) -> float:
    """10 x the reference's own distance from the long double result in the frame's format; where that distance is 0, 8 ulp.  "Is 0"
    means: is not resolved by the format.  A value stored in the format is up to half an ulp from the long double one whatever
    arithmetic made it, so a distance below half an ulp says that the reference's rounding fell luckily, not that a stored result can
    be held to a tenth of an ulp."""
    eps = float(np.finfo(dtype).eps)
    return 10.0 * spread if spread >= 0.5 * eps else 8 * eps
