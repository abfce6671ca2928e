"""The robust / cluster-robust one-model GLM report restated in NumPy (TEST INFRASTRUCTURE ONLY; tests/test_glm_sandwich_cpu.py,
tests/test_glm_sandwich_gpu.py): the definitions of include/pds_lstsq.h (pds_glm_report_robust_* / _cluster_*) at coefficients the
caller BRINGS, in np.longdouble (the truth the tests measure against), or with dtype=np.float64 / np.float32 the same code in the
narrower format, whose distance from the longdouble result is what a budget is made of.  On top of glm_report_reference.py
(_design, _inv_link, _dlink, _var, spd_inverse).  Nothing follows the device's operation order.

    report(X, y, beta, family, bias, kind, codes=None, pw=None, o=None, dtype=np.longdouble) -> dict
        X [n, p], y [n], beta [p'] (bias last), kind in KINDS, codes [n] integers in any order (the cluster kinds), pw / o [n] optional
        std_err, z, p, lo, hi [p'], cov [p', p'], meat, inv, n (rows of positive weight), n_clusters, df_resid
"""
import math

import numpy as np

import glm_report_reference as rr

KINDS = ("hc0", "hc1", "cluster", "cluster0")
CLUSTER_KINDS = ("cluster", "cluster0")


def score_residual(fam, y, mu, pw, dtype):
    """r_i = pw_i (y_i - mu_i) / (V(mu_i) g'(mu_i)); exactly 0 on a row of weight 0, by a select"""
    with np.errstate(all="ignore"):
        r = (y - mu) / (rr._var(fam, mu) * rr._dlink(fam, mu))
        if pw is None:
            return r
        return np.where(pw > 0, pw * r, dtype(0))


def cluster_scores(Z, r, codes):
    """S [G, p']: row g = sum_{i in g} r_i x_i, the clusters in ascending order of their code"""
    order = np.argsort(codes, kind="stable")
    c = np.asarray(codes)[order]
    starts = np.flatnonzero(np.concatenate([[True], c[1:] != c[:-1]]))
    return np.add.reduceat((Z * r[:, None])[order], starts, axis=0)


def report(X, y, beta, family, bias, kind, codes=None, pw=None, o=None, dtype=np.longdouble):
    assert kind in KINDS
    fam = rr.FAMILY_ID[family]
    Z = rr._design(X, bias, dtype)
    yv = np.asarray(y).astype(dtype)
    b = np.asarray(beta).astype(dtype)
    w_ = None if pw is None else np.asarray(pw).astype(dtype)
    n_all, pp = Z.shape
    eta = Z @ b
    if o is not None:
        eta = eta + np.asarray(o).astype(dtype)
    mu = rr._inv_link(fam, eta)
    with np.errstate(all="ignore"):
        wi = 1 / (rr._dlink(fam, mu) ** 2 * rr._var(fam, mu))
        if w_ is not None:
            wi = np.where(w_ > 0, w_ * wi, dtype(0))
    info = Z.T @ (Z * wi[:, None])
    inv = rr.spd_inverse(info, dtype)
    r = score_residual(fam, yv, mu, w_, dtype)
    pos = np.ones(n_all, dtype=bool) if w_ is None else np.asarray(w_ > 0)
    n = int(pos.sum())
    g = 0
    if kind in CLUSTER_KINDS:
        codes = np.asarray(codes)
        S = cluster_scores(Z, r, codes)
        meat = S.T @ S
        g = len(np.unique(codes[pos]))
        c = dtype(1) if kind == "cluster0" else (dtype(g) / dtype(g - 1)) * (dtype(n - 1) / dtype(n - pp))
    else:
        meat = (Z * (r * r)[:, None]).T @ Z
        c = dtype(1) if kind == "hc0" else dtype(n) / dtype(n - pp)
    cov = c * (inv @ meat @ inv)
    cov = (cov + cov.T) / 2
    with np.errstate(invalid="ignore"):
        se = np.sqrt(np.diag(cov))
        z = b / se
    p = rr._erfc(np.abs(z.astype(np.float64)) / math.sqrt(2.0))
    return {"std_err": se, "z": z, "p": p, "lo": b - dtype(rr.Z975) * se, "hi": b + dtype(rr.Z975) * se, "cov": cov, "meat": meat, "inv": inv,
            "n": n, "n_clusters": g, "df_resid": n - pp}


def budget(spread: float, dtype=np.float64, factor: float = 64.0) -> float:
    """`factor` x the narrow reference's own distance from the longdouble result (64: the factor of the weighted GLM report tests for
    fields that pass through the device's exp / log); where that distance is below half an ulp of the format -- not resolved by it --
    8 ulp, the floor of cluster_reference.budget."""
    eps = float(np.finfo(dtype).eps)
    return factor * spread if spread >= 0.5 * eps else 8 * eps
