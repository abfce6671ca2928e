"""
A high-precision restatement of the fixed-effects regressions' standard errors clustered on ANY key (TEST INFRASTRUCTURE ONLY): the
definitions of include/pds_lstsq.h (pds_lin_reg_within_cl_* / pds_lin_reg_within2_cl_*), line by line, in NumPy for any dtype.

    report(F, y, absorb, cluster, std_err="cluster", dtype=np.longdouble, tol=TRUTH_TOL, max_iter=10_000, sweeps=None, fitted=None) -> dict
        F: [n, p] features WITHOUT an intercept column; y: [n]; absorb: ONE integer key column, or a tuple of TWO; cluster: [n] integers
        in any order (the cluster key)

x~, y~ are the columns projected off the absorbed dummies (one key: the group means are subtracted, within_reference.py; two keys: the
alternating sweeps of within2_reference.py), B = (X~'X~)^-1, e the residuals of that fit.  Gc: the distinct cluster keys.
    s_c = sum_{i in c} x~_i e_i,  M = sum_c s_c s_c'  -- formed by np.add.at over the cluster codes on the projected columns
    "cluster0":  V = B M B
    "cluster":   V times Gc / (Gc - 1) * (n - 1) / (n - K),  K = p + sum_f (nested_f ? 0 : A_f) + (some factor nested ? 1 : 0),
                 A_1 = G1, A_2 = G2 - C; factor f is nested when every level of it has all its rows in one cluster
    t, p and the interval: Gc - 1 degrees of freedom
The fit itself (beta, the residuals, r2 ...) is the one of within_reference.report / within2_reference.report, operation for operation.

dummy_cluster0() is the second, independent route: the explicit regression on the features and the dummies of the absorbed keys with the
CR0 sandwich of the clusters on the FULL design (the scores keep their dummy entries); only the feature block enters the comparison
(Frisch-Waugh-Lovell: the feature rows of (X'X)^-1 X' are B X~').
"""
from __future__ import annotations

import numpy as np

import within2_reference as w2r
import within_reference as wr

SE_TYPES = ("cluster", "cluster0")
FIELDS = ("beta", "std_err", "t")

rel, budget = wr.rel, wr.budget
TRUTH_TOL = w2r.TRUTH_TOL


def _dense(codes):
    return np.unique(np.asarray(codes), return_inverse=True)[1].reshape(-1)


def nested(level_codes, cluster_codes) -> bool:
    """every level of the factor has all its rows in one cluster (integers only: the min and max cluster code per level agree)"""
    lv, cl = _dense(level_codes), _dense(cluster_codes)
    lo, hi = np.full(int(lv.max()) + 1, np.iinfo(np.int64).max), np.full(int(lv.max()) + 1, -1)
    np.minimum.at(lo, lv, cl)
    np.maximum.at(hi, lv, cl)
    return bool(np.all(lo == hi))


def parameters(p, g1, a2, nested1, nested2) -> int:
    """K of the definition: a2 = G2 - C (0 with one absorbed key)"""
    return p + (0 if nested1 else g1) + (0 if nested2 else a2) + (1 if (nested1 or nested2) else 0)


def fit(F, y, absorb, dtype=np.longdouble, tol=TRUTH_TOL, max_iter=10_000, sweeps=None) -> dict:
    """The fit without the errors: the projected columns, B, beta and the residuals, as within_reference.report / within2_reference.report
    form them.  report() takes it as `fitted`, so that one projection serves every cluster key and both estimators of a frame."""
    X, yl = np.asarray(F).astype(dtype), np.asarray(y).astype(dtype)
    n, p = X.shape
    two = isinstance(absorb, (tuple, list))
    if two:
        k1, k2 = absorb
        G1, G2, C = w2r.components(k1, k2)
        Zt, n_iter, _ = w2r.demean(np.column_stack([X, yl]), k1, k2, dtype, tol, max_iter, sweeps)
        Xt, yt = Zt[:, :p], Zt[:, p]
        beta, inv = wr._solve(Xt.T @ Xt, Xt.T @ yt, dtype)
        e = yt - Xt @ beta
        a2 = G2 - C
    else:
        k1 = absorb
        order, starts, idx, counts = wr._groups(k1)
        G1, n_iter, a2 = len(starts), None, 0
        cnt = counts.astype(dtype)
        mx = np.add.reduceat(X[order], starts, axis=0) / cnt[:, None]
        my = np.add.reduceat(yl[order], starts) / cnt
        Xt, yt = X - mx[idx], yl - my[idx]
        beta, inv = wr._solve(Xt.T @ Xt, Xt.T @ yt, dtype)
        e = yl - (my - mx @ beta)[idx] - X @ beta
    return {"Xt": Xt, "e": e, "beta": beta, "inv": inv, "G1": G1, "a2": a2, "n_iter": n_iter, "keys": tuple(absorb) if two else (absorb,),
            "dtype": dtype}


def report(F, y, absorb, cluster, std_err="cluster", dtype=np.longdouble, tol=TRUTH_TOL, max_iter=10_000, sweeps=None, fitted=None) -> dict:
    assert std_err in SE_TYPES
    f = fitted if fitted is not None else fit(F, y, absorb, dtype, tol, max_iter, sweeps)
    dtype, Xt, e, beta, inv = f["dtype"], f["Xt"], f["e"], f["beta"], f["inv"]
    n, p = Xt.shape
    flags = tuple(nested(k, cluster) for k in f["keys"])
    cl = _dense(cluster)
    gc = int(cl.max()) + 1
    S = np.zeros((gc, p), dtype=dtype)
    np.add.at(S, cl, Xt * e[:, None])
    meat = S.T @ S
    v0 = np.diag(inv @ meat @ inv)
    K = parameters(p, f["G1"], f["a2"], flags[0], flags[1] if len(flags) == 2 else False)
    c1 = (dtype(gc) / dtype(max(gc - 1, 1))) * (dtype(n - 1) / dtype(n - K))
    se_all = {"cluster0": np.sqrt(v0), "cluster": np.sqrt(v0 * c1)}
    out = {"beta": beta, "std_err": se_all[std_err], "se_all": se_all, "meat": meat, "scores": S, "resid": e, "n_clusters": gc,
           "absorb_nested": flags, "K": K, "df_resid": gc - 1, "n_groups": f["G1"], "n_iter": f["n_iter"]}
    out.update(wr._tail(beta, se_all[std_err], gc - 1))
    return out


def select(out, std_err) -> dict:
    """the report `out` with the standard errors, t, p and the interval of the other cluster form (nothing is fitted again)"""
    out = dict(out)
    out["std_err"] = out["se_all"][std_err]
    out.update(wr._tail(out["beta"], out["std_err"], out["df_resid"]))
    return out


def dummy_cluster0(F, y, absorb, cluster, dtype=np.longdouble) -> dict:
    """The explicit dummy-variable regression with the CR0 sandwich of the clusters on the full design: beta and the CR0 standard errors
    of the feature coefficients.  Solved by an orthogonalisation, dummies first (the design carries the levels of the absorbed keys)."""
    p = np.asarray(F).shape[1]
    D = w2r.dummy_design(F, absorb[0], absorb[1], dtype) if isinstance(absorb, (tuple, list)) else wr.dummy_design(F, absorb, dtype)
    X, yl = np.column_stack([D[:, p:], D[:, :p]]), np.asarray(y).astype(dtype)
    n, q = X.shape
    Q, R = w2r._qr(X)
    Ri = np.zeros_like(R)  # R^-1 by back substitution, column by column
    for j in range(q):
        Ri[j, j] = dtype(1) / R[j, j]
        for i in range(j - 1, -1, -1):
            Ri[i, j] = -(R[i, i + 1:j + 1] @ Ri[i + 1:j + 1, j]) / R[i, i]
    coef, inv = Ri @ (Q.T @ yl), Ri @ Ri.T
    e = yl - X @ coef
    cl = _dense(cluster)
    S = np.zeros((int(cl.max()) + 1, q), dtype=dtype)
    np.add.at(S, cl, X * e[:, None])
    feat = slice(q - p, q)
    return {"beta": coef[feat], "cluster0": np.sqrt(np.diag(inv @ (S.T @ S) @ inv))[feat]}
