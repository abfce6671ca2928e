"""
A high-precision restatement of the fixed-effects (within) regression with one absorbed factor (TEST INFRASTRUCTURE ONLY): the
definitions of include/pds_lstsq.h (pds_lin_reg_within_*), line by line, in NumPy for any dtype.

    report(F, y, codes, std_err="se", dtype=np.longdouble) -> dict
        F: [n, p] features WITHOUT an intercept column; y: [n]; codes: [n] integers in any order (the absorbed key)

With n rows, G distinct codes, m_g the mean of [x, y] over group g and W the within scatter sum_g sum_{i in g} (z_i - m_g)(z_i - m_g)':
    beta solves W_xx beta = W_xy;  alpha_g = m_y,g - m_g' beta;  e_i = y_i - alpha_g - x_i' beta;  pred_i = y_i - e_i
    "se":        V = s2 W_xx^-1, s2 = sum e^2 / (n - G - p), Student t with n - G - p degrees of freedom
    "cluster0":  V = W_xx^-1 M W_xx^-1, M = sum_g s_g s_g', s_g = sum_{i in g} (x_i - m_g) e_i; G - 1 degrees of freedom
    "cluster":   the same V times G / (G - 1) * (n - 1) / (n - p - 1); G - 1 degrees of freedom
    r2 = 1 - sum e^2 / W_yy;  adj_r2 = 1 - (1 - r2)(n - G) / (n - G - p);
    r2_overall = 1 - sum e^2 / (W_yy + sum_g n_g (m_y,g - ybar)^2)
alpha comes back per distinct code in ascending order, pred and resid in the row order given.

`dtype` is the arithmetic of the whole computation: np.longdouble is the truth the tests measure against, np.float64 / np.float32
the same code in the frame's format, whose distance from the long double result is what a budget is made of.  Nothing follows the
device's operation order (the device centres before it forms a residual; this file forms y - alpha - x . beta as the definition
reads).  dummy_report() is the independent formula the reference itself is checked against: the explicit regression on one dummy
column per group, no intercept, scores that keep the dummies.
"""
from __future__ import annotations

import numpy as np

import cluster_reference as cr
import report_reference as rr

SE_TYPES = ("se", "cluster", "cluster0")
SCALARS = ("r2", "adj_r2", "r2_overall")
FIELDS = ("beta", "std_err", "t") + SCALARS  # the report fields a budget is measured for
ROW_FIELDS = ("alpha", "pred", "resid")      # ... and the per-group / per-row outputs

rel, budget = cr.rel, cr.budget


def _groups(codes):
    """(order, starts, idx, counts): rows in ascending code order (stable), the first row of each group there, the group of each row"""
    codes = np.asarray(codes)
    order = np.argsort(codes, kind="stable")
    c = codes[order]
    starts = np.flatnonzero(np.concatenate([[True], c[1:] != c[:-1]]))
    idx = np.empty(len(codes), dtype=np.int64)
    idx[order] = np.cumsum(np.concatenate([[0], (c[1:] != c[:-1]).astype(np.int64)]))
    counts = np.diff(np.concatenate([starts, [len(codes)]]))
    return order, starts, idx, counts


def _solve(A, b, dtype):
    inv = rr.inverse(A, cr._Ops(dtype))
    x = inv @ b
    return x + inv @ (b - A @ x), inv  # one refinement step


def _tail(beta, se_v, dof):
    from scipy import stats as st

    t = beta / se_v
    t64, b64, s64 = t.astype(np.float64), beta.astype(np.float64), se_v.astype(np.float64)
    tc = st.t.ppf(0.975, dof)
    return {"t": t, "p": 2.0 * st.t.sf(np.abs(t64), dof), "ci_lo": b64 - tc * s64, "ci_hi": b64 + tc * s64, "t_dof": dof, "t_crit": float(tc)}


def report(F, y, codes, std_err="se", dtype=np.longdouble) -> dict:
    assert std_err in SE_TYPES
    X, yl = np.asarray(F).astype(dtype), np.asarray(y).astype(dtype)
    n, p = X.shape
    order, starts, idx, counts = _groups(codes)
    g = len(starts)
    cnt = counts.astype(dtype)
    mx = np.add.reduceat(X[order], starts, axis=0) / cnt[:, None]
    my = np.add.reduceat(yl[order], starts) / cnt
    Xc, yc = X - mx[idx], yl - my[idx]
    wxx, wxy, wyy = Xc.T @ Xc, Xc.T @ yc, (yc * yc).sum()
    beta, inv = _solve(wxx, wxy, dtype)
    alpha = my - mx @ beta
    e = yl - alpha[idx] - X @ beta
    pred = yl - e
    sse = (e * e).sum()
    dof = n - g - p
    S = np.add.reduceat((Xc * e[:, None])[order], starts, axis=0)
    meat = S.T @ S
    v0 = np.diag(inv @ meat @ inv)
    c1 = (dtype(g) / dtype(max(g - 1, 1))) * (dtype(n - 1) / dtype(n - p - 1))
    se_all = {"se": np.sqrt(sse / dtype(dof) * np.diag(inv)), "cluster0": np.sqrt(v0), "cluster": np.sqrt(v0 * c1)}
    one = dtype(1)
    r2 = one - sse / wyy
    ybar = (cnt * my).sum() / dtype(n)
    between = (cnt * (my - ybar) ** 2).sum()
    out = {"beta": beta, "std_err": se_all[std_err], "se_all": se_all, "meat": meat, "alpha": alpha, "pred": pred, "resid": e, "sse": sse,
           "r2": r2, "adj_r2": one - (one - r2) * dtype(n - g) / dtype(dof), "r2_overall": one - sse / (wyy + between), "n_groups": g,
           "df_resid": dof if std_err == "se" else g - 1}
    out.update(_tail(beta, se_all[std_err], out["df_resid"]))
    return out


def plain_report(X, y, codes, dtype=np.longdouble) -> dict:
    """Ordinary least squares on the design X as given (no column added): beta, the classical standard errors with n - rank degrees
    of freedom (X has full column rank) and the CR0 standard errors of the clusters `codes`, for every column."""
    Xl, yl = np.asarray(X).astype(dtype), np.asarray(y).astype(dtype)
    n, q = Xl.shape
    order, starts, idx, counts = _groups(codes)
    coef, inv = _solve(Xl.T @ Xl, Xl.T @ yl, dtype)
    e = yl - Xl @ coef
    sse = (e * e).sum()
    S = np.add.reduceat((Xl * e[:, None])[order], starts, axis=0)
    return {"beta": coef, "se": np.sqrt(sse / dtype(n - q) * np.diag(inv)), "cluster0": np.sqrt(np.diag(inv @ (S.T @ S) @ inv))}


def dummy_design(F, codes, dtype=np.longdouble):
    """[F | one column per group], no intercept"""
    _, starts, idx, _ = _groups(codes)
    return np.column_stack([np.asarray(F).astype(dtype), (idx[:, None] == np.arange(len(starts))[None, :]).astype(dtype)])


def dummy_report(F, y, codes, dtype=np.longdouble, flip: bool = False) -> dict:
    """The explicit dummy-variable regression: X = [F | one column per group], no intercept; classical and CR0 standard errors of the
    feature coefficients, the scores X_g' e_g keeping the dummy entries.  flip: the same computation with the columns and the rows in
    the opposite order (another rounding of the same formula: what the comparison's bar is measured with)."""
    p = np.asarray(F).shape[1]
    X, yl, codes = dummy_design(F, codes, dtype), np.asarray(y).astype(dtype), np.asarray(codes)
    feat = slice(0, p)
    if flip:
        X, yl, codes, feat = X[::-1, ::-1], yl[::-1], codes[::-1], slice(X.shape[1] - 1, X.shape[1] - 1 - p, -1)
    r = plain_report(X, yl, codes, dtype)
    return {k: v[feat] for k, v in r.items()}
