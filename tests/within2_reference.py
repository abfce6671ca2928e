"""
A high-precision restatement of the fixed-effects regression with TWO absorbed factors (TEST INFRASTRUCTURE ONLY): the definitions of
include/pds_lstsq.h (pds_lin_reg_within2_*), line by line, in NumPy for any dtype.

    report(F, y, codes1, codes2, std_err="se", dtype=np.longdouble, tol=TRUTH_TOL, max_iter=10_000, sweeps=None) -> dict
        F: [n, p] features WITHOUT an intercept column; y: [n]; codes1 / codes2: [n] integers in any order (the two absorbed keys)

n rows, p features, G1 / G2 occupied levels, C connected components of the bipartite graph of the occupied (level1, level2) cells,
A = G1 + G2 - C the rank of the absorbed dummies.  z~ is the column z projected off both sets of dummies, by alternating sweeps:
    one sweep subtracts the factor-1 level means, then the factor-2 level means, from all p + 1 columns;
    delta = max_j max_level |factor-2 mean subtracted from column j in this sweep| / s_j, s_j the population standard deviation of
    the original column j; the sweeps stop when delta <= tol (ConvergenceError after max_iter sweeps without that).
    beta solves X~'X~ beta = X~'y~;  e = y~ - X~ beta;  pred = y - e
    "se":        V = s2 (X~'X~)^-1, s2 = sum e^2 / (n - p - A), Student t with n - p - A degrees of freedom
    "cluster0":  V = (X~'X~)^-1 M (X~'X~)^-1, M = sum_g s_g s_g', s_g = sum_{i in g} x~_i e_i over the levels g of the FIRST key
    "cluster":   the same V times G1 / (G1 - 1) * (n - 1) / (n - K), K = p + 1 + (A - G1); both cluster forms: G1 - 1 degrees of freedom
    r2 = 1 - sum e^2 / sum y~^2;  adj_r2 = 1 - (1 - r2)(n - A) / (n - A - p);  r2_overall = 1 - sum e^2 / sum (y - ybar)^2

`dtype` is the arithmetic of the whole computation.  The TRUTH the tests measure against is the long double run with the tolerance at
the long double rounding floor (TRUTH_TOL); np.float64 / np.float32 is the same code in the frame's format, whose distance from the
truth is what a budget is made of.  `sweeps=k` runs exactly k sweeps whatever delta says (a run stopped one sweep early is the
yardstick of the truncation error at a loose tolerance).  The result carries "n_iter" and "deltas" (the delta of every sweep).
dummy_report() is the independent formula the reference itself is checked against: the explicit regression on the features, one
dummy per level of key 1 and one per level of key 2 less one level per component.
"""
from __future__ import annotations

import numpy as np

import within_reference as wr

SE_TYPES = wr.SE_TYPES
SCALARS = wr.SCALARS
FIELDS = wr.FIELDS
ROW_FIELDS = ("pred", "resid")
TRUTH_TOL = 1e-18  # long double: eps 1.1e-19; delta stalls a decade below this on the test frames

rel, budget = wr.rel, wr.budget


class ConvergenceError(RuntimeError):
    pass


def components(codes1, codes2):
    """(G1, G2, C): occupied levels of the two keys and the connected components of the graph of the occupied cells (union-find)"""
    _, i1 = np.unique(np.asarray(codes1), return_inverse=True)
    _, i2 = np.unique(np.asarray(codes2), return_inverse=True)
    g1, g2 = int(i1.max()) + 1, int(i2.max()) + 1
    parent = list(range(g1 + g2))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    c = g1 + g2
    for a, b in set(zip(i1.tolist(), (i2 + g1).tolist())):
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[ra] = rb
            c -= 1
    return g1, g2, c


def _level_sums(Z, grp):
    order, starts, idx, counts = grp
    return np.add.reduceat(Z[order], starts, axis=0)


def demean(Z, codes1, codes2, dtype=np.longdouble, tol=TRUTH_TOL, max_iter=10_000, sweeps=None):
    """(Z~, n_iter, deltas): the columns of Z projected off both sets of dummies by alternating sweeps in `dtype` arithmetic"""
    Z = np.array(Z, dtype=dtype)
    s = np.std(np.asarray(Z, dtype=np.longdouble), axis=0).astype(dtype)  # only a scale
    s = np.where(s > 0, s, dtype(1))
    g1, g2 = wr._groups(codes1), wr._groups(codes2)
    c1, c2 = g1[3].astype(dtype)[:, None], g2[3].astype(dtype)[:, None]
    deltas = []
    for it in range(sweeps if sweeps is not None else max_iter):
        Z -= (_level_sums(Z, g1) / c1)[g1[2]]
        m2 = _level_sums(Z, g2) / c2
        Z -= m2[g2[2]]
        deltas.append(float(np.max(np.abs(m2) / s[None, :])))
        if sweeps is None and deltas[-1] <= tol:
            break
    else:
        if sweeps is None:
            raise ConvergenceError(f"did not converge in {max_iter} sweeps: delta = {deltas[-1]:.3e}")
    return Z, len(deltas), deltas


def report(F, y, codes1, codes2, std_err="se", dtype=np.longdouble, tol=TRUTH_TOL, max_iter=10_000, sweeps=None) -> dict:
    assert std_err in SE_TYPES
    X, yl = np.asarray(F).astype(dtype), np.asarray(y).astype(dtype)
    n, p = X.shape
    G1, G2, C = components(codes1, codes2)
    A = G1 + G2 - C
    Zt, n_iter, deltas = demean(np.column_stack([X, yl]), codes1, codes2, dtype, tol, max_iter, sweeps)
    Xt, yt = Zt[:, :p], Zt[:, p]
    beta, inv = wr._solve(Xt.T @ Xt, Xt.T @ yt, dtype)
    e = yt - Xt @ beta
    sse = (e * e).sum()
    dof = n - p - A
    order, starts, idx, counts = wr._groups(codes1)
    S = np.add.reduceat((Xt * e[:, None])[order], starts, axis=0)
    meat = S.T @ S
    v0 = np.diag(inv @ meat @ inv)
    K = p + 1 + (A - G1)
    c1 = (dtype(G1) / dtype(max(G1 - 1, 1))) * (dtype(n - 1) / dtype(n - K))
    se_all = {"se": np.sqrt(sse / dtype(dof) * np.diag(inv)), "cluster0": np.sqrt(v0), "cluster": np.sqrt(v0 * c1)}
    one = dtype(1)
    r2 = one - sse / (yt * yt).sum()
    out = {"beta": beta, "se_all": se_all, "pred": yl - e, "resid": e, "sse": sse, "r2": r2,
           "adj_r2": one - (one - r2) * dtype(n - A) / dtype(n - A - p), "r2_overall": one - sse / ((yl - yl.mean()) ** 2).sum(),
           "n_groups": G1, "n_groups2": G2, "n_components": C, "df_se": dof, "n_iter": n_iter, "deltas": deltas}
    return select(out, std_err)


def select(out, std_err) -> dict:
    """the report `out` with the standard errors, t, p, the interval and df_resid of another estimator (the sweeps are not run again)"""
    out = dict(out)
    out["std_err"] = out["se_all"][std_err]
    out["df_resid"] = out["df_se"] if std_err == "se" else out["n_groups"] - 1
    out.update(wr._tail(out["beta"], out["std_err"], out["df_resid"]))
    return out


def dummy_design(F, codes1, codes2, dtype=np.longdouble):
    """[F | one column per level of key 1 | one column per level of key 2, less the first level of key 2 in every component]"""
    _, i1 = np.unique(np.asarray(codes1), return_inverse=True)
    _, i2 = np.unique(np.asarray(codes2), return_inverse=True)
    g1, g2 = int(i1.max()) + 1, int(i2.max()) + 1
    label = np.arange(g1 + g2)  # min-label propagation over the cells (a third way to the components)
    while True:
        before = label.copy()
        np.minimum.at(label, i1, label[i2 + g1])
        np.minimum.at(label, i2 + g1, label[i1])
        if np.array_equal(before, label):
            break
    lab2 = label[g1:]
    keep = np.array([l for l in range(g2) if l != np.flatnonzero(lab2 == lab2[l])[0]], dtype=np.int64)
    D1 = (i1[:, None] == np.arange(g1)[None, :]).astype(dtype)
    D2 = (i2[:, None] == keep[None, :]).astype(dtype)
    return np.column_stack([np.asarray(F).astype(dtype), D1, D2])


def _qr(X):
    """X = Q R by Gram-Schmidt applied twice per column, in X's dtype (NumPy's QR does not run in long double)"""
    n, q = X.shape
    Q, R = X.copy(), np.zeros((q, q), dtype=X.dtype)
    for j in range(q):
        v = Q[:, j].copy()
        for _ in range(2):
            c = Q[:, :j].T @ v
            v -= Q[:, :j] @ c
            R[:j, j] += c
        R[j, j] = np.sqrt(v @ v)
        Q[:, j] = v / R[j, j]
    return Q, R


def dummy_report(F, y, codes1, codes2, dtype=np.longdouble) -> dict:
    """The explicit dummy-variable regression; classical (n - rank) and CR0 (clusters: key 1, scores keeping the dummy entries)
    standard errors of the feature coefficients.  The design carries the levels of both keys (its Gram matrix is far worse conditioned
    than the projected one), so it is solved by an orthogonalisation, dummies first, and not through the normal equations."""
    p = np.asarray(F).shape[1]
    D = dummy_design(F, codes1, codes2, dtype)
    X, yl = np.column_stack([D[:, p:], D[:, :p]]), np.asarray(y).astype(dtype)
    n, q = X.shape
    Q, R = _qr(X)
    Ri = np.zeros_like(R)  # R^-1 by back substitution, column by column
    for j in range(q):
        Ri[j, j] = dtype(1) / R[j, j]
        for i in range(j - 1, -1, -1):
            Ri[i, j] = -(R[i, i + 1:j + 1] @ Ri[i + 1:j + 1, j]) / R[i, i]
    coef, inv = Ri @ (Q.T @ yl), Ri @ Ri.T
    e = yl - X @ coef
    order, starts, idx, counts = wr._groups(codes1)
    S = np.add.reduceat((X * e[:, None])[order], starts, axis=0)
    feat = slice(q - p, q)
    return {"beta": coef[feat], "se": np.sqrt((e * e).sum() / dtype(n - q) * np.diag(inv))[feat],
            "cluster0": np.sqrt(np.diag(inv @ (S.T @ S) @ inv))[feat]}
