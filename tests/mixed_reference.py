"""
The random-intercept mixed model (REML) written from its definition in NumPy, in a chosen floating-point type.  TEST
INFRASTRUCTURE ONLY: the reference the MixedModel tests hold the device against.

    y = X beta + Z u + e,   u ~ N(0, sigma_g^2 I),   e ~ N(0, sigma_e^2 I),   gamma = sigma_g^2 / sigma_e^2,   H = I + gamma Z Z'

`profile` evaluates the profiled REML deviance

    dev(gamma) = (n - p') ln(r' H^-1 r / (n - p')) + sum_g ln(1 + gamma n_g) + ln det(X' H^-1 X)

the way the model's definition reads: H^-1 is applied to X, y and the residual r through the Woodbury identity (Z'Z is the
diagonal of the group counts, so an apply is an O(n) pass over group sums), X' H^-1 X is factored by a hand-written Cholesky
(np.linalg has no long double), beta solves it, r = y - X beta.  `fit_reml` drives the golden section over gamma in [0, 1e6]:
c = hi - phi (hi - lo), e = lo + phi (hi - lo); while hi - lo >= tol and fewer than max_iter steps: if f(c) < f(e) then hi = e,
e = c, new c, else lo = c, c = e, new e; gamma = (lo + hi) / 2.  Degrees of freedom by containment from np.linalg.matrix_rank.
Every function takes `dtype` (np.float64 or np.longdouble) and keeps all arithmetic in it.
"""
from __future__ import annotations

import numpy as np

MSG_ROWS = "Not enough rows to fit a mixed model with this many fixed effects."
MSG_PD = "X'HiX is not positive definite; design may be rank-deficient."
MSG_VAR = "Residual variance estimate is non-positive."


def cholesky(a: np.ndarray) -> np.ndarray:
    """Lower factor of a symmetric positive definite matrix in a's own dtype; ValueError(MSG_PD) at a pivot that is not > 0."""
    n = a.shape[0]
    l = np.zeros_like(a)
    for j in range(n):
        d = a[j, j] - np.dot(l[j, :j], l[j, :j])
        if not d > 0:
            raise ValueError(MSG_PD)
        l[j, j] = np.sqrt(d)
        for i in range(j + 1, n):
            l[i, j] = (a[i, j] - np.dot(l[i, :j], l[j, :j])) / l[j, j]
    return l


def solve_lower(l: np.ndarray, b: np.ndarray) -> np.ndarray:
    x = np.zeros_like(b)
    for i in range(l.shape[0]):
        x[i] = (b[i] - np.dot(l[i, :i], x[:i])) / l[i, i]
    return x


def solve_upper(u: np.ndarray, b: np.ndarray) -> np.ndarray:
    x = np.zeros_like(b)
    for i in range(u.shape[0] - 1, -1, -1):
        x[i] = (b[i] - np.dot(u[i, i + 1:], x[i + 1:])) / u[i, i]
    return x


def chol_solve(l: np.ndarray, b: np.ndarray) -> np.ndarray:
    return solve_upper(l.T, solve_lower(l, b))


def design(features: np.ndarray, dtype=np.float64) -> np.ndarray:
    """[1 | features]: the intercept first."""
    f = np.asarray(features, dtype=dtype)
    return np.concatenate([np.ones((f.shape[0], 1), dtype=dtype), f], axis=1)


def group_counts(codes: np.ndarray, n_groups: int, dtype=np.float64) -> np.ndarray:
    return np.bincount(codes, minlength=n_groups).astype(dtype)


def apply_hi(v: np.ndarray, codes: np.ndarray, counts: np.ndarray, gamma) -> np.ndarray:
    """(I + gamma Z Z')^-1 v = v - gamma Z (I + gamma Z'Z)^-1 Z' v, for a vector or the columns of a matrix."""
    gs = np.zeros((counts.shape[0],) + v.shape[1:], dtype=v.dtype)
    np.add.at(gs, codes, v)
    scale = gamma / (1 + gamma * counts)
    scaled = gs * (scale if v.ndim == 1 else scale[:, None])
    return v - scaled[codes]


def profile(X: np.ndarray, y: np.ndarray, codes: np.ndarray, n_groups: int, gamma, dtype=np.float64) -> dict:
    """One evaluation at a fixed gamma.  X holds the intercept column already."""
    X = np.asarray(X, dtype=dtype)
    y = np.asarray(y, dtype=dtype)
    gamma = dtype(gamma)
    n, p = X.shape
    counts = group_counts(codes, n_groups, dtype)
    xhx = X.T @ apply_hi(X, codes, counts, gamma)
    xhy = X.T @ apply_hi(y, codes, counts, gamma)
    l = cholesky(xhx)
    beta = chol_solve(l, xhy)
    r = y - X @ beta
    rhr = np.dot(r, apply_hi(r, codes, counts, gamma))
    resid_var = rhr / dtype(n - p)
    if not resid_var > 0:
        raise ValueError(MSG_VAR)
    logdet_h = np.sum(np.log(1 + gamma * counts[counts > 0]))
    logdet_xhx = 2 * np.sum(np.log(np.abs(np.diag(l))))
    deviance = dtype(n - p) * np.log(resid_var) + logdet_h + logdet_xhx
    return {"beta": beta, "resid_var": resid_var, "deviance": deviance, "rhr": rhr, "logdet_h": logdet_h, "logdet_xhx": logdet_xhx,
            "chol": l}


def between_columns(X: np.ndarray, codes: np.ndarray) -> list:
    """Columns of X that are constant inside every group (the intercept among them)."""
    order = np.argsort(codes, kind="stable")
    Xs, cs = np.asarray(X)[order], codes[order]
    starts = np.flatnonzero(np.r_[True, cs[1:] != cs[:-1]])
    first = Xs[np.repeat(starts, np.diff(np.r_[starts, len(cs)]))]
    return [j for j in range(X.shape[1]) if np.array_equal(Xs[:, j], first[:, j])]


def fit_reml(X: np.ndarray, y: np.ndarray, codes: np.ndarray, n_groups: int, max_iter: int = 200, tol: float = 1e-10, dtype=np.float64) -> dict:
    """The whole fit.  X holds the intercept column; codes are dense group numbers 0 .. n_groups - 1, every one of them in use."""
    X = np.asarray(X, dtype=dtype)
    y = np.asarray(y, dtype=dtype)
    n, p = X.shape
    if n <= p:
        raise ValueError(MSG_ROWS)
    n_eval = 0

    def f(g):
        nonlocal n_eval
        n_eval += 1
        return profile(X, y, codes, n_groups, g, dtype)["deviance"]

    phi = (np.sqrt(dtype(5)) - 1) / 2
    lo, hi = dtype(0), dtype(1e6)
    c = hi - phi * (hi - lo)
    e = lo + phi * (hi - lo)
    fc, fe = f(c), f(e)
    for _ in range(max_iter):
        if hi - lo < tol:
            break
        if fc < fe:
            hi, e, fe = e, c, fc
            c = hi - phi * (hi - lo)
            fc = f(c)
        else:
            lo, c, fc = c, e, fe
            e = lo + phi * (hi - lo)
            fe = f(e)
    gamma = (lo + hi) / 2
    fit = profile(X, y, codes, n_groups, gamma, dtype)
    n_eval += 1
    l = fit["chol"]
    cov = np.stack([chol_solve(l, col) for col in np.eye(p, dtype=dtype)], axis=1)
    std_errors = np.sqrt(fit["resid_var"] * np.diag(cov))
    # containment degrees of freedom
    X64 = np.asarray(X, dtype=np.float64)
    between = between_columns(X64, codes)
    g_used = int(np.count_nonzero(np.bincount(codes, minlength=n_groups)))
    ddf_between = g_used - int(np.linalg.matrix_rank(X64[:, between]))
    Z = np.zeros((n, n_groups))
    Z[np.arange(n), codes] = 1.0
    ddf_within = n - int(np.linalg.matrix_rank(np.concatenate([X64, Z], axis=1)))
    dfs = np.array([ddf_between if j in between else ddf_within for j in range(p)], dtype=np.float64)
    return {"coeffs": fit["beta"], "std_errors": std_errors, "dfs": dfs, "gamma": gamma, "resid_variance": fit["resid_var"],
            "n_eval": n_eval, "n_groups": g_used}


def moment_form(X: np.ndarray, y: np.ndarray, codes: np.ndarray, n_groups: int, gamma, dtype=np.float64) -> np.ndarray:
    """[X y]' H^-1 [X y] as W + sum_g c_g m_g m_g', c_g = n_g / (1 + gamma n_g): the form the device computes, here in NumPy."""
    z = np.concatenate([np.asarray(X, dtype=dtype), np.asarray(y, dtype=dtype)[:, None]], axis=1)
    counts = group_counts(codes, n_groups, dtype)
    sums = np.zeros((n_groups, z.shape[1]), dtype=dtype)
    np.add.at(sums, codes, z)
    used = counts > 0
    means = np.zeros_like(sums)
    means[used] = sums[used] / counts[used, None]
    zc = z - means[codes]
    cg = np.where(used, counts / (1 + dtype(gamma) * counts), 0)
    return zc.T @ zc + (means * cg[:, None]).T @ means


def solve_moment_form(m: np.ndarray, n: int, logdet_h):
    """beta, r' H^-1 r, ln det(X' H^-1 X) and the deviance from the Cholesky factor of M (y ordered last)."""
    q = m.shape[0]
    p = q - 1
    l = cholesky(m)
    beta = solve_upper(l[:p, :p].T, l[p, :p].copy())
    rhr = l[p, p] ** 2
    logdet = 2 * np.sum(np.log(np.diag(l)[:p]))
    dev = (n - p) * np.log(rhr / (n - p)) + logdet_h + logdet
    return beta, rhr, logdet, dev
