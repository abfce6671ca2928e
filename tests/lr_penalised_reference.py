"""The penalised least-squares solvers restated in NumPy (csrc/solve.hip: cd_kernel, nnls_kernel), and a solver-independent
optimality check of what they minimise (TEST INFRASTRUCTURE ONLY).

For n rows, features j < p and an optional unpenalised bias last, lin_reg(l1_reg, l2_reg, positive) minimises

    F(beta) = (1 / 2n) |y - X beta - beta_0|^2 + (l2 / 2) sum_{j<p} beta_j^2 + l1 sum_{j<p} |beta_j|      (beta_j >= 0 with `positive`)

by the reference's coordinate descent on the moments G = Z'Z, c = Z'y (Z = [X | 1]), m = n; positive alone (no penalty) is the
reference's NNLS sweep on the same moments, bias included in the sweep and left unclamped.

    sweeps(G, c, m, p, bias, l1, l2, tol, max_iter, positive, dtype)  -> (beta, sweeps run, converged)
    nnls_sweeps(G, c, p, bias, tol, max_iter, dtype)                  -> (beta, sweeps run)
        the sequential sweeps of oracle/pds_oracle_impl.inc (orc_cd_from_gram, orc_nnls_from_gram) line by line, in the arithmetic
        `dtype`: np.longdouble is the truth the tests measure against, np.float64 the same code in the device's format, whose
        distance from the long double result is what a budget is made of.  Nothing follows the device's operation order.
    kkt(X, y, bias, l1, l2, beta, positive)   the largest violation of F's optimality conditions at beta, np.longdouble from the
        frame, no solver and no moments involved
    nnls_kkt(X, y, bias, beta)                the same for NNLS in the kernel's own units (mu = G beta - c, the stopping test)
    budget(spread, dtype), rel(a, b)          cluster_reference's: 10 x the reference's own distance, 8 ulp where that is not resolved
"""
from __future__ import annotations

import numpy as np

from cluster_reference import budget, rel  # noqa: F401  (the tolerance rule and the distance of the report tests, as they stand)

L = np.longdouble


def with_bias(X, bias, dtype=L):
    X = np.asarray(X).astype(dtype)
    return np.concatenate([X, np.ones((X.shape[0], 1), dtype=dtype)], axis=1) if bias else X


_moments = {}


def moments(X, y, bias, dtype=L):
    """(G [p', p'], c [p'], m): Z'Z, Z'y and the row count in the arithmetic `dtype`; the sum of y sits in c's bias slot and the
    column sums in G's bias column.  Kept per frame where the frame is frozen (a long double Gram matrix of 577 columns takes
    seconds): the arrays are read-only and stay referenced here."""
    X, y = np.asarray(X), np.asarray(y)
    key = None
    if not X.flags.writeable and not y.flags.writeable:
        key = (X.__array_interface__["data"][0], X.shape, X.strides, y.__array_interface__["data"][0], bool(bias), np.dtype(dtype).name)
        if key in _moments:
            return _moments[key][:3]
    Z = with_bias(X, bias, dtype)
    out = (Z.T @ Z, Z.T @ y.astype(dtype), Z.shape[0])
    if key is not None:
        for a in out[:2]:
            a.setflags(write=False)
        _moments[key] = out + (X, y)
    return out


def sweeps(G, c, m, p, bias, l1, l2, tol, max_iter, positive, dtype=np.float64):
    """orc_cd_from_gram: zero the coordinate, take the full dot, soft-threshold by m l1, divide by G_jj + m l2; the bias after the
    features; stop when the largest move of a feature coefficient in a sweep is below tol"""
    T = np.dtype(dtype).type
    G = np.asarray(G).astype(dtype)
    c = np.asarray(c).astype(dtype)
    m, l1, l2, tol = T(m), T(l1), T(l2), T(tol)
    pp = p + int(bool(bias))
    zero = T(0)
    lam = m * l1
    norms = np.diag(G) + m * l2
    cols = [np.ascontiguousarray(G[:, j]) for j in range(p)]
    col_sums = np.ascontiguousarray(G[:p, p]) if bias else None
    beta = np.zeros(pp, dtype=dtype)
    it, conv = 0, False
    while it < max_iter:
        max_change = zero
        for j in range(p):
            before = beta[j]
            beta[j] = zero
            main = c[j] - cols[j] @ beta
            if positive and main < zero:
                after = zero
            else:
                mag = abs(main) - lam
                with np.errstate(invalid="ignore", divide="ignore"):
                    after = (-(mag if mag > zero else zero) if (main < zero or (main == zero and np.signbit(main))) else
                             (mag if mag > zero else zero)) / norms[j]
            beta[j] = after
            d = abs(after - before)
            if d > max_change:
                max_change = d
        if bias:
            beta[p] = (c[p] - beta[:p] @ col_sums) / m
        it += 1
        conv = bool(max_change < tol)
        if conv:
            break
    return beta, it, conv


def nnls_sweeps(G, c, p, bias, tol, max_iter, dtype=np.float64):
    """orc_nnls_from_gram: mu = G beta - c carried along; before every sweep the test mu >= -tol everywhere and mu <= tol where
    beta > 0; a sweep moves every coordinate by -mu_k / G_kk and clamps the features at 0"""
    T = np.dtype(dtype).type
    G = np.asarray(G).astype(dtype)
    c = np.asarray(c).astype(dtype)
    tol = T(tol)
    pp = p + int(bool(bias))
    zero = T(0)
    cols = [np.ascontiguousarray(G[:, k]) for k in range(pp)]
    mu = -c.copy()
    beta = np.zeros(pp, dtype=dtype)
    it = 0
    while it < max_iter:
        if bool(np.all(mu >= -tol)) and bool(np.all(mu[beta > zero] <= tol)):
            break
        for k in range(pp):
            beta_k = beta[k]
            update = beta_k - mu[k] / G[k, k]
            if (not bias or k < pp - 1) and not update > zero:
                update = zero
            beta[k] = update
            mu = mu + (update - beta_k) * cols[k]
        it += 1
    return beta, it


def gradient(X, y, bias, l2, beta):
    """g = X'(y - X beta - beta_0) / n - l2 beta over the features, and sum(residual) / n, np.longdouble from the frame"""
    Xl, yl, b = np.asarray(X).astype(L), np.asarray(y).astype(L), np.asarray(beta).astype(L)
    p = Xl.shape[1]
    n = L(Xl.shape[0])
    res = yl - Xl @ b[:p] - (b[p] if bias else L(0))
    return Xl.T @ res / n - L(l2) * b[:p], res.sum() / n


def kkt(X, y, bias, l1, l2, beta, positive=False) -> float:
    """active coordinate: |g_j - l1 sign beta_j|; coordinate at zero: max(|g_j| - l1, 0), with `positive` max(g_j - l1, 0);
    bias: |sum residual| / n; a negative coefficient under `positive` counts with its size"""
    b = np.asarray(beta).astype(L)
    p = np.asarray(X).shape[1]
    g, gb = gradient(X, y, bias, l2, b)
    bf = b[:p]
    l1 = L(l1)
    at_zero = np.maximum((g if positive else np.abs(g)) - l1, 0)
    v = np.where(bf != 0, np.abs(g - l1 * np.sign(bf)), at_zero)
    if positive:
        v = np.maximum(v, np.maximum(-bf, 0))
    out = v.max()
    if bias:
        out = max(out, abs(gb))
    return float(out)


def slack_and_size(X, y, bias, l1, l2, beta, positive=False):
    """(how far inside the threshold the least inactive coordinate sits: min over beta_j = 0 of l1 - |g_j| (l1 - g_j with
    `positive`); the smallest |beta_j| among the active ones); inf where there is none"""
    b = np.asarray(beta).astype(L)
    p = np.asarray(X).shape[1]
    g, _ = gradient(X, y, bias, l2, b)
    zero = b[:p] == 0
    s = L(l1) - (g if positive else np.abs(g))
    return (float(s[zero].min()) if zero.any() else np.inf), (float(np.abs(b[:p][~zero]).min()) if (~zero).any() else np.inf)


def nnls_kkt(X, y, bias, beta) -> float:
    """worst of max(-mu_j, 0), max(mu_j, 0) where beta_j > 0, and |mu_bias|, mu = G beta - c = Z'(Z beta - y) in np.longdouble from
    the frame"""
    Z, yl = with_bias(X, bias), np.asarray(y).astype(L)
    b = np.asarray(beta).astype(L)
    mu = Z.T @ (Z @ b - yl)
    pp = len(b)
    feat = np.arange(pp) < (pp - 1 if bias else pp)
    v = np.where(feat, np.maximum(np.maximum(-mu, 0), np.where(b > 0, np.maximum(mu, 0), 0)), np.abs(mu))
    return float(v.max())


def row_sums(X, y, bias, beta=None):
    """(max_j sum_k |G_jk| / n over the features' rows of the Gram matrix, bias column included: what one unit of movement in every
    other coefficient can do to a coordinate's gradient;  max_j (|c_j| + sum_k |G_jk beta_k|) / n: the size of the terms a gradient
    is the difference of -- one ulp of it is what float64 resolves of a KKT residual).  Magnitudes: float64 is enough."""
    G, c, m = moments(X, y, bias, np.float64)
    p = np.asarray(X).shape[1]
    s = float((np.abs(G[:p]).sum(axis=1) / m).max())
    if beta is None:
        return s, None
    b = np.asarray(beta, dtype=np.float64)
    return s, float(((np.abs(c) + np.abs(G * b[None, :]).sum(axis=1)) / m).max())


def floor_term(own: float, scale: float, dtype=np.float64) -> float:
    """10 x the reference's own residual; 8 ulp of `scale` where float64 does not resolve that residual (below half an ulp of it)"""
    eps = float(np.finfo(dtype).eps)
    return 10.0 * own if own >= 0.5 * eps * scale else 8 * eps * scale
