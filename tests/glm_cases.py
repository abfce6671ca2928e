"""Frames and the per-group oracle for the grouped GLM tests (tests/test_grouped_glm_gpu.py, tools/grouped_glm_bench.py's check):
seeded ragged groups for the four families, and oracle.glm_irls looped over the groups."""
import numpy as np

FAMILIES = ("gaussian", "binomial", "poisson", "gamma")
WIDTHS = (1, 4, 8, 16)


def offsets(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def family_frame(rng, family, sizes, p):
    """X [n, p], y [n], offsets for groups of the given sizes: gaussian / binomial / poisson X ~ N(0, 1), beta_g = s U(-1, 1) with
    s = 0.5 (0.3 at p = 16), eta = X beta_g + 0.2; gamma X ~ U(0.1, 1), eta = 0.5 + X |beta_g|, y ~ Gamma(2, 1 / (2 eta))."""
    off = offsets(sizes)
    n = int(off[-1])
    s = 0.3 if p == 16 else 0.5
    beta = s * rng.uniform(-1.0, 1.0, size=(len(sizes), p))
    gid = np.repeat(np.arange(len(sizes)), sizes)
    if family == "gamma":
        X = rng.uniform(0.1, 1.0, size=(n, p))
        eta = 0.5 + np.einsum("ij,ij->i", X, np.abs(beta)[gid])
        y = rng.gamma(2.0, 1.0 / (2.0 * eta))
    else:
        X = rng.normal(size=(n, p))
        eta = np.einsum("ij,ij->i", X, beta[gid]) + 0.2
        if family == "gaussian":
            y = eta + 0.5 * rng.normal(size=n)
        elif family == "binomial":
            y = (rng.uniform(size=n) < 1.0 / (1.0 + np.exp(-eta))).astype(np.float64)
        else:
            y = rng.poisson(np.exp(eta)).astype(np.float64)
    return np.ascontiguousarray(X), np.ascontiguousarray(y), off


def ragged_sizes(rng, n_groups, p):
    return rng.integers(4 * (p + 1), 401, size=n_groups)


def oracle_by(orc, X, y, off, family, bias, tol=1e-10, max_iter=100):
    """oracle.glm_irls on every group's rows alone: (coeffs [G, p'], n_iter [G]); groups with fewer rows than p' are NaN / 0."""
    G = len(off) - 1
    pp = X.shape[1] + int(bias)
    co = np.full((G, pp), np.nan)
    it = np.zeros(G, dtype=np.int64)
    for g in range(G):
        a, b = int(off[g]), int(off[g + 1])
        if b - a < pp:
            continue
        co[g], it[g] = orc.glm_irls(X[a:b], y[a:b], family=family, add_bias=bias, tol=tol, max_iter=max_iter)
    return co, it


def inv_link(family, eta):
    if family == "binomial":
        e = np.exp(eta)
        return e / (1.0 + e)
    if family == "poisson":
        return np.exp(eta)
    if family == "gamma":
        return 1.0 / eta
    return eta


def eta_in_kernel_order(X, coeffs_per_row, bias):
    """x . beta of every row in the order the device forms it (grouped_irls.hip): start from the bias (0 without one), then one fused
    multiply-add per feature, c = 0 .. p - 1 -- libm's fma, element by element, so that the identity link can be compared to the
    letter (a cancelling dot product in another summation order differs by rounding of its TERMS, which has no bound relative to
    the sum)."""
    import ctypes
    import ctypes.util

    libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    libm.fma.restype = ctypes.c_double
    libm.fma.argtypes = [ctypes.c_double] * 3
    fma = np.frompyfunc(libm.fma, 3, 1)
    p = X.shape[1]
    eta = coeffs_per_row[:, p].astype(np.float64).copy() if bias else np.zeros(X.shape[0])
    for c in range(p):
        eta = fma(X[:, c], coeffs_per_row[:, c], eta).astype(np.float64)
    return eta
