"""Frames for the weighted / offset grouped GLM tests (tests/test_glm_weighted_gpu.py, tests/test_glm_weighted_cpu.py).

default_rng(123), G = 150 ragged groups (glm_cases.ragged_sizes), X from glm_cases.family_frame, then in this order from the same
generator: the weights (integer: choice([0, 1, 2, 3], p = [.15, .45, .25, .15]); real: U(0.25, 4)), the offset (poisson U(-1, 1);
gaussian, binomial N(0, 0.5^2); gamma U(0, 0.5)), beta_g at family_frame's scale (0.5 U(-1, 1), 0.3 U(-1, 1) at p = 16), and y
redrawn from the family with eta = X beta_g + 0.2 + o (gamma: 0.5 + X |beta_g| + o, y ~ Gamma(2, 1 / (2 eta)))."""
import numpy as np

import glm_cases as gc

G = 150
WIDTHS = (1, 8, 16)
KINDS = ("integer", "real")


def draw_weights(rng, n, kind):
    if kind == "integer":
        return rng.choice([0.0, 1.0, 2.0, 3.0], size=n, p=[0.15, 0.45, 0.25, 0.15])
    return rng.uniform(0.25, 4.0, size=n)


def draw_offset(rng, n, family):
    if family == "poisson":
        return rng.uniform(-1.0, 1.0, size=n)
    if family == "gamma":
        return rng.uniform(0.0, 0.5, size=n)
    return rng.normal(0.0, 0.5, size=n)


def draw_y(rng, family, X, beta_rows, o):
    n = len(o)
    if family == "gamma":
        eta = 0.5 + np.einsum("ij,ij->i", X, np.abs(beta_rows)) + o
        return rng.gamma(2.0, 1.0 / (2.0 * eta))
    eta = np.einsum("ij,ij->i", X, beta_rows) + 0.2 + o
    if family == "gaussian":
        return eta + 0.5 * rng.normal(size=n)
    if family == "binomial":
        return (rng.uniform(size=n) < 1.0 / (1.0 + np.exp(-eta))).astype(np.float64)
    return rng.poisson(np.exp(eta)).astype(np.float64)


def frame_for_sizes(rng, family, sizes, p, kind, with_offset=True):
    """(X, y, off, pw, o) for the given group sizes; y follows the offset only when `with_offset` (o is then all zero)"""
    X, _, off = gc.family_frame(rng, family, sizes, p)
    n = len(X)
    pw = draw_weights(rng, n, kind)
    o = draw_offset(rng, n, family)
    if not with_offset:
        o = np.zeros(n)
    s = 0.3 if p == 16 else 0.5
    beta = s * rng.uniform(-1.0, 1.0, size=(len(sizes), p))
    gid = np.repeat(np.arange(len(sizes)), sizes)
    y = draw_y(rng, family, X, beta[gid], o)
    return X, np.ascontiguousarray(y), off, pw, o


def frame(family, p, kind, with_offset=True, n_groups=G):
    rng = np.random.default_rng(123)
    sizes = gc.ragged_sizes(rng, n_groups, p)
    return frame_for_sizes(rng, family, sizes, p, kind, with_offset)


def replicate(X, y, off, pw, o=None):
    """the frame with row i repeated pw_i times (integer weights): (X, y, off (, o))"""
    k = pw.astype(np.int64)
    gid = np.repeat(np.arange(len(off) - 1), np.diff(off))
    sizes = np.bincount(gid, weights=k, minlength=len(off) - 1).astype(np.int64)
    rows = np.repeat(np.arange(len(y)), k)
    out = (np.ascontiguousarray(X[rows]), np.ascontiguousarray(y[rows]), gc.offsets(sizes))
    return out + (np.ascontiguousarray(o[rows]),) if o is not None else out
