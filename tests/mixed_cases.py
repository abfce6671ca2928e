"""Frames and cached reference results shared by the MixedModel tests (test_mixed_model_cpu.py / test_mixed_model_gpu.py).
TEST INFRASTRUCTURE ONLY.  A reference result is computed once per frame and dtype and never changed."""
from __future__ import annotations

import functools

import numpy as np

import mixed_reference as mr

WIDTHS = (1, 4, 8, 15, 16)
GAMMAS = (0.0, 1e-3, 0.5, 10.0, 1e3)
FIXED_SIZES = (1, 2, 63, 64, 65, 127, 128, 129, 300, 1000)  # around the 64-row step, the 128-row residency and the split at 128


@functools.lru_cache(maxsize=None)
def ragged_frame(p: int, seed: int = 1234):
    """Ragged groups, features standard normal plus a constant 3 (the group means dominate the within scatter), the LAST feature
    constant within groups (a between column), y = X beta + 0.7 u_g + e.  Returns (features [n, p], y, offsets, codes)."""
    rng = np.random.default_rng(seed + p)
    sizes = np.concatenate([np.array(FIXED_SIZES), rng.integers(3, 201, size=50)])
    rng.shuffle(sizes)
    codes = np.repeat(np.arange(len(sizes)), sizes)
    n = int(sizes.sum())
    F = rng.normal(size=(n, p)) + 3.0
    F[:, p - 1] = (rng.normal(size=len(sizes)) + 3.0)[codes]
    beta = rng.normal(size=p + 1)
    y = beta[0] + F @ beta[1:] + 0.7 * rng.normal(size=len(sizes))[codes] + rng.normal(size=n)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    for a in (F, y, off, codes):
        a.setflags(write=False)
    return F, y, off, codes


def columns(F):
    return [np.ascontiguousarray(F[:, j]) for j in range(F.shape[1])]


@functools.lru_cache(maxsize=None)
def ref_profile(p: int, dtype_name: str):
    """deviance [k], beta [k, p'], resid_var [k] of the helper at GAMMAS on ragged_frame(p)."""
    dtype = getattr(np, dtype_name)
    F, y, off, codes = ragged_frame(p)
    X = mr.design(F, dtype)
    out = [mr.profile(X, y, codes, len(off) - 1, g, dtype) for g in GAMMAS]
    return (np.array([o["deviance"] for o in out]), np.stack([o["beta"] for o in out]), np.array([o["resid_var"] for o in out]))


@functools.lru_cache(maxsize=None)
def ref_fit(p: int, dtype_name: str):
    dtype = getattr(np, dtype_name)
    F, y, off, codes = ragged_frame(p)
    return mr.fit_reml(mr.design(F, dtype), y, codes, len(off) - 1, dtype=dtype)


def rel(a, b) -> float:
    """Distance of a from the reference b relative to b's size: |a - b| / |b| for scalars, max |a - b| / max |b| for vectors."""
    a = np.asarray(a, dtype=np.longdouble)
    b = np.asarray(b, dtype=np.longdouble)
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


def ulp8(b) -> float:
    """8 units in the last place of a double, relative."""
    return 8 * float(np.finfo(np.float64).eps)


@functools.lru_cache(maxsize=None)
def profile_spread():
    """Per quantity the worst distance between the helper in float64 and in long double over every width and gamma."""
    worst = {"deviance": 0.0, "beta": 0.0, "resid_var": 0.0}
    for p in WIDTHS:
        d64, b64, v64 = ref_profile(p, "float64")
        dld, bld, vld = ref_profile(p, "longdouble")
        for k in range(len(GAMMAS)):
            worst["deviance"] = max(worst["deviance"], rel(d64[k], dld[k]))
            worst["beta"] = max(worst["beta"], rel(b64[k], bld[k]))
            worst["resid_var"] = max(worst["resid_var"], rel(v64[k], vld[k]))
    return worst


FIT_FIELDS = ("gamma", "coeffs", "std_errors", "resid_variance")


@functools.lru_cache(maxsize=None)
def fit_spread(p: int):
    """Per quantity the distance between the helper's own search in float64 and in long double on ragged_frame(p)."""
    f64, fld = ref_fit(p, "float64"), ref_fit(p, "longdouble")
    return {k: rel(f64[k], fld[k]) for k in FIT_FIELDS}


def budget(spread: float) -> float:
    """10 x the helper's own float64-vs-long-double distance; where that distance is 0, 8 ulp."""
    return 10.0 * spread if spread > 0.0 else ulp8(1.0)


@functools.lru_cache(maxsize=None)
def boundary_frame(seed: int = 0):
    """A frame whose y has no group effect at all: y centred within groups, the common mean added back."""
    rng = np.random.default_rng(seed)
    sizes = rng.integers(3, 60, size=40)
    codes = np.repeat(np.arange(len(sizes)), sizes)
    n = int(sizes.sum())
    F = rng.normal(size=(n, 3)) + 3.0
    y = rng.normal(size=n)  # (no dependence on the features either: their group means would otherwise leave a group effect in y)
    gm = np.bincount(codes, weights=y) / sizes
    y = y - gm[codes] + 2.0
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return F, y, off, codes
