"""Frames and cached reference results shared by the cluster-robust report tests (test_cluster_report_cpu.py /
test_cluster_report_gpu.py).  TEST INFRASTRUCTURE ONLY.  A reference result is computed once per frame, estimator and arithmetic and
never changed."""
from __future__ import annotations

import functools

import numpy as np

import cluster_reference as cr

WIDTHS = (1, 4, 8, 15, 16)
FIXED_SIZES = (1, 2, 63, 64, 65, 127, 128, 129, 300, 1000)  # around the 64-row step and the split at 128 (mixed_cases.ragged_frame's)
DTYPES = {"longdouble": np.longdouble, "float64": np.float64, "float32": np.float32}


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def ragged_frame(p: int, f32: bool = False, seed: int = 4321):
    """60 ragged clusters (FIXED_SIZES plus 50 sizes in 3 .. 200, shuffled).  Features: standard normal plus a per-cluster component;
    y = b0 + F b + u_g + e with a per-cluster shock u_g, so that rows of a cluster are correlated and the cluster and the HC errors
    differ by a visible factor.  f32: every value rounded to float32 (and returned as float32).  Returns (F [n, p], y, offsets, codes)."""
    rng = np.random.default_rng(seed + p)
    sizes = np.concatenate([np.array(FIXED_SIZES), rng.integers(3, 201, size=50)])
    rng.shuffle(sizes)
    g = len(sizes)
    codes = np.repeat(np.arange(g), sizes)
    n = int(sizes.sum())
    F = rng.normal(size=(n, p)) + 0.8 * rng.normal(size=(g, p))[codes]
    beta = rng.normal(size=p + 1)
    y = beta[0] + F @ beta[1:] + 1.0 * rng.normal(size=g)[codes] + rng.normal(size=n)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    if f32:
        F, y = F.astype(np.float32), y.astype(np.float32)
    return _freeze(F, y, off, codes)


@functools.lru_cache(maxsize=None)
def equal_frame(g: int, p: int, rows: int = 5, seed: int = 99):
    """g clusters of `rows` rows each (the batch boundaries of the outer-product step).  Where 5 rows each are not enough for the
    model to have a residual at all (n <= p' + 2: two or three clusters at width 16; the library refuses n <= p'), 12 rows each."""
    if g * rows <= p + 3:
        rows = 12
    rng = np.random.default_rng(seed + 100 * g + p)
    n = g * rows
    codes = np.repeat(np.arange(g), rows)
    F = rng.normal(size=(n, p)) + 0.5 * rng.normal(size=(g, p))[codes]
    y = 0.5 + F @ rng.normal(size=p) + rng.normal(size=g)[codes] + rng.normal(size=n)
    off = np.arange(0, n + 1, rows, dtype=np.int64)
    return _freeze(F, y, off, codes)


@functools.lru_cache(maxsize=None)
def singleton_frame(p: int, n: int = 20000, seed: int = 7):
    """Every row its own cluster: more clusters than a launch has waves, so a wave walks several and fills whole batches."""
    rng = np.random.default_rng(seed + p)
    F = rng.normal(size=(n, p))
    y = 1.0 + F @ rng.normal(size=p) + rng.normal(size=n) * (1.0 + np.abs(F[:, 0]))  # heteroskedastic
    return _freeze(F, y, np.arange(n + 1, dtype=np.int64), np.arange(n))


@functools.lru_cache(maxsize=None)
def lopsided_frame(p: int, n: int = 700, seed: int = 17):
    """G = 2: one cluster holds all rows but one (the last row is the other)."""
    rng = np.random.default_rng(seed + p)
    F = rng.normal(size=(n, p))
    y = -0.3 + F @ rng.normal(size=p) + rng.normal(size=n)
    codes = np.zeros(n, dtype=np.int64)
    codes[-1] = 1
    return _freeze(F, y, np.array([0, n - 1, n], dtype=np.int64), codes)


def columns(F):
    return [np.ascontiguousarray(F[:, j]) for j in range(F.shape[1])]


def design(F, bias: bool):
    """[F | 1] in float64 (exact for an f32 frame): what the references take."""
    F = np.asarray(F, dtype=np.float64)
    return np.column_stack([F, np.ones(len(F))]) if bias else F


_FRAMES = {"ragged": ragged_frame, "ragged32": lambda p: ragged_frame(p, True), "equal": None, "singleton": singleton_frame,
           "lopsided": lopsided_frame}


def frame(kind: str, p: int, g: int = 0):
    return equal_frame(g, p) if kind == "equal" else _FRAMES[kind](p)


@functools.lru_cache(maxsize=None)
def ref(kind: str, p: int, bias: bool, se: str, dtype_name: str = "longdouble", g: int = 0):
    F, y, off, codes = frame(kind, p, g)
    return cr.report(design(F, bias), np.asarray(y, dtype=np.float64), codes, se, DTYPES[dtype_name])


@functools.lru_cache(maxsize=None)
def spread(kind: str, p: int, bias: bool, se: str, dtype_name: str = "float64", g: int = 0):
    """Per field the distance between the reference in `dtype_name` arithmetic and in long double on that frame."""
    lo, ld = ref(kind, p, bias, se, dtype_name, g), ref(kind, p, bias, se, "longdouble", g)
    return {k: cr.rel(lo[k], ld[k]) for k in cr.FIELDS}
