"""Frames and cached reference results shared by the fixed-effects regression tests (test_within_cpu.py / test_within_gpu.py).  TEST
INFRASTRUCTURE ONLY.  A reference result is computed once per frame, estimator and arithmetic and never changed.

Every frame carries a per-group LEVEL of about 50 x the within spread in the features and in y: a kernel that forgets to centre, or
centres with the wrong group's mean, is then far outside every budget.  Within a group the first feature follows a trend and the
error has a group-specific slope on that trend, so that the scores of a group do not average out and the clustered and the
classical standard errors differ by a visible factor."""
from __future__ import annotations

import functools

import numpy as np

import within_reference as wr

WIDTHS = (1, 4, 8, 15, 16)
FIXED_SIZES = (1, 2, 63, 64, 65, 127, 128, 129, 300, 1000)  # around the 64-row step and the split at 128 (cluster_cases.FIXED_SIZES)
DTYPES = {"longdouble": np.longdouble, "float64": np.float64, "float32": np.float32}
LEVEL = 50.0


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _make(rng, sizes, p, f32=False):
    """(F [n, p], y, offsets, codes) for groups of the sizes given, in that order"""
    sizes = np.asarray(sizes, dtype=np.int64)
    g, n = len(sizes), int(sizes.sum())
    codes = np.repeat(np.arange(g), sizes)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    pos = np.arange(n) - off[:-1][codes]
    trend = (pos + 0.5) / sizes[codes] - 0.5  # -0.5 .. 0.5 inside every group
    F = rng.normal(size=(n, p)) + LEVEL * rng.normal(size=(g, p))[codes]
    F[:, 0] += 2.0 * trend
    beta = rng.normal(size=p)
    e = rng.normal(size=n) * (0.5 + rng.uniform(size=g))[codes] + 3.0 * rng.normal(size=g)[codes] * trend
    y = LEVEL * rng.normal(size=g)[codes] + (F - F.mean(axis=0)) @ beta / np.sqrt(p) + e
    if f32:
        F, y = F.astype(np.float32), y.astype(np.float32)
    return _freeze(F, y, off, codes)


@functools.lru_cache(maxsize=None)
def ragged_frame(p: int, f32: bool = False, seed: int = 8642):
    """60 ragged groups: FIXED_SIZES plus 50 sizes in 3 .. 200, shuffled.  f32: every value rounded to float32 (returned as float32)."""
    rng = np.random.default_rng(seed + p)
    sizes = np.concatenate([np.array(FIXED_SIZES), rng.integers(3, 201, size=50)])
    rng.shuffle(sizes)
    return _make(rng, sizes, p, f32)


@functools.lru_cache(maxsize=None)
def equal_frame(g: int, p: int, rows: int = 5, seed: int = 77):
    """g groups of `rows` rows each (whole and short batches of the outer-product step); 12 rows each where n - G - p <= 2."""
    if g * rows - g - p <= 2:
        rows = 12
    return _make(np.random.default_rng(seed + 100 * g + p), [rows] * g, p)


@functools.lru_cache(maxsize=None)
def pairs_frame(p: int, g: int = 20000, seed: int = 11):
    """20 000 groups of 2 rows: more groups than a launch has waves."""
    return _make(np.random.default_rng(seed + p), [2] * g, p)


@functools.lru_cache(maxsize=None)
def lopsided_frame(p: int, seed: int = 23):
    """One group of 699 rows and one of 1."""
    return _make(np.random.default_rng(seed + p), [699, 1], p)


@functools.lru_cache(maxsize=None)
def singletons_frame(p: int, seed: int = 31):
    """3 groups of 40, 70 and 25 rows among 200 singletons (which count in n and G and add nothing to W or M)."""
    rng = np.random.default_rng(seed + p)
    sizes = np.concatenate([[40, 70, 25], np.ones(200, dtype=np.int64)])
    rng.shuffle(sizes)
    return _make(rng, sizes, p)


def columns(F):
    return [np.ascontiguousarray(F[:, j]) for j in range(F.shape[1])]


def with_empty_groups(off):
    """(offsets with empty groups in front, in between and behind; the places of the original groups among the new ones)"""
    off = np.asarray(off)
    parts = [np.zeros(3, np.int64)]  # (the offsets start with three empty groups)
    for k in range(len(off) - 1):
        parts.append(np.full(3 if k % 3 == 1 else 1, off[k + 1]))  # every third group is followed by two empty ones
    padded = np.concatenate(parts + [np.full(4, off[-1])])
    return padded, np.flatnonzero(np.diff(padded) > 0)


_FRAMES = {"ragged": ragged_frame, "ragged32": lambda p: ragged_frame(p, True), "equal": None, "pairs": pairs_frame, "lopsided": lopsided_frame,
           "singletons": singletons_frame}


def frame(kind: str, p: int, g: int = 0):
    return equal_frame(g, p) if kind == "equal" else _FRAMES[kind](p)


@functools.lru_cache(maxsize=None)
def ref(kind: str, p: int, se: str, dtype_name: str = "longdouble", g: int = 0):
    F, y, off, codes = frame(kind, p, g)
    return wr.report(np.asarray(F, dtype=np.float64), np.asarray(y, dtype=np.float64), codes, se, DTYPES[dtype_name])


@functools.lru_cache(maxsize=None)
def spread(kind: str, p: int, se: str, dtype_name: str = "float64", g: int = 0):
    """Per field the distance between the reference in `dtype_name` arithmetic and in long double on that frame."""
    lo, ld = ref(kind, p, se, dtype_name, g), ref(kind, p, se, "longdouble", g)
    return {k: wr.rel(lo[k], ld[k]) for k in wr.FIELDS + wr.ROW_FIELDS}
