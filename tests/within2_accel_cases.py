"""Frames, seeds and cached reference results of the accelerated two-factor tests (test_within2_accel_cpu.py / _gpu.py).  TEST
INFRASTRUCTURE ONLY.  The frames are within2_cases.py's generators; a reference result is computed once per frame, arithmetic,
tolerance, sweep count and iteration and never changed.

The SEED of a frame is chosen as within2_cases.find_seed chooses it, for the ACCELERATED run: the first seed for which the float64
restatement's accelerated run (within2_accel_reference.tables) has a delta at its stopping sweep of at most HALF the tolerance, at
1e-8 and at 1e-13 -- a condition on the inputs, asserted before the device is looked at, so that the sweep at which a run stops does
not hang on the last bits of delta.  (within2_cases.SEEDS was chosen for the plain run: with it the accelerated run stops at
0.97 tol on panel p = 16 and at 0.94 tol on singletons p = 1.)  "movers" is exempt and keeps seed 0: its delta creeps towards the
tolerance (0.92 tol at the stop), whatever the seed.

Three more frames for the device tests:
    "one2":   every row in ONE level of factor 2 (Delta2 has one row per column)
    "many2":  3 000 levels of key 1 x 10 rows, random codes of key 2 in [0, 5 000): 4 986 occupied codes at p = 4 -- more than the 4 096
              waves the level kernel starts at most (16 per compute unit x 256), so a wave walks more than one level and the records of
              a cycle come from 4 096 workgroups
    balanced_frame (within2_cases): one sweep is the whole projection; the loop stops at sweep 2, before any extrapolation.
"""
from __future__ import annotations

import functools

import numpy as np

import within2_accel_reference as ar
import within2_cases as c2
import within2_effects_reference as fxr
import within2_reference as w2r

TOLS = c2.TOLS
DTYPES = c2.DTYPES
columns = c2.columns


@functools.lru_cache(maxsize=None)
def one2_frame(p: int, seed: int = 0):
    rng = np.random.default_rng([71, p, seed])
    sizes = rng.integers(3, 90, size=40)
    return c2._make(rng, sizes, np.zeros(int(sizes.sum()), dtype=np.int64), p)


@functools.lru_cache(maxsize=None)
def many2_frame(p: int, seed: int = 0, workers: int = 3000, rows: int = 10, codes: int = 5000):
    rng = np.random.default_rng([73, p, seed])
    k2 = np.unique(rng.integers(0, codes, size=workers * rows), return_inverse=True)[1].reshape(-1)  # dense: every code occupied
    return c2._make(rng, [rows] * workers, k2, p)


_FRAMES = dict(c2._FRAMES, one2=one2_frame, many2=many2_frame)

# find_seed() made this table (0 where none is listed)
SEEDS = {("panel", 4): 3, ("small3", 3): 1}


def _stops_clear(Z, c1, c_2) -> bool:
    return all(ar.tables(Z, c1, c_2, np.float64, TOLS[t], accel=True)[4][-1] <= 0.5 * TOLS[t] for t in ("default", "tight"))


def find_seed(kind: str, p: int, limit: int = 200) -> int:
    for s in range(limit):
        F, y, off, c1, c_2 = _FRAMES[kind](p, s)
        if _stops_clear(np.column_stack([np.asarray(F, dtype=np.float64), np.asarray(y, dtype=np.float64)]), c1, c_2):
            return s
    raise RuntimeError("no seed")


def seed(kind: str, p: int) -> int:
    return SEEDS.get((kind, p), 0)


def frame(kind: str, p: int):
    return _FRAMES[kind](p, seed(kind, p))


@functools.lru_cache(maxsize=None)
def _base(kind: str, p: int, dtype_name: str, tol_name: str, sweeps, accel: bool):
    F, y, off, c1, c_2 = frame(kind, p)
    return ar.fit(np.asarray(F, dtype=np.float64), np.asarray(y, dtype=np.float64), c1, c_2, "se", DTYPES[dtype_name], TOLS[tol_name], sweeps=sweeps,
                  accel=accel)


def ref(kind: str, p: int, se: str, dtype_name: str = "float64", tol_name: str = "default", sweeps=None, accel: bool = True):
    """the restatement's run (within2_accel_reference.fit): report fields, pred / resid, effects / effects2, n_iter, deltas"""
    return w2r.select(_base(kind, p, dtype_name, tol_name, sweeps, accel), se)


@functools.lru_cache(maxsize=None)
def _truth(kind: str, p: int):
    """the long double PLAIN run at TRUTH_TOL: within2_reference.report, and the effects of within2_effects_reference.effects"""
    F, y, off, c1, c_2 = frame(kind, p)
    F64, y64 = np.asarray(F, dtype=np.float64), np.asarray(y, dtype=np.float64)
    same = kind in c2._FRAMES and c2.SEEDS.get((kind, p), 0) == seed(kind, p)  # (then it is within2_cases' cached truth)
    out = dict(c2._base(kind, p, "longdouble", "truth", None) if same else w2r.report(F64, y64, c1, c_2, "se"))
    fx = fxr.effects(F64, y64, c1, c_2)
    out["effects"], out["effects2"] = fx["effects"], fx["effects2"]
    return out


def truth(kind: str, p: int, se: str):
    return w2r.select(_truth(kind, p), se)


@functools.lru_cache(maxsize=None)
def _columns_truth(kind: str, p: int):
    F, y, off, c1, c_2 = frame(kind, p)
    return w2r.demean(np.column_stack([np.asarray(F, dtype=np.float64), np.asarray(y, dtype=np.float64)]), c1, c_2)[0]


@functools.lru_cache(maxsize=None)
def columns_run(kind: str, p: int, tol_name: str, accel: bool):
    """(sweeps, delta at the stop, distance of the projected columns from the long double truth's relative to their size) of the float64
    restatement run to its own criterion"""
    F, y, off, c1, c_2 = frame(kind, p)
    Z = np.column_stack([np.asarray(F, dtype=np.float64), np.asarray(y, dtype=np.float64)])
    got, _, _, n_iter, deltas = ar.tables(Z, c1, c_2, np.float64, TOLS[tol_name], accel=accel)
    want = _columns_truth(kind, p)
    return n_iter, deltas[-1], float(np.max(np.abs(got - want)) / np.max(np.abs(want)))
