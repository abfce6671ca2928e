"""Frames and cached reference results shared by the two-factor fixed-effects tests (test_within2_cpu.py / test_within2_gpu.py).  TEST
INFRASTRUCTURE ONLY.  A reference result is computed once per frame, arithmetic, tolerance and sweep count and never changed.

Every frame carries a LEVEL of about 50 x the within spread on BOTH factors, in the features and in y: a kernel that forgets one of
the two projections, or subtracts another level's mean, is then far outside every budget.  Rows are in ascending order of key 1 (so
the offsets form applies); inside a level of key 1 the first feature follows a trend and the error has a level-specific slope on it,
so that the clustered and the classical standard errors differ by a visible factor."""
from __future__ import annotations

import functools

import numpy as np

import within2_reference as w2r
import within_cases as wc

WIDTHS = wc.WIDTHS
DTYPES = wc.DTYPES
LEVEL = wc.LEVEL
TOLS = {"default": 1e-8, "tight": 1e-13, "truth": w2r.TRUTH_TOL}


def _make(rng, sizes, codes2, p, f32=False):
    """(F [n, p], y, offsets of key 1, codes1, codes2) for levels of key 1 of the sizes given, in that order"""
    sizes = np.asarray(sizes, dtype=np.int64)
    g, n = len(sizes), int(sizes.sum())
    codes2 = np.asarray(codes2, dtype=np.int64)
    g2 = int(codes2.max()) + 1
    codes = np.repeat(np.arange(g), sizes)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    pos = np.arange(n) - off[:-1][codes]
    trend = (pos + 0.5) / sizes[codes] - 0.5
    F = rng.normal(size=(n, p)) + LEVEL * rng.normal(size=(g, p))[codes] + LEVEL * rng.normal(size=(g2, p))[codes2]
    F[:, 0] += 2.0 * trend
    beta = rng.normal(size=p)
    e = rng.normal(size=n) * (0.5 + rng.uniform(size=g))[codes] + 3.0 * rng.normal(size=g)[codes] * trend
    y = LEVEL * rng.normal(size=g)[codes] + LEVEL * rng.normal(size=g2)[codes2] + (F - F.mean(axis=0)) @ beta / np.sqrt(p) + e
    if f32:
        F, y = F.astype(np.float32), y.astype(np.float32)
    return wc._freeze(F, y, off, codes, codes2)


@functools.lru_cache(maxsize=None)
def ragged_frame(p: int, g2: int = 7, f32: bool = False, seed: int = 0):
    """60 ragged levels of key 1 (within_cases.FIXED_SIZES plus 50 sizes in 3 .. 200, shuffled), random codes of key 2 in [0, g2)"""
    rng = np.random.default_rng([4711, g2, p, seed])
    sizes = np.concatenate([np.array(wc.FIXED_SIZES), rng.integers(3, 201, size=50)])
    rng.shuffle(sizes)
    return _make(rng, sizes, rng.integers(0, g2, size=int(sizes.sum())), p, f32)


@functools.lru_cache(maxsize=None)
def panel_frame(p: int, seed: int = 0, firms: int = 200, years: int = 12):
    """An entry/exit panel: every firm is present over a random span of the years (at least half of them)"""
    rng = np.random.default_rng([99, p, seed])
    sizes = rng.integers(years // 2, years + 1, size=firms)
    first = np.array([rng.integers(0, years - s + 1) for s in sizes])
    last = first + sizes - 1
    codes2 = np.concatenate([np.arange(f, l + 1) for f, l in zip(first, last)])
    return _make(rng, sizes, codes2, p)


@functools.lru_cache(maxsize=None)
def blocks_frame(p: int, seed: int = 0, blocks: int = 3):
    """`blocks` components: block b has 8 levels of key 1 (10 .. 40 rows) whose rows take 4 + b levels of key 2 no other block uses"""
    rng = np.random.default_rng([5, blocks, p, seed])
    sizes, codes2, base = [], [], 0
    for b in range(blocks):
        s = rng.integers(10, 41, size=8)
        sizes.append(s)
        codes2.append(base + rng.integers(0, 4 + b, size=int(s.sum())))
        codes2[-1][: 4 + b] = base + np.arange(4 + b)  # every level is occupied
        base += 4 + b
    return _make(rng, np.concatenate(sizes), np.concatenate(codes2), p)


@functools.lru_cache(maxsize=None)
def singletons_frame(p: int, seed: int = 0):
    """3 levels of key 1 of 400, 700 and 250 rows among 200 singletons; 5 levels of key 2"""
    rng = np.random.default_rng([31, p, seed])
    sizes = np.concatenate([[400, 700, 250], np.ones(200, dtype=np.int64)])
    rng.shuffle(sizes)
    return _make(rng, sizes, rng.integers(0, 5, size=int(sizes.sum())), p)


@functools.lru_cache(maxsize=None)
def movers_frame(p: int = 4, seed: int = 0, workers: int = 300, firms: int = 40, rows: int = 6, movers: int = 30):
    """Few movers: 300 levels of key 1 with 6 rows each in 40 levels of key 2.  A worker stays in one level of key 2, except that one
    worker out of each level but the last changes to the NEXT level halfway (so the graph of the cells is connected, through single
    rows) and `movers` more change to a random level: the sweeps converge slowly."""
    rng = np.random.default_rng([17, p, seed])
    home = np.arange(workers) % firms
    codes2 = np.repeat(home, rows).reshape(workers, rows)
    for w in range(firms - 1):  # (worker w < firms has home w)
        codes2[w, rows // 2:] = w + 1
    for w in rng.choice(np.arange(firms, workers), size=movers, replace=False):
        codes2[w, rows // 2:] = (home[w] + 1 + rng.integers(0, firms - 1)) % firms
    return _make(rng, [rows] * workers, codes2.reshape(-1), p)


@functools.lru_cache(maxsize=None)
def small_frame(g2: int = 5, seed: int = 0):
    """p = 3, G1 = 12 (12 rows each), G2 = g2: the frame of the dummy-variable comparisons"""
    rng = np.random.default_rng([3, g2, seed])
    return _make(rng, [12] * 12, rng.integers(0, g2, size=144), 3)


@functools.lru_cache(maxsize=None)
def balanced_frame(p: int = 3, firms: int = 9, years: int = 6, seed: int = 8):
    """A complete balanced panel: every cell holds exactly one row"""
    return _make(np.random.default_rng(seed), [years] * firms, np.tile(np.arange(years), firms), p)


columns = wc.columns

_FRAMES = {"ragged7": lambda p, s: ragged_frame(p, 7, False, s), "ragged300": lambda p, s: ragged_frame(p, 300, False, s),
           "ragged7_32": lambda p, s: ragged_frame(p, 7, True, s), "ragged300_32": lambda p, s: ragged_frame(p, 300, True, s), "panel": panel_frame,
           "blocks": blocks_frame, "singletons": singletons_frame, "movers": movers_frame, "small5": lambda p, s: small_frame(5, s),
           "small3": lambda p, s: small_frame(3, s)}

# The seed of a frame (0 where none is listed): the first one for which the float64 reference's delta at its stopping sweep is at most
# HALF the tolerance, at 1e-8 and at 1e-13 -- a condition on the inputs the GPU tests assert before they look at the device, so that
# the sweep at which a run stops does not hang on the last bits of delta.  find_seed() is the search that made this table.
SEEDS = {("ragged7", 4): 1, ("ragged300", 1): 3, ("ragged300", 4): 3, ("ragged300", 16): 2, ("ragged300_32", 16): 2, ("panel", 4): 1,
         ("panel", 16): 7, ("singletons", 1): 1, ("small5", 3): 3, ("small3", 3): 1}


def find_seed(kind: str, p: int, limit: int = 200) -> int:
    for s in range(limit):
        F, y, off, c1, c2 = _FRAMES[kind](p, s)
        Z = np.column_stack([np.asarray(F, dtype=np.float64), np.asarray(y, dtype=np.float64)])
        if all(w2r.demean(Z, c1, c2, np.float64, TOLS[t])[2][-1] <= 0.5 * TOLS[t] for t in ("default", "tight")):
            return s
    raise RuntimeError("no seed")


def frame(kind: str, p: int):
    return _FRAMES[kind](p, SEEDS.get((kind, p), 0))


@functools.lru_cache(maxsize=None)
def _base(kind: str, p: int, dtype_name: str, tol_name: str, sweeps):
    F, y, off, c1, c2 = frame(kind, p)
    return w2r.report(np.asarray(F, dtype=np.float64), np.asarray(y, dtype=np.float64), c1, c2, "se", DTYPES[dtype_name], TOLS[tol_name], sweeps=sweeps)


def ref(kind: str, p: int, se: str, dtype_name: str = "longdouble", tol_name: str = "truth", sweeps=None):
    return w2r.select(_base(kind, p, dtype_name, tol_name, sweeps), se)


def truth(kind: str, p: int, se: str):
    return ref(kind, p, se)


@functools.lru_cache(maxsize=None)
def spread(kind: str, p: int, se: str, fmt: str = "float64", tol_name: str = "tight"):
    """Per field the distance from the truth of the yardstick run for a frame stored in `fmt`.
    tol "tight" (rounding dominates): the reference in `fmt` arithmetic.  In float64 it runs to its own criterion; float32 arithmetic
    cannot reach a delta of 1e-13 (its level means carry 1e-9 of rounding), so it runs the number of sweeps the float64 run took.
    tol "default" (truncation dominates): the float64 run stopped ONE SWEEP EARLIER than its own criterion."""
    own = ref(kind, p, se, "float64", tol_name)
    if tol_name == "tight":
        lo = own if fmt == "float64" else ref(kind, p, se, fmt, tol_name, own["n_iter"])
    else:
        lo = ref(kind, p, se, "float64", tol_name, own["n_iter"] - 1)
    ld = truth(kind, p, se)
    return {k: w2r.rel(lo[k], ld[k]) for k in w2r.FIELDS + w2r.ROW_FIELDS}
