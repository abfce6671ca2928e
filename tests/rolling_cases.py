"""Frames, truth and launch geometry of the row-by-row rolling / expanding tests (test_rolling_cases_cpu.py,
test_rolling_tiles_gpu.py).  TEST INFRASTRUCTURE ONLY.

Integer frames.  Features are integers in [-4, 4] ({+-1 .. +-4} for the one-coefficient frames with a two-row window, so that no
window is singular), y = X beta + c + e with integer beta in [-3, 3] (no zero), c in {0, 2} and e in [-2, 2].  Every moment product z_a z_b,
z_a y is then an integer of at most 4 * 148 in magnitude, every window or prefix sum of them an exact integer far below 2^53 at the
frame sizes used here (test_rolling_cases_cpu.py asserts it), and every value is a float32.  The device's fma increments, its
scans in any order and its tile anchors therefore reproduce the true window Gram EXACTLY; what is left between the device and the
truth is the rounding of one p' x p' solve.

Truth.  Per row, NumPy: cumulative sums of the integer products in float64 (exact), windows as differences of those sums,
np.linalg.solve on the stacked systems with lambda on every diagonal.  Rows holding a non-finite value are zeroed and counted out,
as OnlineLR::update does.

Geometry.  The constants of rolling.hip / rolling_seg_dev.hpp are restated below; parse_constants() reads the same values out of
the source text and the CPU test compares the two -- whoever changes one of them must change this module.
"""
from __future__ import annotations

import functools
import re
from collections import namedtuple
from pathlib import Path

import numpy as np

CSRC = Path(__file__).resolve().parent.parent / "polars_ds_extension_amd" / "csrc"

# ---------------------------------------------------------------------------------------------------------- constants, restated
SEG_K = 4                 # kSegK: consecutive rows per lane (rolling_seg_dev.hpp)
SEG_STAGE = 64 * SEG_K    # kSegStage
SEG_TILE = 4096           # kSegTile: expanding tiles, up to 8 coefficients
ROLL_TILE = 16384         # PDS_ROLL_TILE: rolling tiles, up to 8 coefficients
TILE_ROWS = 4096          # kTileRows: the lane = row kernel (9 .. 12 coefficients; its totals mode)
ROLL_WAVES = 2            # kRollWaves: waves per block of the lane = row kernel
PREFIX_CHUNK = 32         # kPrefixChunk: tiles per chunk of the three-launch prefix
SEG_BLOCKS_PER_CU = 4     # rolling_seg_kernel: one-wave blocks per compute unit
TOTALS_BLOCKS_PER_CU = 12 # rolling_totals_kernel: one-wave blocks per compute unit
ROW_BLOCKS_PER_CU = 4     # rolling_kernel / rolling_kernel_1w: two-wave blocks per compute unit (2 * PDS_ROLL_WPE)
ADVANCE_LANES = 64        # grp_advance: group starts settled by its one coalesced load; more fall through to the binary search

COND_MAX = 1e4            # every compared window / prefix has cond(G + lambda I) <= COND_MAX (asserted by the CPU test)
F64_TOL = 1e-10           # normwise relative distance of a coefficient row


def parse_constants() -> dict:
    """the same constants, read out of the kernels' source text"""
    seg = (CSRC / "rolling_seg_dev.hpp").read_text()
    hip = (CSRC / "rolling.hip").read_text()
    grp = (CSRC / "rolling_groups_dev.hpp").read_text()

    def one(pattern, text):
        m = re.findall(pattern, text)
        assert len(m) == 1, (pattern, m)
        return int(m[0])

    k = one(r"constexpr int kSegK = (\d+);", seg)
    assert len(re.findall(r"constexpr int kSegStage = 64 \* kSegK;", seg)) == 1
    wpe = one(r"#define PDS_ROLL_WPE (\d+)", hip)
    assert len(re.findall(r"int per_cu = 2 \* PDS_ROLL_WPE;", hip)) == 1
    caps = [int(v) for v in re.findall(r"ctx->num_cus \* (\d+)\)", hip)]
    assert sorted(set(caps)) == [4, 12] and caps.count(12) == 2 and caps.count(4) == 3, caps
    # (the two-wave kernels: num_cus * per_cu; the seg kernel 3 x "* 4"; the totals kernel 2 x "* 12")
    return {
        "SEG_K": k, "SEG_STAGE": 64 * k,
        "SEG_TILE": one(r"constexpr int kSegTile = (\d+);", seg),
        "ROLL_TILE": one(r"#define PDS_ROLL_TILE (\d+)", seg),
        "TILE_ROWS": one(r"constexpr int kTileRows = (\d+);", hip),
        "ROLL_WAVES": one(r"constexpr int kRollWaves = (\d+);", hip),
        "PREFIX_CHUNK": one(r"constexpr int kPrefixChunk = (\d+);", hip),
        "SEG_BLOCKS_PER_CU": 4, "TOTALS_BLOCKS_PER_CU": 12, "ROW_BLOCKS_PER_CU": 2 * wpe,
        "ADVANCE_LANES": one(r"return c < (\d+) \? g \+ c : grp_find\(off, g \+ \d+, ng - 1, r\);", grp),
    }


# ---------------------------------------------------------------------------------------------------------- launch geometry
# kernel kinds: "seg_rolling" / "seg_expanding" (rolling_seg_kernel, MODE 0 / 2), "totals" (rolling_totals_kernel), "row"
# (rolling_kernel / rolling_kernel_1w in any mode)
def tile_rows(kind: str) -> int:
    return {"seg_rolling": ROLL_TILE, "seg_expanding": SEG_TILE, "totals": SEG_TILE, "row": TILE_ROWS}[kind]


def n_tiles(kind: str, n: int) -> int:
    return -(-n // tile_rows(kind))


def n_waves(kind: str, n: int, num_cus: int = 256, rolling_waves: int = 0) -> int:
    """waves one launch starts on a frame of n rows: the launcher's grid, under the "rolling_waves" cap"""
    t = max(n_tiles(kind, n), 1)
    if kind == "row":
        blocks = min(max(-(-t // ROLL_WAVES), 1), num_cus * ROW_BLOCKS_PER_CU)
        if rolling_waves > 0:
            blocks = min(blocks, max(rolling_waves // ROLL_WAVES, 1))
        return blocks * ROLL_WAVES
    blocks = min(t, num_cus * (TOTALS_BLOCKS_PER_CU if kind == "totals" else SEG_BLOCKS_PER_CU))
    if rolling_waves > 0:
        blocks = min(blocks, rolling_waves)
    return blocks


def tiles_per_wave(kind: str, n: int, num_cus: int = 256, rolling_waves: int = 0) -> np.ndarray:
    """how many tiles each wave of the launch walks: `for (t = first; t < ntiles; t += stride)`"""
    t, nw = n_tiles(kind, n), n_waves(kind, n, num_cus, rolling_waves)
    return np.array([len(range(w, t, nw)) for w in range(nw)])


def first_turn_rows(kind: str, num_cus: int = 256) -> int:
    """smallest frame at which some wave of the DEFAULT grid walks a second tile"""
    per_cu = {"seg_rolling": SEG_BLOCKS_PER_CU, "seg_expanding": SEG_BLOCKS_PER_CU, "totals": TOTALS_BLOCKS_PER_CU,
              "row": ROW_BLOCKS_PER_CU * ROLL_WAVES}[kind]
    return num_cus * per_cu * tile_rows(kind) + 1


def n_chunks(n: int) -> int:
    """chunks of the expanding fit's tile prefix"""
    return -(-n_tiles("totals", n) // PREFIX_CHUNK)


def kernels_of(kind: str, pp: int, grouped: bool = False):
    """the tiled kernels one call launches"""
    if pp <= 8:
        return ("seg_rolling",) if kind == "rolling" else ("totals", "seg_expanding")
    assert not grouped, "grouped fits beyond 8 coefficients take rolling_wide.hip"
    return ("row",)


# ---------------------------------------------------------------------------------------------------------- frames
N_ROLL = 7 * ROLL_TILE + 8229   # 8 rolling tiles, the last one ragged (8 229 rows, no multiple of 4)
N_EXP = 9 * SEG_TILE + 1537     # 10 expanding / lane = row tiles, the last one ragged (1 537 rows)
N_CHUNKS9 = 1_060_000           # 259 tiles, 9 chunks: the 8-unrolled loop of chunk_prefix_kernel and its remainder
N_SEED_FRONT = 300_001          # rows in front of the seeded tail (no multiple of a tile: the tail's tiles cut the frame elsewhere)
N_CHUNKS2 = 140_000             # 35 tiles, 2 chunks
N_GROUP_EXP = 210_001           # the grouped expanding frame: a 140 000-row group from row 60 000 on
N_GROUP_LONG = 400_001          # ... and one whose long group crosses two chunk borders with a start-free chunk in between
N_TINY = 2 * ROLL_TILE + 1001   # the one-coefficient frame of tiny and empty groups


def lead_block(pp: int, bias: bool) -> np.ndarray:
    """p' rows of features whose [x, (1)] matrix is well conditioned: the first rows of a group of an expanding frame, so that the
    prefixes of p', p' + 1, ... rows are compared too (p' random integer rows are singular now and then)"""
    p = pp - int(bias)
    B = np.zeros((pp, p))
    B[:p, :p] = 4.0 * np.eye(p)
    if bias:
        B[p, :] = -4.0
    return B


@functools.lru_cache(maxsize=8)
def _frame(seed: int, n: int, pp: int, bias: bool, tiny: bool, lead_at: tuple):
    rng = np.random.default_rng(seed)
    p = pp - int(bias)
    if tiny:
        X = rng.choice(np.array([-4.0, -3.0, -2.0, -1.0, 1.0, 2.0, 3.0, 4.0]), size=(n, p))
    else:
        X = rng.integers(-4, 5, size=(n, p)).astype(np.float64)
    for s in lead_at:
        X[s:s + pp] = lead_block(pp, bias)
    beta = rng.choice(np.array([-3.0, -2.0, -1.0, 1.0, 2.0, 3.0]), size=p)  # (no zero: a one-coefficient fit of pure noise can be exactly 0)
    y = X @ beta + (2.0 if bias else 0.0) + rng.integers(-2, 3, size=n)
    X.flags.writeable = False
    y.flags.writeable = False
    return X, y


def integer_frame(seed, n, pp, bias, tiny=False, lead_at=()):
    """(X [n, p], y [n]) float64, read-only and cached; `lead_at`: rows at which a lead_block is written"""
    return _frame(int(seed), int(n), int(pp), bool(bias), bool(tiny), tuple(int(s) for s in lead_at))


def uniform_frame(seed, n, pp, bias):
    """a NON-integer frame (as test_rolling_vs_oracle builds it): for the same-bits runs only"""
    rng = np.random.default_rng(seed)
    p = pp - int(bias)
    X = rng.random((n, p))
    y = X @ rng.normal(size=p) + (0.4 if bias else 0.0) + 0.1 * rng.normal(size=n)
    return X, y


# ---- group layouts (offsets: G + 1 int64 values, empty groups as repeated offsets)
def offsets_rolling(n: int = N_ROLL) -> np.ndarray:
    """8 rolling tiles.  Group starts: on a tile start (2T), one row before (T - 1) and one row after (3T + 1) a tile start, at
    row indices = 1, 2, 3 mod 4 inside a lane (5, 10, 15, 6T + 777 + ...), an empty group, groups shorter than any window, and
    one group longer than two tiles ([3T + 1, 6T + 777))."""
    T = ROLL_TILE
    starts = [0, 5, 10, 15, 300, 300, 2000, T - 1, 2 * T, 2 * T + 50, 2 * T + 50 + 299, 3 * T + 1, 6 * T + 777, 6 * T + 777 + 513,
              6 * T + 777 + 513 + 1026, 7 * T - 2, n - 3, n]
    off = np.array(starts, dtype=np.int64)
    assert np.all(np.diff(off) >= 0) and off[-1] == n
    return off


TINY_RUN_AT = 5 * SEG_STAGE          # first row of the run of 150 tiny groups: a stage start, so the run sits in ONE stage
TINY_RUN_GROUPS = 150
TINY_EMPTY_AT = ROLL_TILE + 3 * SEG_STAGE + 7
TINY_EMPTY_GROUPS = 70


def offsets_tiny(n: int = N_TINY) -> np.ndarray:
    """p' = 1, window 2: 150 groups of 1 - 3 rows inside one stage, later 70 empty groups at one row, each run followed by a long
    group -- more than 64 group starts (or 64 offsets) between two consecutive stages: grp_advance's binary search."""
    sizes = np.tile([1, 2, 1, 3, 1, 2, 1, 1, 2, 1], TINY_RUN_GROUPS // 10)  # 150 groups, 225 rows
    assert len(sizes) == TINY_RUN_GROUPS and sizes.sum() <= SEG_STAGE
    run = TINY_RUN_AT + np.concatenate([[0], np.cumsum(sizes)])  # 151 offsets: the last one opens the long group
    off = np.concatenate([[0, 3, 700], run, [TINY_EMPTY_AT] * (TINY_EMPTY_GROUPS + 1), [TINY_EMPTY_AT + 9000, n - 1, n]]).astype(np.int64)
    assert np.all(np.diff(off) >= 0) and off[-1] == n
    return off


def offsets_expanding(n: int = N_GROUP_EXP) -> np.ndarray:
    """groups in front whose starts set tile flags and the first chunk's flag, then ONE long group from row 60 000 -- the middle
    of the first chunk of 32 tiles -- to 9 000 rows before the end (140 000 rows at the default n: across the chunk border at
    131 072; at N_GROUP_LONG across two borders, the chunk between them without a start), then short groups."""
    big0, big1 = 60_000, n - 10_001
    starts = [0, 3, 53, SEG_TILE, SEG_TILE + 1, 9000, 9000, 30_000 + 2, big0, big1, big1 + 3, big1 + 3 + 4099, n - 2, n]
    off = np.array(starts, dtype=np.int64)
    assert np.all(np.diff(off) >= 0) and off[-1] == n
    return off


def lead_rows(off, pp):
    """first rows of the groups that hold at least p' rows"""
    off = np.asarray(off)
    return tuple(int(s) for s, e in zip(off[:-1], off[1:]) if e - s >= pp)


# ---------------------------------------------------------------------------------------------------------- truth
def moment_products(X, y, bias):
    """per row: [upper triangle of z z' (row-major, a <= b), z y, 1] with z = [x, (1)] -- zeros for a non-finite row; and the mask"""
    n = len(y)
    Z = np.c_[X, np.ones(n)] if bias else np.asarray(X, np.float64)
    y = np.asarray(y, np.float64)
    fin = np.isfinite(Z).all(axis=1) & np.isfinite(y)
    Zc, yc = np.where(fin[:, None], Z, 0.0), np.where(fin, y, 0.0)
    iu = np.triu_indices(Z.shape[1])
    return np.concatenate([Zc[:, iu[0]] * Zc[:, iu[1]], Zc * yc[:, None], fin[:, None].astype(np.float64)], axis=1), fin, Zc


def prefix_sums(P):
    """C[r] = sum of the rows in front of row r (float64; exact for the integer frames)"""
    C = np.zeros((P.shape[0] + 1, P.shape[1]))
    np.cumsum(P, axis=0, out=C[1:])
    return C


Truth = namedtuple("Truth", "valid rows beta pred finite cond znorm")


def truth(X, y, bias, kind, w, lam=0.0, off=None, min_size=0, want_cond=False, want_beta=True) -> Truth:
    """Every row of a rolling (window w) or expanding (start_with w) fit, per group when `off` is given.
    valid [n] uint8: the rule (r - group start >= w - 1, and >= min_size finite rows in the window when min_size > 0);
    rows: the valid rows; beta [len(rows), p'], pred [len(rows)] (NaN where the row itself is non-finite), finite [len(rows)],
    cond [len(rows)] = cond_2(G + lambda I) (want_cond), znorm = |z_r|."""
    n = len(y)
    P, fin, Zc = moment_products(X, y, bias)
    C = prefix_sums(P)
    pp = Zc.shape[1]
    ng = pp * (pp + 1) // 2
    r = np.arange(n, dtype=np.int64)
    s = np.zeros(n, np.int64) if off is None else np.asarray(off)[np.searchsorted(off, r, side="right") - 1]
    lo = np.maximum(s, r - w + 1) if kind == "rolling" else s
    valid = r - s >= w - 1
    if min_size > 0:
        valid &= (C[r + 1, -1] - C[lo, -1]) >= min_size
    rows = np.flatnonzero(valid)
    M = C[rows + 1] - C[lo[rows]]
    iu = np.triu_indices(pp)
    A = np.zeros((len(rows), pp, pp))
    A[:, iu[0], iu[1]] = M[:, :ng]
    A[:, iu[1], iu[0]] = M[:, :ng]
    A[:, np.arange(pp), np.arange(pp)] += lam
    beta = pred = None
    if want_beta:
        beta = np.linalg.solve(A, M[:, ng:ng + pp, None])[..., 0]
        pred = np.einsum("ij,ij->i", Zc[rows], beta)
        pred[~fin[rows]] = np.nan
    cond = None
    if want_cond:
        ev = np.linalg.eigvalsh(A)
        cond = ev[:, -1] / np.maximum(ev[:, 0], 1e-300)
        cond[ev[:, 0] <= 0] = np.inf
    return Truth(valid.astype(np.uint8), rows, beta, pred, fin[rows], cond, np.linalg.norm(Zc[rows], axis=1))


def exact_integer_moments(X, y, bias):
    """(float64 prefix sums, the same sums in int64): equal iff the float64 cumulative sums are exact"""
    P, _, _ = moment_products(X, y, bias)
    return prefix_sums(P), np.concatenate([np.zeros((1, P.shape[1]), np.int64), np.cumsum(P.astype(np.int64), axis=0)])


# ---------------------------------------------------------------------------------------------------------- cases
# kind: "rolling" | "expanding"; w: window / start_with; waves: the "rolling_waves" setting of the capped run (0: default grid
# only); layout: None | "rolling" | "tiny" | "expanding" | "expanding_long"; skip: min_valid_rows of the skipping variant (0: off);
# f32: float32 frame and outputs
Case = namedtuple("Case", "name kind n pp bias w lam waves layout skip f32 seed")

PAIRS8 = [(1, False), (2, False), (2, True), (3, True), (4, False), (4, True), (5, False), (6, False), (6, True), (7, True),
          (8, False), (8, True)]       # every PP of the seg kernel with FULLP 0, 1 and 2
PAIRS12 = [(9, False), (10, False), (10, True), (11, True), (12, False), (12, True)]  # the lane = row kernel, FULLP 0, 1, 2
CAP = 3   # "rolling_waves" of section A: three one-wave blocks; ONE two-wave block (3 rounds down to a whole block)


def _tag(pp, bias):
    return f"p{pp}{'b' if bias else ''}"


def _case(name, kind, n, pp, bias, w, lam=0.0, waves=CAP, layout=None, skip=0, f32=False, seed=None):
    seed = 1000 + 10 * pp + int(bias) if seed is None else seed
    return Case(name, kind, n, pp, bias, w, lam, waves, layout, skip, f32, seed)


def section_a():
    cs = []
    for pp, bias in PAIRS8:
        t = _tag(pp, bias)
        for w in (256, 40, 300):
            cs.append(_case(f"A-{t}-roll{w}", "rolling", N_ROLL, pp, bias, w))
        cs.append(_case(f"A-{t}-exp", "expanding", N_EXP, pp, bias, pp))
    for pp, bias in PAIRS12:
        t = _tag(pp, bias)
        cs.append(_case(f"A-{t}-roll64", "rolling", N_EXP, pp, bias, 64))
        cs.append(_case(f"A-{t}-exp", "expanding", N_EXP, pp, bias, pp))
    cs.append(_case("A-p2b-roll20000", "rolling", N_ROLL, 2, True, 20_000))  # a window longer than a tile
    cs.append(_case("A-p8b-roll256-ridge", "rolling", N_ROLL, 8, True, 256, lam=0.1))
    cs.append(_case("A-p10b-exp-ridge", "expanding", N_EXP, 10, True, 10, lam=0.1))
    for pp, bias in ((4, True), (5, False), (8, False)):
        t = _tag(pp, bias)
        for w in (256, 40):
            cs.append(_case(f"A-{t}-roll{w}-f32", "rolling", N_ROLL, pp, bias, w, f32=True))
        cs.append(_case(f"A-{t}-exp-f32", "expanding", N_EXP, pp, bias, pp, f32=True))
    # the skipping variant: min_valid_rows = w - 1, so a window holding two bad rows is invalid and one holding one is valid
    cs.append(_case("A-p8-roll256-skip", "rolling", N_ROLL, 8, False, 256, skip=255))
    cs.append(_case("A-p3b-roll40-skip", "rolling", N_ROLL, 3, True, 40, skip=39))
    cs.append(_case("A-p10-roll64-skip", "rolling", N_EXP, 10, False, 64, skip=63))
    return cs


def section_b():
    return [
        _case("B-p3b-exp-9chunks", "expanding", N_CHUNKS9, 3, True, 3, waves=0),
        _case("B-p8-exp-2chunks", "expanding", N_CHUNKS2, 8, False, 8, waves=0),
        _case("B-p10b-exp-2chunks", "expanding", N_CHUNKS2, 10, True, 10, waves=0),
    ]


def section_c():
    cs = []
    for i, (pp, bias) in enumerate(PAIRS8):
        t = _tag(pp, bias)
        w = (40, 256, 300)[i % 3]
        cs.append(_case(f"C-{t}-roll{w}", "rolling", N_ROLL, pp, bias, w, layout="rolling"))
        n0 = pp if i % 2 == 0 else 50
        cs.append(_case(f"C-{t}-exp{n0}", "expanding", N_GROUP_EXP, pp, bias, n0, layout="expanding"))
    cs.append(_case("C-p2b-exp2-long", "expanding", N_GROUP_LONG, 2, True, 2, layout="expanding_long"))
    cs.append(_case("C-p1-roll2-tiny", "rolling", N_TINY, 1, False, 2, waves=2, layout="tiny"))
    cs.append(_case("C-p1-exp2-tiny", "expanding", N_TINY, 1, False, 2, waves=2, layout="tiny"))
    return cs


def all_cases():
    return section_a() + section_b() + section_c()


def case_offsets(case):
    return {None: lambda n: None, "rolling": offsets_rolling, "tiny": offsets_tiny, "expanding": offsets_expanding,
            "expanding_long": offsets_expanding}[case.layout](case.n)


def skip_tiles(case):
    """the skipping cases' bad rows sit around tiles that a wave of the capped launch walks SECOND and THIRD"""
    kern = kernels_of(case.kind, case.pp)[0]
    nw = n_waves(kern, case.n, 256, case.waves)
    return kern, (nw + 1, 2 * nw)   # wave 1's second tile, wave 0's third


def bad_rows(case):
    """rows made non-finite: t0 - w, t0 - 1, t0 and t1 - 1 of the two tiles of skip_tiles()"""
    if not case.skip:
        return np.zeros(0, np.int64)
    kern, tiles = skip_tiles(case)
    T = tile_rows(kern)
    rows = []
    for t in tiles:
        t0, t1 = t * T, min((t + 1) * T, case.n)
        rows += [t0 - case.w, t0 - 1, t0, t1 - 1]
    return np.array(sorted(set(rows)), dtype=np.int64)


def case_frame(case):
    """(X, y, off): the case's frame (float64; the f32 cases cast it, exactly) with its non-finite rows, and its group offsets"""
    off = case_offsets(case)
    if case.kind == "expanding":
        lead = lead_rows(off, case.pp) if off is not None else (0,)
    else:
        lead = ()
    X, y = integer_frame(case.seed, case.n, case.pp, case.bias, tiny=case.layout == "tiny" or case.pp == 1, lead_at=lead)
    bad = bad_rows(case)
    if len(bad):
        X, y = X.copy(), y.copy()
        for i, r in enumerate(bad):  # NaN in a feature, +inf in y, -inf in the last feature, in turn
            if i % 3 == 0:
                X[r, 0] = np.nan
            elif i % 3 == 1:
                y[r] = np.inf
            else:
                X[r, -1] = -np.inf
    return X, y, off


def case_truth(case, want_cond=False, want_beta=True) -> Truth:
    X, y, off = case_frame(case)
    return truth(X, y, case.bias, case.kind, case.w, case.lam, off=off, min_size=case.skip, want_cond=want_cond, want_beta=want_beta)


# section D: shift invariance, bit for bit -- (p', window, frame rows); the frame spans several tiles of the kernel behind the shift
SHIFTS = (1, 3, 255, 257, 4095, 16385)
SHIFT_CONFIGS = [(8, 256, 3 * ROLL_TILE + 16385 + 1021), (8, 300, 3 * ROLL_TILE + 16385 + 1021), (10, 64, 3 * TILE_ROWS + 16385 + 1021)]
