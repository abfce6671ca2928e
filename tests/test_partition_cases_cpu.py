"""
The inputs and the reference of tests/test_partition_route_gpu.py, checked without a GPU (tests/partition_cases.py).

For every (p, bias, dtype) that file uses: the partition route's gate, restated in Python, accepts the frame (the proof that a call
took the route is the library's pds_debug_last_by_key_route, asserted on the device); the frame has the bucket shapes its docstring
promises -- an empty bucket, a one-chunk bucket with two heavy keys, a three-chunk bucket whose last chunk is shorter than a tile;
and the reference is sound on its own: on every compared group the f64 oracle lies within F64_TOL / 100 of the extended-precision
truth (so no compared group needs a conditioning exception), and the oracle refuses exactly the constructed null groups.
"""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import partition_cases as pc  # noqa: E402

CASES = pc.cases()
IDS = [f"p{p}-{'bias' if b else 'nobias'}-{np.dtype(d).name}" for p, b, d in CASES]


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle

    oracle.build()
    return oracle


def test_cases_cover_every_instantiation():
    """16 f64 widths (12 padded widths of the accumulate kernel, every unpadded one too); f32: all 12 padded widths and record sizes of
    1 .. 5 sixteen-byte pieces; f64 record sizes 2 .. 9 pieces; p' = 17 present."""
    assert [c[0] for c in CASES if c[2] is np.float64] == list(range(1, 17)) and pc.bias_of(16) and not pc.bias_of(1)
    assert {pc.layout(p, 4)["pc"] for p in pc.F32_WIDTHS} == {1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 14, 16}
    assert {pc.layout(p, 4)["rs"] // 16 for p in pc.F32_WIDTHS} == {1, 2, 3, 4, 5}
    # (f64 records are 2 .. 9 pieces: the scatter kernel's tenth size, 160 bytes, is reached by no width in either type)
    assert {pc.layout(p, 8)["rs"] // 16 for p in pc.F64_WIDTHS} == set(range(2, 10))
    assert {pc.layout(p, 8)["tile"] for p in pc.F64_WIDTHS} == {256, 512} and {pc.layout(p, 4)["tile"] for p in pc.F32_WIDTHS} == {512}
    assert any(p in (9, 11, 13, 15) for p in pc.F32_WIDTHS) and set(pc.HOST_WIDTHS) <= set(pc.F64_WIDTHS)
    for p in pc.F64_WIDTHS:
        assert pc.layout(p, 8)["B"] == pc.layout(p, 4)["B"] == pc.ids_per_bucket(p)


@pytest.mark.parametrize("p,bias,dtype", CASES, ids=IDS)
def test_frame_takes_the_route_and_has_its_buckets(p, bias, dtype):
    f = pc.frame(p, bias, dtype)
    isz = np.dtype(dtype).itemsize
    L = pc.layout(p, isz)
    N, B = len(f.keys), f.B
    assert f.X.dtype == dtype and f.y.dtype == dtype and f.keys.dtype == np.int64 and f.X.shape == (N, p)
    # ---- the gate
    kmin, kmax = int(f.keys.min()), int(f.keys.max())
    assert kmin < 0 and kmin % B != 0 and f.base == kmin - kmin % B
    assert pc.MIN_ROWS <= N <= 130_000 and kmax - f.base + 1 <= 4 * N
    nb = pc.gate(p, N, kmin, kmax, isz)
    assert nb == len(f.bucket_sizes()) and 0 < nb <= pc.KEY_SLOTS
    assert nb * B * L["nvp"] * 8 <= 2 * N * (p + 1) * isz
    assert np.any(np.diff(f.keys) < 0)  # (shuffled: an ordered frame never reaches the route)
    # ---- the constructed facts are those of the shuffled frame
    uk, cnt = np.unique(f.keys, return_counts=True)
    assert np.array_equal(uk, f.uk) and np.array_equal(cnt, f.cnt)
    # ---- buckets
    bs = f.bucket_sizes()
    bk = (f.uk - f.base) // B
    light = f.buckets["light"]
    assert len(light) >= 4 and light[0] == 0 and light[-1] == nb - 1
    assert bs[f.buckets["empty"]] == 0 and np.count_nonzero(bs == 0) == 1
    assert ((f.uk - f.base)[bk == nb - 1] % B).max() < B // 2  # the last bucket is only partly used
    lg = f.kind == "light"
    assert np.all((f.uk - f.base)[lg] % 3 == 2) and np.all(bs[light] < pc.CHUNK)
    ordinary = ~f.big & ~f.small
    assert f.cnt[ordinary].min() >= 3 * f.pp + 8 and f.cnt[ordinary].max() <= 3 * f.pp + 120
    assert np.all(f.cnt[f.small] < f.pp) and (f.small.sum() >= 3 if f.pp > 1 else not f.small.any())
    assert (f.collinear.sum() >= 3 if p >= 2 else not f.collinear.any()) and not (f.small & f.collinear).any()
    assert not f.null[~lg].any() and np.array_equal(f.null, f.small | f.collinear)
    for g in np.flatnonzero(f.collinear):
        A, _ = f.group(g)
        assert np.array_equal(A[:, 1], 2.0 * A[:, 0])  # (exact in either type)
    # heavy: one chunk, two keys of >= 30 % each -- far above 64 records of a 256- or 512-record tile
    hb = f.buckets["heavy"]
    hv = np.flatnonzero(f.big & (bk == hb))
    assert len(hv) == 2 and bs[hb] < pc.CHUNK and np.count_nonzero(bk == hb) == 14
    assert np.all(f.cnt[hv] >= 0.3 * bs[hb]) and np.all(f.cnt[hv] * L["tile"] / bs[hb] > 1.5 * pc.HEAVY)
    assert set(((f.uk - f.base)[hv] % B).tolist()) == {1, B - 1}
    # giant: exactly three chunks, the last at most 256 records; one key with > 90 %: more than 256 records of it per 512-record tile
    gb = f.buckets["giant"]
    gi = np.flatnonzero(f.big & (bk == gb))
    assert len(gi) == 1 and np.count_nonzero(bk == gb) == 11
    assert -(-bs[gb] // pc.CHUNK) == 3 and 0 < bs[gb] - 2 * pc.CHUNK <= 256
    assert f.cnt[gi[0]] > 0.9 * bs[gb] and (L["tile"] < 512 or f.cnt[gi[0]] * 512 / bs[gb] > 256)
    assert int(f.big.sum()) == 3


@pytest.mark.parametrize("p,bias,dtype", CASES, ids=IDS)
def test_reference_alone(orc, p, bias, dtype):
    """the f64 oracle against the extended-precision truth on every compared group, and its null groups against the constructed ones"""
    f = pc.frame(p, bias, dtype)
    t = pc.truth(f)
    co, nu = pc.oracle_by(orc, f)
    assert np.array_equal(nu, f.null), np.flatnonzero(nu != f.null)
    ok = ~f.null
    assert np.isfinite(t[ok]).all() and np.isnan(t[~ok]).all()
    d = pc.nrel_rows(co[ok], t[ok])
    print(f"p={p} bias={bias} {np.dtype(dtype).name}: {ok.sum()} compared groups, worst oracle-to-truth distance {d.max():.2e}")
    assert d.max() < pc.F64_TOL / 100


def test_smallest_groups_are_well_conditioned(orc):
    """3p' + 8 rows at p' = 17, 9 and 1: f64 Cholesky against the extended-precision truth stays below 1e-14"""
    for p, bias in ((16, True), (8, True), (1, False)):
        f = pc.frame(p, bias, np.float64)
        t = pc.truth(f)
        ok = np.flatnonzero(~f.null)
        g = ok[np.argmin(f.cnt[ok])]
        A, y = f.group(g)
        b = orc.pl_lr(A[:, :p], y, add_bias=bias, solver="choleskey")
        assert pc.nrel_rows(b[None], t[g][None])[0] < 1e-14, (p, bias, int(f.cnt[g]))


def test_big_frame_passes_the_gate_beyond_the_slots():
    x, y, keys, uk, beta = pc.big_frame()
    n = len(keys)
    nb = pc.gate(1, n, int(keys.min()), int(keys.max()), 8)
    assert nb > 16384 and nb > pc.KEY_SLOTS and nb * 4 > 64 * 1024  # (the histogram's LDS passes 64 KiB)
    assert len(uk) > 3_000_000 and np.all(np.isfinite(beta)) and np.all(np.diff(uk) > 0)
    assert set(np.unique(x).tolist()) == {1.0, 2.0, 3.0} and np.all(y == np.round(y)) and np.abs(y).max() <= 4


def test_gate_refuses_what_the_route_refuses():
    """the restated gate at its own limits: rows, range, buckets, table size"""
    assert pc.gate(8, (1 << 16) - 1, 0, 999, 8) == 0 and pc.gate(8, 1 << 16, 0, 999, 8) == 4
    assert pc.gate(8, 1 << 16, 0, 4 * (1 << 16), 8) == 0          # range > 4 N
    assert pc.gate(17, 1 << 20, 0, 999, 8) == 0
    assert pc.gate(1, 1 << 24, 0, 32768 * 256 - 1, 8) == 32768 and pc.gate(1, 1 << 24, 0, 32768 * 256, 8) == 0
    assert pc.gate(1, 1 << 16, 0, 200_000, 8) == 0                # table: 782 x 256 x 7 x 8 > 2 x 65536 x 2 x 8
    assert pc.gate(8, 1 << 16, -1, 254, 8) == 2                   # a negative smallest key: the base is rounded DOWN
