"""tests/steady_cases.py restates the work split of the streaming launchers; this pins it at 256 CUs (the MI355X) to the numbers of
DESIGN.md's table, and checks that every row count tests/test_steady_state_gpu.py uses does put the kernels into their steady-state
loop.  A changed grid cap or unit size shows here first, without a GPU."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import steady_cases as sc  # noqa: E402

F64, F32 = sc.F64, sc.F32


@pytest.mark.parametrize("kind,dtype,p,t,second", [
    ("small", F64, 11, 262_144, 2049 * 128), ("small", F32, 11, 524_288, 2049 * 256),
    ("small", F64, 1, 262_144, 262_272), ("small", F32, 16, 524_288, 524_544),
    ("pass2", F64, 7, 262_144, 262_272), ("pass2", F32, 16, 524_288, 524_544),
    ("mid", F64, 17, 65_536, 1025 * 64), ("mid", F64, 32, 65_536, 65_600), ("mid", F64, 33, 32_768, 1025 * 32),
    ("mid", F64, 64, 32_768, 32_800), ("mid", F32, 32, 131_072, 1025 * 128), ("mid", F32, 33, 65_536, 1025 * 64),
    ("leverage_mid", F64, 20, 65_536, 65_600), ("leverage_mid", F64, 40, 32_768, 32_800),
    ("pass2_wide", F64, 20, 524_288, 524_289), ("pass2_wide", F32, 40, 524_288, 524_289),
    ("grouped_pred", F64, 3, 1_048_576, 1_048_577), ("grouped_pred", F32, 18, 2_097_152, 2_097_153),
])
def test_thresholds_at_256_cus(kind, dtype, p, t, second):
    assert sc.one_unit_rows(kind, dtype, p, 256) == t
    assert sc.second_unit_rows(kind, dtype, p, 256) == second
    at = sc.units_per_wave(kind, dtype, p, t, 256)
    assert at.min() == 1 and at.max() == 1 and sc.tail_rows(kind, dtype, p, t) == 0
    assert sc.units_per_wave(kind, dtype, p, second - 1, 256).max() == 1
    two = sc.units_per_wave(kind, dtype, p, second, 256)
    assert two.max() == 2 and int((two == 2).sum()) == 1 and int(two.sum()) == len(two) + 1


def test_the_ragged_unit_behind_the_loop_is_not_a_trip():
    """pass2_kernel past 262 144 rows: the last wave takes the ragged rows behind its loop, with no prefetch -- its double-buffered
    register sets swap for the first time at 262 272 rows."""
    u = sc.units_per_wave("pass2", F64, 5, 262_145, 256)
    assert u.max() == 1 and sc.tail_rows("pass2", F64, 5, 262_145) == 1
    assert sc.units_per_wave("pass2", F64, 5, 262_272, 256)[-1] == 2


def test_small_grids_follow_the_row_count():
    # below the cap the grid shrinks with the frame: one tile per wave or none, whatever the row count
    for n in (1, 127, 128, 129, 4096, 100_003, 262_144):
        for kind in ("small", "pass2", "grouped_pred"):
            assert sc.units_per_wave(kind, F64, 4, n, 256).max() <= 1
    assert len(sc.units_per_wave("small", F64, 4, 1000, 256)) == 8 and len(sc.units_per_wave("mid", F64, 20, 1000, 256)) == 1024
    assert sc.units_per_wave("pass2_wide", F64, 20, 1000, 256).tolist() == [1] * 16
    with pytest.raises(ValueError):
        sc.unit_rows("small", F64, 17)
    with pytest.raises(ValueError):
        sc.unit_rows("leverage_mid", F32, 20)


@pytest.mark.parametrize("num_cus", [256, 304, 64])
def test_every_gpu_case_is_in_steady_state(num_cus):
    cases = sc.steady_cases()
    assert len(cases) >= 90
    for kind, dtype, p, units in cases:
        n = sc.rows(kind, dtype, p, num_cus, units=units)
        u = sc.units_per_wave(kind, dtype, p, n, num_cus)
        assert u.max() >= 3 and int((u == 2).sum()) >= 1 and u.min() >= 2, (kind, dtype, p, n)
        assert sc.tail_rows(kind, dtype, p, n) > 0, (kind, dtype, p, n)
        assert len(u) == sc.n_waves(kind, dtype, p, 1 << 40, num_cus)
    # section 3 sits at rows("small"): pass2_kernel is dealt the same way
    for dtype in (F64, F32):
        for p in sc.SMALL_P:
            assert sc.rows("small", dtype, p, num_cus) == sc.rows("pass2", dtype, p, num_cus)
    # the un-fused route runs both of its kernels at the larger of their two row counts
    for p in (20, 40):
        n = sc.nofuse_rows(p, num_cus)
        for kind in ("pass2_wide", "leverage_mid", "mid"):
            u = sc.units_per_wave(kind, F64, p, n, num_cus)
            assert u.max() >= 3 and u.min() >= 2 and sc.tail_rows(kind, F64, p, n) > 0
    # the exact-integer Gram frames stay below 2^24 (f32's integers)
    for dtype in (F64, F32):
        for p in sc.SMALL_P + sc.MID_P:
            kind = "small" if p <= 16 else "mid"
            if num_cus <= 256:
                assert 9 * sc.rows(kind, dtype, p, num_cus) < 2 ** 24


@pytest.mark.parametrize("dtype", [F64, F32])
@pytest.mark.parametrize("p", sc.BOUNDARY_P)
def test_boundary_sizes(p, dtype):
    kind = "small" if p <= 16 else "mid"
    for num_cus in (256, 80):
        for n, each, last, tail in sc.boundary_rows(kind, dtype, p, num_cus):
            u = sc.units_per_wave(kind, dtype, p, n, num_cus)
            assert len(u) == sc.n_waves(kind, dtype, p, 1 << 40, num_cus)
            assert np.all(u[:-1] == each) and u[-1] == last and sc.tail_rows(kind, dtype, p, n) == tail, (n, u)


def test_frames_are_what_they_say():
    X, y, w = sc.integer_frame(1, 5000, 7, np.float32)
    assert X.dtype == np.float32 and set(np.unique(X)) == set(range(-3, 4)) and set(np.unique(w)) == {0, 1}
    Z = np.c_[X, np.ones(5000), y].astype(np.int64)
    assert np.array_equal(sc.integer_gram(X, y), Z.T @ Z)
    assert np.array_equal(sc.integer_gram(X, y, w), Z.T @ (Z * w.astype(np.int64)[:, None]))
    for pp in (1, 4, 19):
        s = sc.pred_group_sizes(3, 700_003, pp, 128, 3)
        assert s.sum() == 700_003 and s.min() == 0 and s[-5:].sum() == 0 and s.max() > 9 * 128
        ones = np.flatnonzero(s == 1)
        assert np.max(np.diff(np.flatnonzero(np.diff(ones) != 1))) >= 2000  # a run of thousands of one-row groups
    pk = {1: "1", 2: "2", 3: "4", 4: "4", 16: "16"}
    seen = {(pk.get(p, "8" if p <= 8 else "0"), f) for p, f, _ in sc.GLM_CASES}
    assert len(seen) == 24 and {p for p, _, _ in sc.GLM_CASES} == set(range(1, 17))  # every family at every packing, every width
    assert {(p, se) for p, _, se in sc.REPORT_CASES if p in (1, 2, 4, 8)} >= {(1, "hc1"), (2, "hc3"), (4, "hc2")}
