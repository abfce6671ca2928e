"""
How the fused grouped kernel deals groups to its waves (csrc/grouped_split_dev.hpp), through the host restatement
pds_grouped_fused_split: for every wave count and every share of the second half of the grid the waves' group ranges are in order
and partition [0, n_groups) -- nothing lost, nothing doubled -- on offsets with empty groups, one giant group, offsets[0] > 0, fewer
groups than waves and a single group; the ranges follow the rule the kernel states (a group belongs to the wave in whose row
share its first row lies); and the second half's share of the rows is what was asked for.  No GPU.
"""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent

WAVES = [1, 2, 3, 4, 7, 8, 64, 2048]
SHARES = [0, 1, 250, 455, 500, 700, 999]


@pytest.fixture(scope="module")
def so():
    sys.path.insert(0, str(ROOT))
    from polars_ds_extension_amd import _build, _lib

    if not _lib.LIB_PATH.exists():
        _build.build()
    lib = _lib.load()
    lib.pds_grouped_fused_split.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    return lib


def split(so, off, waves, late):
    off = np.ascontiguousarray(off, dtype=np.int64)
    first = np.full(waves, -7, dtype=np.int64)
    end = np.full(waves, -7, dtype=np.int64)
    rc = so.pds_grouped_fused_split(off.ctypes.data, len(off) - 1, waves, late, first.ctypes.data, end.ctypes.data)
    assert rc == 0, so.pds_last_error()
    return first, end


def row_of(w, W, total, late):
    """grouped_split_dev.hpp fused_split_row, restated with Python integers"""
    H = W // 2
    if late <= 0 or late >= 1000 or H == 0:
        return total * w // W
    E = W - H
    late_rows = total * late // 1000
    early = total - late_rows
    return early * w // E if w <= E else early + late_rows * (w - E) // H


def frames():
    rng = np.random.default_rng(20250)
    out = {}
    sizes = rng.integers(0, 300, size=5000)
    sizes[rng.random(5000) < 0.2] = 0  # empty groups, runs of them
    out["ragged_with_empty"] = (0, sizes)
    sizes = rng.integers(1, 50, size=400)
    sizes[123] = 1_000_000  # one giant group: many waves own nothing
    out["one_giant"] = (0, sizes)
    out["offsets0_positive"] = (123_457, rng.integers(0, 200, size=3000))
    out["fewer_groups_than_waves"] = (5, np.array([100, 0, 3, 129, 0]))
    out["single_group"] = (0, np.array([1000]))
    out["single_empty_group"] = (9, np.array([0]))
    out["all_empty"] = (0, np.zeros(17, dtype=np.int64))
    out["trailing_empty"] = (0, np.array([128, 128, 0, 0, 0]))
    out["equal_100"] = (0, np.full(10_000, 100))
    return out


@pytest.mark.parametrize("name", list(frames()))
def test_waves_partition_the_groups_in_order(so, name):
    base, sizes = frames()[name]
    off = base + np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    G, total = len(sizes), int(off[-1] - off[0])
    for W in WAVES:
        for late in SHARES:
            first, end = split(so, off, W, late)
            assert first[0] == 0 and end[-1] == G, (W, late)
            assert np.all(first <= end), (W, late)
            assert np.array_equal(end[:-1], first[1:]), (W, late)  # in order, nothing lost, nothing doubled
            # the ownership rule: a group belongs to the wave in whose row share its first row lies
            bounds = np.array([off[0] + row_of(w, W, total, late) for w in range(W + 1)], dtype=np.int64)
            assert bounds[0] == off[0] and bounds[-1] == off[-1] and np.all(np.diff(bounds) >= 0)
            starts = off[:-1]
            for w in range(W):
                g0, g1 = int(first[w]), int(end[w])
                if g0 < g1:
                    lo = bounds[w] if w > 0 else starts[g0]
                    assert starts[g0] >= lo and (w == W - 1 or starts[g1 - 1] < bounds[w + 1]), (W, late, w)
                    assert g0 == 0 or w == 0 or starts[g0 - 1] < bounds[w], (W, late, w)


def test_second_half_gets_its_share_of_the_rows(so):
    """Equal groups, a device-filling grid: the second half of the waves holds late / 1000 of the rows, and within a half the
    waves hold equal shares (to one group)."""
    G, R, W = 1_000_000, 100, 2048
    off = np.arange(0, G * R + 1, R, dtype=np.int64)
    for late in (455, 500, 300):
        first, end = split(so, off, W, late)
        n = end - first
        assert abs(int(n[W // 2:].sum()) - G * late // 1000) <= 1
        assert n[: W // 2].max() - n[: W // 2].min() <= 1 and n[W // 2:].max() - n[W // 2:].min() <= 1
    f0, e0 = split(so, off, W, 0)
    assert (e0 - f0).max() - (e0 - f0).min() <= 1


def test_bad_arguments_are_refused(so):
    off = np.array([0, 10], dtype=np.int64)
    a = np.zeros(4, dtype=np.int64)
    assert so.pds_grouped_fused_split(off.ctypes.data, 1, 0, 0, a.ctypes.data, a.ctypes.data) != 0
    assert so.pds_grouped_fused_split(off.ctypes.data, 1, 2, 1000, a.ctypes.data, a.ctypes.data) != 0
    assert so.pds_grouped_fused_split(None, 1, 2, 0, a.ctypes.data, a.ctypes.data) != 0
