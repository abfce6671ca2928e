"""
The host restatement of the fused grouped kernel's share entry (pds_grouped_fused_split: the kernel's rule, a lower bound over the
offsets per wave boundary) on the offset shapes of tests/share_entry_cases.py: leading, trailing and interior runs of empty groups,
one group several shares long, 1 / 63 / 64 / 65 / 4 097 groups.  For every wave count and share the waves' group ranges are in order
and partition [0, n_groups), and every bound is the FIRST index whose offset reaches the wave's first row (numpy's searchsorted,
side="left", says the same).  No GPU.
"""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(Path(__file__).resolve().parent))
from share_entry_cases import N_GROUPS, offsets_for  # noqa: E402

WAVES = [1, 2, 3, 7, 64, 65, 2048]
SHARES = [0, 1, 300, 455, 700, 999]


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
    first = np.full(waves, -7, dtype=np.int64)
    end = np.full(waves, -7, dtype=np.int64)
    rc = so.pds_grouped_fused_split(off.ctypes.data, len(off) - 1, waves, late, first.ctypes.data, end.ctypes.data)
    assert rc == 0, so.pds_last_error()
    return first, end


def row_of(w, W, total, late):
    """grouped_split_dev.hpp fused_split_row, with Python integers"""
    H = W // 2
    if late <= 0 or late >= 1000 or H == 0:
        return total * w // W
    E = W - H
    late_rows = total * late // 1000
    early = total - late_rows
    return early * w // E if w <= E else early + late_rows * (w - E) // H


@pytest.mark.parametrize("base", [0, 123_457])
@pytest.mark.parametrize("n_groups", N_GROUPS)
def test_partition_and_first_of_equal_offsets(so, n_groups, base):
    off = np.ascontiguousarray(offsets_for(n_groups, 3, base=base))
    G, total = n_groups, int(off[-1] - off[0])
    for W in WAVES:
        for late in SHARES:
            first, end = split(so, off, W, late)
            assert first[0] == 0 and end[-1] == G, (W, late)
            assert np.all(first <= end) and np.array_equal(end[:-1], first[1:]), (W, late)  # in order, nothing lost, nothing doubled
            keys = np.array([int(off[0]) + row_of(w, W, total, late) for w in range(1, W)], dtype=np.int64)
            want = np.searchsorted(off[:G], keys, side="left")  # first index whose offset is >= the key, over offsets[0 .. G)
            assert np.array_equal(first[1:], want), (W, late)
