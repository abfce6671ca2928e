"""Offset shapes for the share entry of the fused grouped kernel (csrc/grouped_split_dev.hpp), shared by
tests/test_gpu_share_entry.py and tests/test_share_entry_cpu.py: leading, trailing and interior runs of empty groups (runs of equal
offsets: the lower bound must land on the FIRST of them) and one group longer than several waves' shares, at group counts around
a wavefront's 64 lanes (1, 63, 64, 65) and past 64 squared (4 097): the sizes at which a search by the whole wave changes its number of
rounds, should the entry become one (DESIGN.md 9, item 0a'')."""
import numpy as np

N_GROUPS = [1, 63, 64, 65, 4097]
SPLITS = [(2, 0), (2, 700), (3, 300), (7, 0), (7, 999), (64, 455), (65, 1), (0, 0)]  # (grouped_fused_waves, grouped_fused_late_permille)


def sizes_for(n_groups: int, p: int, seed: int = 0) -> np.ndarray:
    rng = np.random.default_rng(1000 + n_groups + seed)
    sizes = rng.integers(p + 2, p + 12, size=n_groups)
    if n_groups == 1:
        return np.array([700])
    k = max(1, n_groups // 16)
    sizes[:k] = 0                                       # leading empty groups
    sizes[-k:] = 0                                      # trailing empty groups
    mid = n_groups // 2
    sizes[mid: mid + 2 * k] = 0                         # an interior run
    sizes[rng.random(n_groups) < 0.1] = 0               # and scattered ones
    sizes[n_groups // 3] = max(700, int(sizes.sum()))   # one group as long as all the others together: several shares wide
    return sizes


def offsets_for(n_groups: int, p: int, base: int = 0, seed: int = 0) -> np.ndarray:
    return base + np.concatenate([[0], np.cumsum(sizes_for(n_groups, p, seed))]).astype(np.int64)
