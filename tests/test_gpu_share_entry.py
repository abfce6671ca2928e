"""
The share entry of the fused grouped kernel (csrc/grouped_fused.hip: every wave searches the offsets for the lower bounds of its
row share, csrc/grouped_split_dev.hpp) must land on the FIRST index of a run of equal offsets, or groups are fitted twice or not
at all.  Every forced split (context options "grouped_fused_waves" /
"grouped_fused_late_permille") is compared bit for bit with a forced ONE-wave launch, which searches nothing, on offsets with
leading, trailing and interior empty groups and one group several shares long, at 1, 63, 64, 65 and 4 097 groups
(tests/share_entry_cases.py).  An empty group is null, so a group a wave skipped or took twice shows in the flags as well.
"""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
from share_entry_cases import N_GROUPS, SPLITS, offsets_for  # noqa: E402

pytestmark = pytest.mark.gpu
P = 3


@pytest.fixture(scope="module")
def pds():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import polars_ds_extension_amd as m

    m.config.LIN_REG_EXPR_F64 = True
    return m


@pytest.fixture(scope="module")
def ctx(pds):
    import torch

    c = pds.Context(0)
    c.set_stream(torch.cuda.current_stream())
    yield c
    c.close()


def fit(pds, ctx, cols, y, off, waves, late):
    ctx.set_option("grouped_fused_waves", waves)
    ctx.set_option("grouped_fused_late_permille", late)
    try:
        co, nu = pds.lin_reg_by(*cols, target=y, group_offsets=off, add_bias=False, ctx=ctx)
        return co.cpu().numpy(), nu.cpu().numpy()
    finally:
        ctx.set_option("grouped_fused_waves", 0)
        ctx.set_option("grouped_fused_late_permille", 0)


@pytest.mark.parametrize("base", [0, 37])
@pytest.mark.parametrize("n_groups", N_GROUPS)
def test_every_split_equals_the_one_wave_launch(pds, ctx, n_groups, base):
    import torch

    off = offsets_for(n_groups, P, base=base)
    N = int(off[-1]) + 3
    rng = np.random.default_rng(7 + n_groups)
    X = rng.normal(size=(N, P))
    y = X @ rng.normal(size=P) + 0.1 * rng.normal(size=N)
    cols = [torch.from_numpy(np.ascontiguousarray(X[:, j])).cuda() for j in range(P)]
    ty, toff = torch.from_numpy(y).cuda(), torch.from_numpy(off).cuda()
    co1, nu1 = fit(pds, ctx, cols, ty, toff, 1, 0)
    empty = np.diff(off) == 0
    assert np.array_equal(nu1.astype(bool), empty)  # (every non-empty group has at least P + 2 rows)
    assert np.isfinite(co1[~empty]).all()
    for waves, late in SPLITS:
        co, nu = fit(pds, ctx, cols, ty, toff, waves, late)
        assert np.array_equal(nu, nu1), (waves, late)
        assert np.array_equal(co.view(np.uint64), co1.view(np.uint64)), (waves, late)
