"""
The fused grouped kernel under unequal row shares (csrc/grouped_split_dev.hpp; context options "grouped_fused_waves" and
"grouped_fused_late_permille").  Which wave fits a group does not enter the group's arithmetic, so every split must return the
SAME BITS: each case runs `lin_reg_by` once as the launcher would (checked against the oracle at test_gpu_parity.test_grouped's
tolerance) and again on three to five waves with the second half of the grid holding from 0.1 % to 99.9 % of the rows -- waves
that own nothing, waves that start and end inside a tile, groups that end exactly on a tile edge, a 700-row group that swallows
several waves' ranges, groups with fewer rows than features, offsets[0] > 0, a row count that is no multiple of the tile, and a
collinear group that the kernel marks for the second pass from a late wave.  Frames stay below 20 000 rows.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F64_TOL = 1e-10  # test_gpu_parity.py
F32_TOL = 1e-4
SPLITS = [(3, 300), (3, 700), (4, 1), (4, 999), (5, 455), (2, 500)]  # (grouped_fused_waves, grouped_fused_late_permille)


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


def dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def frame(p, bias, dtype, seed, base=0, n_groups=150):
    """Group sizes from {0, 1, 3, 99, 100, 128, 129, 700}; the frame starts at row `base` of its columns (offsets[0] = base)."""
    rng = np.random.default_rng(seed)
    sizes = rng.choice([0, 1, 3, 99, 100, 128, 129, 700], size=n_groups, p=[0.1, 0.08, 0.08, 0.2, 0.2, 0.15, 0.15, 0.04])
    sizes[0], sizes[1] = 128, 128  # two groups that end exactly on (f64) tile edges when base = 0
    sizes[n_groups // 2] = 700
    sizes[-3:] = [100, 0, 0]       # trailing empty groups
    sizes[2] = 129
    while sizes.sum() + base > 19_900:
        sizes[np.argmax(sizes == 100)] = 3
    off = base + np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    N = int(off[-1]) + 5  # rows behind the last group are not part of the frame
    X = rng.normal(size=(N, p))
    y = np.zeros(N)
    for g in range(n_groups):
        s = slice(off[g], off[g + 1])
        y[s] = X[s] @ rng.normal(size=p) + 0.1 * rng.normal(size=sizes[g]) + (0.7 if bias else 0.0)
    coll = int(np.flatnonzero(sizes == 129)[-1])  # a collinear group late in the frame: marked, refitted by the second pass
    if p >= 2:
        X[off[coll]: off[coll + 1], 1] = 2.0 * X[off[coll]: off[coll + 1], 0]
    return X.astype(dtype), y.astype(dtype), off, sizes, coll


def fit(pds, ctx, X, y, off, bias, waves=0, late=0):
    ctx.set_option("grouped_fused_waves", waves)
    ctx.set_option("grouped_fused_late_permille", late)
    try:
        co, nu = pds.lin_reg_by(*[dev(X[:, j]) for j in range(X.shape[1])], target=dev(y), group_offsets=off, add_bias=bias, ctx=ctx)
    finally:
        ctx.set_option("grouped_fused_waves", 0)
        ctx.set_option("grouped_fused_late_permille", 0)
    return co.cpu().numpy(), nu.cpu().numpy().astype(bool)


def check_oracle(orc, X, y, off, sizes, bias, co, nu, tol):
    p = X.shape[1]
    lo, hi = int(off[0]), int(off[-1])
    X64, y64 = X[lo:hi].astype(np.float64), y[lo:hi].astype(np.float64)
    co_o, nu_o = orc.grouped_lr([y64] + [X64[:, j] for j in range(p)], off - lo, add_bias=bias, nthreads=4)
    assert np.array_equal(nu, nu_o)
    assert np.isnan(co[nu]).all()
    ok = ~nu
    err = np.linalg.norm(co[ok] - co_o[ok], axis=1) / np.linalg.norm(co_o[ok], axis=1)
    well = sizes[ok] >= 2 * (p + bias) + 8
    print(f"max normwise distance to the oracle over {int(well.sum())} well-sized groups: {np.max(err[well]):.3e} (bound {tol:g})")
    assert np.max(err[well]) < tol
    if tol == F64_TOL:  # the small groups: held to their own conditioning, as test_grouped does
        idx = np.flatnonzero(ok)
        for g in idx[err >= tol]:
            sl = slice(off[g] - lo, off[g + 1] - lo)
            Xg = np.c_[X64[sl], np.ones(sizes[g])] if bias else X64[sl]
            bound = 64 * np.finfo(np.float64).eps * np.linalg.cond(Xg.T @ Xg)
            assert err[np.searchsorted(idx, g)] < bound, f"group {g} ({sizes[g]} rows)"


CASES = [(16, False, "f64", 0), (16, True, "f64", 37), (8, True, "f64", 0), (8, False, "f64", 129), (4, False, "f64", 1),
         (12, True, "f64", 0), (16, False, "f32", 0), (8, True, "f32", 255), (4, True, "f32", 0), (12, False, "f32", 3)]


@pytest.mark.parametrize("p,bias,kind,base", CASES)
def test_every_split_returns_the_same_bits(pds, orc, ctx, p, bias, kind, base):
    dtype = np.float64 if kind == "f64" else np.float32
    pds.config.LIN_REG_EXPR_F64 = kind == "f64"
    try:
        X, y, off, sizes, coll = frame(p, bias, dtype, seed=4000 + 10 * p + bias, base=base)
        co0, nu0 = fit(pds, ctx, X, y, off, bias)
        assert co0.dtype == dtype
        assert nu0[sizes < p + bias].all() and nu0[coll] and nu0.sum() < len(sizes)
        check_oracle(orc, X, y, off, sizes, bias, co0.astype(np.float64), nu0, F64_TOL if kind == "f64" else F32_TOL)
        for waves, late in SPLITS:
            co, nu = fit(pds, ctx, X, y, off, bias, waves, late)
            assert np.array_equal(nu, nu0), (waves, late)
            assert np.array_equal(co, co0, equal_nan=True), (waves, late)
    finally:
        pds.config.LIN_REG_EXPR_F64 = True


def test_same_context_three_frames_in_a_row(pds, ctx):
    """One context, three frames of different sizes under a forced split, then the first again: nothing of a call outlives it."""
    outs = []
    frames = [frame(16, True, np.float64, seed=s, n_groups=n) for s, n in ((1, 150), (2, 12), (3, 60))]
    for X, y, off, sizes, coll in frames:
        ref = fit(pds, ctx, X, y, off, True)
        got = fit(pds, ctx, X, y, off, True, 3, 700)
        assert np.array_equal(got[1], ref[1]) and np.array_equal(got[0], ref[0], equal_nan=True)
        outs.append(ref)
    X, y, off, sizes, coll = frames[0]
    again = fit(pds, ctx, X, y, off, True, 4, 250)
    assert np.array_equal(again[1], outs[0][1]) and np.array_equal(again[0], outs[0][0], equal_nan=True)


def test_option_range(pds, ctx):
    from polars_ds_extension_amd import _lib

    with pytest.raises(_lib.PdsError):
        ctx.set_option("grouped_fused_late_permille", 1000)
    with pytest.raises(_lib.PdsError):
        ctx.set_option("grouped_fused_late_permille", -1)
    ctx.set_option("grouped_fused_late_permille", 0)
