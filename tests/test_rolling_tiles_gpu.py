"""Rolling and expanding fits (rolling.hip, rolling_seg_dev.hpp) past one tile per wave, compared at EVERY row.

The default grids give every wave of a frame below 4.2 M (expanding), 8.4 M (9 - 12 coefficients) or 16.8 M rows (rolling) one
tile, so the tile loops, the anchors of a wave's later tiles and the prefetch across them are reached here through the context
option "rolling_waves" (a cap on the waves a launch starts), on frames of 8 - 10 tiles.  The frames are exact-integer frames
(tests/rolling_cases.py): the device's window moments are the true ones, and what is compared is one p' x p' solve per row --
against the project's contract (normwise 1e-10 in f64, the final rounding in f32), with no tolerance of its own.

A  tile loops under the cap, every instantiation; each case a second time on the default grid: the same bits
B  the three-launch tile prefix with 2 and 9 chunks, and seeded
C  the grouped forms: group starts at every position relative to tiles, stages and lanes; grp_advance's binary search
D  shift invariance, bit for bit
Each case prints its worst distance."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import rolling_cases as rc  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pds():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import polars_ds_extension_amd as m

    m.config.LIN_REG_EXPR_F64 = True
    return m


def dev(a):
    import torch

    return torch.from_numpy(np.array(a, order="C")).cuda()  # (a copy: the cached frames are read-only)


def host(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32, 1: np.uint8}[a.dtype.itemsize])


def spills(pds):
    from polars_ds_extension_amd import _lib

    return int(_lib.load().pds_ctx_workspace_spills(pds.default_context()._h))


def fit(pds, kind, X, y, off, w, bias, lam=0.0, skip=0, f32=False, waves=0, seed_moments=None):
    """(coeffs, pred, valid) as NumPy arrays, with "rolling_waves" = waves for this call"""
    ctx = pds.default_context()
    dt = np.float32 if f32 else np.float64
    cols = [dev(X[:, j].astype(dt)) for j in range(X.shape[1])]
    t = dev(y.astype(dt))
    before = ctx.get_option("rolling_waves")
    ctx.set_option("rolling_waves", waves)
    pds.config.LIN_REG_EXPR_F64 = not f32
    try:
        assert ctx.get_option("rolling_waves") == max(waves, 0)
        if off is None and kind == "rolling":
            out = pds.rolling_lin_reg(*cols, target=t, window_size=w, add_bias=bias, l2_reg=lam, skip_non_finite=skip > 0,
                                      min_valid_rows=skip if skip > 0 else None)
        elif off is None:
            out = pds.recursive_lin_reg(*cols, target=t, start_with=w, add_bias=bias, l2_reg=lam, seed_moments=seed_moments)
        elif kind == "rolling":
            out = pds.rolling_lin_reg_by(*cols, target=t, group_offsets=dev(off), window_size=w, add_bias=bias, l2_reg=lam)
        else:
            out = pds.recursive_lin_reg_by(*cols, target=t, group_offsets=dev(off), start_with=w, add_bias=bias, l2_reg=lam)
    finally:
        pds.config.LIN_REG_EXPR_F64 = True
        ctx.set_option("rolling_waves", before)
    co, pr, va = (host(o) for o in out)
    assert co.dtype == dt and pr.dtype == dt and co.shape == (len(y), X.shape[1] + int(bias))
    return co, pr, va


def fit_case(pds, case, X, y, off, waves):
    return fit(pds, case.kind, X, y, off, case.w, case.bias, case.lam, case.skip, case.f32, waves)


def check(name, out, tr, f32=False):
    """validity flags exactly the rule; coefficients at EVERY valid row within the contract; pred within its propagation"""
    co, pr, va = out
    np.testing.assert_array_equal(va, tr.valid)
    inval = tr.valid == 0
    assert np.isnan(co[inval]).all() and np.isnan(pr[inval]).all()
    got = co[tr.rows]
    bnorm = np.linalg.norm(tr.beta, axis=1)
    pbound = rc.F64_TOL * tr.znorm * bnorm  # pred_r = z_r . beta_r: the contract on beta_r, propagated (test_baseline_sizes.py)
    fin = tr.finite
    if not f32:
        # (a two-row window of integers can fit EXACTLY zero: the device's moments are exact, so it must return zero there too)
        dn = np.linalg.norm(got - tr.beta, axis=1)
        d = np.where(bnorm > 0, dn / np.where(bnorm > 0, bnorm, 1.0), np.where(dn == 0, 0.0, np.inf))
        worst, unit = float(d.max()), "nrel"
        assert worst < rc.F64_TOL, (name, int(tr.rows[np.argmax(d)]), worst)
    else:
        # the arithmetic is f64 either way: only the final rounding differs -- at most one f32 ulp from float32(truth)
        t32 = tr.beta.astype(np.float32)
        d = np.abs(got.astype(np.float64) - t32.astype(np.float64)) / np.spacing(np.abs(t32)).astype(np.float64)
        worst, unit = float(d.max()), "f32 ulp"
        assert worst <= 1.0, (name, int(tr.rows[np.argmax(d.max(axis=1))]), worst)
        pbound = pbound + np.spacing(np.abs(tr.pred.astype(np.float32))).astype(np.float64)  # ... and pred's own rounding
    dp = np.abs(pr[tr.rows][fin].astype(np.float64) - tr.pred[fin])
    assert np.all(dp <= pbound[fin]), (name, int(tr.rows[fin][np.argmax(dp - pbound[fin])]))
    assert np.isnan(pr[tr.rows][~fin]).all()  # a non-finite row: x_r . beta is NaN in the reference too
    pos = pbound[fin] > 0  # (an all-zero row z_r has pred 0 and bound 0)
    print(f"{name}: {len(tr.rows)} rows, worst {unit} {worst:.2e}, worst pred / bound {float(np.max(dp[pos] / pbound[fin][pos])):.2e}")
    return worst


def same_bits(a, b, what):
    for u, v, part in zip(a, b, ("coeffs", "pred", "valid")):
        np.testing.assert_array_equal(bits(u), bits(v), err_msg=f"{what}: {part}")


# ------------------------------------------------------------------------------------------------------------ A and C
@pytest.mark.parametrize("case", rc.section_a() + rc.section_c(), ids=lambda c: c.name)
def test_tile_loops_under_the_cap(pds, case):
    """every wave walks 2 - 5 tiles (rolling_cases.tiles_per_wave; the CPU test checks the geometry): values at every row, and
    the same bits on the default grid, where every wave walks one"""
    X, y, off = rc.case_frame(case)
    tr = rc.case_truth(case)
    capped = fit_case(pds, case, X, y, off, case.waves)
    assert spills(pds) == 0
    plain = fit_case(pds, case, X, y, off, 0)
    assert spills(pds) == 0
    check(case.name, capped, tr, case.f32)
    same_bits(capped, plain, f"{case.name}: rolling_waves {case.waves} against the default grid")


@pytest.mark.parametrize("kind,pp,bias,w,n", [("rolling", 8, False, 256, rc.N_ROLL), ("rolling", 3, True, 40, rc.N_ROLL),
                                              ("expanding", 4, True, 50, rc.N_EXP), ("rolling", 10, False, 64, rc.N_EXP),
                                              ("expanding", 10, False, 50, rc.N_EXP)])
def test_same_bits_on_a_non_integer_frame(pds, kind, pp, bias, w, n):
    """the option changes no result bit -- also where the sums round: a tile's anchor and arithmetic do not depend on its wave"""
    X, y = rc.uniform_frame(40 + pp, n, pp, bias)
    plain = fit(pds, kind, X, y, None, w, bias)
    for waves in (rc.CAP, 1):
        same_bits(fit(pds, kind, X, y, None, w, bias, waves=waves), plain, f"rolling_waves {waves}")
    assert np.isfinite(plain[0][w - 1:]).all()
    if kind == "rolling" and pp <= 8:  # the grouped form of the same frame, one group: the GROUPED instantiation under the cap
        off = np.array([0, n], np.int64)
        same_bits(fit(pds, kind, X, y, off, w, bias, waves=rc.CAP), fit(pds, kind, X, y, off, w, bias), "grouped, rolling_waves 3")


# ------------------------------------------------------------------------------------------------------------ B
_B = {c.name: c for c in rc.section_b()}
_truths = {}


def _b_truth(name):
    if name not in _truths:  # (computed once: the seeded test compares against the same rows)
        _truths[name] = rc.case_truth(_B[name])
    return _truths[name]


@pytest.mark.parametrize("name", list(_B), ids=str)
def test_prefix_chunks(pds, name):
    """the expanding fit's tile prefix with more than one chunk of 32 tiles, on the default grid, at every row"""
    case = _B[name]
    assert rc.n_chunks(case.n) >= 2
    X, y, off = rc.case_frame(case)
    out = fit_case(pds, case, X, y, off, 0)
    assert spills(pds) == 0
    check(name, out, _b_truth(name))
    same_bits(fit_case(pds, case, X, y, off, 5), out, f"{name}: rolling_waves 5")


def test_prefix_chunks_seeded(pds):
    """the 9-chunk frame's rows from 300 001 on, seeded with the moments of the rows in front (integers: an exact seed)"""
    case = _B["B-p3b-exp-9chunks"]
    X, y, _ = rc.case_frame(case)
    k = rc.N_SEED_FRONT
    seed = pds.gram_moments(*[dev(X[:k, j]) for j in range(X.shape[1])], target=dev(y[:k]))
    Z = np.c_[X[:k], np.ones(k), y[:k]]
    assert np.array_equal(seed, Z.T @ Z)
    out = fit(pds, "expanding", X[k:], y[k:], None, case.w, case.bias, seed_moments=seed)
    assert spills(pds) == 0
    tr = _b_truth(case.name)
    keep = tr.rows >= k
    assert keep.sum() == case.n - k
    tail = rc.Truth(np.ones(case.n - k, np.uint8), tr.rows[keep] - k, tr.beta[keep], tr.pred[keep], tr.finite[keep], None, tr.znorm[keep])
    check("B-p3b-exp-9chunks-seeded", out, tail)


# ------------------------------------------------------------------------------------------------------------ D
@pytest.mark.parametrize("pp,w,n", rc.SHIFT_CONFIGS, ids=lambda v: str(v))
def test_shift_invariance_bit_for_bit(pds, pp, w, n):
    """row k + i of the fit on the frame equals row i of the fit on frame[k:], for every i >= w - 1: with exact integer moments the
    solver's input is the same whatever tile, stage or lane the row lands in, and the same instructions run on it"""
    X, y = rc.integer_frame(7000 + pp + w, n, pp, False)
    base = fit(pds, "rolling", X, y, None, w, False)
    assert np.isfinite(base[0][w - 1:]).all()
    for k in rc.SHIFTS:
        cut = fit(pds, "rolling", X[k:], y[k:], None, w, False)
        for u, v, part in zip(base, cut, ("coeffs", "pred", "valid")):
            a, b = bits(u[k + w - 1:]), bits(v[w - 1:])
            bad = np.flatnonzero((a != b).reshape(len(a), -1).any(axis=1))
            assert len(bad) == 0, f"shift {k}: {part} differs at {len(bad)} rows, first at row {int(bad[0]) + w - 1} of the shifted frame"
    print(f"D p'={pp} w={w}: {len(rc.SHIFTS)} shifts, every row the same bits")
