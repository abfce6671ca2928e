"""The references of the lasso / elastic-net / NNLS tests, checked on the CPU (no device): the NumPy restatement against the C oracle,
the KKT residual against a closed form, the recorded long double fixed points against the KKT conditions computed from the frames,
and the conditions every shipped frame has to meet for the device tests (tests/test_lr_penalised_gpu.py) to mean something:

  * the float64 oracle converges below max_iter (tol 1e-10, 5 000 sweeps); on the three frames around the prefetch border in under
    2 000 sweeps;
  * 10 % .. 90 % of the feature coefficients of the fixed point are zero at every width >= 8, for every penalty set;
  * the inactive coordinates sit inside the threshold, and the active ones away from zero, by at least 1 000 x the budget the device's
    coefficients get (10 x the oracle's own distance from the fixed point, times max |beta|);
  * the oracle has the fixed point's zero set and meets the KKT bound the device is held to.

Seeds: 77 + width, except where lr_penalised_cases.SEEDS names another one because that seed missed a condition."""
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT))

import lr_penalised_cases as lc  # noqa: E402
import lr_penalised_reference as ref  # noqa: E402

L = np.longdouble
SMALL = [(1, True), (1, False), (8, True), (8, False), (17, True), (65, False)]


def test_long_double_is_wider():
    assert np.finfo(L).eps < 1e-18


# ---- 1. the restatement is the oracle's iteration
@pytest.mark.parametrize("pen", list(lc.PENALTIES))
@pytest.mark.parametrize("p,bias", SMALL)
def test_sweeps_restates_the_oracle(orc, p, bias, pen):
    X, y, _ = lc.frame(p)
    l1, l2, pos = lc.PENALTIES[pen]
    G, c, m = ref.moments(X, y, bias, np.float64)
    pp = p + int(bias)
    cs, ys = (G[:p, p], c[p]) if bias else (np.zeros(0), 0.0)
    for tol, cap in ((lc.TOL, 1), (lc.TOL, 2), (lc.TOL, 3), (lc.TOL, lc.MAX_ITER)):
        mine, it, conv = ref.sweeps(G, c, m, p, bias, l1, l2, tol, cap, pos, np.float64)
        theirs, it_o, conv_o = orc.cd_from_gram(G, c, cs, ys, float(m), l1, l2, bias, tol, cap, pos)
        assert (it, conv) == (it_o, conv_o), (cap, it, it_o)
        assert len(mine) == pp and ref.rel(mine, theirs) <= 1e-13 if np.any(theirs) else not np.any(mine)
        assert np.array_equal(mine == 0, theirs == 0)
    assert conv and it < lc.MAX_ITER


@pytest.mark.parametrize("p,bias", SMALL)
def test_nnls_sweeps_restates_the_oracle(p, bias):
    X, y, _ = lc.frame(p)
    G, c, m = ref.moments(X, y, bias, np.float64)
    for cap in (1, 2, 3, lc.MAX_ITER):
        mine, it = ref.nnls_sweeps(G, c, p, bias, lc.TOL, cap, np.float64)
        theirs, it_o = lc.oracle_nnls_from_gram(G, c, bias, lc.TOL, cap)
        assert it == it_o, (cap, it, it_o)
        assert ref.rel(mine, theirs) <= 1e-13 and np.array_equal(mine == 0, theirs == 0)
    assert it < lc.MAX_ITER


# ---- 2. the KKT residual against a closed form
@pytest.mark.parametrize("positive", [False, True])
def test_kkt_on_an_orthogonal_design(positive):
    rng = np.random.default_rng(5)
    n, p, l1, l2 = 64, 6, 0.25, 0.5
    Q, _ = np.linalg.qr(rng.normal(size=(n, p)))
    X = Q * np.sqrt(n)  # X'X / n = I up to float64 rounding
    y = X @ np.array([2.0, -1.5, 0.1, -0.2, 0.9, 0.0]) + 0.05 * rng.normal(size=n)
    z = (X.astype(L).T @ y.astype(L)) / L(n)
    want = np.sign(z) * np.maximum(np.abs(z) - L(l1), 0) / (1 + L(l2))
    if positive:
        want = np.where(z < 0, L(0), want)
    assert 0 < np.count_nonzero(want) < p  # both kinds of coordinate are there
    assert ref.kkt(X, y, False, l1, l2, want, positive) <= 1e-14  # (the design is orthogonal to ~1e-16 only)
    G, c, m = ref.moments(X, y, False)
    got, it, conv = ref.sweeps(G, c, m, p, False, l1, l2, 1e-17, 100, positive, L)
    assert conv and ref.rel(got, want) <= 1e-14 and np.array_equal(got == 0, want == 0)
    assert ref.kkt(X, y, False, l1, l2, got, positive) <= 1e-17
    # a moved active coefficient shows with its size times (1 + l2); a dropped one with |z_j| - l1; a woken one with l1 + l2 d - ...
    j = int(np.flatnonzero(want != 0)[0])
    moved = want.copy()
    moved[j] += L(1e-6)
    assert abs(ref.kkt(X, y, False, l1, l2, moved, positive) - 1e-6 * (1 + l2)) <= 1e-12
    dropped = want.copy()
    dropped[j] = 0
    assert abs(ref.kkt(X, y, False, l1, l2, dropped, positive) - float(abs(z[j]) - l1)) <= 1e-12
    k = int(np.flatnonzero(want == 0)[0])
    woken = want.copy()
    woken[k] = L(1e-3)
    assert ref.kkt(X, y, False, l1, l2, woken, positive) >= float(l1 - abs(z[k])) * 0.99
    if positive:
        neg = want.copy()
        neg[k] = L(-1e-3)
        assert ref.kkt(X, y, False, l1, l2, neg, True) >= 1e-3
    # NNLS on the same design: beta = max(z, 0), and its residual in the units of G beta - c
    b = np.maximum(z, 0)
    assert ref.nnls_kkt(X, y, False, b) <= 1e-13 * n
    b2 = b.copy()
    b2[int(np.flatnonzero(b > 0)[0])] += L(1e-6)
    assert abs(ref.nnls_kkt(X, y, False, b2) - 1e-6 * n) <= 1e-10


def test_kkt_bias_term():
    X, y, _ = lc.frame(8)
    c = lc.case(8, True, "enet")
    off = c["star"].copy()
    off[8] += L(1e-6)
    assert abs(ref.kkt(X, y, True, 0.03, 0.05, off) - 1e-6) <= 1e-9  # sum(residual) / n moves by the bias's move


# ---- 3. the long double fixed points
@pytest.mark.parametrize("pen", lc.ALL_PENS)
@pytest.mark.parametrize("p,bias", SMALL)
def test_fixed_point_recomputed(p, bias, pen):
    """`sweeps` in long double at tol 1e-17 meets the KKT conditions to 1e-15, and is what the record holds"""
    fresh, rec = lc.case(p, bias, pen, True), lc.case(p, bias, pen)
    assert fresh["star_kkt"] <= 1e-15
    assert np.array_equal(fresh["star"], rec["star"]) and fresh["star_sweeps"] == rec["star_sweeps"]
    assert np.array_equal(fresh["floor"], rec["floor"])


@pytest.mark.parametrize("p,bias", lc.WIDTHS)
def test_frame_conditions(p, bias):
    """every recorded fixed point is one (from the frame, no solver), and the frame meets the conditions of the module docstring"""
    X, y, _ = lc.frame(p)
    assert X.shape == ((2 * p, p) if p >= 575 else (3 * p + 40, p))
    for pen in lc.ALL_PENS:
        c = lc.case(p, bias, pen)
        top = float(np.abs(c["star"]).max())
        margin = 1000.0 * c["budget"] * top
        zf = float(c["zero"].mean())
        print(f"p={p} bias={bias} {pen}: fixed point kkt {c['star_kkt']:.1e} after {c['star_sweeps']} sweeps; oracle {c['oracle_sweeps']} sweeps, "
              f"{c['own']:.1e} from it (budget {c['budget']:.1e}), kkt {c['oracle_kkt']:.1e} (bound {c['kkt_bound']:.1e}: {c['kkt_parts']}); "
              f"zero {zf:.0%}, slack {c['slack']:.1e}, smallest active {c['size']:.1e}, margin {margin:.1e}")
        assert c["star_kkt"] <= 1e-15
        assert c["oracle_converged"] and c["oracle_sweeps"] < lc.MAX_ITER and c["star_sweeps"] < lc.STAR_CAP
        if p >= 575:
            assert c["oracle_sweeps"] < 2000  # (hundreds: 13 .. 1 014)
        if p >= 8:
            assert 0.1 <= zf <= 0.9, (pen, zf)
        assert c["slack"] >= margin and c["size"] >= margin, (pen, c["slack"], c["size"], margin)
        assert np.array_equal(c["oracle"][:p] == 0, c["zero"])
        assert c["oracle_kkt"] <= c["kkt_bound"]
        assert lc.convex(X, 0.0)  # rows > p: check (b) applies to every penalty set
        if pen != "nnls":  # the bound at the default tol, used at p = 65 and 129
            ob = lc.oracle_of(X, y, bias, pen, lc.TOL_DEFAULT, lc.MAX_ITER)[0]
            assert lc.kkt_of(X, y, bias, pen, ob) <= lc.kkt_bound(X, y, bias, pen, lc.TOL_DEFAULT, c["floor"])[0]


# ---- 4. the special frames
@pytest.mark.parametrize("kind", list(lc.ORDER))
def test_order_frames(kind):
    """the copy makes the Gram matrix singular; which of the twins carries the weight is a matter of the update order: with the copy
    moved in front of column 3, the first sweep gives another answer"""
    X, y, _ = lc.order_frame(kind)
    k = lc.ORDER[kind]
    assert np.array_equal(X[:, k], X[:, 3]) and (k // 64 != 0) == (kind == "other_chunk")
    G, c, m = ref.moments(X, y, False, np.float64)
    assert np.linalg.matrix_rank(G) == lc.ORDER_P - 1
    l1, l2, pos = lc.PENALTIES["lasso"]
    a = ref.sweeps(G, c, m, lc.ORDER_P, False, l1, l2, lc.TOL, 1, pos, L)[0]
    perm = np.arange(lc.ORDER_P)
    perm[[0, k]] = perm[[k, 0]]  # the copy first
    Gp, cp, _ = ref.moments(X[:, perm], y, False, np.float64)
    b = ref.sweeps(Gp, cp, m, lc.ORDER_P, False, l1, l2, lc.TOL, 1, pos, L)[0]
    back = np.empty_like(b)
    back[perm] = b
    assert abs(a[3]) > 0 and ref.rel(back, a) > 1e-3
    for n_sweeps in (1, 2, 3, 5):
        for bias in (True, False):
            star, own = lc.partial(kind, lc.ORDER_P, bias, "lasso", n_sweeps)
            assert np.isfinite(own) and own < 1e-12


@pytest.mark.parametrize("positive", [False, True])
@pytest.mark.parametrize("p", [8, 65])
def test_saturated_frames(p, positive):
    X, y, l1 = lc.saturated_frame(p, positive)
    for bias in (True, False):
        ob, it, conv = lc.oracle_of(X, y, bias, (l1, 0.0, positive))
        G, c, m = ref.moments(X, y, bias)
        star, it_l, conv_l = ref.sweeps(G, c, m, p, bias, l1, 0.0, lc.TOL, lc.MAX_ITER, positive, L)
        assert conv and conv_l and not np.any(ob[:p]) and not np.any(star[:p])
        if bias:
            mean = y.astype(L).sum() / L(len(y))
            assert abs(star[p] - mean) <= 4 * np.finfo(L).eps * abs(mean)
            assert abs(mean) > 0.5 * np.abs(y).mean()  # (no cancellation in sum y: 4 ulp of the mean is what a float64 sum can hold)
    if positive:  # every feature is clamped, not thresholded
        Xl, yl = X.astype(L), y.astype(L)
        assert np.all(Xl.T @ yl < 0) and np.all(Xl.T @ (yl - yl.mean()) < 0)


@pytest.mark.parametrize("p", list(lc.ZERO_COLS))
def test_zero_column_frame(p):
    X, y, _ = lc.zero_column_frame(p)
    keep = np.arange(p) != lc.ZERO_COLS[p]
    for bias in (True, False):
        for pen in ((0.03, 0.05, False), (0.0, 0.1, True)):
            full, it, conv = lc.oracle_of(X, y, bias, pen)
            less, it2, conv2 = lc.oracle_of(np.ascontiguousarray(X[:, keep]), y, bias, pen)
            assert conv and conv2 and it == it2
            assert full[lc.ZERO_COLS[p]] == 0.0
            assert np.array_equal(np.delete(full, lc.ZERO_COLS[p]), less)


@pytest.mark.parametrize("p,bias", lc.GROUPED)
def test_grouped_frames(p, bias):
    X, y, off = lc.grouped_frame(p, bias)
    pp = p + int(bias)
    sizes = np.diff(off)
    assert len(sizes) == 40 and (sizes == 0).any() and sizes.max() == 5 * pp and (pp == 1 or ((sizes > 0) & (sizes < pp)).any())
    for pen in lc.ALL_PENS:
        cases = lc.grouped_case(p, bias, pen)
        assert [c is None for c in cases] == list(sizes < pp)
        worst = {"own": 0.0, "kkt": 0.0, "sweeps": 0}
        for g, c in enumerate(cases):
            if c is None:
                continue
            margin = 1000.0 * c["budget"] * float(np.abs(c["star"]).max())
            assert c["star_kkt"] <= 1e-15
            assert c["oracle_converged"] and c["oracle_sweeps"] < lc.MAX_ITER, (g, pen)
            assert c["slack"] >= margin and c["size"] >= margin, (g, pen, c["slack"], c["size"], margin)
            assert np.array_equal(c["oracle"][:p] == 0, c["zero"])
            assert c["oracle_kkt"] <= c["kkt_bound"]
            worst = {"own": max(worst["own"], c["own"]), "kkt": max(worst["kkt"], c["oracle_kkt"]), "sweeps": max(worst["sweeps"], c["oracle_sweeps"])}
        print(f"grouped p={p} bias={bias} {pen}: oracle worst {worst}")
