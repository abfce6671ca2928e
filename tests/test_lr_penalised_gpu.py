"""Lasso, elastic-net and NNLS fits on the MI355X (cd_kernel, nnls_kernel in csrc/solve.hip, through lin_reg, lin_reg_by, ElasticNet and
elastic_net_fit) against the optimality conditions of what they minimise and against the reference's iteration sweep by sweep.

Frames (lr_penalised_cases.py): correlated features, sparse true coefficients, at every width where the kernels or their call path
take another turn -- 1, 8, 16, 17, the 64-coordinate chunks (63, 64, 65, 128, 129), the one-copy return of the coefficients (252, 253),
the register prefetch (575, 576, 577) -- with and without a bias, under four penalty sets and under `positive` alone (NNLS); two
frames with a duplicated column, on which the answer depends on the update order; saturated frames; a zero column; grouped frames
with empty and short groups; f32 copies.  test_lr_penalised_cpu.py establishes on the CPU that these frames have zeros and active
coordinates with room around the threshold.

What is asserted, the reference side and its budget computed on the CPU and printed before anything on the device is asserted:

  a. KKT at convergence.  The device result's residual (lr_penalised_reference.kkt, long double from the frame, no solver) is at
     most tol max_j sum_k |G_jk| / n + 10 F: the first term follows from the stopping rule in exact arithmetic, F is the residual of
     the float64 oracle run to tol 1e-300 (8 ulp of the gradient's terms where that is not resolved).  At tol 1e-10, and at the
     default 1e-5 for p = 65 and 129, where a sweep that stopped early would miss by orders of magnitude.  NNLS: tol + 10 F in the
     units of G beta - c.
  b. Support and distance.  The coefficients within 10 x the float64 oracle's own distance from the long double fixed point
     (distance = max |a - b| / max |b|; 8 ulp where the oracle's is not resolved); the zero set equal to the fixed point's.
  c. Sweep by sweep.  After max_iter = 1, 2, 3, 5 sweeps nothing has converged, and the device holds the long double restatement's
     iterate within 10 x the float64 restatement's own distance from it: any other update order gives other iterates.
  d. Saturated frames give exact zeros and the mean of y; a zero column gets 0.0 and changes no bit of the others.
  e. lin_reg_by: (a) and (b) per group, null flags, every group the bits of a call on it alone, a NaN in one group moves no other.
  f. ElasticNet / elastic_net_fit: (a), also with l1 = 0 (coordinate descent forced).
  g. f32 frames: the residual on the values as stored, at most 10 x that of the oracle's f32 run under the library's f32 caps.
  h. Two calls give the same bits.

Measured on the MI355X (worst over the cases of a family; the reference's own figure on the same cases beside it -- the float64
oracle for (a), (b), (e), (f), the float64 restatement for (c), the oracle's f32 run for (g)).  (a), (e), (f) as fractions of the
bound: a fit that stops by the rule sits just below tol times the row sum (NNLS: just below tol), the oracle as much as the device.
                                                                     device    reference
  a  KKT / bound, coordinate descent, tol 1e-10      (92 fits)       0.13      0.13
  a  KKT / bound, NNLS, tol 1e-10                    (23 fits)       0.92      0.92
  a  KKT / bound at the default tol, p = 65, 129     (20 fits)       0.91      0.91
  b  distance from the long double fixed point      (115 fits)       6.2e-10   6.2e-10    (worst device / oracle on one fit: 1.8)
  c  distance after 1, 2, 3, 5 sweeps, CD           (368 fits)       1.3e-14   8.0e-15
  c  distance after 1, 2, 3 sweeps, NNLS             (69 fits)       6.7e-15   5.0e-15
  c  the order frames                                (32 fits)       3.3e-15   3.0e-15
  d  saturated frames: every feature exactly 0; the bias 0 ulp (p = 8) and 1 ulp (p = 65) from the mean of y
  d  zero column: 0.0, and the other coefficients bit for bit those of the fit without it (p = 8, and p = 80 with the column in
     the second chunk; across the widths 64 | 65 the two fits' moments come from different kernels and the bits differ)
  e  grouped KKT / bound                           (875 groups)      0.99      0.99
  e  grouped distance from the fixed point         (875 groups)      4.7e-10   4.7e-10
  f  ElasticNet / elastic_net_fit KKT / bound        (16 fits)       0.15      0.15
  g  f32 KKT residual, one model                     (20 fits)       7.3e-04   9.5e-04    (worst device / oracle on one fit: 1.4)
  g  f32 KKT residual, grouped                     (500 groups)      1.1e-03   1.1e-03    (worst device / oracle on one group: 9.5)
  (every case passed its own budget; the rows show the worst of each column, not one case.)  With `j0 = jc + 1` changed to
  `jc + 2` in cd_kernel, (c), (a), (b), (e), (f) fail (80 of 93 tests); with the update of max_change dropped, the same ones (84).
"""
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT))

import lr_penalised_cases as lc  # noqa: E402
import lr_penalised_reference as ref  # noqa: E402

pytestmark = pytest.mark.gpu

L = np.longdouble
EN_PENS = [(0.0, 0.1, False), (0.03, 0.03, False)]
_fits = {}  # (p, bias, pen) -> the device's coefficients at TOL / MAX_ITER, shared by (a) and (b)


@pytest.fixture(scope="module")
def pds():
    import polars_ds_extension_amd as m

    m.config.LIN_REG_EXPR_F64 = True
    return m


def cols(X):
    return [np.ascontiguousarray(X[:, j]) for j in range(X.shape[1])]


def args_of(pen):
    if pen == "nnls":
        return dict(positive=True)
    l1, l2, pos = lc.PENALTIES[pen] if isinstance(pen, str) else pen
    return dict(l1_reg=l1, l2_reg=l2, positive=pos)


def fit(pds, X, y, bias, pen, tol=lc.TOL, max_iter=lc.MAX_ITER):
    got = pds.lin_reg(*cols(X), target=y, add_bias=bias, tol=tol, max_iter=max_iter, **args_of(pen))
    assert got is not None and got.dtype == (np.float64 if pds.config.LIN_REG_EXPR_F64 else np.float32)
    assert got.shape == (X.shape[1] + int(bias),)
    return got


def fit_by(pds, X, y, off, bias, pen, tol=lc.TOL, max_iter=lc.MAX_ITER):
    co, nu = pds.lin_reg_by(*cols(X), target=y, group_offsets=off, add_bias=bias, tol=tol, max_iter=max_iter, **args_of(pen))
    return co, nu.astype(bool)


def converged_fit(pds, p, bias, pen):
    if (p, bias, pen) not in _fits:
        X, y, _ = lc.frame(p)
        _fits[(p, bias, pen)] = fit(pds, X, y, bias, pen)
    return _fits[(p, bias, pen)]


def measured(family, device, reference):
    print(f"MEASURED | {family} | device {device:.1e} | reference {reference:.1e}")


# ---- a. KKT at convergence
@pytest.mark.parametrize("p,bias", lc.WIDTHS)
def test_kkt_at_convergence(pds, p, bias):
    refs = {pen: lc.case(p, bias, pen) for pen in lc.ALL_PENS}  # on the CPU first
    for pen, c in refs.items():
        print(f"p={p} bias={bias} {pen}: oracle kkt {c['oracle_kkt']:.2e} after {c['oracle_sweeps']} sweeps, bound {c['kkt_bound']:.2e} {c['kkt_parts']}")
    for pen, c in refs.items():
        got = converged_fit(pds, p, bias, pen)
        k = lc.kkt_of(c["X"], c["y"], bias, pen, got)
        print(f"p={p} bias={bias} {pen}: device kkt {k:.2e}")
        measured("a nnls" if pen == "nnls" else "a cd", k / c["kkt_bound"], c["oracle_kkt"] / c["kkt_bound"])
        assert np.all(np.isfinite(got)) and k <= c["kkt_bound"], (pen, k, c["kkt_bound"])


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("p", [65, 129])
def test_kkt_at_the_default_tol(pds, p, bias):
    X, y, _ = lc.frame(p)
    bounds, own = {}, {}
    for pen in lc.ALL_PENS:
        bounds[pen] = lc.kkt_bound(X, y, bias, pen, lc.TOL_DEFAULT, lc.case(p, bias, pen)["floor"])[0]
        own[pen] = lc.kkt_of(X, y, bias, pen, lc.oracle_of(X, y, bias, pen, lc.TOL_DEFAULT, lc.MAX_ITER)[0])
        print(f"p={p} bias={bias} {pen} tol={lc.TOL_DEFAULT}: oracle kkt {own[pen]:.2e}, bound {bounds[pen]:.2e}")
    for pen in lc.ALL_PENS:
        k = lc.kkt_of(X, y, bias, pen, fit(pds, X, y, bias, pen, tol=lc.TOL_DEFAULT))
        print(f"p={p} bias={bias} {pen} tol={lc.TOL_DEFAULT}: device kkt {k:.2e}")
        measured("a default tol", k / bounds[pen], own[pen] / bounds[pen])
        assert k <= bounds[pen], (pen, k, bounds[pen])


# ---- b. support and distance
@pytest.mark.parametrize("p,bias", lc.WIDTHS)
def test_support_and_distance(pds, p, bias):
    refs = {pen: lc.case(p, bias, pen) for pen in lc.ALL_PENS}
    for pen, c in refs.items():
        assert lc.convex(c["X"], args_of(pen).get("l2_reg", 0.0))
        print(f"p={p} bias={bias} {pen}: oracle {c['own']:.2e} from the fixed point, budget {c['budget']:.2e}, {int(c['zero'].sum())} of {p} zero")
    for pen, c in refs.items():
        got = converged_fit(pds, p, bias, pen)
        d = ref.rel(got, c["star"])
        print(f"p={p} bias={bias} {pen}: device {d:.2e} from the fixed point")
        measured("b distance", d, c["own"])
        assert d <= c["budget"], (pen, d, c["own"])
        assert np.array_equal(got[:p] == 0, c["zero"]), (pen, np.flatnonzero((got[:p] == 0) != c["zero"]))


# ---- c. sweep by sweep
def _sweep_check(pds, kind, X, y, p, bias, pen, family, also=None):
    counts = (1, 2, 3) if pen == "nnls" else (1, 2, 3, 5)
    want = {n: lc.partial(kind, p, bias, pen, n) for n in counts}
    for n, (star, own) in want.items():
        print(f"{kind} p={p} bias={bias} {pen} after {n}: float64 restatement {own:.2e} from long double, budget {ref.budget(own):.2e}")
    for n, (star, own) in want.items():
        got = fit(pds, X, y, bias, pen, max_iter=n)
        d = ref.rel(got, star)
        print(f"{kind} p={p} bias={bias} {pen} after {n}: device {d:.2e}")
        measured(family, d, own)
        assert d <= ref.budget(own), (pen, n, d, own)
        if also is not None:  # the copy's coefficient on its own, absolute against max |beta|
            assert abs(L(got[also]) - star[also]) <= ref.budget(own) * np.abs(star).max(), (pen, n, got[also], star[also])


@pytest.mark.parametrize("p,bias", lc.WIDTHS)
def test_sweep_by_sweep(pds, p, bias):
    X, y, _ = lc.frame(p)
    for pen in lc.ALL_PENS:
        _sweep_check(pds, "width", X, y, p, bias, pen, "c nnls" if pen == "nnls" else "c cd")


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("kind", list(lc.ORDER))
def test_sweep_by_sweep_on_the_order_frames(pds, kind, bias):
    X, y, _ = lc.order_frame(kind)
    for pen in ("lasso", "lasso+"):
        _sweep_check(pds, kind, X, y, lc.ORDER_P, bias, pen, "c order frames", also=lc.ORDER[kind])


# ---- d. saturation and the zero column
@pytest.mark.parametrize("positive", [False, True])
@pytest.mark.parametrize("p", [8, 65])
def test_saturated(pds, p, positive):
    X, y, l1 = lc.saturated_frame(p, positive)
    mean = float(y.astype(L).sum() / L(len(y)))
    for bias in (True, False):
        for cap in (1, lc.MAX_ITER):
            got = fit(pds, X, y, bias, (l1, 0.0, positive), max_iter=cap)
            assert np.all(got[:p] == 0.0), got
            if bias:
                ulps = abs(got[p] - mean) / np.spacing(abs(mean))
                print(f"saturated p={p} positive={positive} max_iter={cap}: bias {ulps:.1f} ulp from mean y")
                assert ulps <= 4


@pytest.mark.parametrize("p", list(lc.ZERO_COLS))
def test_zero_column(pds, p):
    X, y, _ = lc.zero_column_frame(p)
    keep = np.arange(p) != lc.ZERO_COLS[p]
    Xk = np.ascontiguousarray(X[:, keep])
    for bias in (True, False):
        for pen in ((0.03, 0.05, False), (0.0, 0.1, True)):
            full = fit(pds, X, y, bias, pen)
            less = fit(pds, Xk, y, bias, pen)
            assert full[lc.ZERO_COLS[p]] == 0.0
            assert np.array_equal(np.delete(full, lc.ZERO_COLS[p]), less), (bias, pen)


# ---- e. grouped
@pytest.mark.parametrize("p,bias", lc.GROUPED)
def test_grouped(pds, p, bias):
    X, y, off = lc.grouped_frame(p, bias)
    pp = p + int(bias)
    sizes = np.diff(off)
    refs = {pen: lc.grouped_case(p, bias, pen) for pen in lc.ALL_PENS}
    fitted = [g for g in range(len(sizes)) if sizes[g] >= pp]
    for pen, cases in refs.items():
        print(f"grouped p={p} bias={bias} {pen}: oracle worst kkt / bound {max(cases[g]['oracle_kkt'] / cases[g]['kkt_bound'] for g in fitted):.2e}, "
              f"worst distance {max(cases[g]['own'] for g in fitted):.2e}")
    victim = fitted[len(fitted) // 2]
    Xn = X.copy()
    Xn[off[victim] + 1, p // 2] = np.nan
    for pen, cases in refs.items():
        co, nu = fit_by(pds, X, y, off, bias, pen)
        assert co.shape == (len(sizes), pp)
        assert np.array_equal(nu, sizes < pp) and np.isnan(co[nu]).all() and np.isfinite(co[~nu]).all()
        for g in fitted:
            c = cases[g]
            k, d = lc.kkt_of(c["X"], c["y"], bias, pen, co[g]), ref.rel(co[g], c["star"])
            measured("e grouped kkt", k / c["kkt_bound"], c["oracle_kkt"] / c["kkt_bound"])
            measured("e grouped distance", d, c["own"])
            assert k <= c["kkt_bound"], (pen, g, k, c["kkt_bound"])
            assert d <= c["budget"], (pen, g, d, c["own"])
            assert np.array_equal(co[g, :p] == 0, c["zero"]), (pen, g)
            a, b = int(off[g]), int(off[g + 1])
            alone, nu1 = fit_by(pds, X[a:b], y[a:b], np.array([0, b - a], dtype=np.int64), bias, pen)
            assert not nu1[0] and np.array_equal(alone[0], co[g]), (pen, g)
        con, nun = fit_by(pds, Xn, y, off, bias, pen)
        others = np.arange(len(sizes)) != victim
        assert np.array_equal(nun[others], nu[others]) and np.array_equal(con[others], co[others], equal_nan=True), pen


# ---- f. ElasticNet / elastic_net_fit
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("p", [8, 65])
def test_elastic_net(pds, p, bias):
    from polars_ds_extension_amd.linear_models import ElasticNet

    X, y, _ = lc.frame(p)
    bounds, own = {}, {}
    for pen in EN_PENS:
        own[pen] = lc.kkt_of(X, y, bias, pen, lc.oracle_of(X, y, bias, pen)[0])
        bounds[pen] = lc.kkt_bound(X, y, bias, pen, lc.TOL)[0]
        print(f"ElasticNet p={p} bias={bias} {pen}: oracle kkt {own[pen]:.2e}, bound {bounds[pen]:.2e}")
        assert own[pen] <= bounds[pen]
    for pen in EN_PENS:
        en = ElasticNet(l1_reg=pen[0], l2_reg=pen[1], has_bias=bias, tol=lc.TOL, max_iter=lc.MAX_ITER).fit(X, y)
        a = np.concatenate([en.coeffs(), [en.bias()]]) if bias else en.coeffs()
        b = pds.lstsq.elastic_net_fit(*cols(X), target=y, l1_reg=pen[0], l2_reg=pen[1], add_bias=bias, tol=lc.TOL, max_iter=lc.MAX_ITER)
        for name, got in (("ElasticNet", a), ("elastic_net_fit", b)):
            k = lc.kkt_of(X, y, bias, pen, got)
            print(f"{name} p={p} bias={bias} {pen}: device kkt {k:.2e}")
            measured("f elastic net", k / bounds[pen], own[pen] / bounds[pen])
            assert got.shape == (p + int(bias),) and k <= bounds[pen], (name, pen, k, bounds[pen])


# ---- g. f32 frames
def _f32_oracle(X32, y32, bias, pen):
    o = lc.orc()
    kw = args_of(pen)
    return o.pl_lr(X32, y32, add_bias=bias, tol=lc.TOL_F32, f32_path=True, l1_reg=kw.get("l1_reg", 0.0), l2_reg=kw.get("l2_reg", 0.0),
                   positive=kw["positive"])


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("p", [8, 65])
def test_f32(pds, p, bias):
    X, y, _ = lc.frame(p)
    X32, y32 = X.astype(np.float32), y.astype(np.float32)
    Xw, yw = lc.as_f32(X, y)
    Xg, yg, off = lc.grouped_frame(p, bias)
    Xg32, yg32 = Xg.astype(np.float32), yg.astype(np.float32)
    Xgw, ygw = lc.as_f32(Xg, yg)
    pp = p + int(bias)
    fitted = [g for g in range(len(off) - 1) if off[g + 1] - off[g] >= pp]
    own, own_g = {}, {}
    for pen in lc.ALL_PENS:  # on the CPU first: the oracle's f32 arithmetic on the same stored values
        ob = _f32_oracle(X32, y32, bias, pen)
        assert ob.dtype == np.float32
        own[pen] = lc.kkt_of(Xw, yw, bias, pen, ob.astype(np.float64))
        own_g[pen] = [lc.kkt_of(Xgw[off[g]:off[g + 1]], ygw[off[g]:off[g + 1]], bias, pen,
                                _f32_oracle(Xg32[off[g]:off[g + 1]], yg32[off[g]:off[g + 1]], bias, pen).astype(np.float64)) for g in fitted]
        print(f"f32 p={p} bias={bias} {pen}: oracle f32 kkt {own[pen]:.2e}; grouped {min(own_g[pen]):.2e} .. {max(own_g[pen]):.2e}")
    pds.config.LIN_REG_EXPR_F64 = False
    try:
        for pen in lc.ALL_PENS:
            got = fit(pds, X32, y32, bias, pen, tol=lc.TOL_F32)
            k = lc.kkt_of(Xw, yw, bias, pen, got.astype(np.float64))
            print(f"f32 p={p} bias={bias} {pen}: device kkt {k:.2e}")
            measured("g f32", k, own[pen])
            assert k <= 10.0 * own[pen], (pen, k, own[pen])
            co, nu = fit_by(pds, Xg32, yg32, off, bias, pen, tol=lc.TOL_F32)
            assert co.dtype == np.float32 and np.array_equal(nu, np.diff(off) < pp)
            for i, g in enumerate(fitted):
                k = lc.kkt_of(Xgw[off[g]:off[g + 1]], ygw[off[g]:off[g + 1]], bias, pen, co[g].astype(np.float64))
                measured("g f32 grouped", k, own_g[pen][i])
                assert k <= 10.0 * own_g[pen][i], (pen, g, k, own_g[pen][i])
    finally:
        pds.config.LIN_REG_EXPR_F64 = True


# ---- h. determinism
def test_two_calls_give_the_same_bits(pds):
    X, y, _ = lc.frame(65)
    Xg, yg, off = lc.grouped_frame(65, True)
    for pen in ("enet", "lasso+", "nnls"):
        for bias in (True, False):
            assert np.array_equal(fit(pds, X, y, bias, pen), fit(pds, X, y, bias, pen))
        a, b = fit_by(pds, Xg, yg, off, True, pen), fit_by(pds, Xg, yg, off, True, pen)
        assert np.array_equal(a[0], b[0], equal_nan=True) and np.array_equal(a[1], b[1])
