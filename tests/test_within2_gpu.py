"""lin_reg / lin_reg_report(absorb=[k1, k2]) on the MI355X against the NumPy restatement (within2_reference.py): the truth is its long
double run with the tolerance at the long double rounding floor.

Frames (within2_cases.py): seeded, every one with a level of about 50 x the within spread on BOTH factors.  60 ragged levels of key 1
-- 1, 2, 63, 64, 65, 127, 128, 129, 300 and 1 000 rows plus 50 sizes in 3 .. 200 -- with random codes of key 2 in G2 = 7 and in
G2 = 300, at widths 1, 4, 8, 15 and 16 in f64 and at width 16 in f32; an entry/exit panel of 200 firms x 12 years; three components;
3 levels among 200 singletons; "few movers" (300 x 40, 6 rows each: 971 sweeps at 1e-8).  Each on the default context and on one with
"within_split_rows" = 128 (which cuts the long levels of key 1 and every level of key 2 into chunks of 128 gathered rows), with all
three `std_err` values and the fit-only call, checked in beta, the standard error, t, p, the interval, r2, adj_r2, r2_overall, pred,
resid, df_resid, n_groups, n_groups2 and n_components.

Budgets (the project's standing rule): the device may be at most 10 x as far from the truth as the yardstick run is on that frame
(8 ulp of the frame's format where that distance is below half an ulp); distance = max |a - b| / max |b| per field.
  absorb_tol = 1e-13: rounding dominates; the yardstick is the reference in the frame's format run to its own criterion (float32
    arithmetic cannot reach a delta of 1e-13 and runs the float64 run's number of sweeps).
  absorb_tol = 1e-8 (the default): truncation dominates; the yardstick is the reference's float64 run stopped ONE SWEEP EARLIER than its
    own criterion, a run legitimately one sweep short.
  The device's n_iter is within +-1 of the float64 reference's.  As a condition on the INPUTS the tests assert on the CPU that the
  reference's delta at its stopping sweep is at most half the tolerance (the seeds are chosen for it).  Not on the few-movers frame:
  its delta falls by 2 % a sweep, so every delta near the stop is within a factor 2 of the tolerance whatever the seed.
The yardstick's distances are measured on the CPU inside the tests, before anything on the device is asserted, and printed.  p-values
and the interval get what the budgets of t, beta and the standard error let through plus 1e-10 for the special functions.

Measured on the MI355X (worst over widths, the three estimators and both split settings; the yardstick's distance from the truth
beside it; "sweeps": the device's / the float64 reference's n_iter, equal in every case):
                                    beta     std_err  t        r2       adj_r2   r2_overall pred     resid    sweeps
  ragged, G2 = 7     1e-13 device     8.7e-16  1.1e-15  2.9e-15  1.7e-14  1.2e-14  5.3e-17    1.9e-16  5.5e-15  8 - 9
                           yardstick  2.4e-15  1.0e-15  4.1e-15  8.0e-15  1.2e-14  5.3e-17    4.2e-15  2.2e-13
                     1e-8  device     9.2e-16  7.7e-11  1.3e-10  8.0e-15  6.5e-15  5.3e-17    6.4e-12  3.0e-10  6
                           yardstick  3.0e-13  4.9e-09  8.4e-09  1.1e-13  1.1e-13  5.3e-17    6.9e-09  3.3e-07
  ragged, G2 = 300   1e-13 device     8.6e-16  5.6e-15  1.3e-14  4.6e-16  4.2e-16  5.0e-17    4.2e-16  2.6e-14  13 - 14
                           yardstick  2.0e-15  6.0e-15  1.1e-14  3.0e-16  3.4e-16  5.0e-17    2.0e-15  2.3e-13
                     1e-8  device     9.6e-16  4.0e-10  6.5e-10  6.5e-16  6.9e-16  5.0e-17    4.9e-11  4.2e-09  8 - 9
                           yardstick  2.9e-14  4.9e-09  8.4e-09  1.1e-14  1.1e-14  5.0e-17    7.3e-09  6.3e-07
  ragged f32, G2 = 7 1e-13 device     2.6e-08  5.0e-08  3.8e-08  1.5e-08  1.9e-08  2.6e-17    5.1e-08  3.8e-08  9
                           yardstick  1.3e-06  1.0e-06  1.5e-06  1.2e-07  8.5e-08  2.2e-08    5.5e-08  1.3e-06
                     1e-8  device     2.6e-08  5.0e-08  3.8e-08  1.5e-08  1.9e-08  2.6e-17    5.1e-08  3.8e-08  6
                           yardstick  3.0e-13  4.9e-09  8.4e-09  1.1e-13  1.1e-13  2.6e-17    6.9e-09  3.3e-07
  ragged f32, 300    1e-13 device     3.3e-08  4.8e-08  4.1e-08  1.4e-09  1.6e-08  1.9e-17    3.9e-08  3.4e-08  14
                           yardstick  6.7e-07  4.6e-07  1.8e-06  1.4e-09  1.1e-07  1.2e-08    6.1e-08  2.4e-06
                     1e-8  device     3.3e-08  4.8e-08  4.1e-08  1.4e-09  1.6e-08  1.9e-17    3.9e-08  3.4e-08  9
                           yardstick  6.6e-15  2.3e-09  8.4e-09  7.9e-15  8.2e-15  1.9e-17    1.6e-09  9.1e-08
  panel 200 x 12     1e-13 device     4.3e-16  5.5e-14  3.5e-14  1.2e-15  1.6e-15  4.6e-17    3.7e-16  1.8e-14  16 - 17
                           yardstick  5.6e-16  5.5e-14  3.6e-14  4.2e-16  6.2e-16  4.6e-17    9.4e-16  5.1e-14
                     1e-8  device     7.9e-16  8.6e-09  5.5e-09  4.2e-16  4.7e-16  4.6e-17    4.0e-11  2.1e-09  10 - 11
                           yardstick  4.7e-14  6.3e-08  4.0e-08  1.3e-13  1.3e-13  4.6e-17    7.6e-10  5.7e-08
  three components   1e-13 device     1.9e-16  4.0e-14  5.7e-14  1.1e-15  1.1e-15  4.8e-17    1.2e-15  4.6e-14  14
                           yardstick  5.0e-16  4.1e-14  5.8e-14  2.7e-16  2.7e-16  4.8e-17    4.2e-15  1.7e-13
                     1e-8  device     3.2e-16  5.3e-09  7.5e-09  1.0e-15  1.1e-15  4.8e-17    1.5e-10  6.1e-09  9
                           yardstick  1.9e-13  5.6e-08  7.9e-08  1.9e-13  1.9e-13  6.3e-17    5.8e-09  2.3e-07
  3 + 200 singletons 1e-13 device     9.8e-16  4.1e-14  8.5e-14  1.3e-16  2.4e-16  5.1e-17    1.5e-15  1.1e-13  17 - 18
                           yardstick  7.2e-16  3.9e-14  8.6e-14  7.2e-17  2.4e-16  5.1e-17    7.6e-15  5.7e-13
                     1e-8  device     7.5e-16  2.3e-09  4.6e-09  3.8e-16  5.8e-16  5.1e-17    8.6e-11  6.4e-09  11 - 12
                           yardstick  4.1e-14  1.4e-08  2.8e-08  1.7e-14  1.7e-14  5.1e-17    2.6e-09  2.0e-07
  few movers, "se"   1e-8  device     2.8e-12  1.6e-12  4.5e-12  7.4e-12  7.4e-12  1.2e-16    1.4e-08  7.8e-07  971
                           yardstick  3.0e-12  1.7e-12  4.7e-12  7.7e-12  7.8e-12  1.2e-16    1.5e-08  8.3e-07
  (the worst rows are per column, not per case: every case passed its own frame's budget; a distance below half an ulp has the
  8-ulp budget.  The standard errors at 1e-8 are those of the clustered forms: the meat is the most sensitive to what the sweeps
  leave.)  Device against device, p = 3, G1 = 12, G2 = 3, against lin_reg_report on the 3 features + 13 dummies + bias: beta 1.7e-12
  (bar 2.3e-11: the dummy design carries the levels), classical errors 6.5e-13 (5.4e-12), CR0 1.5e-12 (4.1e-12).
  The first run missed one check, mended in the test's own arithmetic: a p-value below the format's smallest normal number (SciPy's
  0.0 against the library's 8.9e-316 at t = 39) has no relative accuracy in either tail function, so the bound's absolute term is
  that number, not one subnormal step.
"""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT))

import within2_cases as c2  # noqa: E402
import within2_reference as w2r  # noqa: E402

pytestmark = pytest.mark.gpu

SE_NAME = {"se": "std_err", "cluster": "cluster_se", "cluster0": "cluster0_se"}
QUANTILE_TOL = 1e-10  # (tests/test_within_gpu.py: the library's Student t quantile and tail against SciPy's)
TAIL_TOL = 1e-10
FIELDS = w2r.FIELDS + w2r.ROW_FIELDS


@pytest.fixture(scope="module")
def pds():
    import polars_ds_extension_amd as pds

    return pds


@pytest.fixture(scope="module")
def contexts(pds):
    """the default context, and one whose split threshold cuts every level above 128 rows"""
    ctxs = {"whole": pds.default_context(), "cut": pds.Context(0)}
    ctxs["cut"].set_option("within_split_rows", 128)
    yield ctxs
    ctxs["cut"].close()


def _run(pds, F, y, k1, k2, se, ctx=None, f32=False, tol=1e-8, **kw):
    kw.setdefault("return_pred", True)
    pds.config.LIN_REG_EXPR_F64 = not f32
    try:
        return pds.lin_reg_report(*c2.columns(F), target=y, absorb=[k1, k2], std_err=se, absorb_tol=tol, ctx=ctx, **kw)
    finally:
        pds.config.LIN_REG_EXPR_F64 = True


def _inputs_ok(kind, p, tol_name):
    """the condition on the inputs: the float64 reference does not stop within a factor 2 of the tolerance"""
    own = c2.ref(kind, p, "se", "float64", tol_name)
    assert own["deltas"][-1] <= 0.5 * c2.TOLS[tol_name], (kind, p, tol_name, own["deltas"][-2:])


def _check(got, kind, p, se, tol_name, what, fmt="float64"):
    """every field of a device report against the truth within the budget of its frame and tolerance"""
    from scipy import stats as st

    assert np.finfo(np.longdouble).eps < 1e-18  # the reference has to be wider than the arithmetic under test
    sp = c2.spread(kind, p, se, fmt, tol_name)  # measured first, on the CPU
    want = c2.truth(kind, p, se)
    own = c2.ref(kind, p, se, "float64", tol_name)
    dt = c2.DTYPES[fmt]
    eps = float(np.finfo(dt).eps)
    for k in ("n_groups", "n_groups2", "n_components", "df_resid"):
        assert got[k] == want[k], (k, got[k], want[k])
    assert abs(got["n_iter"] - own["n_iter"]) <= 1, (got["n_iter"], own["n_iter"])
    assert SE_NAME[se] in got and (se == "se" or "std_err" not in got)
    vals = {"beta": got["beta"], "std_err": got[SE_NAME[se]], "t": got["t"], "r2": got["r2"][0], "adj_r2": got["adj_r2"][0],
            "r2_overall": got["r2_overall"], "pred": got["pred"], "resid": got["resid"]}
    assert got["beta"].dtype == dt and np.asarray(got["pred"]).dtype == dt
    dist = {k: w2r.rel(vals[k], want[k]) for k in FIELDS}
    print(f"{what} {kind} p={p} {se} {fmt} tol={tol_name}: sweeps {got['n_iter']} (reference {own['n_iter']}); device vs truth "
          f"{ {k: f'{v:.1e}' for k, v in dist.items()} }; yardstick vs truth { {k: f'{v:.1e}' for k, v in sp.items()} }")
    bud = {k: w2r.budget(sp[k], dt) for k in FIELDS}
    for k in FIELDS:
        assert dist[k] <= bud[k], (k, dist[k], sp[k])
    t_o = np.asarray(want["t"], dtype=np.float64)
    dof = want["t_dof"]
    dt_bound = bud["t"] * np.max(np.abs(t_o))
    p_o = want["p"]
    # (below the format's smallest NORMAL number a p-value has lost its relative accuracy in either tail function -- SciPy's 0.0 against
    # the library's 8.9e-316 at t = 39 with 6 249 degrees of freedom -- so the absolute term is that number, not one subnormal step)
    dp_bound = 2.0 * st.t.pdf(np.maximum(np.abs(t_o) - dt_bound, 0.0), dof) * dt_bound + (TAIL_TOL + eps) * p_o + float(np.finfo(dt).tiny)
    assert np.all(np.abs(np.asarray(got["p>|t|"], dtype=np.float64) - p_o) <= dp_bound), (np.asarray(got["p>|t|"]) - p_o, dp_bound)
    b_o, s_o = np.asarray(want["beta"], dtype=np.float64), np.asarray(want["std_err"], dtype=np.float64)
    ci_bound = bud["beta"] * np.max(np.abs(b_o)) + want["t_crit"] * (bud["std_err"] + QUANTILE_TOL) * np.max(s_o) + eps * np.max(np.abs(want["ci_hi"]))
    assert np.all(np.abs(np.asarray(got["0.025"], dtype=np.float64) - want["ci_lo"]) <= ci_bound)
    assert np.all(np.abs(np.asarray(got["0.975"], dtype=np.float64) - want["ci_hi"]) <= ci_bound)
    return dist


def _check_fit_only(pds, F, y, k1, k2, full, ctx, tol, f32=False):
    """lin_reg(absorb=[k1, k2]): the pass without the scores gives the report's beta, pred and resid, bit for bit"""
    pds.config.LIN_REG_EXPR_F64 = not f32
    try:
        beta = pds.lin_reg(*c2.columns(F), target=y, absorb=[k1, k2], absorb_tol=tol, ctx=ctx)
        b2, pred, resid = pds.lin_reg(*c2.columns(F), target=y, absorb=[k1, k2], absorb_tol=tol, return_pred=True, ctx=ctx)
    finally:
        pds.config.LIN_REG_EXPR_F64 = True
    assert np.array_equal(beta, full["beta"]) and np.array_equal(b2, beta)
    assert np.array_equal(pred, full["pred"]) and np.array_equal(resid, full["resid"])


def _same_bits(a, b, skip=()):
    assert a.keys() == b.keys()
    for k in a:
        if k in skip:
            continue
        if k in ("features", "n_groups", "n_groups2", "n_components", "n_iter", "df_resid", "r2_overall"):
            assert a[k] == b[k], k
        else:
            x, y = (v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v) for v in (a[k], b[k]))
            assert np.array_equal(x, y, equal_nan=True), k


def _all_ways(pds, contexts, kind, p, fmt="float64"):
    f32 = fmt == "float32"
    F, y, off, k1, k2 = c2.frame(kind, p)
    for tol_name in ("default", "tight"):
        _inputs_ok(kind, p, tol_name)
    for split in ("whole", "cut"):
        for tol_name in ("default", "tight"):
            tol = c2.TOLS[tol_name]
            for se in w2r.SE_TYPES:
                got = _run(pds, F, y, k1, k2, se, ctx=contexts[split], f32=f32, tol=tol)
                _check(got, kind, p, se, tol_name, split, fmt)
            _check_fit_only(pds, F, y, k1, k2, got, contexts[split], tol, f32)


# ---- 1. ragged levels of key 1, few and many levels of key 2
@pytest.mark.parametrize("g2", [7, 300])
@pytest.mark.parametrize("p", c2.WIDTHS)
def test_ragged(pds, contexts, p, g2):
    kind = f"ragged{g2}"
    w = c2.truth(kind, p, "cluster")
    ratio = np.asarray(w["se_all"]["cluster"] / w["se_all"]["se"], dtype=np.float64)
    assert np.max(np.abs(ratio - 1.0)) > 0.1  # the estimator matters on this frame
    _all_ways(pds, contexts, kind, p)


@pytest.mark.parametrize("g2", [7, 300])
def test_ragged_f32(pds, contexts, g2):
    _all_ways(pds, contexts, f"ragged{g2}_32", 16, "float32")


# ---- 2. the entry/exit panel, three components, singletons
@pytest.mark.parametrize("p", [4, 16])
def test_panel(pds, contexts, p):
    _all_ways(pds, contexts, "panel", p)


def test_three_components(pds, contexts):
    assert c2.truth("blocks", 4, "se")["n_components"] == 3
    _all_ways(pds, contexts, "blocks", 4)


@pytest.mark.parametrize("p", [1, 8])
def test_singletons(pds, contexts, p):
    F, y, off, k1, k2 = c2.frame("singletons", p)
    assert int((np.diff(off) == 1).sum()) == 200
    _all_ways(pds, contexts, "singletons", p)


# ---- 3. slow convergence, and the sweep limit
def test_few_movers(pds):
    F, y, off, k1, k2 = c2.frame("movers", 4)
    own = c2.ref("movers", 4, "se", "float64", "default")
    assert own["n_iter"] > 500  # slow by construction
    got = _run(pds, F, y, k1, k2, "se")
    _check(got, "movers", 4, "se", "default", "whole")


def test_sweep_limit(pds):
    from polars_ds_extension_amd._lib import PdsError

    F, y, off, k1, k2 = c2.frame("movers", 4)
    with pytest.raises(PdsError, match=r"did not converge in 50 sweeps \(last delta = \d\.\d+e-\d+") as e:
        _run(pds, F, y, k1, k2, "se", absorb_max_iter=50)
    assert e.value.code == -6  # PDS_ERR_NUMERIC
    assert _run(pds, F, y, k1, k2, "se", tol=1e-2, absorb_max_iter=50)["n_iter"] <= 50  # the context is usable, the limit is a limit


# ---- 4. collinearity with the second key
def test_function_of_key2_is_refused(pds):
    from polars_ds_extension_amd._lib import PdsError

    F, y, off, k1, k2 = c2.frame("ragged7", 4)
    cols = c2.columns(F)
    level2 = np.cos(np.asarray(k2, dtype=np.float64)) * 3.0 + 1.0  # a function of key 2 alone: varies inside every level of key 1
    with pytest.raises(PdsError, match="feature column 2 is a function of the absorbed keys") as e:
        pds.lin_reg_report(cols[0], cols[1], level2, cols[2], target=y, absorb=[k1, k2])
    assert e.value.code == -6
    both = level2 + np.asarray(k1, dtype=np.float64)  # ... and a sum of functions of the two keys
    with pytest.raises(PdsError, match="feature column 0 is a function of the absorbed keys"):
        pds.lin_reg_report(both, cols[1], target=y, absorb=[k1, k2])
    assert pds.lin_reg_report(*cols, target=y, absorb=[k1, k2])["n_groups2"] == 7


# ---- 5. the C ABI's offsets form; by key on a shuffled frame; two calls; host and device frames
def _grouped_raw(pds, ctx, F, y, off, codes2, n_levels2, se, tol=1e-8, max_iter=10_000):
    from polars_ds_extension_amd import _lib
    from polars_ds_extension_amd.lstsq import _Cols

    cols = c2.columns(F)
    n, p = len(y), len(cols)
    cs = _Cols(np.ascontiguousarray(y), cols)
    outs = {k: np.empty(p) for k in ("beta", "std_err", "t", "p", "ci_lower", "ci_upper")}
    rep = _lib.ReportF64(*[C.c_void_p(o.ctypes.data) for o in outs.values()], 0.0, 0.0)
    pred, resid = np.empty(n), np.empty(n)
    extra = _lib.Within2Out(C.c_void_p(pred.ctypes.data), C.c_void_p(resid.ctypes.data), 0.0, 0, 0, 0, 0, 0)
    off = np.ascontiguousarray(off, dtype=np.int64)
    codes2 = np.ascontiguousarray(codes2, dtype=np.int32)
    rc = ctx._lib.pds_lin_reg_within2_grouped_f64(ctx._h, cs.cols, p, C.c_int64(n), C.c_void_p(off.ctypes.data), C.c_int64(len(off) - 1),
                                                  C.c_void_p(codes2.ctypes.data), C.c_int64(n_levels2), cs.space, _lib.WITHIN_SE_TYPES[se],
                                                  C.c_double(tol), max_iter, C.byref(rep), C.byref(extra))
    out = dict(outs, pred=pred, resid=resid, r2=rep.r2, adj_r2=rep.adj_r2, r2_overall=extra.r2_overall, df_resid=extra.df_resid,
               n_groups=extra.n_groups_used, n_groups2=extra.n_groups2_used, n_components=extra.n_components, n_iter=extra.n_iter)
    return rc, out


def _assert_raw_equals(raw, rep, se, row_map=None):
    for a, b in (("beta", "beta"), ("std_err", SE_NAME[se]), ("t", "t"), ("p", "p>|t|"), ("ci_lower", "0.025"), ("ci_upper", "0.975")):
        assert np.array_equal(raw[a], rep[b]), a
    assert raw["r2"] == rep["r2"][0] and raw["adj_r2"] == rep["adj_r2"][0]
    for k in ("r2_overall", "df_resid", "n_groups", "n_groups2", "n_components", "n_iter"):
        assert raw[k] == rep[k], k
    for k in ("pred", "resid"):
        assert np.array_equal(raw[k] if row_map is None else raw[k][row_map], rep[k]), k


@pytest.mark.parametrize("p", [4, 16])
def test_forms_agree(pds, contexts, p):
    import torch

    F, y, off, k1, k2 = c2.frame("ragged300", p)
    F, y = np.asarray(F), np.asarray(y)
    keys1, keys2 = k1 * 7 - 200, k2 * 3 - 50  # negative, sparse
    n = len(y)
    n2 = len(np.unique(k2))
    for split in ("whole", "cut"):
        ctx = contexts[split]
        for se in ("se", "cluster"):
            ordered = pds.lin_reg_report(*c2.columns(F), target=y, std_err=se, absorb=[keys1, keys2], return_pred=True, ctx=ctx)
            _same_bits(pds.lin_reg_report(*c2.columns(F), target=y, std_err=se, absorb=[keys1, keys2], return_pred=True, ctx=ctx), ordered)  # two calls
            _check(ordered, "ragged300", p, se, "default", "sparse keys " + split)
            codes2 = np.unique(keys2, return_inverse=True)[1]
            rc, raw = _grouped_raw(pds, ctx, F, y, off, codes2, n2, se)  # ordered keys move nothing: the bits of the offsets form
            assert rc == 0
            _assert_raw_equals(raw, ordered, se)
            rc, spare = _grouped_raw(pds, ctx, F, y, off, codes2 * 2 + 1, 2 * n2 + 3, se)  # unused codes count nowhere
            assert rc == 0 and spare["n_groups2"] == n2
            _assert_raw_equals(spare, ordered, se)
            # rows shuffled: the stable sort + gather brings them into the order of key 1; per-row outputs come back where the rows are
            perm = np.random.default_rng(5).permutation(n)
            order = perm[np.argsort(keys1[perm], kind="stable")]
            shuffled = pds.lin_reg_report(*c2.columns(F[perm]), target=y[perm], std_err=se, absorb=[keys1[perm], keys2[perm]], return_pred=True, ctx=ctx)
            rc, on_ordered = _grouped_raw(pds, ctx, F[order], y[order], off, codes2[order], n2, se)
            assert rc == 0
            inv = np.empty(n, dtype=np.int64)
            inv[np.argsort(keys1[perm], kind="stable")] = np.arange(n)  # row i of the shuffled frame is row inv[i] of the ordered one
            _assert_raw_equals(on_ordered, shuffled, se, row_map=inv)
            # CUDA tensors give the bits of the host frame
            dev = torch.device("cuda", 0)
            tc = [torch.from_numpy(np.array(c)).to(dev) for c in c2.columns(F[perm])]
            t_key = pds.lin_reg_report(*tc, target=torch.from_numpy(y[perm]).to(dev), std_err=se, return_pred=True, ctx=ctx,
                                       absorb=[torch.from_numpy(keys1[perm]).to(dev), torch.from_numpy(keys2[perm]).to(dev)])
            assert t_key["pred"].is_cuda
            _same_bits(t_key, shuffled)
        beta, pred, resid = pds.lin_reg(*c2.columns(F[perm]), target=y[perm], absorb=[keys1[perm], keys2[perm]], return_pred=True, ctx=ctx)
        assert np.array_equal(beta, shuffled["beta"]) and np.array_equal(pred, shuffled["pred"]) and np.array_equal(resid, shuffled["resid"])


def test_c_abi_refusals(pds):
    F, y, off, k1, k2 = c2.frame("ragged7", 4)
    ctx = pds.default_context()
    bad = np.array(k2)
    bad[17] = 7
    for codes, tol, it, want in ((bad, 1e-8, 100, -1), (-np.asarray(k2) - 1, 1e-8, 100, -1), (k2, 0.0, 100, -1), (k2, -1.0, 100, -1),
                                 (k2, float("nan"), 100, -1), (k2, 1e-8, 0, -1)):
        rc, _ = _grouped_raw(pds, ctx, F, y, off, codes, 7, "se", tol, it)
        assert rc == want, (tol, it, rc)
    rc, ok = _grouped_raw(pds, ctx, F, y, off, k2, 7, "se")
    assert rc == 0 and ok["n_groups2"] == 7 and ok["n_components"] == 1


def test_names_and_fields(pds):
    from polars_ds_extension_amd._lib import PdsError

    F, y, off, k1, k2 = c2.frame("ragged7", 4)
    a = pds.lin_reg_report(*c2.columns(F), target=y, absorb=(k1, k2), std_err="cluster0", feature_names=list("abcd"))
    assert list(a) == ["features", "beta", "cluster0_se", "t", "p>|t|", "0.025", "0.975", "r2", "adj_r2", "r2_overall", "n_groups", "df_resid",
                       "n_groups2", "n_components", "n_iter"]
    assert a["n_groups"] == 60 and a["df_resid"] == 59 and a["n_groups2"] == 7 and a["n_components"] == 1
    b = pds.lin_reg_report(*c2.columns(F), target=y, absorb=[k1, k2])
    assert b["df_resid"] == len(y) - 4 - (60 + 7 - 1) and "pred" not in b
    with pytest.raises(PdsError, match="HC0 - HC3") as e:
        pds.lin_reg_report(*c2.columns(F), target=y, absorb=[k1, k2], std_err="hc1")
    assert e.value.code == -5
    one = pds.lin_reg_report(*c2.columns(F), target=y, absorb=k1)  # one key is another model
    assert "n_groups2" not in one and w2r.rel(one["beta"], b["beta"]) > 1e-3


# ---- 6. device against device: the dummy-variable regression
def test_against_dummy_columns(pds):
    """p = 3, G1 = 12, G2 = 3: the two-key fit against lin_reg_report on the 3 features + 11 + 2 dummies + bias (16 columns, the most
    lin_reg_report takes).  beta and the classical standard errors of the features, and CR0 against std_err="cluster0" clustered on
    key 1.  Bar: the SUM of the two calls' own budgets on that frame at absorb_tol = 1e-13 -- 10 x what the two-key reference, and
    10 x what the plain regression on that dummy design, lose in float64 against long double (8 ulp where below half an ulp)."""
    import within_reference as wr

    F, y, off, k1, k2 = c2.frame("small3", 3)
    F, y = np.asarray(F), np.asarray(y)
    assert c2.truth("small3", 3, "se")["n_components"] == 1
    D = np.column_stack([(k1[:, None] == np.arange(1, 12)[None, :]), (k2[:, None] == np.arange(1, 3)[None, :])]).astype(np.float64)
    Z = np.column_stack([F, D])
    Zb = np.column_stack([Z, np.ones(len(y))])
    plain = {dt: wr.plain_report(Zb, y, k1, c2.DTYPES[dt]) for dt in ("float64", "longdouble")}
    sp_plain = {k: wr.rel(plain["float64"][k][:3], plain["longdouble"][k][:3]) for k in ("beta", "se", "cluster0")}
    for se, other_name, key in (("se", "std_err", "se"), ("cluster0", "cluster0_se", "cluster0")):
        sp_two = c2.spread("small3", 3, se, "float64", "tight")
        a = _run(pds, F, y, k1, k2, se, tol=1e-13)
        kw = {"cluster": k1} if se == "cluster0" else {}
        b = pds.lin_reg_report(*c2.columns(Z), target=y, add_bias=True, std_err=se, **kw)
        d = {"beta": wr.rel(a["beta"], b["beta"][:3]), "std_err": wr.rel(a[SE_NAME[se]], b[other_name][:3])}
        bar = {"beta": wr.budget(sp_two["beta"]) + wr.budget(sp_plain["beta"]), "std_err": wr.budget(sp_two["std_err"]) + wr.budget(sp_plain[key])}
        print(f"absorb=[k1, k2] vs 13 dummies + bias, {se}: {d}; bars {bar} from two-key {sp_two['beta']:.2e} / {sp_two['std_err']:.2e}, plain {sp_plain}")
        for k in d:
            assert d[k] <= bar[k], (se, k, d[k], bar[k])
