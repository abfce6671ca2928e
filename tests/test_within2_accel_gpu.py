"""The accelerated (Irons-Tuck) iteration of lin_reg / lin_reg_report / fixed_effects(absorb=[k1, k2], absorb_accel="irons_tuck") on the
MI355X against its NumPy restatement in the device's table arithmetic (within2_accel_reference.py).  The truth is the long double
PLAIN run with the tolerance at the long double rounding floor (within2_reference.py / within2_effects_reference.py).

Frames (within2_accel_cases.py; its seeds are chosen for the accelerated run): few movers p 4 (1 800 rows), the entry/exit panel p 4 and
p 16, 60 ragged levels x 300 codes p 16 in f64 and in f32, three components p 4 (the components share one c_j per column), 3 levels among
200 singletons p 1, ONE occupied level of factor 2, the balanced panel (converged at sweep 2: no extrapolation), unused codes of factor 2
between the used ones (the C ABI's offsets form), and "many2": 30 000 rows with 4 986 occupied codes of factor 2.  The level kernel
starts min(occupied codes, 16 waves x 256 compute units = 4 096) one-wave workgroups and writes one record of the two dot products per
workgroup: from 2 occupied codes on the sums span more than one record and more than one workgroup, and above 4 096 occupied codes a
wave walks more than one level (890 waves walk two levels here), so both the per-wave accumulation and the 4 096-record sum are
exercised.  Each on the default context and on one with "within_split_rows" = 128.

Sweep count: the device's n_iter EQUALS the float64 restatement's on every seeded frame at 1e-8 and 1e-13 (the seeds' condition --
the restatement's delta at its stopping sweep is at most half the tolerance -- is asserted first, on the CPU).  Few movers: within 2
(one cycle) of the restatement's, and at most one fifth of the device's own plain count in the same test.
Accuracy: every report field, pred / resid and the effects may be at most 10 x as far from the truth as the float64 RESTATEMENT run
for the number of sweeps the device took (8 ulp of the frame's format where that distance is below half an ulp); distance =
max |a - b| / max |b| per field.  The yardstick is measured on the CPU and printed before the device is asserted.  p-values and the
interval get what the budgets of t, beta and the standard error let through plus 1e-10 for the special functions.

Measured on the MI355X (worst over "se" / "cluster" and both split settings; "restatement": the float64 restatement run for the
device's number of sweeps, its distance from the truth; "sweeps": the device's n_iter, equal to the restatement's own on every seeded
frame; few movers: 87 = the restatement's at 1e-8, 160 against 159 at 1e-13, against 971 and 1 768 plain sweeps on the device):
                                             beta     std_err  t        r2       adj_r2   r2_over  pred     resid    effects  effects2 sweeps
  panel, p 4              1e-8  device       4.9e-16  4.3e-09  1.5e-09  1.6e-16  7.1e-17  3.6e-17  6.7e-12  3.8e-10  1.7e-11  3.7e-11  8
                                restatement  1.1e-15  4.3e-09  1.5e-09  1.3e-16  2.2e-16  3.6e-17  1.7e-11  9.7e-10  1.7e-11  3.7e-11
  panel, p 4              1e-13 device       5.3e-16  1.4e-14  5.4e-15  4.4e-16  3.6e-16  3.6e-17  2.4e-16  1.3e-14  8.4e-16  1.2e-15  12
                                restatement  5.3e-16  1.4e-14  5.9e-15  1.6e-16  7.1e-17  3.6e-17  5.8e-16  3.2e-14  9.8e-16  9.8e-16
  panel, p 16             1e-8  device       5.5e-16  9.4e-10  4.0e-10  5.5e-16  5.0e-16  3.4e-17  6.0e-11  3.3e-09  9.3e-11  3.7e-10  9
                                restatement  7.4e-16  9.4e-10  4.0e-10  1.9e-16  1.2e-16  3.4e-17  1.6e-10  8.8e-09  9.3e-11  3.7e-10
  panel, p 16             1e-13 device       6.8e-16  2.8e-14  1.4e-14  5.6e-16  8.8e-16  3.4e-17  1.9e-15  1.1e-13  3.1e-15  1.2e-14  13
                                restatement  1.2e-15  2.8e-14  1.3e-14  1.9e-16  1.2e-16  3.4e-17  5.0e-15  2.8e-13  2.9e-15  1.2e-14
  ragged300, p 16         1e-8  device       1.5e-15  2.1e-10  3.4e-10  1.0e-15  1.1e-15  9.2e-18  1.7e-11  1.0e-09  1.3e-11  3.2e-11  8
                                restatement  7.9e-16  2.1e-10  3.4e-10  4.4e-16  3.6e-16  9.2e-18  7.3e-11  4.5e-09  1.3e-11  3.2e-11
  ragged300, p 16         1e-13 device       6.4e-16  4.2e-15  7.1e-15  1.0e-15  1.1e-15  9.2e-18  4.4e-16  2.6e-14  6.7e-16  8.2e-16  11
                                restatement  1.0e-15  4.3e-15  5.9e-15  4.4e-16  3.6e-16  9.2e-18  3.4e-15  2.1e-13  8.3e-16  1.5e-15
  ragged300 f32, p 16     1e-8  device       2.5e-08  4.7e-08  3.8e-08  2.2e-08  5.1e-10  5.4e-18  4.6e-08  4.5e-08  3.8e-08  4.4e-08  8
                                restatement  1.5e-15  2.1e-10  3.4e-10  8.2e-17  2.7e-16  5.4e-18  7.3e-11  4.5e-09  1.3e-11  3.2e-11
  ragged300 f32, p 16     1e-13 device       2.5e-08  4.7e-08  3.8e-08  2.2e-08  5.1e-10  5.4e-18  4.6e-08  4.5e-08  3.8e-08  4.4e-08  11
                                restatement  1.7e-15  4.6e-15  8.2e-15  8.2e-17  2.7e-16  5.4e-18  3.4e-15  2.1e-13  1.1e-15  1.6e-15
  three components, p 4   1e-8  device       5.7e-16  5.0e-09  7.0e-09  2.7e-16  2.7e-16  4.8e-17  1.3e-10  5.3e-09  2.2e-10  4.4e-10  7
                                restatement  2.0e-15  5.0e-09  7.0e-09  2.0e-15  2.0e-15  4.8e-17  4.7e-10  1.9e-08  2.2e-10  4.4e-10
  three components, p 4   1e-13 device       1.4e-16  4.9e-15  7.0e-15  7.0e-16  7.0e-16  4.8e-17  1.5e-16  4.9e-15  2.2e-16  3.2e-16  11
                                restatement  3.6e-16  5.4e-15  7.8e-15  5.9e-16  6.1e-16  4.8e-17  4.1e-16  1.6e-14  3.9e-16  4.8e-16
  singletons, p 1         1e-8  device       9.6e-16  2.0e-09  2.0e-09  8.3e-17  3.8e-17  2.6e-17  1.8e-11  1.3e-09  3.6e-11  1.4e-10  7
                                restatement  2.1e-17  2.0e-09  2.0e-09  8.3e-17  3.8e-17  2.6e-17  1.1e-10  8.0e-09  3.6e-11  1.4e-10
  singletons, p 1         1e-13 device       4.9e-16  4.7e-14  4.7e-14  1.4e-16  1.9e-16  2.6e-17  1.7e-15  1.2e-13  3.3e-15  1.2e-14  10
                                restatement  4.5e-16  4.6e-14  4.7e-14  1.4e-16  3.8e-17  2.6e-17  1.1e-14  7.7e-13  2.9e-15  1.1e-14
  one level of key 2, p 2 1e-8  device       3.8e-17  3.8e-16  4.2e-16  9.7e-16  1.0e-15  5.7e-18  8.1e-17  1.8e-16  8.4e-17  0 exact  1
                                restatement  9.0e-16  3.8e-16  1.3e-15  2.4e-16  2.0e-16  5.7e-18  3.1e-16  7.1e-15  3.4e-16  0 exact
  one level of key 2, p 2 1e-13 device       3.8e-17  3.8e-16  4.2e-16  9.7e-16  1.0e-15  5.7e-18  8.1e-17  1.8e-16  8.4e-17  0 exact  1
                                restatement  9.0e-16  3.8e-16  1.3e-15  2.4e-16  2.0e-16  5.7e-18  3.1e-16  7.1e-15  3.4e-16  0 exact
  4 986 codes, p 4        1e-8  device       3.0e-16  1.8e-10  1.9e-10  3.7e-16  3.7e-16  3.0e-17  1.0e-10  7.8e-09  2.1e-10  4.1e-10  15
                                restatement  3.0e-15  1.8e-10  1.9e-10  9.4e-17  9.8e-17  3.0e-17  1.6e-10  1.2e-08  2.1e-10  4.1e-10
  4 986 codes, p 4        1e-13 device       3.0e-16  2.4e-15  2.2e-15  9.4e-17  9.8e-17  3.0e-17  1.3e-15  9.3e-14  2.7e-15  4.9e-15  23
                                restatement  3.9e-15  2.3e-15  4.1e-15  3.7e-16  3.7e-16  3.0e-17  1.9e-15  1.4e-13  4.1e-15  5.4e-15
  few movers, p 4         1e-8  device       1.5e-13  7.7e-13  4.0e-14  1.5e-14  1.6e-14  1.4e-17  1.6e-09  8.7e-08  1.1e-08  1.7e-08  87
                                restatement  1.5e-13  7.9e-13  4.1e-14  1.7e-14  1.7e-14  1.4e-17  1.7e-09  9.2e-08  1.1e-08  1.7e-08
  few movers, p 4         1e-13 device       8.7e-17  4.2e-16  9.1e-17  2.6e-16  2.2e-16  1.4e-17  1.5e-14  8.5e-13  1.7e-13  2.6e-13  160
                                restatement  1.4e-16  2.1e-16  3.2e-16  2.6e-16  2.2e-16  1.4e-17  1.5e-14  8.1e-13  1.6e-13  2.4e-13
  (every case passed its own budget; a distance below half an ulp has the 8-ulp budget; the f32 frame's outputs are stored in f32.
  gamma of the one-level frame is exactly 0.0 in the truth, the restatement and on the device.)
"""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT))

import within2_accel_cases as ac  # noqa: E402
import within2_accel_reference as ar  # noqa: E402
import within2_cases as c2  # noqa: E402
import within2_reference as w2r  # noqa: E402

pytestmark = pytest.mark.gpu

SE_NAME = {"se": "std_err", "cluster": "cluster_se", "cluster0": "cluster0_se"}
QUANTILE_TOL = 1e-10  # (tests/test_within_gpu.py: the library's Student t quantile and tail against SciPy's)
TAIL_TOL = 1e-10
FIELDS = w2r.FIELDS + w2r.ROW_FIELDS + ar.EFFECT_FIELDS
SEEDED = (("panel", 4, "float64"), ("panel", 16, "float64"), ("ragged300", 16, "float64"), ("ragged300_32", 16, "float32"), ("blocks", 4, "float64"),
          ("singletons", 1, "float64"), ("one2", 2, "float64"), ("many2", 4, "float64"))
IT = "irons_tuck"


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


def _np(v):
    return v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)


def _fixed(pds, fr, se="se", ctx=None, f32=False, tol=1e-8, accel=IT, **kw):
    F, y, off, k1, k2 = fr
    kw.setdefault("return_pred", True)
    pds.config.LIN_REG_EXPR_F64 = not f32
    try:
        return pds.fixed_effects(*ac.columns(F), target=y, absorb=[k1, k2], std_err=se, absorb_tol=tol, absorb_accel=accel, ctx=ctx, **kw)
    finally:
        pds.config.LIN_REG_EXPR_F64 = True


def _report(pds, fr, se="se", ctx=None, tol=1e-8, accel=IT, **kw):
    F, y, off, k1, k2 = fr
    kw.setdefault("return_pred", True)
    return pds.lin_reg_report(*ac.columns(F), target=y, absorb=[k1, k2], std_err=se, absorb_tol=tol, absorb_accel=accel, ctx=ctx, **kw)


def _same_bits(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], (int, float, list)):
            assert a[k] == b[k], k
        else:
            assert np.array_equal(_np(a[k]), _np(b[k]), equal_nan=True), k


def _inputs_ok(kind, p, tol_name):
    """the condition on the inputs: the float64 restatement's accelerated run does not stop within a factor 2 of the tolerance"""
    own = ac.ref(kind, p, "se", "float64", tol_name)
    assert own["deltas"][-1] <= 0.5 * ac.TOLS[tol_name], (kind, p, tol_name, own["deltas"][-2:])


def _check(got, kind, p, se, tol_name, what, fmt="float64"):
    """every field of a device result against the truth, within 10 x the float64 restatement run for the device's number of sweeps"""
    from scipy import stats as st

    assert np.finfo(np.longdouble).eps < 1e-18  # the reference has to be wider than the arithmetic under test
    yard = ac.ref(kind, p, se, "float64", tol_name, sweeps=got["n_iter"])  # measured first, on the CPU
    want = ac.truth(kind, p, se)
    fields = tuple(k for k in FIELDS if np.any(np.asarray(want[k]) != 0))
    for k in set(FIELDS) - set(fields):  # (gamma of a frame with ONE level of key 2: exactly 0.0 by the normalisation, in every run)
        assert k == "effects2" and not np.any(_np(got[k]) != 0) and not np.any(yard[k] != 0)
    sp = {k: w2r.rel(yard[k], want[k]) for k in fields}
    dt = ac.DTYPES[fmt]
    eps = float(np.finfo(dt).eps)
    for k in ("n_groups", "n_groups2", "n_components", "df_resid"):
        assert got[k] == want[k], (k, got[k], want[k])
    vals = {"beta": got["beta"], "std_err": got[SE_NAME[se]], "t": got["t"], "r2": got["r2"][0], "adj_r2": got["adj_r2"][0],
            "r2_overall": got["r2_overall"], "pred": got["pred"], "resid": got["resid"], "effects": got["effects"], "effects2": got["effects2"]}
    assert got["beta"].dtype == dt and np.asarray(got["pred"]).dtype == dt and got["effects"].dtype == dt
    dist = {k: w2r.rel(vals[k], want[k]) for k in fields}
    print(f"{what} {kind} p={p} {se} {fmt} tol={tol_name}: sweeps {got['n_iter']}; device vs truth "
          f"{ {k: f'{v:.1e}' for k, v in dist.items()} }; restatement vs truth { {k: f'{v:.1e}' for k, v in sp.items()} }")
    bud = {k: w2r.budget(sp[k], dt) for k in fields}
    for k in fields:
        assert dist[k] <= bud[k], (k, dist[k], sp[k])
    t_o = np.asarray(want["t"], dtype=np.float64)
    dof = want["t_dof"]
    dt_bound = bud["t"] * np.max(np.abs(t_o))
    p_o = want["p"]
    dp_bound = 2.0 * st.t.pdf(np.maximum(np.abs(t_o) - dt_bound, 0.0), dof) * dt_bound + (TAIL_TOL + eps) * p_o + float(np.finfo(dt).tiny)
    assert np.all(np.abs(np.asarray(got["p>|t|"], dtype=np.float64) - p_o) <= dp_bound), (np.asarray(got["p>|t|"]) - p_o, dp_bound)
    b_o, s_o = np.asarray(want["beta"], dtype=np.float64), np.asarray(want["std_err"], dtype=np.float64)
    ci_bound = bud["beta"] * np.max(np.abs(b_o)) + want["t_crit"] * (bud["std_err"] + QUANTILE_TOL) * np.max(s_o) + eps * np.max(np.abs(want["ci_hi"]))
    assert np.all(np.abs(np.asarray(got["0.025"], dtype=np.float64) - want["ci_lo"]) <= ci_bound)
    assert np.all(np.abs(np.asarray(got["0.975"], dtype=np.float64) - want["ci_hi"]) <= ci_bound)


# ---- 1. the seeded frames: sweep count equal to the restatement's, accuracy, the three calls agree, two calls give equal bits
@pytest.mark.parametrize("kind,p,fmt", SEEDED)
def test_seeded_frames(pds, contexts, kind, p, fmt):
    f32 = fmt == "float32"
    fr = ac.frame(kind, p)
    for tol_name in ("default", "tight"):
        _inputs_ok(kind, p, tol_name)
    for split in ("whole", "cut"):
        for tol_name in ("default", "tight"):
            tol = ac.TOLS[tol_name]
            own = ac.ref(kind, p, "se", "float64", tol_name)
            for se in ("se", "cluster"):
                got = _fixed(pds, fr, se, contexts[split], f32, tol)
                assert got["n_iter"] == own["n_iter"], (split, tol_name, got["n_iter"], own["n_iter"])
                _check(got, kind, p, se, tol_name, split, fmt)
            _same_bits(_fixed(pds, fr, se, contexts[split], f32, tol), got)  # two calls
            if f32:
                continue
            rep = _report(pds, fr, se, contexts[split], tol)  # the report and the fit-only call: the same bits
            _same_bits({k: got[k] for k in rep}, rep)
            F, y, off, k1, k2 = fr
            beta, pred, resid = pds.lin_reg(*ac.columns(F), target=y, absorb=[k1, k2], absorb_tol=tol, absorb_accel=IT, return_pred=True,
                                            ctx=contexts[split])
            assert np.array_equal(beta, got["beta"]) and np.array_equal(pred, got["pred"]) and np.array_equal(resid, got["resid"])
    if kind == "one2":  # one occupied level: converged at the first sweep
        assert own["n_iter"] == 1
    if kind == "many2":
        assert got["n_groups2"] > 4096  # more occupied codes than the level kernel has waves


# ---- 2. few movers: the point of the feature
def test_few_movers(pds, contexts):
    fr = ac.frame("movers", 4)
    assert ac.seed("movers", 4) == 0
    for split in ("whole", "cut"):
        for tol_name, plain_want in (("default", 971), ("tight", None)):
            tol = ac.TOLS[tol_name]
            own = ac.ref("movers", 4, "se", "float64", tol_name)
            plain = _report(pds, fr, "se", contexts[split], tol, accel="none", return_pred=False)
            got = _fixed(pds, fr, "se", contexts[split], False, tol)
            print(f"{split} movers tol={tol_name}: device sweeps plain {plain['n_iter']}, accelerated {got['n_iter']}; restatement {own['n_iter']}")
            assert plain_want is None or plain["n_iter"] == plain_want
            assert abs(got["n_iter"] - own["n_iter"]) <= 2, (got["n_iter"], own["n_iter"])
            assert 5 * got["n_iter"] <= plain["n_iter"], (got["n_iter"], plain["n_iter"])
            _check(got, "movers", 4, "se", tol_name, split)


# ---- 3. no extrapolation: the balanced panel stops at sweep 2 with the plain run's bits
def test_balanced_panel_stops_before_any_extrapolation(pds, contexts):
    fr = c2.balanced_frame()
    for split in ("whole", "cut"):
        for tol in (1e-8, 1e-13):
            acc = _fixed(pds, fr, "se", contexts[split], tol=tol)
            assert acc["n_iter"] == 2
            _same_bits(acc, _fixed(pds, fr, "se", contexts[split], tol=tol, accel="none"))


# ---- 4. the C ABI: unused codes between the used ones; shuffled rows by key against the offsets form on the ordered frame
def _grouped_raw(ctx, F, y, off, codes2, n_levels2, se, accel, tol=1e-8, max_iter=10_000):
    from polars_ds_extension_amd import _lib
    from polars_ds_extension_amd.lstsq import _Cols

    cols = ac.columns(F)
    n, p = len(y), len(cols)
    cs = _Cols(np.ascontiguousarray(y), cols)
    outs = {k: np.empty(p) for k in ("beta", "std_err", "t", "p", "ci_lower", "ci_upper")}
    rep = _lib.ReportF64(*[C.c_void_p(o.ctypes.data) for o in outs.values()], 0.0, 0.0)
    pred, resid = np.empty(n), np.empty(n)
    extra = _lib.Within2Out(C.c_void_p(pred.ctypes.data), C.c_void_p(resid.ctypes.data), 0.0, 0, 0, 0, 0, 0)
    off = np.ascontiguousarray(off, dtype=np.int64)
    codes2 = np.ascontiguousarray(codes2, dtype=np.int32)
    before = ctx.get_option("within2_accel")
    ctx.set_option("within2_accel", accel)
    try:
        rc = ctx._lib.pds_lin_reg_within2_grouped_f64(ctx._h, cs.cols, p, C.c_int64(n), C.c_void_p(off.ctypes.data), C.c_int64(len(off) - 1),
                                                      C.c_void_p(codes2.ctypes.data), C.c_int64(n_levels2), cs.space, _lib.WITHIN_SE_TYPES[se],
                                                      C.c_double(tol), max_iter, C.byref(rep), C.byref(extra))
    finally:
        ctx.set_option("within2_accel", before)
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


@pytest.mark.parametrize("kind,p", [("panel", 4), ("ragged300", 16), ("many2", 4)])
def test_forms_agree(pds, contexts, kind, p):
    F, y, off, k1, k2 = ac.frame(kind, p)
    F, y = np.asarray(F), np.asarray(y)
    n, n2 = len(y), len(np.unique(k2))
    codes2 = np.unique(k2, return_inverse=True)[1].reshape(-1)
    for split in ("whole", "cut"):
        ctx = contexts[split]
        ordered = _report(pds, (F, y, off, k1, k2), "cluster", ctx)
        assert ordered["n_iter"] == ac.ref(kind, p, "se", "float64", "default")["n_iter"]
        rc, raw = _grouped_raw(ctx, F, y, off, codes2, n2, "cluster", 1)  # ordered keys move nothing: the bits of the offsets form
        assert rc == 0
        _assert_raw_equals(raw, ordered, "cluster")
        rc, spare = _grouped_raw(ctx, F, y, off, codes2 * 2 + 1, 2 * n2 + 3, "cluster", 1)  # unused codes between the used ones count nowhere
        assert rc == 0 and spare["n_groups2"] == n2
        _assert_raw_equals(spare, ordered, "cluster")
        rc, plain = _grouped_raw(ctx, F, y, off, codes2, n2, "cluster", 0)  # option 0 through the C ABI: the plain call's bits
        assert rc == 0
        _assert_raw_equals(plain, _report(pds, (F, y, off, k1, k2), "cluster", ctx, accel="none"), "cluster")
        assert plain["n_iter"] > raw["n_iter"]
        # rows shuffled: the by-key form gives the bits of the offsets form on the key-ordered frame, per-row outputs where the rows are
        perm = np.random.default_rng(5).permutation(n)
        order = perm[np.argsort(k1[perm], kind="stable")]
        shuffled = _report(pds, (F[perm], y[perm], None, k1[perm], k2[perm]), "cluster", ctx)
        rc, on_ordered = _grouped_raw(ctx, F[order], y[order], off, codes2[order], n2, "cluster", 1)
        assert rc == 0
        inv = np.empty(n, dtype=np.int64)
        inv[np.argsort(k1[perm], kind="stable")] = np.arange(n)  # row i of the shuffled frame is row inv[i] of the ordered one
        _assert_raw_equals(on_ordered, shuffled, "cluster", row_map=inv)
        _same_bits(_report(pds, (F[perm], y[perm], None, k1[perm], k2[perm]), "cluster", ctx), shuffled)  # two calls


# ---- 5. off means off; the option and the argument -- on contexts without a split and with within_split_rows = 128
@pytest.mark.parametrize("split", ["whole", "cut"])
def test_off_means_off(pds, contexts, split):
    from polars_ds_extension_amd._lib import PdsError

    movers, panel = ac.frame("movers", 4), ac.frame("panel", 4)
    n_acc = ac.ref("panel", 4, "se", "float64", "default")["n_iter"]
    shared = contexts[split]
    fresh, zero, one = pds.Context(0), pds.Context(0), pds.Context(0)
    try:
        if split == "cut":
            for ctx in (fresh, zero, one):
                ctx.set_option("within_split_rows", 128)
        assert fresh.get_option("within2_accel") == 0  # the default
        zero.set_option("within2_accel", 0)
        one.set_option("within2_accel", 1)
        for fr, n_plain in ((movers, 971), (panel, None)):
            a = _fixed(pds, fr, "se", shared, accel="none")
            assert n_plain is None or a["n_iter"] == n_plain
            for ctx in (fresh, zero, shared):
                _same_bits(_fixed(pds, fr, "se", ctx, accel=None), a)
            _same_bits(_fixed(pds, fr, "se", one, accel="none"), a)
            assert one.get_option("within2_accel") == 1 and shared.get_option("within2_accel") == 0
        plain = a
        # a context whose option is 1 is used by a call with absorb_accel=None
        acc = _fixed(pds, panel, "se", shared)
        assert acc["n_iter"] == n_acc < plain["n_iter"]
        _same_bits(_fixed(pds, panel, "se", one, accel=None), acc)
        # ... and the option is back at its old value after a call that set it, on both kinds of context
        assert shared.get_option("within2_accel") == 0  # (after "irons_tuck" on it)
        _same_bits(_fixed(pds, panel, "se", shared, accel=None), plain)
        # ... including a call that raised
        with pytest.raises(PdsError, match="did not converge in 3 sweeps"):
            _fixed(pds, panel, "se", fresh, absorb_max_iter=3)
        assert fresh.get_option("within2_accel") == 0
        _same_bits(_fixed(pds, panel, "se", fresh, accel=None), plain)
        with pytest.raises(PdsError, match="did not converge in 3 sweeps"):
            _fixed(pds, panel, "se", one, accel="none", absorb_max_iter=3)
        assert one.get_option("within2_accel") == 1
        _same_bits(_fixed(pds, panel, "se", one, accel=None), acc)
        # ... and when the option was set through the C handle, not through this object
        assert fresh._lib.pds_ctx_set_option(fresh._h, b"within2_accel", C.c_longlong(1)) == 0
        _same_bits(_fixed(pds, panel, "se", fresh, accel="none"), plain)
        assert fresh.get_option("within2_accel") == 1
        _same_bits(_fixed(pds, panel, "se", fresh, accel=None), acc)
        # any other value of the option is refused and changes nothing
        for bad in (2, -1):
            with pytest.raises(PdsError, match="within2_accel") as e:
                one.set_option("within2_accel", bad)
            assert e.value.code == -1  # PDS_ERR_INVALID
        assert one.get_option("within2_accel") == 1
        _same_bits(_fixed(pds, panel, "se", one, accel=None), acc)
        with pytest.raises(PdsError, match="unknown context option"):
            one.get_option("within2_acceleration")
        assert shared.get_option("within_split_rows") == (128 if split == "cut" else 0)
    finally:
        for ctx in (fresh, zero, one):
            ctx.close()


# ---- 6. the sweep limit counts sweeps: reached in the middle of a cycle or at its end, the same error, nothing returned
@pytest.mark.parametrize("split", ["whole", "cut"])
def test_sweep_limit_in_mid_cycle(pds, contexts, split):
    from polars_ds_extension_amd._lib import PdsError

    fr, ctx = ac.frame("movers", 4), contexts[split]
    for limit in (51, 50, 1):
        with pytest.raises(PdsError, match=rf"did not converge in {limit} sweeps \(last delta = \d\.\d+e-\d+") as e:
            _fixed(pds, fr, ctx=ctx, absorb_max_iter=limit)
        assert e.value.code == -6  # PDS_ERR_NUMERIC
    own = ac.ref("movers", 4, "se", "float64", "default")["n_iter"]
    assert abs(_fixed(pds, fr, ctx=ctx, absorb_max_iter=own + 2)["n_iter"] - own) <= 2  # the context is usable, the limit is a limit
