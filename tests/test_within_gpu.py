"""lin_reg / lin_reg_report(absorb= | absorb_offsets=) on the MI355X against the NumPy restatement (within_reference.py) in long double.

Frames (within_cases.py): seeded, every one with a per-group level of about 50 x the within spread.  60 ragged groups -- 1, 2, 63,
64, 65, 127, 128, 129, 300 and 1 000 rows plus 50 sizes in 3 .. 200 -- at widths 1, 4, 8, 15 and 16, f64 and f32, each on the default
context and on one with "within_split_rows" = 128, which cuts the 129-, 300- and 1 000-row groups; equal groups of 5 rows (G = 2 .. 9:
whole and short batches of the outer-product step); 20 000 pairs (more groups than waves); one group of 699 rows beside one of 1;
3 groups among 200 singletons; offsets with empty groups.  Every frame runs all three `std_err` values and the fit-only call, and is
checked in beta, the standard error, t, p, the interval, r2, adj_r2, r2_overall, alpha, pred, resid, df_resid and n_groups.

Budgets (the project's standing rule, tests/test_cluster_report_gpu.py).  The device may be at most 10 x as far from the long double
result as the reference's own arithmetic in the frame's format is on that frame (8 ulp where that distance is below half an ulp);
distance = max |a - b| / max |b| per field.  An f32 frame is compared on the values as stored in f32, its budget made from the
reference run in float32 arithmetic on those values.  The reference's distances are measured on the CPU inside the tests, before
anything on the device is asserted, and printed.  p-values and the interval get what the budgets of t, beta and the standard error
let through plus 1e-10 for the special functions (TAIL_TOL, QUANTILE_TOL).

Measured on the MI355X (worst over widths, the three estimators and both split settings; the reference's own arithmetic in the
frame's format against long double beside it):
                                    beta     std_err  t        r2       adj_r2   r2_overall alpha    pred     resid
  ragged, f64            device     6.8e-16  1.7e-15  1.0e-15  2.4e-15  3.6e-15  5.0e-17    9.1e-16  2.3e-16  5.5e-15
                         reference  1.6e-15  1.0e-15  6.2e-15  1.0e-15  8.9e-16  5.0e-17    2.0e-15  4.5e-16  1.5e-14
  ragged, f32            device     3.2e-08  5.6e-08  5.4e-08  3.9e-08  3.6e-08  5.4e-17    3.4e-08  4.2e-08  3.9e-08
                         reference  6.2e-07  4.9e-07  1.7e-06  4.2e-07  8.3e-07  2.7e-08    8.2e-07  2.4e-07  7.3e-06
  equal groups G=2..9    device     6.3e-15  1.8e-14  5.1e-12  1.1e-14  2.8e-14  5.3e-17    6.9e-15  3.0e-16  3.6e-14
                         reference  3.8e-15  3.5e-14  4.2e-12  1.2e-14  9.4e-13  5.8e-17    4.6e-15  1.1e-15  1.1e-13
  20 000 pairs           device     5.4e-16  6.0e-16  4.0e-16  1.2e-16  6.6e-17  4.5e-17    7.5e-16  1.8e-16  1.2e-14
                         reference  4.8e-16  8.2e-16  6.1e-16  1.2e-16  6.6e-17  4.5e-17    4.9e-16  2.1e-16  1.9e-14
  699 + 1, "se"          device     1.2e-15  7.5e-16  6.8e-16  1.3e-16  1.7e-16  2.9e-17    4.5e-15  1.9e-16  3.5e-15
                         reference  8.4e-16  8.1e-16  3.9e-16  3.9e-16  4.4e-16  2.9e-17    1.6e-15  4.7e-16  8.8e-15
  3 groups + 200 single  device     7.5e-16  8.5e-16  2.9e-15  2.0e-15  6.6e-16  4.0e-17    3.4e-16  7.3e-17  2.5e-15
                         reference  7.3e-16  3.2e-15  3.7e-15  2.8e-15  3.8e-15  4.0e-17    3.0e-16  1.6e-16  4.7e-15
  (the worst rows are per column, not per case: every case passed its own frame's budget.)  699 + 1 with the clustered errors: the
  only group with a within spread has, by the normal equations, a score of exactly zero, so the clustered error is 0 and what any
  arithmetic returns for it is rounding noise -- the reference's float64 is 1.2e+03 from its long double there, the device 1.4e+03,
  t is 1.0 off in both; beta, r2, alpha, pred and resid are those of the "se" row.  Device against device, p = 3, G = 12, against
  lin_reg_report on the 3 features + 11 dummies + bias: beta 6.1e-12 (bar 1.1e-11: the dummy design carries the group levels),
  classical errors 8.8e-13 (3.1e-12), CR0 2.2e-12 (5.7e-12).
  The first run missed two checks, both mended in the test's own arithmetic and not by a wider tolerance: a float32 p-value below the
  format's range (2.98e-123, stored as 0) needs one subnormal step in its bound, and the bound on p takes the t density at the near
  end of t's budget, not at t (it understated the 699 + 1 clustered case, where t is noise).  A third was the library's: the
  p-values of this report come from student_t_sf_wide since (stats.cpp), because student_t_sf, which restates the reference library's
  algorithm, is 2.1e-10 from SciPy at t = 1.56 with 19 999 degrees of freedom (the 20 000 pairs), outside TAIL_TOL.
"""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT))

import within_cases as wc  # noqa: E402
import within_reference as wr  # noqa: E402

pytestmark = pytest.mark.gpu

SE_NAME = {"se": "std_err", "cluster": "cluster_se", "cluster0": "cluster0_se"}
QUANTILE_TOL = 1e-10  # (tests/test_cluster_report_gpu.py: the library's Student t quantile and tail against SciPy's)
TAIL_TOL = 1e-10


@pytest.fixture(scope="module")
def pds():
    import polars_ds_extension_amd as pds

    return pds


@pytest.fixture(scope="module")
def contexts(pds):
    """the default context, and one whose split threshold cuts every group above 128 rows"""
    ctxs = {"whole": pds.default_context(), "cut": pds.Context(0)}
    ctxs["cut"].set_option("within_split_rows", 128)
    yield ctxs
    ctxs["cut"].close()


def _run(pds, F, y, se, ctx=None, f32=False, **kw):
    kw.setdefault("return_effects", True)
    kw.setdefault("return_pred", True)
    pds.config.LIN_REG_EXPR_F64 = not f32
    try:
        return pds.lin_reg_report(*wc.columns(F), target=y, std_err=se, ctx=ctx, **kw)
    finally:
        pds.config.LIN_REG_EXPR_F64 = True


def _check(got, kind, p, se, what, fmt="float64", g=0, alpha_at=None):
    """every field of a device report against the long double reference within the budget of its frame"""
    from scipy import stats as st

    assert np.finfo(np.longdouble).eps < 1e-18  # the reference has to be wider than the arithmetic under test
    sp = wc.spread(kind, p, se, fmt, g)  # measured first, on the CPU
    want = wc.ref(kind, p, se, "longdouble", g)
    dt = wc.DTYPES[fmt]
    eps = float(np.finfo(dt).eps)
    assert got["n_groups"] == want["n_groups"] and got["df_resid"] == want["df_resid"]
    assert SE_NAME[se] in got and (se == "se" or "std_err" not in got)
    alpha = np.asarray(got["effects"])
    if alpha_at is not None:  # offsets with empty groups: NaN there
        empty = np.ones(len(alpha), dtype=bool)
        empty[alpha_at] = False
        assert np.all(np.isnan(alpha[empty])) and not np.any(np.isnan(alpha[alpha_at]))
        alpha = alpha[alpha_at]
    vals = {"beta": got["beta"], "std_err": got[SE_NAME[se]], "t": got["t"], "r2": got["r2"][0], "adj_r2": got["adj_r2"][0],
            "r2_overall": got["r2_overall"], "alpha": alpha, "pred": got["pred"], "resid": got["resid"]}
    assert got["beta"].dtype == dt and np.asarray(got["pred"]).dtype == dt and alpha.dtype == dt
    fields = wr.FIELDS + wr.ROW_FIELDS
    dist = {k: wr.rel(vals[k], want[k]) for k in fields}
    print(f"{what} {kind} p={p} g={g} {se} {fmt}: device vs long double {dist}; reference {fmt} vs long double {sp}")
    bud = {k: wr.budget(sp[k], dt) for k in fields}
    for k in fields:
        assert dist[k] <= bud[k], (k, dist[k], sp[k])
    t_o = np.asarray(want["t"], dtype=np.float64)
    dof = want["t_dof"]
    dt_bound = bud["t"] * np.max(np.abs(t_o))
    p_o = want["p"]
    # (a p-value below the format's range is stored as a subnormal or as 0: one subnormal step on top of the relative terms)
    # the density is taken at the near end of what t's budget allows, where it is largest (a first-order term at t itself
    # understates the change when the budget is not small against t: a frame whose clustered error is 0 up to rounding)
    dp_bound = 2.0 * st.t.pdf(np.maximum(np.abs(t_o) - dt_bound, 0.0), dof) * dt_bound + (TAIL_TOL + eps) * p_o + float(np.finfo(dt).smallest_subnormal)
    assert np.all(np.abs(np.asarray(got["p>|t|"], dtype=np.float64) - p_o) <= dp_bound), (np.asarray(got["p>|t|"]) - p_o, dp_bound)
    b_o, s_o = np.asarray(want["beta"], dtype=np.float64), np.asarray(want["std_err"], dtype=np.float64)
    ci_bound = bud["beta"] * np.max(np.abs(b_o)) + want["t_crit"] * (bud["std_err"] + QUANTILE_TOL) * np.max(s_o) + eps * np.max(np.abs(want["ci_hi"]))
    assert np.all(np.abs(np.asarray(got["0.025"], dtype=np.float64) - want["ci_lo"]) <= ci_bound)
    assert np.all(np.abs(np.asarray(got["0.975"], dtype=np.float64) - want["ci_hi"]) <= ci_bound)
    return dist


def _check_fit_only(pds, F, y, off, full, ctx, f32=False):
    """lin_reg(absorb_offsets=): the pass without the scores gives the report's beta, pred and resid, bit for bit"""
    pds.config.LIN_REG_EXPR_F64 = not f32
    try:
        beta = pds.lin_reg(*wc.columns(F), target=y, absorb_offsets=off, ctx=ctx)
        b2, pred, resid = pds.lin_reg(*wc.columns(F), target=y, absorb_offsets=off, return_pred=True, ctx=ctx)
    finally:
        pds.config.LIN_REG_EXPR_F64 = True
    assert np.array_equal(beta, full["beta"]) and np.array_equal(b2, beta)
    assert np.array_equal(pred, full["pred"]) and np.array_equal(resid, full["resid"])


def _same_bits(a, b, skip=()):
    assert a.keys() == b.keys()
    for k in a:
        if k in skip:
            continue
        if k in ("features", "n_groups", "df_resid", "r2_overall"):
            assert a[k] == b[k], k
        else:
            x, y = (v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v) for v in (a[k], b[k]))
            assert np.array_equal(x, y, equal_nan=True), k


# ---- 1. ragged frames
@pytest.mark.parametrize("fmt", ["float64", "float32"])
@pytest.mark.parametrize("p", wc.WIDTHS)
def test_ragged(pds, contexts, p, fmt):
    f32 = fmt == "float32"
    kind = "ragged32" if f32 else "ragged"
    F, y, off, codes = wc.frame(kind, p)
    w = wc.ref(kind, p, "cluster")
    ratio = np.asarray(w["se_all"]["cluster"] / w["se_all"]["se"], dtype=np.float64)
    print(f"p={p}: clustered / classical standard errors {ratio}")
    assert np.max(np.abs(ratio - 1.0)) > 0.1  # the estimator matters on this frame
    for split in ("whole", "cut"):
        for se in wr.SE_TYPES:
            got = _run(pds, F, y, se, ctx=contexts[split], f32=f32, absorb_offsets=off)
            _check(got, kind, p, se, split, fmt)
        _check_fit_only(pds, F, y, off, got, contexts[split], f32)


# ---- 2. batch boundaries of the outer-product step
@pytest.mark.parametrize("p", [1, 16])
@pytest.mark.parametrize("g", [2, 3, 4, 5, 6, 7, 8, 9])
def test_batches(pds, contexts, g, p):
    F, y, off, codes = wc.equal_frame(g, p)
    for se in wr.SE_TYPES:
        got = _run(pds, F, y, se, absorb_offsets=off)
        _check(got, "equal", p, se, "whole", g=g)
    _check_fit_only(pds, F, y, off, got, None)


# ---- 3. more groups than waves; lopsided; singletons
@pytest.mark.parametrize("p", [1, 16])
def test_pairs(pds, p):
    F, y, off, codes = wc.pairs_frame(p)
    for se in wr.SE_TYPES:
        _check(_run(pds, F, y, se, absorb_offsets=off), "pairs", p, se, "whole")


@pytest.mark.parametrize("split", ["whole", "cut"])
@pytest.mark.parametrize("p", [4, 16])
def test_lopsided(pds, contexts, p, split):
    F, y, off, codes = wc.lopsided_frame(p)
    for se in wr.SE_TYPES:
        got = _run(pds, F, y, se, ctx=contexts[split], absorb_offsets=off)
        assert got["n_groups"] == 2
        _check(got, "lopsided", p, se, split)


@pytest.mark.parametrize("p", [1, 8, 16])
def test_singletons(pds, p):
    """A singleton counts in n and G, adds nothing to W or M, and has alpha = y - x' beta: its residual is exactly zero."""
    F, y, off, codes = wc.singletons_frame(p)
    single = np.flatnonzero(np.diff(off) == 1)
    assert len(single) == 200
    for se in wr.SE_TYPES:
        got = _run(pds, F, y, se, absorb_offsets=off)
        assert got["n_groups"] == 203
        _check(got, "singletons", p, se, "whole")
        assert np.all(got["resid"][off[single]] == 0.0) and np.array_equal(got["pred"][off[single]], np.asarray(y)[off[single]])


# ---- 4. empty groups; two calls
@pytest.mark.parametrize("split", ["whole", "cut"])
@pytest.mark.parametrize("p", [4, 16])
def test_empty_groups_change_no_bit(pds, contexts, p, split):
    F, y, off, codes = wc.ragged_frame(p)
    padded, place = wc.with_empty_groups(off)
    for se in ("se", "cluster"):
        base = _run(pds, F, y, se, ctx=contexts[split], absorb_offsets=off)
        _same_bits(_run(pds, F, y, se, ctx=contexts[split], absorb_offsets=off), base)  # two calls
        got = _run(pds, F, y, se, ctx=contexts[split], absorb_offsets=padded)
        _same_bits(got, base, skip=("effects", "effect_keys"))
        assert len(got["effects"]) == len(padded) - 1 and np.array_equal(got["effects"][place], base["effects"])
        _check(got, "ragged", p, se, split + " padded", alpha_at=place)


# ---- 5. device against device: the dummy-variable regression
def test_against_dummy_columns(pds):
    """p = 3, G = 12: the absorbed fit against lin_reg_report on the 3 features + 11 dummies + bias (the 16 columns lin_reg_report's
    cluster form takes).  beta and the classical standard errors of the features, and CR0 against std_err="cluster0" clustered on the
    same key.  Bar: the SUM of the two calls' own budgets on that frame -- 10 x what the within reference, and 10 x what the plain
    regression on that dummy design, lose in float64 against long double (8 ulp where that is below half an ulp)."""
    F, y, off, codes = wc.equal_frame(12, 3)
    F, y = np.asarray(F), np.asarray(y)
    D = (codes[:, None] == np.arange(1, 12)[None, :]).astype(np.float64)
    Z = np.column_stack([F, D])
    Zb = np.column_stack([Z, np.ones(len(y))])
    plain = {dt: wr.plain_report(Zb, y, codes, wc.DTYPES[dt]) for dt in ("float64", "longdouble")}
    sp_plain = {k: wr.rel(plain["float64"][k][:3], plain["longdouble"][k][:3]) for k in ("beta", "se", "cluster0")}
    for se, other_name, key in (("se", "std_err", "se"), ("cluster0", "cluster0_se", "cluster0")):
        sp_within = wc.spread("equal", 3, se, g=12)
        a = _run(pds, F, y, se, absorb_offsets=off)
        kw = {"cluster": codes} if se == "cluster0" else {}
        b = pds.lin_reg_report(*wc.columns(Z), target=y, add_bias=True, std_err=se, **kw)
        d = {"beta": wr.rel(a["beta"], b["beta"][:3]), "std_err": wr.rel(a[SE_NAME[se]], b[other_name][:3])}
        bar = {"beta": wr.budget(sp_within["beta"]) + wr.budget(sp_plain["beta"]), "std_err": wr.budget(sp_within["std_err"]) + wr.budget(sp_plain[key])}
        print(f"absorb vs 11 dummies + bias, {se}: {d}; bars {bar} from within {sp_within['beta']:.2e} / {sp_within['std_err']:.2e}, plain {sp_plain}")
        for k in d:
            assert d[k] <= bar[k], (se, k, d[k], bar[k])


# ---- 6. by-key forms
@pytest.mark.parametrize("p", [4, 16])
def test_forms_agree(pds, contexts, p):
    import torch

    F, y, off, codes = wc.ragged_frame(p)
    cols = wc.columns(F)
    keys = codes * 7 - 200  # negative, sparse
    n = len(y)
    kw = dict(return_effects=True, return_pred=True)
    for split in ("whole", "cut"):
        ctx = contexts[split]
        for se in ("se", "cluster"):
            base = pds.lin_reg_report(*cols, target=y, std_err=se, absorb_offsets=off, ctx=ctx, **kw)
            ordered = pds.lin_reg_report(*cols, target=y, std_err=se, absorb=keys, ctx=ctx, **kw)  # ordered keys: nothing moves
            _same_bits(ordered, base, skip=("effect_keys",))
            assert np.array_equal(ordered["effect_keys"], np.unique(keys)) and np.array_equal(base["effect_keys"], np.arange(len(off) - 1))
            # rows shuffled: the stable sort + gather brings them into key order; per-row outputs come back where the rows are
            perm = np.random.default_rng(5).permutation(n)
            order = perm[np.argsort(keys[perm], kind="stable")]
            on_ordered = pds.lin_reg_report(*[c[order] for c in cols], target=y[order], std_err=se, absorb_offsets=off, ctx=ctx, **kw)
            shuffled = pds.lin_reg_report(*[c[perm] for c in cols], target=y[perm], std_err=se, absorb=keys[perm], ctx=ctx, **kw)
            inv = np.empty(n, dtype=np.int64)
            inv[np.argsort(keys[perm], kind="stable")] = np.arange(n)  # row i of the shuffled frame is row inv[i] of the ordered one
            _same_bits(shuffled, on_ordered, skip=("effect_keys", "pred", "resid"))
            assert np.array_equal(shuffled["pred"], on_ordered["pred"][inv]) and np.array_equal(shuffled["resid"], on_ordered["resid"][inv])
            assert np.array_equal(shuffled["effect_keys"], np.unique(keys))
            _same_bits(pds.lin_reg_report(*[c[perm] for c in cols], target=y[perm], std_err=se, absorb=keys[perm], ctx=ctx, **kw), shuffled)
            # CUDA tensors, offsets and keys
            dev = torch.device("cuda", 0)
            tcols = [torch.from_numpy(np.array(c)).to(dev) for c in cols]
            ty = torch.from_numpy(np.array(y)).to(dev)
            t_off = pds.lin_reg_report(*tcols, target=ty, std_err=se, absorb_offsets=torch.from_numpy(np.array(off)).to(dev), ctx=ctx, **kw)
            assert t_off["pred"].is_cuda and t_off["effects"].is_cuda
            _same_bits(t_off, base)
            t_key = pds.lin_reg_report(*[c[perm] for c in tcols], target=ty[perm], std_err=se, absorb=torch.from_numpy(keys[perm]).to(dev), ctx=ctx, **kw)
            _same_bits(t_key, shuffled)
        # lin_reg by key, fit only
        beta, pred, resid = pds.lin_reg(*[c[perm] for c in cols], target=y[perm], absorb=keys[perm], return_pred=True, ctx=ctx)
        assert np.array_equal(beta, shuffled["beta"]) and np.array_equal(pred, shuffled["pred"]) and np.array_equal(resid, shuffled["resid"])
        back = np.argsort(perm)  # original row j is row back[j] of the shuffled frame
        _check(dict(shuffled, pred=shuffled["pred"][back], resid=shuffled["resid"][back]), "ragged", p, "cluster", "shuffled " + split)


def test_names_and_fields(pds):
    F, y, off, codes = wc.ragged_frame(4)
    a = pds.lin_reg_report(*wc.columns(F), target=y, absorb=codes, std_err="cluster0", feature_names=list("abcd"))
    assert a["features"] == list("abcd")
    assert list(a) == ["features", "beta", "cluster0_se", "t", "p>|t|", "0.025", "0.975", "r2", "adj_r2", "r2_overall", "n_groups", "df_resid"]
    assert a["n_groups"] == 60 and a["df_resid"] == 59
    b = pds.lin_reg_report(*wc.columns(F), target=y, absorb=codes, return_effects=True)
    assert "std_err" in b and b["df_resid"] == len(y) - 60 - 4 and len(b["effects"]) == 60 and "pred" not in b
    plain = pds.lin_reg_report(*wc.columns(F), target=y, add_bias=True)  # the plain report is another model and keeps its fields
    assert "n_groups" not in plain and wr.rel(plain["beta"][:4], a["beta"]) > 0.05


# ---- 7. refusals
def test_refusals(pds):
    from polars_ds_extension_amd import _lib
    from polars_ds_extension_amd._lib import PdsError
    from polars_ds_extension_amd.lstsq import _Cols

    F, y, off, codes = wc.ragged_frame(4)
    cols = wc.columns(F)
    n = len(y)
    c12, y12 = [c[:12] for c in cols], y[:12]
    assert pds.lin_reg_report(*c12, target=y12, absorb=np.repeat(np.arange(6), 2))["df_resid"] == 2  # 12 - 6 - 4 = 2: fits
    with pytest.raises(PdsError, match="#rows - #groups - #features <= 0") as e:
        pds.lin_reg_report(*c12, target=y12, absorb=np.array([0, 0, 1, 1, 2, 2, 3, 3, 4, 5, 6, 7]))  # 12 - 8 - 4 = 0
    assert e.value.code == -3  # PDS_ERR_TOO_FEW_ROWS
    for se in ("cluster", "cluster0"):
        with pytest.raises(PdsError, match="at least two non-empty groups") as e:
            pds.lin_reg_report(*cols, target=y, absorb=np.zeros(n, dtype=np.int64), std_err=se)  # G = 1
        assert e.value.code == -1
        with pytest.raises(PdsError, match="at least two non-empty groups") as e:
            pds.lin_reg_report(*cols, target=y, absorb_offsets=np.array([0, 0, n]), std_err=se)  # one of the two is empty
        assert e.value.code == -1
    assert pds.lin_reg_report(*cols, target=y, absorb=np.zeros(n, dtype=np.int64))["n_groups"] == 1  # classical errors take one group
    bad = off.copy()
    bad[3], bad[4] = off[4], off[3]
    for o in (bad, off[:-1], off[1:]):  # decreasing; rows behind / in front of every group
        with pytest.raises(PdsError, match="non-decreasing and cover the frame") as e:
            pds.lin_reg_report(*cols, target=y, absorb_offsets=o)
        assert e.value.code == -1
    # a feature that is constant inside every group is collinear with the effects: named by its index
    level = np.asarray(codes, dtype=np.float64) * 3.0 + 1.0
    with pytest.raises(PdsError, match="feature column 2 is constant inside every group") as e:
        pds.lin_reg_report(cols[0], cols[1], level, cols[2], target=y, absorb=codes)
    assert e.value.code == -6  # PDS_ERR_NUMERIC
    with pytest.raises(PdsError, match="not positive definite") as e:
        pds.lin_reg_report(cols[0], cols[1], cols[0], target=y, absorb=codes)  # a repeated column
    assert e.value.code == -6
    with pytest.raises(PdsError, match="up to 16 feature columns") as e:
        pds.lin_reg_report(*[cols[0]] * 17, target=y, absorb=codes)
    assert e.value.code == -5  # PDS_ERR_UNSUPPORTED
    with pytest.raises(PdsError, match="HC0 - HC3") as e:
        pds.lin_reg_report(*cols, target=y, absorb=codes, std_err="hc2")
    assert e.value.code == -5
    with pytest.raises(NotImplementedError, match="weights"):
        pds.lin_reg_report(*cols, target=y, absorb=codes, weights=np.ones(n))
    # the C ABI itself: HC codes are unsupported, other codes invalid; a failed call leaves the context usable
    ctx = pds.default_context()
    cs = _Cols(y, cols)
    outs = [np.empty(4) for _ in range(6)]
    rep = _lib.ReportF64(*[C.c_void_p(o.ctypes.data) for o in outs], 0.0, 0.0)
    k = np.ascontiguousarray(codes, dtype=np.int64)
    ng = C.c_int64(0)
    for code, rc_want in ((1, -5), (4, -5), (7, -1), (0x100, -1)):
        rc = ctx._lib.pds_lin_reg_within_by_key_f64(ctx._h, cs.cols, C.c_void_p(k.ctypes.data), 4, C.c_int64(n), cs.space, code, C.c_int64(n), None,
                                                    C.byref(rep), None, C.byref(ng))
        assert rc == rc_want, (code, rc)
    # more distinct keys than max_groups, with the effects asked for: refused, the count reported
    alpha = np.empty(10)
    extra = _lib.WithinOut(C.c_void_p(alpha.ctypes.data), None, None, 0.0, 0, 0)
    rc = ctx._lib.pds_lin_reg_within_by_key_f64(ctx._h, cs.cols, C.c_void_p(k.ctypes.data), 4, C.c_int64(n), cs.space, 0, C.c_int64(10), None,
                                                C.byref(rep), C.byref(extra), C.byref(ng))
    assert rc == -1 and ng.value == 60
    assert pds.lin_reg_report(*cols, target=y, absorb=codes)["n_groups"] == 60
