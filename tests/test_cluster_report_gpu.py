"""lin_reg_report(std_err="cluster" | "cluster0") on the MI355X against the NumPy restatement (cluster_reference.py) in long double.

Frames (cluster_cases.py): seeded; 60 ragged clusters -- 1, 2, 63, 64, 65, 127, 128, 129, 300 and 1 000 rows plus 50 sizes in 3 .. 200
-- with a per-cluster shock in the residuals; widths 1, 4, 8, 15 and 16, bias on and off, f64 and f32; each run as is and with
"cluster_split_rows" = 128, which cuts the 129-, 300- and 1 000-row clusters.  Equal clusters of 5 rows (G = 2 .. 9) at every cap
on the waves ("cluster_waves" = 1, 2 and the default: a launch never starts more waves than there are clusters, so under the
default every cluster has a wave of its own and under the cap 1 one wave walks them all, through whole and short batches of the
outer-product step); 20 000 singletons (more clusters than waves); one cluster with all rows but one.

Budgets.  The device may be at most 10 x as far from the long double result as the reference's own arithmetic in the frame's
format is on that frame (8 ulp where that distance is 0); distance = max |a - b| / max |b| per field.  The format is float64 for an
f64 frame.  For an f32 frame the report comes back in float32 fields (pds_report_f32), which cannot be closer than half a float32
ulp to anything: its frame is compared on the values as stored in f32 and its budget is made the same way from the reference run in
float32 arithmetic on those values.  The reference's distances are measured on the CPU inside the tests, before anything on the
device is asserted, and printed.  p-values and the interval come from special functions: they are bounded by what the budgets of
t, beta and the standard error let through, plus 1e-10 relative for the special function itself (TAIL_TOL, QUANTILE_TOL below).

Measured on the MI355X (worst over widths, bias, estimators and every split / wave setting; the reference's own arithmetic in the
frame's format against long double beside it):
                                      beta     std_err  t        r2       adj_r2
  ragged, f64            device       8.5e-16  1.4e-15  1.0e-15  4.0e-15  4.0e-15
                         reference    2.1e-15  1.9e-15  2.7e-15  1.2e-15  1.7e-15
  ragged, f32            device       9.8e-08  2.0e-07  1.9e-07  3.2e-07  3.7e-07
                         reference    3.3e-06  1.1e-06  2.9e-06  3.8e-07  3.7e-07
  equal clusters G=2..9  device       9.5e-15  1.4e-13  8.7e-11  3.4e-15  2.3e-14
                         reference    4.1e-15  3.0e-14  1.9e-11  9.7e-16  2.3e-14
  20 000 singletons      device       6.6e-16  5.8e-16  6.6e-16  1.9e-14  2.1e-14
                         reference    3.3e-15  5.8e-16  3.1e-15  1.9e-14  2.1e-14
  all rows but one       device       4.5e-16  9.2e-13  2.0e-12  9.1e-17  1.2e-16
                         reference    4.2e-16  8.4e-13  2.6e-12  5.1e-17  1.7e-17
  singletons, device against device: cluster0 vs hc0 / cluster vs hc1: beta 0 (the same bits), std_err 9.3e-17 / 1.8e-16, r2 2.3e-14
  (the worst rows are per column, not per case: every case passed its own frame's budget.  With plain sums of e^2 the first run
  missed one: ragged p = 4 without bias under the split, adj_r2 2.9e-15 against a budget of 2.6e-15 -- r2 is small there and
  magnifies the last bits of sum e^2; the sum is compensated since.)
"""
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT))

import cluster_cases as cc  # noqa: E402
import cluster_reference as cr  # noqa: E402

pytestmark = pytest.mark.gpu

SE_NAME = {"cluster": "cluster_se", "cluster0": "cluster0_se"}
# The library's Student t tail and 97.5 % quantile restate the reference library's algorithms, which is the project's contract (1e-10)
# and not SciPy's accuracy away from the exact values (stats.cpp's header; measured on the CPU, no device involved: the quantile 4e-11
# from SciPy over dof 1 .. 20 000, the tail 6e-11 over |t| <= 1 000 at those dof): p and the interval get that term.
QUANTILE_TOL = 1e-10
TAIL_TOL = 1e-10


@pytest.fixture(scope="module")
def pds():
    import polars_ds_extension_amd as pds

    return pds


@pytest.fixture(scope="module")
def contexts(pds):
    """the default context; one whose split threshold cuts every cluster above 128 rows; caps of one and two waves"""
    made = {"cut": ("cluster_split_rows", 128), "w1": ("cluster_waves", 1), "w2": ("cluster_waves", 2)}
    ctxs = {"whole": pds.default_context()}
    for name, (opt, v) in made.items():
        ctxs[name] = pds.Context(0)
        ctxs[name].set_option(opt, v)
    yield ctxs
    for name in made:
        ctxs[name].close()


def _run(pds, F, y, se, bias, ctx=None, f32=False, **kw):
    if not f32:
        return pds.lin_reg_report(*cc.columns(F), target=y, add_bias=bias, std_err=se, ctx=ctx, **kw)
    pds.config.LIN_REG_EXPR_F64 = False
    try:
        return pds.lin_reg_report(*cc.columns(F), target=y, add_bias=bias, std_err=se, ctx=ctx, **kw)
    finally:
        pds.config.LIN_REG_EXPR_F64 = True


def _check(got, kind, p, bias, se, what, fmt="float64", g=0):
    """every field of a device report against the long double reference within the budget of its frame"""
    from scipy import stats as st

    assert np.finfo(np.longdouble).eps < 1e-18  # the reference has to be wider than the arithmetic under test
    sp = cc.spread(kind, p, bias, se, fmt, g)  # measured first, on the CPU
    want = cc.ref(kind, p, bias, se, "longdouble", g)
    dt = cc.DTYPES[fmt]
    eps = float(np.finfo(dt).eps)
    assert got["n_clusters"] == want["n_clusters"]
    assert SE_NAME[se] in got and "std_err" not in got
    vals = {"beta": got["beta"], "std_err": got[SE_NAME[se]], "t": got["t"], "r2": got["r2"][0], "adj_r2": got["adj_r2"][0]}
    dist = {k: cr.rel(vals[k], want[k]) for k in cr.FIELDS}
    print(f"{what} {kind} p={p} bias={bias} {se} {fmt}: device vs long double {dist}; reference {fmt} vs long double {sp}")
    bud = {k: cr.budget(sp[k], dt) for k in cr.FIELDS}
    for k in cr.FIELDS:
        assert dist[k] <= bud[k], (k, dist[k], sp[k])
    t_o = np.asarray(want["t"], dtype=np.float64)
    dof = want["t_dof"]
    dt_bound = bud["t"] * np.max(np.abs(t_o))
    p_o = want["p"]
    dp_bound = 2.0 * st.t.pdf(np.abs(t_o), dof) * dt_bound + (TAIL_TOL + eps) * p_o
    assert np.all(np.abs(np.asarray(got["p>|t|"], dtype=np.float64) - p_o) <= dp_bound), (np.asarray(got["p>|t|"]) - p_o, dp_bound)
    b_o, s_o = np.asarray(want["beta"], dtype=np.float64), np.asarray(want["std_err"], dtype=np.float64)
    ci_bound = bud["beta"] * np.max(np.abs(b_o)) + want["t_crit"] * (bud["std_err"] + QUANTILE_TOL) * np.max(s_o) + eps * np.max(np.abs(want["ci_hi"]))
    assert np.all(np.abs(np.asarray(got["0.025"], dtype=np.float64) - want["ci_lo"]) <= ci_bound)
    assert np.all(np.abs(np.asarray(got["0.975"], dtype=np.float64) - want["ci_hi"]) <= ci_bound)
    return dist


def _same_bits(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if k in ("features", "n_clusters"):
            assert a[k] == b[k], k
        else:
            assert np.array_equal(a[k], b[k]), k


# ---- 1. ragged frames
@pytest.mark.parametrize("fmt", ["float64", "float32"])
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("p", cc.WIDTHS)
def test_ragged(pds, contexts, p, bias, fmt):
    f32 = fmt == "float32"
    kind = "ragged32" if f32 else "ragged"
    F, y, off, codes = cc.frame(kind, p)
    # on the CPU first: the estimator must matter on this frame, or the test could pass on the wrong one
    w = cc.ref(kind, p, bias, "cluster")
    ratio = np.asarray(w["se_all"]["cluster"] / w["se_all"]["hc1"], dtype=np.float64)
    print(f"p={p} bias={bias}: cluster / hc1 standard errors {ratio}")
    assert np.max(np.abs(ratio - 1.0)) > 0.2
    for se in cr.SE_TYPES:
        for split in ("whole", "cut"):
            got = _run(pds, F, y, se, bias, ctx=contexts[split], f32=f32, cluster_offsets=off)
            assert got["beta"].dtype == cc.DTYPES[fmt]
            _check(got, kind, p, bias, se, split, fmt)


# ---- 2. batch boundaries of the outer-product step
@pytest.mark.parametrize("p", [1, 16])
@pytest.mark.parametrize("g", [2, 3, 4, 5, 7, 8, 9])
def test_batches(pds, contexts, g, p):
    F, y, off, codes = cc.equal_frame(g, p)
    for waves in ("whole", "w1", "w2"):
        for se in cr.SE_TYPES:
            got = _run(pds, F, y, se, True, ctx=contexts[waves], cluster_offsets=off)
            _check(got, "equal", p, True, se, waves, g=g)


@pytest.mark.parametrize("p", [1, 16])
def test_all_empty_but_three(pds, contexts, p):
    """Empty clusters in the offsets are not counted and change no output bit, whichever wave would have walked them."""
    F, y, off, codes = cc.equal_frame(3, p)
    padded = np.concatenate([np.zeros(40, np.int64), off[:2], np.full(7, off[1]), off[2:], np.full(50, off[3])])
    for waves in ("whole", "w1", "w2"):
        base = _run(pds, F, y, "cluster", True, ctx=contexts[waves], cluster_offsets=off)
        got = _run(pds, F, y, "cluster", True, ctx=contexts[waves], cluster_offsets=padded)
        assert got["n_clusters"] == 3
        _same_bits(got, base)
        _check(got, "equal", p, True, "cluster", waves + " padded", g=3)


# ---- 3. all-singleton clusters
@pytest.mark.parametrize("p", [1, 16])
def test_singletons(pds, p):
    """G = n: CR0 is HC0 and CR1 is HC1 (G / (G - 1) (n - 1) / (n - p') = n / (n - p')) in beta, se and r2; t, p and the interval use
    n - 1 degrees of freedom instead of n - p' and are checked against the reference."""
    F, y, off, codes = cc.singleton_frame(p)
    for se, hc in (("cluster0", "hc0"), ("cluster", "hc1")):
        got = _run(pds, F, y, se, True, cluster_offsets=off)
        dist = _check(got, "singleton", p, True, se, "singletons")
        other = pds.lin_reg_report(*cc.columns(F), target=y, add_bias=True, std_err=hc)
        sp = cc.spread("singleton", p, True, se)
        d = {"beta": cr.rel(got["beta"], other["beta"]), "std_err": cr.rel(got[SE_NAME[se]], other[hc + "_se"]),
             "r2": cr.rel(got["r2"][0], other["r2"][0])}
        print(f"singletons p={p}: {se} vs {hc} on the device {d}; budgets from {sp}")
        for k in d:
            assert d[k] <= cr.budget(sp[k]), (k, d[k], sp[k])
        assert got["n_clusters"] == len(y)


# ---- 4. one cluster with all rows but one
@pytest.mark.parametrize("split", ["whole", "cut"])
@pytest.mark.parametrize("p", [4, 16])
def test_lopsided(pds, contexts, p, split):
    F, y, off, codes = cc.lopsided_frame(p)
    for se in cr.SE_TYPES:
        got = _run(pds, F, y, se, True, ctx=contexts[split], cluster_offsets=off)
        assert got["n_clusters"] == 2
        _check(got, "lopsided", p, True, se, split)


# ---- 5. by-key forms
@pytest.mark.parametrize("p", [4, 16])
def test_forms_agree(pds, contexts, p):
    import torch

    F, y, off, codes = cc.ragged_frame(p)
    cols = cc.columns(F)
    keys = codes * 7 - 200  # negative, sparse
    for split in ("whole", "cut"):
        ctx = contexts[split]
        base = pds.lin_reg_report(*cols, target=y, add_bias=True, std_err="cluster", cluster_offsets=off, ctx=ctx)
        _same_bits(pds.lin_reg_report(*cols, target=y, add_bias=True, std_err="cluster", cluster_offsets=off, ctx=ctx), base)  # two calls
        _same_bits(pds.lin_reg_report(*cols, target=y, add_bias=True, std_err="cluster", cluster=keys, ctx=ctx), base)  # ordered: nothing moves
        dev = torch.device("cuda", 0)
        tcols = [torch.from_numpy(c).to(dev) for c in cols]
        ty = torch.from_numpy(np.ascontiguousarray(y)).to(dev)
        _same_bits(pds.lin_reg_report(*tcols, target=ty, add_bias=True, std_err="cluster", cluster_offsets=torch.from_numpy(off).to(dev),
                                      ctx=ctx), base)
        _same_bits(pds.lin_reg_report(*tcols, target=ty, add_bias=True, std_err="cluster", cluster=torch.from_numpy(keys).to(dev), ctx=ctx),
                   base)
        # rows shuffled: the stable sort + gather brings them into key order; the offsets form on that frame gives the same bits
        perm = np.random.default_rng(5).permutation(len(y))
        order = perm[np.argsort(keys[perm], kind="stable")]
        ordered = pds.lin_reg_report(*[c[order] for c in cols], target=y[order], add_bias=True, std_err="cluster", cluster_offsets=off, ctx=ctx)
        shuffled = pds.lin_reg_report(*[c[perm] for c in cols], target=y[perm], add_bias=True, std_err="cluster", cluster=keys[perm], ctx=ctx)
        _same_bits(shuffled, ordered)
        _same_bits(pds.lin_reg_report(*[c[perm] for c in cols], target=y[perm], add_bias=True, std_err="cluster", cluster=keys[perm], ctx=ctx),
                   shuffled)
        _check(shuffled, "ragged", p, True, "cluster", "shuffled " + split)
        assert shuffled["n_clusters"] == len(off) - 1


def test_y_var_and_names(pds):
    """`y_var` given is used as given; the other standard errors keep their columns and take no cluster argument."""
    F, y, off, codes = cc.ragged_frame(4)
    cols = cc.columns(F)
    a = pds.lin_reg_report(*cols, target=y, add_bias=True, std_err="cluster0", cluster=codes, feature_names=list("abcd"))
    b = pds.lin_reg_report(*cols, target=y, add_bias=True, std_err="cluster0", cluster=codes, y_var=float(np.var(y, ddof=1)))
    assert a["features"] == ["a", "b", "c", "d", "__bias__"]
    assert list(a) == ["features", "beta", "cluster0_se", "t", "p>|t|", "0.025", "0.975", "r2", "adj_r2", "n_clusters"]
    assert np.array_equal(a["beta"], b["beta"]) and np.array_equal(a["cluster0_se"], b["cluster0_se"])
    assert abs(a["r2"][0] - b["r2"][0]) <= 1e-13
    plain = pds.lin_reg_report(*cols, target=y, add_bias=True, std_err="hc1")
    assert "hc1_se" in plain and "n_clusters" not in plain
    assert np.array_equal(plain["beta"], a["beta"])


# ---- 6. refusals
def test_refusals(pds):
    from polars_ds_extension_amd._lib import PdsError

    F, y, off, codes = cc.ragged_frame(4)
    cols = cc.columns(F)
    kw = dict(target=y, add_bias=True, std_err="cluster")
    with pytest.raises(PdsError, match="at least two non-empty clusters") as e:
        pds.lin_reg_report(*cols, cluster=np.zeros(len(y), dtype=np.int64), **kw)  # G = 1
    assert e.value.code == -1
    with pytest.raises(PdsError, match="at least two non-empty clusters") as e:
        pds.lin_reg_report(*cols, cluster_offsets=np.array([0, 0, len(y)]), **kw)  # one of the two is empty
    assert e.value.code == -1
    with pytest.raises(PdsError, match="up to 16 feature columns") as e:
        pds.lin_reg_report(*[cols[0]] * 17, cluster=codes, **kw)
    assert e.value.code == -5  # PDS_ERR_UNSUPPORTED
    with pytest.raises(PdsError, match="weights are not supported") as e:
        pds.lin_reg_report(*cols, cluster=codes, weights=np.ones(len(y)), **kw)
    assert e.value.code == -5
    with pytest.raises(ValueError, match="exactly one of"):
        pds.lin_reg_report(*cols, cluster=codes, cluster_offsets=off, **kw)
    with pytest.raises(ValueError, match="exactly one of"):
        pds.lin_reg_report(*cols, **kw)
    with pytest.raises(ValueError, match="go with std_err"):
        pds.lin_reg_report(*cols, target=y, add_bias=True, std_err="hc1", cluster=codes)
    bad = off.copy()
    bad[3], bad[4] = off[4], off[3]
    with pytest.raises(PdsError, match="non-decreasing and cover the frame") as e:
        pds.lin_reg_report(*cols, cluster_offsets=bad, **kw)
    assert e.value.code == -1
    with pytest.raises(PdsError, match="non-decreasing and cover the frame") as e:
        pds.lin_reg_report(*cols, cluster_offsets=off[:-1], **kw)  # leaves rows outside every cluster
    assert e.value.code == -1
    with pytest.raises(PdsError, match="No conclusive result") as e:
        pds.lin_reg_report(*[c[:5] for c in cols], target=y[:5], add_bias=True, std_err="cluster", cluster=np.arange(5))  # n = p'
    assert e.value.code == -3  # PDS_ERR_TOO_FEW_ROWS
    # the existing entry points keep refusing the new codes, and a failed call leaves the context usable
    ctx = pds.default_context()
    import ctypes as C

    from polars_ds_extension_amd import _lib
    from polars_ds_extension_amd.lstsq import _Cols

    cs = _Cols(y, cols)
    outs = [np.empty(5) for _ in range(6)]
    rep = _lib.ReportF64(*[C.c_void_p(o.ctypes.data) for o in outs], 0.0, 0.0)
    for code in (5, 6):
        rc = ctx._lib.pds_lin_reg_report_f64(ctx._h, cs.cols, None, 4, C.c_int64(len(y)), cs.space, 1, code, C.c_double(1.0), C.byref(rep))
        assert rc == -1
    assert pds.lin_reg_report(*cols, cluster=codes, **kw)["n_clusters"] == len(off) - 1
