"""lin_reg_report / fixed_effects(absorb=..., cluster_key=) on the MI355X against the NumPy restatement (within_cluster_reference.py): the
truth is its long double run (two absorbed keys: with the tolerance at the long double rounding floor).

Frames.  One absorbed key: 18 groups of 1 .. 1 000 rows (within_cases' sizes around the 64-row step and the split at 128, plus eight
long ones) crossed by a cluster key whose NINE clusters hold exactly 1, 2, 63, 64, 65, 1 023, 1 024, 1 025 and 2 049 rows -- one lane,
the wave boundary, one, two and three chunks with a clamped tail -- at widths 1, 4, 15 and 16, f64 and f32, each on the default context
and on one with "within_split_rows" = 128 (which cuts the factor-1 chunks AND caps a cluster chunk at 128 rows); 12 equal groups crossed
by 2, 3, 4, 5, 8 and 9 clusters (whole and short batches of the four-score outer product); 20 000 groups of two rows crossed by 20 000
two-row clusters (more clusters than waves); within_cases' ragged frame with a cluster key equal to the absorbed key, coarser and
nested (the groups of a cluster not adjacent), crossing, with unused codes between the used ones (C ABI: codes * 2 + 1,
n_levels = 2 n + 3) and one row per cluster, in the offsets form and in the by-key form on shuffled rows.  Two absorbed keys
(within2_cases' ragged and panel frames, absorb_tol = 1e-13, where rounding dominates): clustered on key 2, and on a third column that is
nested over key 1; the grouped two-key symbol once through the C ABI.  Both estimators everywhere; fixed_effects(cluster_key=) once.  Every case is checked in beta, the standard error,
t, p, the interval, df_resid, n_clusters and absorb_nested, and beta, r2, adj_r2, r2_overall, pred, resid, n_iter and the effects must
be the bits of the same call without cluster_key.

Budgets (the project's standing rule, tests/test_within_gpu.py, tests/test_cluster_report_gpu.py).  The device may be at most 10 x as far
from the long double result as the restatement in the frame's own format is on that frame (8 ulp where that distance is below half an
ulp); distance = max |a - b| / max |b| per field.  An f32 frame is compared on the values as stored, its budget made from the
restatement in float32 arithmetic (two keys: run for the float64 run's number of sweeps).  The restatement's distances are measured on
the CPU inside the tests, before anything from the device is asserted, and printed.  p-values and the interval get what the budgets of
t, beta and the standard error let through plus 1e-10 for the special functions.  A frame on which the float64 restatement is more than
1e-6 from long double (a degenerate cluster score block) is not used: the tests assert that on the CPU.

Device against device: two calls give equal bits; the by-key form on shuffled rows gives the bits of the grouped form on the frame
ordered by a stable sort of key 1; cluster_key = the absorbed key gives the df_resid and n_clusters of the existing std_err="cluster"
call and its standard errors within the two calls' summed budgets (the summation order differs); two keys with cluster_key = k2 against
absorb=[k2, k1], std_err="cluster", both at absorb_tol = 1e-12, within the two calls' summed budgets plus the sweeps' distance from the
truth measured for that frame by the restatement at that tolerance -- on the CR0 errors, and on the "cluster" errors once each is
freed of its own (n - 1) / (n - K): the two DEFINITIONS count K = p + G1 + 1 and K = p + 1 + (A - G2), C apart (the header gives the
components to the second key).  A bad code and a key with one cluster in all are PDS_ERR_INVALID, and the context works afterwards.

Measured on the MI355X (worst over widths, both estimators, both split settings and both forms; the restatement's own arithmetic in
the frame's format against long double beside it):
                                                            beta     std_err  t
  cluster sizes 1 .. 2 049, f64                device       6.0e-16  7.2e-15  1.3e-14
                                               restatement  1.3e-15  1.2e-14  6.9e-14
  cluster sizes 1 .. 2 049, f32                device       3.1e-08  4.0e-08  4.8e-08
                                               restatement  6.1e-07  5.8e-06  2.0e-05
  2 .. 9 clusters, f64                         device       3.9e-16  2.2e-14  7.2e-14
                                               restatement  5.1e-16  1.9e-14  7.6e-14
  20 000 two-row clusters, f64                 device       5.4e-16  6.0e-16  4.0e-16
                                               restatement  4.8e-16  6.7e-16  4.8e-16
  ragged, four relations, both forms, f64      device       5.6e-16  1.1e-15  3.3e-15
                                               restatement  1.2e-15  1.9e-15  8.5e-15
  ragged, four relations, both forms, f32      device       3.1e-08  4.6e-08  5.0e-08
                                               restatement  1.8e-07  7.2e-07  2.8e-06
  two keys (1e-13), f64                        device       7.8e-16  8.4e-14  1.0e-13
                                               restatement  5.6e-16  1.3e-13  1.1e-13
  two keys (1e-13), f32                        device       3.3e-08  4.1e-08  3.9e-08
                                               restatement  6.7e-07  5.4e-07  1.0e-06
  (the worst rows are per column, not per case: every case passed its own frame's budget; a distance below half an ulp has the 8-ulp
  budget.)  Every bit-equality held on the first run.  Device against device: cluster_key = the absorbed key against the existing
  std_err="cluster" call 3.5e-17 .. 8.6e-16 (bars 1.6e-14 .. 2.1e-14); cluster_key = k2 against absorb=[k2, k1] at 1e-12: ragged CR0
  6.0e-15 and CR1 free of its factor 6.0e-15 (the sweeps' distance from the truth 2.9e-14), panel 5.0e-13 and 5.0e-13 (9.6e-13).
"""
import ctypes as C
import functools
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT))

import within2_cases as c2  # noqa: E402
import within2_reference as w2r  # noqa: E402
import within_cases as wc  # noqa: E402
import within_cluster_reference as wcr  # noqa: E402
import within_reference as wr  # noqa: E402

pytestmark = pytest.mark.gpu

SE_NAME = {"cluster": "cluster_se", "cluster0": "cluster0_se"}
QUANTILE_TOL = 1e-10  # (tests/test_within_gpu.py: the library's Student t quantile and tail against SciPy's)
TAIL_TOL = 1e-10
DEGENERATE = 1e-6     # a frame on which the float64 restatement is further than this from long double is replaced, not waived
CLUSTER_SIZES = (1, 2, 63, 64, 65, 1023, 1024, 1025, 2049)
GROUP_SIZES = wc.FIXED_SIZES + (700, 737, 500, 500, 400, 300, 200, 100)  # 5 316 rows, as the clusters
FIT_FIELDS = ("beta", "r2", "adj_r2", "r2_overall", "pred", "resid", "n_iter", "effects", "effect_keys", "effects2", "effect_keys2", "component",
              "component2", "n_groups", "n_groups2", "n_components", "features")
TIGHT = c2.TOLS["tight"]


@pytest.fixture(scope="module")
def pds():
    import polars_ds_extension_amd as pds

    return pds


@pytest.fixture(scope="module")
def contexts(pds):
    """the default context, and one whose split threshold cuts every group above 128 rows and caps a cluster chunk at 128 rows"""
    ctxs = {"whole": pds.default_context(), "cut": pds.Context(0)}
    ctxs["cut"].set_option("within_split_rows", 128)
    yield ctxs
    ctxs["cut"].close()


def _np(v):
    return v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)


# ---- frames of this file (seeded; a reference is computed once per frame and arithmetic and never changed)
@functools.lru_cache(maxsize=None)
def sizes_frame(p: int, f32: bool = False):
    """(F, y, offsets, group codes, cluster key): GROUP_SIZES crossed by clusters of exactly CLUSTER_SIZES rows"""
    rng = np.random.default_rng(4100 + p)
    F, y, off, codes = wc._make(rng, GROUP_SIZES, p, f32)
    ck = rng.permutation(np.repeat(np.arange(len(CLUSTER_SIZES)), CLUSTER_SIZES)) * 11 - 40
    assert len(ck) == len(y) and tuple(np.bincount((ck + 40) // 11)) == CLUSTER_SIZES
    return wc._freeze(F, y, off, codes, ck)


def _crossing(n, levels, seed):
    """`levels` clusters, every one occupied, unrelated to the row order"""
    rng = np.random.default_rng(seed)
    return rng.permutation(np.arange(n) % levels) * 3 - 7


def _coarser(k1, seed, levels):
    """a key nested over k1 with `levels` levels: the groups of a cluster are not adjacent"""
    lv = np.unique(np.asarray(k1), return_inverse=True)[1].reshape(-1)
    g = int(lv.max()) + 1
    return (np.random.default_rng(seed).permutation(g) % levels)[lv] + 100


# ---- the restatement, cached per frame and arithmetic
_FITS = {}


def _fitted(name, F, y, absorb, dtype_name, tol=wcr.TRUTH_TOL, sweeps=None):
    key = (name, dtype_name, tol, sweeps)
    if key not in _FITS:
        _FITS[key] = wcr.fit(np.asarray(F, dtype=np.float64), np.asarray(y, dtype=np.float64), absorb, wc.DTYPES[dtype_name], tol, sweeps=sweeps)
    return _FITS[key]


def _refs(name, F, y, absorb, ck, se, fmt, tol=None):
    """(truth, the restatement in the frame's format): one absorbed key -- plain arithmetic; two -- the yardstick of test_within2_gpu.py
    at a tolerance where rounding dominates (float64: its own criterion; float32: the float64 run's number of sweeps)"""
    truth = wcr.report(None, None, None, ck, se, fitted=_fitted(name, F, y, absorb, "longdouble"))
    if tol is None:
        own = _fitted(name, F, y, absorb, fmt)
    else:
        own = _fitted(name, F, y, absorb, "float64", tol)
        if fmt == "float32":
            own = _fitted(name, F, y, absorb, "float32", tol, own["n_iter"])
    return truth, wcr.report(None, None, None, ck, se, fitted=own)


def _check(got, truth, own, se, fmt, what):
    """beta, the standard error, t, p and the interval of a device report against the truth within the budget of its frame; the counts"""
    from scipy import stats as st

    assert np.finfo(np.longdouble).eps < 1e-18  # the reference has to be wider than the arithmetic under test
    dt = wc.DTYPES[fmt]
    eps = float(np.finfo(dt).eps)
    sp = {k: wcr.rel(own[k], truth[k]) for k in wcr.FIELDS}  # measured first, on the CPU
    if fmt == "float64":
        assert max(sp.values()) <= DEGENERATE, (what, sp)  # no degenerate cluster score block
    assert np.all(np.asarray(truth["std_err"], dtype=np.float64) > 0)
    assert (got["df_resid"], got["n_clusters"], tuple(got["absorb_nested"])) == (truth["df_resid"], truth["n_clusters"], tuple(truth["absorb_nested"])), \
        (what, got["df_resid"], got["n_clusters"], got["absorb_nested"], truth["absorb_nested"])
    assert SE_NAME[se] in got and "std_err" not in got and got["beta"].dtype == dt
    vals = {"beta": got["beta"], "std_err": got[SE_NAME[se]], "t": got["t"]}
    dist = {k: wcr.rel(vals[k], truth[k]) for k in wcr.FIELDS}
    print(f"{what} {se} {fmt}: device vs long double { {k: f'{v:.1e}' for k, v in dist.items()} }; restatement {fmt} vs long double "
          f"{ {k: f'{v:.1e}' for k, v in sp.items()} }")
    bud = {k: wcr.budget(sp[k], dt) for k in wcr.FIELDS}
    for k in wcr.FIELDS:
        assert dist[k] <= bud[k], (what, k, dist[k], sp[k])
    t_o = np.asarray(truth["t"], dtype=np.float64)
    dof = truth["t_dof"]
    dt_bound = bud["t"] * np.max(np.abs(t_o))
    p_o = truth["p"]
    # (the density at the near end of what t's budget allows; below the format's smallest normal number a p-value has lost its relative
    # accuracy in either tail function: tests/test_within2_gpu.py)
    dp_bound = 2.0 * st.t.pdf(np.maximum(np.abs(t_o) - dt_bound, 0.0), dof) * dt_bound + (TAIL_TOL + eps) * p_o + float(np.finfo(dt).tiny)
    assert np.all(np.abs(np.asarray(got["p>|t|"], dtype=np.float64) - p_o) <= dp_bound), (what, np.asarray(got["p>|t|"]) - p_o, dp_bound)
    b_o, s_o = np.asarray(truth["beta"], dtype=np.float64), np.asarray(truth["std_err"], dtype=np.float64)
    ci_bound = bud["beta"] * np.max(np.abs(b_o)) + truth["t_crit"] * (bud["std_err"] + QUANTILE_TOL) * np.max(s_o) + eps * np.max(np.abs(truth["ci_hi"]))
    assert np.all(np.abs(np.asarray(got["0.025"], dtype=np.float64) - truth["ci_lo"]) <= ci_bound), what
    assert np.all(np.abs(np.asarray(got["0.975"], dtype=np.float64) - truth["ci_hi"]) <= ci_bound), what
    return dist, bud


def _same_fit(got, base):
    """everything but the errors is what the call without cluster_key returns, bit for bit"""
    assert set(got) - set(base) == {"n_clusters", "absorb_nested"} and set(base) <= set(got)
    for k in base:
        if k not in FIT_FIELDS:
            continue
        if isinstance(base[k], (int, float, list)):
            assert got[k] == base[k], k
        else:
            assert np.array_equal(_np(got[k]), _np(base[k]), equal_nan=True), k


def _same_bits(a, b, skip=()):
    assert a.keys() == b.keys()
    for k in a:
        if k in skip:
            continue
        if isinstance(a[k], (int, float, list, tuple)):
            assert a[k] == b[k], k
        else:
            assert np.array_equal(_np(a[k]), _np(b[k]), equal_nan=True), k


def _run(pds, F, y, se, ctx=None, f32=False, **kw):
    kw.setdefault("return_pred", True)
    pds.config.LIN_REG_EXPR_F64 = not f32
    try:
        return pds.lin_reg_report(*wc.columns(F), target=y, std_err=se, ctx=ctx, **kw)
    finally:
        pds.config.LIN_REG_EXPR_F64 = True


# ---- 1. cluster sizes around the lane, the wave and the chunk
@pytest.mark.parametrize("fmt", ["float64", "float32"])
@pytest.mark.parametrize("p", [1, 4, 15, 16])
def test_cluster_sizes(pds, contexts, p, fmt):
    f32 = fmt == "float32"
    F, y, off, codes, ck = sizes_frame(p, f32)
    name = ("sizes", p, f32)
    for split in ("whole", "cut"):
        for se in wcr.SE_TYPES:
            truth, own = _refs(name, F, y, codes, ck, se, fmt)
            got = _run(pds, F, y, se, ctx=contexts[split], f32=f32, absorb_offsets=off, cluster_key=ck, return_effects=True)
            _check(got, truth, own, se, fmt, f"sizes p={p} {split}")
            assert got["n_clusters"] == 9 and got["absorb_nested"] == (False,)
            _same_fit(got, _run(pds, F, y, se, ctx=contexts[split], f32=f32, absorb_offsets=off, return_effects=True))
        _same_bits(_run(pds, F, y, se, ctx=contexts[split], f32=f32, absorb_offsets=off, cluster_key=ck, return_effects=True), got)  # two calls


# ---- 2. whole and short batches of the four-score outer product; more clusters than waves
@pytest.mark.parametrize("p", [1, 16])
@pytest.mark.parametrize("gc", [2, 3, 4, 5, 8, 9])
def test_cluster_counts(pds, gc, p):
    F, y, off, codes = wc.equal_frame(12, p, 20)
    ck = _crossing(len(y), gc, 50 + gc)
    for se in wcr.SE_TYPES:
        truth, own = _refs(("equal", p), F, y, codes, ck, se, "float64")
        got = _run(pds, F, y, se, absorb_offsets=off, cluster_key=ck)
        _check(got, truth, own, se, "float64", f"equal p={p} Gc={gc}")
        assert got["n_clusters"] == gc and got["df_resid"] == gc - 1
    _same_fit(got, _run(pds, F, y, se, absorb_offsets=off))


@pytest.mark.parametrize("p", [1, 16])
def test_more_clusters_than_waves(pds, p):
    F, y, off, codes = wc.pairs_frame(p)
    n = len(y)
    ck = np.random.default_rng(9).permutation(np.repeat(np.arange(n // 2), 2))  # 20 000 two-row clusters that cross the 20 000 groups
    for se in wcr.SE_TYPES:
        truth, own = _refs(("pairs", p), F, y, codes, ck, se, "float64")
        got = _run(pds, F, y, se, absorb_offsets=off, cluster_key=ck)
        _check(got, truth, own, se, "float64", f"pairs p={p}")
        assert got["n_clusters"] == n // 2 == 20000 and got["absorb_nested"] == (False,)
    _same_fit(got, _run(pds, F, y, se, absorb_offsets=off))


# ---- 3. the relations of the cluster key to the absorbed key; both forms of the one-key pipeline
def _relations(codes, n):
    return {"equal": np.asarray(codes) * 3 + 1, "nested": _coarser(codes, 5, 7), "crossing": _crossing(n, 50, 6),
            "one row per cluster": np.random.default_rng(7).permutation(n)}


@pytest.mark.parametrize("fmt", ["float64", "float32"])
def test_relations_and_forms(pds, contexts, fmt):
    f32 = fmt == "float32"
    kind = "ragged32" if f32 else "ragged"
    p = 4
    F, y, off, codes = wc.frame(kind, p)
    cols, n = wc.columns(F), len(y)
    keys = codes * 7 - 200
    perm = np.random.default_rng(5).permutation(n)
    srt = np.argsort(keys[perm], kind="stable")
    order = perm[srt]  # the frame ordered by a stable sort of key 1, as the by-key form orders it
    inv = np.empty(n, dtype=np.int64)
    inv[srt] = np.arange(n)
    for rel_name, ck in _relations(codes, n).items():
        want_nested = rel_name in ("equal", "nested")
        for split in ("whole", "cut"):
            ctx = contexts[split]
            for se in wcr.SE_TYPES:
                truth, own = _refs((kind, p), F, y, codes, ck, se, fmt)
                got = _run(pds, F, y, se, ctx=ctx, f32=f32, absorb_offsets=off, cluster_key=ck)
                _check(got, truth, own, se, fmt, f"{kind} {rel_name} offsets {split}")
                assert got["absorb_nested"] == (want_nested,)
            _same_fit(got, _run(pds, F, y, se, ctx=ctx, f32=f32, absorb_offsets=off))
            # the by-key form on shuffled rows: the bits of the grouped form on the ordered frame; per-row outputs where the rows are
            shuffled = _run(pds, np.asarray(F)[perm], np.asarray(y)[perm], se, ctx=ctx, f32=f32, absorb=keys[perm], cluster_key=ck[perm])
            on_ordered = _run(pds, np.asarray(F)[order], np.asarray(y)[order], se, ctx=ctx, f32=f32, absorb_offsets=off, cluster_key=ck[order])
            _same_bits(shuffled, on_ordered, skip=("pred", "resid"))
            assert np.array_equal(shuffled["pred"], on_ordered["pred"][inv]) and np.array_equal(shuffled["resid"], on_ordered["resid"][inv])
            _check(shuffled, truth, own, se, fmt, f"{kind} {rel_name} by key, shuffled {split}")
            _same_fit(shuffled, _run(pds, np.asarray(F)[perm], np.asarray(y)[perm], se, ctx=ctx, f32=f32, absorb=keys[perm]))


def test_cuda_tensors(pds):
    import torch

    F, y, off, codes = wc.ragged_frame(4)
    ck = _crossing(len(y), 50, 6)
    dev = torch.device("cuda", 0)
    tcols = [torch.from_numpy(np.array(c)).to(dev) for c in wc.columns(F)]
    ty = torch.from_numpy(np.array(y)).to(dev)
    host = _run(pds, F, y, "cluster", absorb=codes, cluster_key=ck)
    for key in (torch.from_numpy(ck).to(dev), ck, torch.from_numpy(ck.astype(np.int32))):
        got = pds.lin_reg_report(*tcols, target=ty, std_err="cluster", absorb=torch.from_numpy(np.array(codes)).to(dev), cluster_key=key, return_pred=True)
        assert got["pred"].is_cuda
        _same_bits(got, host)


# ---- 4. the relation to the existing call clustered on the absorbed key
@pytest.mark.parametrize("p", [4, 16])
def test_cluster_key_equal_to_the_absorbed_key(pds, contexts, p):
    F, y, off, codes = wc.ragged_frame(p)
    for split in ("whole", "cut"):
        for se in wcr.SE_TYPES:
            truth, own = _refs(("ragged", p), F, y, codes, codes, se, "float64")
            new = _run(pds, F, y, se, ctx=contexts[split], absorb_offsets=off, cluster_key=codes)
            old = _run(pds, F, y, se, ctx=contexts[split], absorb_offsets=off)
            _same_fit(new, old)
            assert new["df_resid"] == old["df_resid"] and new["n_clusters"] == old["n_groups"] and new["absorb_nested"] == (True,)
            bar = wcr.budget(wcr.rel(own["std_err"], truth["std_err"])) + wr.budget(wc.spread("ragged", p, se)["std_err"])
            d = wcr.rel(new[SE_NAME[se]], old[SE_NAME[se]])
            print(f"ragged p={p} {split} {se}: cluster_key = the absorbed key vs the existing call {d:.2e}, bar {bar:.2e}")
            assert d <= bar


# ---- 5. two absorbed keys
TWO_KEY = (("ragged7", 4, "float64"), ("panel", 4, "float64"), ("panel", 16, "float64"), ("ragged300_32", 16, "float32"))


def _run2(pds, F, y, k1, k2, se, ctx=None, f32=False, tol=TIGHT, fx=False, **kw):
    kw.setdefault("return_pred", True)
    pds.config.LIN_REG_EXPR_F64 = not f32
    try:
        fn = pds.fixed_effects if fx else pds.lin_reg_report
        return fn(*c2.columns(F), target=y, absorb=[k1, k2], std_err=se, absorb_tol=tol, ctx=ctx, **kw)
    finally:
        pds.config.LIN_REG_EXPR_F64 = True


@pytest.mark.parametrize("kind,p,fmt", TWO_KEY)
def test_two_keys(pds, contexts, kind, p, fmt):
    f32 = fmt == "float32"
    F, y, off, k1, k2 = c2.frame(kind, p)
    own64 = c2.ref(kind, p, "se", "float64", "tight")
    assert own64["deltas"][-1] <= 0.5 * TIGHT  # the condition on the inputs of test_within2_gpu.py: the stop does not hang on delta's last bits
    for rel_name, ck, nested_want in (("on key 2", np.asarray(k2), (False, True)), ("on a key nested over key 1", _coarser(k1, 8, 9), (True, False))):
        for split in ("whole", "cut"):
            for se in wcr.SE_TYPES:
                truth, own = _refs((kind, p), F, y, (k1, k2), ck, se, fmt, TIGHT)
                got = _run2(pds, F, y, k1, k2, se, ctx=contexts[split], f32=f32, cluster_key=ck)
                _check(got, truth, own, se, fmt, f"{kind} p={p} {rel_name} {split}")
                assert got["absorb_nested"] == nested_want and abs(got["n_iter"] - own64["n_iter"]) <= 1
            _same_fit(got, _run2(pds, F, y, k1, k2, se, ctx=contexts[split], f32=f32))
    _same_bits(_run2(pds, F, y, k1, k2, se, ctx=contexts[split], f32=f32, cluster_key=ck), got)  # two calls


def test_two_keys_by_key_on_shuffled_rows(pds, contexts):
    """the construction of test_within2_accel_gpu.py: the by-key form on shuffled rows against the same call on the frame ordered by a
    stable sort of key 1 (ordered keys move nothing: the grouped form's bits)"""
    F, y, off, k1, k2 = c2.frame("panel", 4)
    F, y, n = np.asarray(F), np.asarray(y), len(y)
    ck = np.asarray(k2)
    perm = np.random.default_rng(5).permutation(n)
    srt = np.argsort(k1[perm], kind="stable")
    order = perm[srt]
    inv = np.empty(n, dtype=np.int64)
    inv[srt] = np.arange(n)
    for split in ("whole", "cut"):
        shuffled = _run2(pds, F[perm], y[perm], k1[perm], k2[perm], "cluster", ctx=contexts[split], cluster_key=ck[perm])
        ordered = _run2(pds, F[order], y[order], k1[order], k2[order], "cluster", ctx=contexts[split], cluster_key=ck[order])
        _same_bits(shuffled, ordered, skip=("pred", "resid"))
        assert np.array_equal(shuffled["pred"], ordered["pred"][inv]) and np.array_equal(shuffled["resid"], ordered["resid"][inv])


def test_fixed_effects_with_a_cluster_key(pds):
    F, y, off, k1, k2 = c2.frame("panel", 4)
    ck = _coarser(k1, 8, 9)
    truth, own = _refs(("panel", 4), F, y, (k1, k2), ck, "cluster", "float64", TIGHT)
    got = _run2(pds, F, y, k1, k2, "cluster", fx=True, cluster_key=ck)
    _check(got, truth, own, "cluster", "float64", "fixed_effects panel p=4")
    base = _run2(pds, F, y, k1, k2, "cluster", fx=True)
    assert "effects" in base and "effects2" in base and "component" in base
    _same_fit(got, base)
    rep = _run2(pds, F, y, k1, k2, "cluster", cluster_key=ck)
    for k in rep:
        assert np.array_equal(_np(rep[k]), _np(got[k])) if hasattr(rep[k], "shape") else rep[k] == got[k], k


@pytest.mark.parametrize("kind,p", [("ragged7", 4), ("panel", 4)])
def test_second_key_against_swapped_keys(pds, kind, p):
    """cluster_key = k2 against absorb=[k2, k1], std_err="cluster", both at absorb_tol = 1e-12.  Bound: the two calls' standing budgets
    plus the sweeps' distance from the truth, measured for this frame by the restatement at the same tolerance in float64.  K differs
    by the definition (see the module's text): the "cluster" errors are compared free of their own (n - 1) / (n - K)."""
    tol = 1e-12
    F, y, off, k1, k2 = c2.frame(kind, p)
    F64, y64, n = np.asarray(F, dtype=np.float64), np.asarray(y, dtype=np.float64), len(y)
    G1, G2, Cc = w2r.components(k1, k2)
    truth_new = wcr.report(None, None, None, k2, "cluster0", fitted=_fitted((kind, p), F, y, (k1, k2), "longdouble"))
    at_tol_new = wcr.report(None, None, None, k2, "cluster0", fitted=_fitted((kind, p), F, y, (k1, k2), "float64", tol))
    truth_old = w2r.report(F64, y64, k2, k1, "cluster0")
    at_tol_old = w2r.report(F64, y64, k2, k1, "cluster0", np.float64, tol)
    sweeps = wcr.rel(at_tol_new["std_err"], truth_new["std_err"]) + wcr.rel(at_tol_old["std_err"], truth_old["std_err"])
    # the standing budget of each call: 10 x the float64 restatement's distance from the truth where rounding dominates (8 ulp at least)
    tight_new = wcr.report(None, None, None, k2, "cluster0", fitted=_fitted((kind, p), F, y, (k1, k2), "float64", TIGHT))
    tight_old = w2r.report(F64, y64, k2, k1, "cluster0", np.float64, TIGHT)
    bar = wcr.budget(wcr.rel(tight_new["std_err"], truth_new["std_err"])) + wcr.budget(wcr.rel(tight_old["std_err"], truth_old["std_err"])) + sweeps
    new0 = _run2(pds, F, y, k1, k2, "cluster0", tol=tol, cluster_key=k2)
    old0 = _run2(pds, F, y, k2, k1, "cluster0", tol=tol)
    new1 = _run2(pds, F, y, k1, k2, "cluster", tol=tol, cluster_key=k2)
    old1 = _run2(pds, F, y, k2, k1, "cluster", tol=tol)
    assert new1["df_resid"] == old1["df_resid"] == G2 - 1 and new1["n_clusters"] == old1["n_groups"] == G2 and new1["absorb_nested"] == (False, True)
    d0 = wcr.rel(new0["cluster0_se"], old0["cluster0_se"])
    k_new, k_old = p + G1 + 1, p + 1 + (G1 - Cc)
    d1 = wcr.rel(new1["cluster_se"] * np.sqrt((n - k_new) / (n - 1.0)), old1["cluster_se"] * np.sqrt((n - k_old) / (n - 1.0)))
    print(f"{kind} p={p}: cluster_key=k2 vs absorb=[k2, k1]: CR0 {d0:.2e}, CR1 free of its factor {d1:.2e}; sweeps' distance from the truth {sweeps:.2e}; bar {bar:.2e}")
    assert d0 <= bar and d1 <= bar


# ---- 6. the C ABI: unused codes; refusals; the context afterwards
def _abi_call(pds, ctx, F, y, off, codes32, n_levels, se_code=5):
    from polars_ds_extension_amd import _lib
    from polars_ds_extension_amd.lstsq import _Cols

    p, n = F.shape[1], len(y)
    cs = _Cols(np.ascontiguousarray(y), wc.columns(F))
    outs = [np.empty(p) for _ in range(6)]
    rep = _lib.ReportF64(*[C.c_void_p(o.ctypes.data) for o in outs], 0.0, 0.0)
    extra = _lib.WithinOut(None, None, None, 0.0, 0, 0)
    o = np.ascontiguousarray(off, dtype=np.int64)
    ck = _lib.ClusterKey(C.c_void_p(codes32.ctypes.data), n_levels, -1, -1, -1)
    rc = ctx._lib.pds_lin_reg_within_cl_grouped_f64(ctx._h, cs.cols, p, C.c_int64(n), C.c_void_p(o.ctypes.data), C.c_int64(len(o) - 1), cs.space, se_code,
                                                    C.byref(rep), C.byref(extra), C.byref(ck))
    return rc, outs, extra, ck


def test_unused_codes_and_refusals(pds):
    from polars_ds_extension_amd import _lib
    from polars_ds_extension_amd._lib import PdsError
    from polars_ds_extension_amd.lstsq import _Cols

    F, y, off, codes = wc.ragged_frame(4)
    F, y, n = np.asarray(F), np.asarray(y), len(y)
    ctx = pds.default_context()
    single = np.random.default_rng(7).permutation(n)  # one row per cluster
    want = _run(pds, F, y, "cluster", absorb_offsets=off, cluster_key=single)
    sparse = np.ascontiguousarray(single * 2 + 1, dtype=np.int32)  # unused codes between the used ones, in front and behind
    rc, outs, extra, ck = _abi_call(pds, ctx, F, y, off, sparse, 2 * n + 3)
    assert rc == 0 and (ck.n_clusters, ck.nested1, ck.nested2, extra.df_resid) == (n, 0, 0, n - 1)
    assert np.array_equal(outs[0], want["beta"]) and np.array_equal(outs[1], want["cluster_se"]) and np.array_equal(outs[3], want["p>|t|"])
    old = _run(pds, F, y, "cluster", absorb_offsets=off)
    # a code outside the range, above and below: PDS_ERR_INVALID, found before anything is indexed by it
    for bad_value in (2 * n + 3, -1, np.iinfo(np.int32).max):
        bad = sparse.copy()
        bad[n // 2] = bad_value
        rc, _, _, _ = _abi_call(pds, ctx, F, y, off, bad, 2 * n + 3)
        assert rc == -1 and b"outside [0, n_levels)" in ctx._lib.pds_last_error()
    # "se" with a cluster key; one cluster in all
    rc, _, _, _ = _abi_call(pds, ctx, F, y, off, sparse, 2 * n + 3, se_code=0)
    assert rc == -1
    rc, _, _, ck1 = _abi_call(pds, ctx, F, y, off, np.full(n, 4, dtype=np.int32), 9)
    assert rc == -1 and ck1.n_clusters == 1 and b"at least two occupied clusters" in ctx._lib.pds_last_error()
    with pytest.raises(PdsError, match="at least two occupied clusters") as e:
        _run(pds, F, y, "cluster0", absorb=codes, cluster_key=np.zeros(n, dtype=np.int64))
    assert e.value.code == -1
    # the context works afterwards: the same bits as before the refusals
    rc, outs2, _, ck2 = _abi_call(pds, ctx, F, y, off, sparse, 2 * n + 3)
    assert rc == 0 and ck2.n_clusters == n and all(np.array_equal(a, b) for a, b in zip(outs, outs2))
    _same_bits(_run(pds, F, y, "cluster", absorb_offsets=off), old)
    # cl == NULL is the existing call
    lib = _lib.load()
    outs3 = [np.empty(4) for _ in range(6)]
    rep = _lib.ReportF64(*[C.c_void_p(o.ctypes.data) for o in outs3], 0.0, 0.0)
    cs = _Cols(np.ascontiguousarray(y), wc.columns(F))
    o = np.ascontiguousarray(off, dtype=np.int64)
    rc = lib.pds_lin_reg_within_cl_grouped_f64(ctx._h, cs.cols, 4, C.c_int64(n), C.c_void_p(o.ctypes.data), C.c_int64(len(o) - 1), cs.space, 5,
                                               C.byref(rep), None, None)
    assert rc == 0 and np.array_equal(outs3[1], old["cluster_se"]) and np.array_equal(outs3[0], old["beta"])


def test_two_key_grouped_entry_point(pds):
    """pds_lin_reg_within2_cl_grouped_f64 with offsets of key 1, dense codes of key 2, fx = NULL and a sparse cluster key: the bits of the
    Python call, which goes through the by-key symbol (ordered keys move nothing)"""
    from polars_ds_extension_amd import _lib
    from polars_ds_extension_amd.lstsq import _Cols

    F, y, off, k1, k2 = c2.frame("ragged7", 4)
    n, p = len(y), 4
    ck = _coarser(k1, 8, 9)
    want = _run2(pds, F, y, k1, k2, "cluster", cluster_key=ck)
    ctx = pds.default_context()
    cs = _Cols(np.ascontiguousarray(y), c2.columns(F))
    outs = [np.empty(p) for _ in range(6)]
    rep = _lib.ReportF64(*[C.c_void_p(o.ctypes.data) for o in outs], 0.0, 0.0)
    pred, resid = np.empty(n), np.empty(n)
    extra = _lib.Within2Out(C.c_void_p(pred.ctypes.data), C.c_void_p(resid.ctypes.data), 0.0, 0, 0, 0, 0, 0)
    o = np.ascontiguousarray(off, dtype=np.int64)
    codes2 = np.ascontiguousarray(np.unique(k2, return_inverse=True)[1].reshape(-1), dtype=np.int32)
    codes_c = np.ascontiguousarray(np.unique(ck, return_inverse=True)[1].reshape(-1) * 3 + 2, dtype=np.int32)  # unused codes around the used ones
    key = _lib.ClusterKey(C.c_void_p(codes_c.ctypes.data), 3 * 9 + 5, -1, -1, -1)
    rc = ctx._lib.pds_lin_reg_within2_cl_grouped_f64(ctx._h, cs.cols, p, C.c_int64(n), C.c_void_p(o.ctypes.data), C.c_int64(len(o) - 1),
                                                     C.c_void_p(codes2.ctypes.data), C.c_int64(int(codes2.max()) + 1), cs.space, 5, C.c_double(TIGHT), 10_000,
                                                     C.byref(rep), C.byref(extra), None, C.byref(key))
    assert rc == 0, ctx._lib.pds_last_error()
    assert (key.n_clusters, key.nested1, key.nested2, extra.df_resid, extra.n_iter) == (9, 1, 0, 8, want["n_iter"])
    for a, b in zip(outs, ("beta", "cluster_se", "t", "p>|t|", "0.025", "0.975")):
        assert np.array_equal(a, want[b]), b
    assert np.array_equal(pred, want["pred"]) and np.array_equal(resid, want["resid"]) and extra.r2_overall == want["r2_overall"]


def test_names_and_fields(pds):
    F, y, off, codes = wc.ragged_frame(4)
    ck = _crossing(len(y), 50, 6)
    a = pds.lin_reg_report(*wc.columns(F), target=y, absorb=codes, std_err="cluster0", cluster_key=ck, feature_names=list("abcd"))
    assert list(a) == ["features", "beta", "cluster0_se", "t", "p>|t|", "0.025", "0.975", "r2", "adj_r2", "r2_overall", "n_groups", "df_resid",
                       "n_clusters", "absorb_nested"]
    assert (a["n_groups"], a["n_clusters"], a["df_resid"], a["absorb_nested"]) == (60, 50, 49, (False,))
