"""
Robust and cluster-robust standard errors of the one-model GLM report on the device (lstsq.glm_report(std_err="hc0" | "hc1" |
"cluster" | "cluster0"): pds_glm_report_robust_* / _cluster_grouped_* / _cluster_by_key_*, csrc/glm_meat.hip) against the NumPy
restatement of tests/glm_sandwich_reference.py.

The budget is MEASURED, not fixed in advance: the device's std_err and cov are compared, at the DEVICE's coefficients, with the
longdouble restatement; the bound is 64 x the float64 (f32 frames: float32) restatement's own distance from the longdouble one on the
same frame -- the factor test_glm_weighted_report_gpu.check_budget uses for fields that pass through the device's exp / log -- and
8 ulp where that distance is below half an ulp of the format (the floor of cluster_reference.budget).  cov is compared on the
correlation scale (glm_report_reference.cov_err); z, p and the interval follow from the std_err budget as in check_budget.  Every
test prints its worst error / spread.  Frames: tests/glm_sandwich_cases.py.
"""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import cluster_reference as cr  # noqa: E402
import glm_cases as gc  # noqa: E402
import glm_report_reference as rr  # noqa: E402
import glm_sandwich_cases as sc  # noqa: E402
import glm_sandwich_reference as sr  # noqa: E402
import glm_weighted_cases as wc  # noqa: E402
from test_glm_weighted_gpu import cols_of, dev, np_, pds  # noqa: E402,F401  (pds: the fixture)

pytestmark = pytest.mark.gpu

TOL, MAX_ITER = sc.TOL, sc.MAX_ITER
FIELDS = ("beta", "std_err", "z", "p>|z|", "0.025", "0.975", "cov", "deviance", "null_deviance", "pearson_chi2", "dispersion", "df_resid",
          "n_iter", "report_null", "n_clusters")
FIT_FIELDS = ("beta", "n_iter", "deviance", "null_deviance", "dispersion", "df_resid")


def report(pds, X, y, family, bias, kind, off=None, codes=None, pw=None, o=None, space="device", ctx=None, tol=TOL):
    put = dev if space == "device" else (lambda a: a)
    d = pds.glm_report(*cols_of(X, space), target=put(y), family=family, add_bias=bias, tol=tol, max_iter=MAX_ITER, std_err=kind,
                       cluster=None if codes is None else put(codes), cluster_offsets=None if off is None else put(off),
                       weights=None if pw is None else put(pw), offset=None if o is None else put(o), return_cov=True, ctx=ctx)
    return {k: (v if isinstance(v, (list, str, int)) else np_(v)) for k, v in d.items()}


def same_bits(a, b, what, fields=FIELDS):
    for k in fields:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True), f"{what}: {k} differs"


def check(d, X, y, family, bias, kind, codes, pw, o, what, dtype=np.float64):
    """the device's fields against the longdouble restatement at the device's own coefficients; returns the std_err budget"""
    assert d["report_null"] == 0 and d["n_iter"] < MAX_ITER, f"{what}: null report or no convergence"
    if dtype == np.float32:  # (the device saw the f32-rounded frame)
        X, y = X.astype(np.float32), y.astype(np.float32)
        pw = None if pw is None else pw.astype(np.float32)
        o = None if o is None else o.astype(np.float32)
    beta = d["beta"].astype(np.float64)
    with np.errstate(all="ignore"):
        hi = sr.report(X, y, beta, family, bias, kind, codes, pw, o)
        lo = sr.report(X, y, beta, family, bias, kind, codes, pw, o, dtype=dtype)
    assert np.isfinite(hi["std_err"].astype(np.float64)).all(), f"{what}: the reference is not finite"
    out = {"std_err": (rr.rel_err(d["std_err"], hi["std_err"]), rr.rel_err(lo["std_err"], hi["std_err"])),
           "cov": (rr.cov_err(d["cov"][None], hi["cov"][None]), rr.cov_err(lo["cov"][None], hi["cov"][None]))}
    worst = max(err / max(spread, 0.5 * float(np.finfo(dtype).eps)) for err, spread in out.values())
    print(f"{what}: worst error / spread {worst:.3g}  " + "  ".join(f"{k} {e:.2g}/{s:.2g}" for k, (e, s) in out.items()))
    for k, (err, spread) in out.items():
        assert err <= sr.budget(spread, dtype), f"{what}: {k} error {err:.3g} above the budget {sr.budget(spread, dtype):.3g} (spread {spread:.3g})"
    assert d["n_clusters"] == hi["n_clusters"], f"{what}: n_clusters {d['n_clusters']} != {hi['n_clusters']}"
    assert d["df_resid"] == hi["df_resid"], f"{what}: df_resid"
    se_budget = sr.budget(out["std_err"][1], dtype) + 2 * float(np.finfo(dtype).eps)  # (and the rounding of the quotient itself)
    z_ref, p_ref = hi["z"].astype(np.float64), hi["p"]
    assert rr.rel_err(d["z"], hi["z"]) <= se_budget, f"{what}: z"
    floor = 1e-300 if dtype == np.float64 else float(np.finfo(dtype).smallest_subnormal)  # (a p the format cannot store is stored as 0)
    assert (np.abs(d["p>|z|"] - p_ref) <= (1.0 + z_ref * z_ref) * se_budget * p_ref + floor).all(), f"{what}: p"
    scale = np.abs(beta) + np.abs(hi["std_err"].astype(np.float64))
    for k, r in (("0.025", "lo"), ("0.975", "hi")):
        assert (np.abs(d[k] - hi[r].astype(np.float64)) <= se_budget * scale).all(), f"{what}: {k}"
    return se_budget


def kind_args(kind, off, codes, form="offsets"):
    if kind in sr.CLUSTER_KINDS:
        return {"off": off} if form == "offsets" else {"codes": codes}
    return {}


# ------------------------------------------------------------------------------------------------------------ 1. the ragged frame
@pytest.mark.parametrize("kind", sc.KINDS)
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("p", sc.WIDTHS)
@pytest.mark.parametrize("family", gc.FAMILIES)
def test_ragged_frame(pds, family, p, bias, kind):
    X, y, off, codes, pw, o = sc.ragged(family, p)
    d = report(pds, X, y, family, bias, kind, pw=pw, o=o, **kind_args(kind, off, codes))
    check(d, X, y, family, bias, kind, codes, pw, o, f"ragged {family} p={p} bias={bias} {kind}")
    if kind in sr.CLUSTER_KINDS:
        assert d["n_clusters"] == (9 if pw[0] == 0 else 10)  # (p = 16, gamma: the one-row cluster has weight 0)


@pytest.mark.parametrize("kind", sc.KINDS)
@pytest.mark.parametrize("p", sc.WIDTHS)
def test_ragged_frame_f32(pds, p, kind):
    X, y, off, codes, pw, o = sc.ragged("poisson", p)
    pds.config.LIN_REG_EXPR_F64 = False
    try:
        d = report(pds, X, y, "poisson", True, kind, pw=pw, o=o, tol=1e-6, **kind_args(kind, off, codes))
    finally:
        pds.config.LIN_REG_EXPR_F64 = True
    assert d["std_err"].dtype == np.float32
    check(d, X, y, "poisson", True, kind, codes, pw, o, f"ragged f32 poisson p={p} {kind}", dtype=np.float32)


@pytest.mark.parametrize("kind", sc.KINDS)
@pytest.mark.parametrize("p", sc.WIDTHS)
def test_ragged_frame_host(pds, p, kind):
    X, y, off, codes, pw, o = sc.ragged("binomial", p)
    d = report(pds, X, y, "binomial", True, kind, pw=pw, o=o, space="host", **kind_args(kind, off, codes))
    assert isinstance(d["std_err"], np.ndarray)
    check(d, X, y, "binomial", True, kind, codes, pw, o, f"ragged host binomial p={p} {kind}")


# ------------------------------------------------------------------------------------------------------------ 2. park batches
@pytest.mark.parametrize("kind", sr.CLUSTER_KINDS)
@pytest.mark.parametrize("G", [2, 3, 4, 5, 8, 9])
def test_park_batches(pds, G, kind):
    rng = np.random.default_rng(900 + G)
    X, y = sc.plain_frame(rng, "poisson", 5 * G, 3)
    off = gc.offsets([5] * G)
    d = report(pds, X, y, "poisson", True, kind, off=off, ctx=one_wave(pds))  # (one wave: all the clusters through ONE park)
    check(d, X, y, "poisson", True, kind, sc.codes_of(off), None, None, f"park G={G} {kind}")
    assert d["n_clusters"] == G


_CTX = {}


def ctx_with(pds, **options):
    """a context of its own per option set (module lifetime)"""
    key = tuple(sorted(options.items()))
    if key not in _CTX:
        _CTX[key] = pds.Context(0)
        for k, v in options.items():
            _CTX[key].set_option(k, v)
    return _CTX[key]


def one_wave(pds):
    return ctx_with(pds, cluster_waves=1)


# ------------------------------------------------------------------------------------------------------------ 3. long clusters
@pytest.mark.parametrize("kind", sr.CLUSTER_KINDS)
@pytest.mark.parametrize("family", ["binomial", "gamma"])
def test_long_cluster_split(pds, family, kind):
    X, y, off, codes = sc.lopsided(family, 5)
    whole = report(pds, X, y, family, True, kind, off=off)
    cut = report(pds, X, y, family, True, kind, off=off, ctx=ctx_with(pds, cluster_split_rows=64))
    check(cut, X, y, family, True, kind, codes, None, None, f"long cluster {family} {kind} split 64")
    assert cut["n_clusters"] == whole["n_clusters"] == len(off) - 1
    diff = rr.rel_err(cut["std_err"], whole["std_err"])
    print(f"long cluster {family} {kind}: split 64 vs default {diff:.3g}")
    assert diff <= 1e-12
    same_bits(cut, whole, "long cluster: the fit", FIT_FIELDS)


def test_long_cluster_zero_weight_count(pds):
    """a long cluster whose rows all have weight 0 is cut into chunks and still not counted"""
    X, y, off, codes = sc.lopsided("poisson", 3)
    pw = np.ones(len(y))
    pw[off[3]:off[4]] = 0.0  # (the 500-row cluster)
    d = report(pds, X, y, "poisson", True, "cluster", off=off, pw=pw, ctx=ctx_with(pds, cluster_split_rows=64))
    check(d, X, y, "poisson", True, "cluster", codes, pw, None, "long cluster of weight 0")
    assert d["n_clusters"] == len(off) - 2


# ------------------------------------------------------------------------------------------------------------ 4. HC row ranges
@pytest.mark.parametrize("kind", ["hc0", "hc1"])
@pytest.mark.parametrize("n", [6, 63, 64, 65, 257, 4097])
def test_hc_row_ranges(pds, n, kind):
    p = 4  # with the bias p' = 5: n = 6 is p' + 1
    rng = np.random.default_rng(4000 + n)
    family = "gaussian" if n == 6 else "poisson"  # (six rows: a family whose fit exists whatever the draw)
    X, y = sc.plain_frame(rng, family, n, p)
    d = report(pds, X, y, family, True, kind)
    check(d, X, y, family, True, kind, None, None, None, f"hc rows n={n} {kind}")
    assert d["n_clusters"] == 0
    if n == 4097:
        for waves in (1, 3):
            dw = report(pds, X, y, family, True, kind, ctx=ctx_with(pds, cluster_waves=waves))
            check(dw, X, y, family, True, kind, None, None, None, f"hc rows n={n} {kind} waves={waves}")
            diff = rr.rel_err(dw["std_err"], d["std_err"])
            print(f"hc rows n={n} {kind}: {waves} wave(s) vs default {diff:.3g}")
            assert diff <= 1e-12


# ------------------------------------------------------------------------------------------------------------ 5. forms
@pytest.mark.parametrize("kind", sr.CLUSTER_KINDS)
def test_forms_equal_bits(pds, kind):
    X, y, off, codes, pw, o = sc.ragged("poisson", 7)
    a = report(pds, X, y, "poisson", True, kind, off=off, pw=pw, o=o)
    same_bits(a, report(pds, X, y, "poisson", True, kind, off=off, pw=pw, o=o), "the same call twice")
    same_bits(a, report(pds, X, y, "poisson", True, kind, codes=codes * 3 + 11, pw=pw, o=o), "offsets vs ordered keys")
    same_bits(a, report(pds, X, y, "poisson", True, kind, off=off, pw=pw, o=o, space="host"), "device vs host frame")
    same_bits(a, report(pds, X, y, "poisson", True, kind, codes=codes, pw=pw, o=o, space="host"), "device offsets vs host keys")
    empty = np.concatenate([[0, 0], off[1:4], [off[3], off[3]], off[4:], [off[-1]]]).astype(np.int64)
    same_bits(a, report(pds, X, y, "poisson", True, kind, off=empty, pw=pw, o=o), "empty clusters in the offsets")
    perm = np.random.default_rng(5).permutation(len(y))
    s = report(pds, X[perm], y[perm], "poisson", True, kind, codes=codes[perm], pw=pw[perm], o=o[perm])
    diff = rr.rel_err(s["std_err"], a["std_err"])
    print(f"forms {kind}: shuffled rows vs ordered {diff:.3g}")
    assert diff <= 1e-9 and s["n_clusters"] == a["n_clusters"] and s["df_resid"] == a["df_resid"]


@pytest.mark.parametrize("kind", ["hc0", "hc1"])
def test_forms_equal_bits_hc(pds, kind):
    X, y, off, codes, pw, o = sc.ragged("binomial", 7)
    a = report(pds, X, y, "binomial", True, kind, pw=pw, o=o)
    same_bits(a, report(pds, X, y, "binomial", True, kind, pw=pw, o=o), "the same call twice")
    same_bits(a, report(pds, X, y, "binomial", True, kind, pw=pw, o=o, space="host"), "device vs host frame")


# ------------------------------------------------------------------------------------------------------------ 6. fit identity
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("kind", sc.KINDS)
@pytest.mark.parametrize("family", gc.FAMILIES)
def test_fit_identity(pds, family, kind, weighted):
    X, y, off, codes, pw, o = sc.ragged(family, 7)
    if not weighted:
        pw = o = None
    d = report(pds, X, y, family, True, kind, pw=pw, o=o, **kind_args(kind, off, codes))
    put = lambda a: None if a is None else dev(a)  # noqa: E731
    g = pds.glm_report_by(*cols_of(X, "device"), target=dev(y), group_offsets=dev(np.array([0, len(y)], dtype=np.int64)), family=family,
                          add_bias=True, tol=TOL, max_iter=MAX_ITER, weights=put(pw), offset=put(o))
    for k in FIT_FIELDS:
        assert np.array_equal(np.asarray(d[k]), np_(g[k])[0], equal_nan=True), f"{family} {kind} weighted={weighted}: {k} differs from glm_report_by"


# ------------------------------------------------------------------------------------------------------------ 7. weights
@pytest.mark.parametrize("kind", sc.KINDS)
def test_zero_weight_cluster_appended(pds, kind):
    X, y, off, codes, pw, o = sc.ragged("poisson", 7)
    rng = np.random.default_rng(7)
    k = 70
    X2 = np.concatenate([X, rng.normal(size=(k, X.shape[1]))])
    y2 = np.concatenate([y, rng.poisson(3.0, size=k).astype(np.float64)])
    pw2, o2 = np.concatenate([pw, np.zeros(k)]), np.concatenate([o, rng.uniform(-1, 1, size=k)])
    off2 = np.concatenate([off, [off[-1] + k]]).astype(np.int64)
    codes2 = sc.codes_of(off2)
    a = report(pds, X, y, "poisson", True, kind, pw=pw, o=o, **kind_args(kind, off, codes))
    b = report(pds, X2, y2, "poisson", True, kind, pw=pw2, o=o2, **kind_args(kind, off2, codes2))
    ba = check(a, X, y, "poisson", True, kind, codes, pw, o, f"zero-weight cluster {kind}: without")
    bb = check(b, X2, y2, "poisson", True, kind, codes2, pw2, o2, f"zero-weight cluster {kind}: with")
    assert b["n_clusters"] == a["n_clusters"] and b["df_resid"] == a["df_resid"]
    diff = rr.rel_err(b["std_err"], a["std_err"])
    print(f"zero-weight cluster {kind}: with vs without {diff:.3g}")
    assert diff <= ba + bb  # (the two budgets: rows of weight 0 reach no sum of the fit or of the meat)


@pytest.mark.parametrize("family", gc.FAMILIES)
def test_integer_weights_are_replication(pds, family):
    """cluster sums are linear in the weights (the HC meats are not, and are not compared): the replicate test's yardstick, 100 x tol"""
    X, y, off, codes, pw, o = sc.ragged(family, 7)
    Xr, yr, offr, orep = wc.replicate(X, y, off, pw, o)
    a = report(pds, X, y, family, True, "cluster0", off=off, pw=pw, o=o)
    b = report(pds, Xr, yr, family, True, "cluster0", off=offr, o=orep)
    diff = rr.rel_err(a["std_err"], b["std_err"])
    print(f"integer weights {family}: weighted vs replicated {diff:.3g}")
    assert diff <= 100 * TOL
    assert a["n_clusters"] == b["n_clusters"]  # (n, and df_resid with it, counts rows: the replicated frame has more)


# ------------------------------------------------------------------------------------------------------------ 8. gaussian = linear
@pytest.mark.parametrize("kind", sr.CLUSTER_KINDS)
@pytest.mark.parametrize("p", sc.WIDTHS)
def test_gaussian_is_the_linear_cluster_report(pds, p, kind):
    X, y, off, codes, _, _ = sc.ragged("gaussian", p, weighted=False)
    d = report(pds, X, y, "gaussian", True, kind, off=off)
    b_glm = check(d, X, y, "gaussian", True, kind, codes, None, None, f"gaussian p={p} {kind}")
    lin = pds.lin_reg_report(*cols_of(X, "device"), target=dev(y), add_bias=True, std_err=kind, cluster_offsets=dev(off))
    se_lin = np_(lin[f"{kind}_se"])
    Z = np.concatenate([X, np.ones((len(X), 1))], axis=1)
    hi, lo = cr.report(Z, y, codes, kind), cr.report(Z, y, codes, kind, dtype=np.float64)
    b_lin = cr.budget(cr.rel(lo["std_err"], hi["std_err"]))
    diff = rr.rel_err(d["std_err"], se_lin)
    print(f"gaussian p={p} {kind}: GLM route vs lin_reg_report {diff:.3g} (budgets {b_glm:.3g} + {b_lin:.3g})")
    assert diff <= b_glm + b_lin
    assert d["n_clusters"] == lin["n_clusters"]


# ------------------------------------------------------------------------------------------------------------ 10. refusals
def raw_call(pds, X, y, se_code, off=None):
    """the C entry points with any se_type / width (lstsq.glm_report refuses these before the library is asked)"""
    from polars_ds_extension_amd import _lib, lstsq

    cols = lstsq._Cols(y, [np.ascontiguousarray(X[:, j]) for j in range(X.shape[1])])
    ctx = lstsq.default_context()
    outs, rep = lstsq._glm_report_outs(cols, 1, X.shape[1] + 1, False)
    ng = C.c_int64(0)
    tail = (cols.space, 1, C.c_int(1), C.c_int(1), C.c_double(TOL), C.c_int(MAX_ITER), C.c_int(se_code), outs["beta"][1], outs["n_iter"][1],
            C.byref(rep), C.byref(ng))
    if off is None:
        rc = ctx.fn("pds_glm_report_robust")(ctx._h, cols.cols, None, None, cols.n_feat, C.c_int64(cols.n_rows), *tail)
    else:
        rc = ctx.fn("pds_glm_report_cluster_grouped")(ctx._h, cols.cols, None, None, cols.n_feat, C.c_int64(cols.n_rows),
                                                      C.c_void_p(off.ctypes.data), C.c_int64(len(off) - 1), *tail)
    return rc, _lib.load().pds_last_error().decode()


def test_refusals(pds):
    from polars_ds_extension_amd._lib import PdsError

    rng = np.random.default_rng(10)
    X, y = sc.plain_frame(rng, "poisson", 40, 17)
    off = gc.offsets([10, 10, 20])
    codes = sc.codes_of(off)
    # more than 16 features
    rc, msg = raw_call(pds, X, y, 1)
    assert rc == -5 and "up to 16 feature columns" in msg
    rc, msg = raw_call(pds, X, y, 5, off)
    assert rc == -5 and "up to 16 feature columns" in msg
    with pytest.raises(NotImplementedError, match="16 feature"):
        pds.glm_report(*cols_of(X, "host"), target=y, family="poisson", std_err="hc0")
    X = np.ascontiguousarray(X[:, :3])
    # HC2 / HC3: unsupported; any other se_type: invalid
    for code in (3, 4):
        for o_ in (None, off):
            rc, msg = raw_call(pds, X, y, code, o_)
            assert rc == -5 and "HC2 / HC3" in msg
    for code, o_ in ((0, None), (5, None), (6, None), (7, None), (0, off), (1, off), (2, off), (-1, off)):
        rc, msg = raw_call(pds, X, y, code, o_)
        assert rc == -1 and "se_type is" in msg, (code, msg)
    with pytest.raises(NotImplementedError, match="leverages"):
        pds.glm_report(*cols_of(X, "host"), target=y, family="poisson", std_err="hc3")
    with pytest.raises(ValueError, match="not one of"):
        pds.glm_report(*cols_of(X, "host"), target=y, family="poisson", std_err="robust")
    # a cluster form with G < 2: one cluster, and two of which one has no row of positive weight
    for kind in sr.CLUSTER_KINDS:
        with pytest.raises(PdsError, match="at least two non-empty clusters") as e:
            report(pds, X, y, "poisson", True, kind, off=np.array([0, 0, 40, 40], dtype=np.int64))
        assert e.value.code == -1
        pw = np.ones(40)
        pw[:20] = 0.0
        with pytest.raises(PdsError, match="at least two non-empty clusters") as e:
            report(pds, X, y, "poisson", True, kind, codes=np.repeat([4, 9], 20), pw=pw)
        assert e.value.code == -1
    # offsets that do not cover the frame
    with pytest.raises(PdsError, match="cover the frame") as e:
        report(pds, X, y, "poisson", True, "cluster", off=np.array([0, 10, 30], dtype=np.int64))
    assert e.value.code == -1
    # hc1 / cluster with n <= p': by the rows, and by the rows of positive weight
    for kind in ("hc1", "cluster"):
        ka = kind_args(kind, np.array([0, 2, 4], dtype=np.int64), None)
        with pytest.raises(PdsError, match="#Data <= #features") as e:
            report(pds, X[:4], y[:4], "poisson", True, kind, **ka)
        assert e.value.code == -3
        pw = np.zeros(40)
        pw[[0, 11, 25, 39]] = 1.0
        with pytest.raises(PdsError, match="#Data <= #features") as e:
            report(pds, X, y, "poisson", True, kind, pw=pw, **kind_args(kind, off, codes))
        assert e.value.code == -3
    # the argument rules of the clusters
    with pytest.raises(ValueError, match="exactly one of"):
        pds.glm_report(*cols_of(X, "host"), target=y, family="poisson", std_err="cluster")
    with pytest.raises(ValueError, match="exactly one of"):
        pds.glm_report(*cols_of(X, "host"), target=y, family="poisson", std_err="cluster0", cluster=codes, cluster_offsets=off)
    for kind in ("se", "hc0", "hc1"):
        with pytest.raises(ValueError, match="go with std_err"):
            pds.glm_report(*cols_of(X, "host"), target=y, family="poisson", std_err=kind, cluster=codes)


def test_null_fit_has_a_null_report(pds):
    """an all-zero feature column: I has no inverse -- every report field is NaN except df_resid / n_clusters, report_null = 1"""
    rng = np.random.default_rng(11)
    X, y = sc.plain_frame(rng, "poisson", 60, 3)
    X[:, 1] = 0.0
    off = gc.offsets([20, 20, 20])
    for kind in sc.KINDS:
        d = report(pds, X, y, "poisson", True, kind, **kind_args(kind, off, None))
        assert d["report_null"] == 1 and d["df_resid"] == 60 - 4 and "is_null" not in d  # (one flag on the robust route)
        for k in ("std_err", "z", "p>|z|", "0.025", "0.975", "cov", "deviance", "null_deviance", "pearson_chi2", "dispersion"):
            assert np.isnan(d[k]).all(), (kind, k)
        assert d["n_clusters"] == (3 if kind in sr.CLUSTER_KINDS else 0)


def test_se_routes_to_glm_report_by(pds):
    X, y, off, codes, pw, o = sc.ragged("gamma", 7)
    d = report(pds, X, y, "gamma", True, "se", pw=pw, o=o)
    g = pds.glm_report_by(*cols_of(X, "device"), target=dev(y), group_offsets=dev(np.array([0, len(y)], dtype=np.int64)), family="gamma",
                          add_bias=True, tol=TOL, max_iter=MAX_ITER, weights=dev(pw), offset=dev(o), return_cov=True)
    for k in ("beta", "std_err", "z", "p>|z|", "0.025", "0.975", "cov", "deviance", "dispersion", "df_resid", "n_iter"):
        assert np.array_equal(np.asarray(d[k]), np_(g[k])[0], equal_nan=True), k
    assert d["std_err_type"] == "se" and d["n_clusters"] == 0 and d["std_err"].shape == (8,)
    assert d["is_null"] == 0 and d["report_null"] == 0  # ("se": the fit's own flag too)
