"""glm_report(absorb= | absorb_offsets=) on the MI355X against the NumPy restatement (glm_within_reference.py) in long double.

Frames: tests/glm_within_cases.py -- 14 ragged groups at every edge of the 4-row instruction, the 64-row step and the 128-row
residency, integer weights 0 .. 3, an offset, the four families at widths 1, 7 and 16, each on the default context and on one with
"within_split_rows" = 64, which cuts the 65 .. 200-row groups into chunks.

Budgets are measured, not fixed (the project's rule, glm_sandwich_reference.budget): a field may be 64 x as far from the long double
result as the reference's own arithmetic in the frame's format is on that frame (the factor for fields through the device's exp / log),
8 ulp where that distance is below half an ulp.  Distance = max |a - b| / max |b| per field (cov: on the correlation scale).  beta and
alpha are measured against the long double maximum-likelihood fit of the dummy design, the report fields against the reference at the
DEVICE's beta and alpha.  The device runs to tol = 1e-14 (f64 frames): the last step is then below the rounding the budgets measure,
so the "last W_xx" of the definition is the W_xx at the returned coefficients.  Every test prints its figures before it asserts.

Measured on the MI355X (worst over families, widths, the three `std_err` and both split settings; the reference's own arithmetic in
the frame's format against long double beside it):
                          beta     alpha    std_err  deviance chi2     pred     cov
  f64 frames  device      1.6e-15  4.8e-16  4.1e-15  1.3e-16  1.3e-16  7.8e-16  1.3e-14
              reference   3.6e-15  2.8e-15  1.3e-15  1.4e-16  1.6e-16  2.7e-16  4.0e-15
  f32 frames  device      4.4e-08  5.2e-08  5.0e-07  5.1e-08  7.0e-08  6.3e-08  1.3e-06
              reference   1.5e-06  9.3e-07  7.1e-07  7.8e-08  9.9e-08  2.5e-07  2.2e-06
  (worst rows are per column, not per case; the largest error / spread of any case was 6.5, the budget factor is 64.)  The first run
  missed two checks, both mended in the test's own set-up and not by a wider tolerance: the poisson device-against-device case ran at
  tol 1e-13, where the one-step-older W_xx is 2.2e-13 from the information at beta (now 1e-14, as everywhere here), and an f32
  p-value of 2e-80 is stored as 0 (the absolute floor of the p check is the format's smallest normal number).
"""
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT))

import glm_report_reference as rr  # noqa: E402
import glm_sandwich_reference as sr  # noqa: E402
import glm_within_cases as wc  # noqa: E402
import glm_within_reference as wr  # noqa: E402

pytestmark = pytest.mark.gpu

KINDS = ("se", "cluster", "cluster0")
TOL = {np.float64: 1e-14, np.float32: 1e-6}
LIN_SE = {"se": "std_err", "cluster": "cluster_se", "cluster0": "cluster0_se"}
ERR = {"invalid": -1, "too_few": -3, "unsupported": -5, "numeric": -6}
_CACHE = {}


@pytest.fixture(scope="module")
def pds():
    import polars_ds_extension_amd as pds

    return pds


@pytest.fixture(scope="module")
def contexts(pds):
    """the default context, and one whose split threshold cuts every group above 64 rows"""
    ctxs = {"whole": pds.default_context(), "cut": pds.Context(0)}
    ctxs["cut"].set_option("within_split_rows", 64)
    yield ctxs
    ctxs["cut"].close()


def dist(a, ref):
    """max |a - ref| / max |ref| over the finite entries of ref"""
    a, ref = np.asarray(a).astype(np.longdouble), np.asarray(ref).astype(np.longdouble)
    m = np.isfinite(ref)
    if not m.any():
        return 0.0
    return float(np.max(np.abs(a[m] - ref[m])) / max(float(np.max(np.abs(ref[m]))), 1e-300))


def stored(f, dtype):
    """the frame as the device sees it: its values rounded to the frame's type"""
    return {k: (v.astype(dtype).astype(np.float64) if k in ("X", "y", "pw", "o") else v) for k, v in f.items()}


def refs(family, p, dtype=np.float64):
    """computed once per frame and left unchanged: the stored frame, the long double dummy MLE, the narrow fit of the definition"""
    key = (family, p, dtype)
    if key not in _CACHE:
        f = stored(wc.frame(family, p), dtype)
        ml = wr.dummy_mle(f["X"], f["y"], f["codes"], family, f["pw"], f["o"])
        lo = wr.fit(f["X"], f["y"], f["codes"], family, f["pw"], f["o"], tol=TOL[dtype], dtype=dtype)
        _CACHE[key] = (f, ml, lo)
    return _CACHE[key]


def cols(X):
    return [np.ascontiguousarray(X[:, j]) for j in range(X.shape[1])]


def run(pds, f, family, kind, dtype=np.float64, ctx=None, by="offsets", weights=True, offset=True, **kw):
    kw.setdefault("return_effects", True)
    kw.setdefault("return_pred", True)
    kw.setdefault("return_cov", True)
    kw.setdefault("tol", TOL[dtype])
    groups = {"absorb_offsets": f["off"]} if by == "offsets" else {"absorb": f["codes"]}
    pds.config.LIN_REG_EXPR_F64 = dtype == np.float64
    try:
        return pds.glm_report(*cols(f["X"]), target=f["y"], family=family, std_err=kind, ctx=ctx, weights=f["pw"] if weights else None,
                              offset=f["o"] if offset else None, **groups, **kw)
    finally:
        pds.config.LIN_REG_EXPR_F64 = True


def np_(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


def check(d, f, ml, lo, family, p, kind, dtype, what):
    """every field of a device report within the measured budget of its frame"""
    assert np.finfo(np.longdouble).eps < 1e-18  # the reference has to be wider than the arithmetic under test
    eps = float(np.finfo(dtype).eps)
    beta, alpha, pred = np_(d["beta"]), np_(d["effects"]), np_(d["pred"])
    assert beta.dtype == dtype and alpha.dtype == dtype and pred.dtype == dtype
    assert d["converged"] and 2 <= d["n_iter"] <= 12, d["n_iter"]
    # ---- counts: exact
    assert d["n_groups_dropped"] == wc.DROPPED[(family, p)] == int(ml["drop"].sum())
    assert d["n_groups"] == len(wc.SIZES) - d["n_groups_dropped"]
    assert d["n_rows_used"] == int(ml["used"].sum())
    assert d["df_resid"] == d["n_rows_used"] - d["n_groups"] - p
    assert d["std_err_type"] == kind and d["n_clusters"] == (0 if kind == "se" else d["n_groups"])
    assert np.array_equal(np.isnan(alpha), ml["drop"])
    assert np.array_equal(np.isnan(pred), ml["drop"][f["codes"]]), "pred is NaN exactly on the rows of dropped groups"
    assert np.array_equal(np_(d["effect_keys"]), np.arange(len(wc.SIZES)))
    # ---- beta and alpha against the long double dummy MLE
    out = {"beta": (dist(beta, ml["beta"]), dist(lo["beta"], ml["beta"])), "alpha": (dist(alpha, ml["alpha"]), dist(lo["alpha"], ml["alpha"]))}
    # ---- the report at the device's coefficients
    hi = wr.report_at(f["X"], f["y"], f["codes"], family, beta, alpha, kind, f["pw"], f["o"])
    nr = wr.report_at(f["X"], f["y"], f["codes"], family, beta, alpha, kind, f["pw"], f["o"], dtype=dtype)
    assert np.isfinite(hi["std_err"].astype(np.float64)).all(), f"{what}: the reference is not finite"
    for k in ("std_err", "deviance", "pearson_chi2", "dispersion", "pred"):
        out[k] = (dist(np_(d[k]), hi[k]), dist(nr[k], hi[k]))
    out["cov"] = (rr.cov_err(np_(d["cov"])[None], hi["cov"][None]), rr.cov_err(nr["cov"][None], hi["cov"][None]))
    worst = max(err / max(spread, 0.5 * eps) for err, spread in out.values())
    print(f"{what}: worst error / spread {worst:.3g}  " + "  ".join(f"{k} {e:.2g}/{s:.2g}" for k, (e, s) in out.items()))
    for k, (err, spread) in out.items():
        assert err <= sr.budget(spread, dtype), f"{what}: {k} error {err:.3g} above the budget {sr.budget(spread, dtype):.3g} (spread {spread:.3g})"
    # ---- z, p and the interval follow from beta and the standard error
    se_budget = sr.budget(out["std_err"][1], dtype) + sr.budget(out["beta"][1], dtype) + 2 * eps
    z = np_(d["z"]).astype(np.float64)
    assert dist(z, hi["z"]) <= se_budget, f"{what}: z"
    # (a p below the format's normal range is stored with fewer digits, and as 0 below its range: 2e-80 in an f32 report)
    np.testing.assert_allclose(np_(d["p>|z|"]).astype(np.float64), rr._erfc(np.abs(z) / np.sqrt(2.0)), rtol=64 * eps,
                               atol=float(np.finfo(dtype).smallest_normal))
    scale = float(np.max(np.abs(hi["hi"]).astype(np.float64)))
    for k, r in (("0.025", "lo"), ("0.975", "hi")):
        assert float(np.max(np.abs(np_(d[k]).astype(np.longdouble) - hi[r]))) <= (se_budget + 2 * eps) * scale, f"{what}: {k}"
    assert np.isnan(d["null_deviance"]) and d["report_null"] == 0
    return out


# ------------------------------------------------------------------------------------------------- 1. the ragged frame
@pytest.mark.parametrize("split", ["whole", "cut"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("p", wc.WIDTHS)
@pytest.mark.parametrize("family", wc.FAMILIES)
def test_ragged_frame(pds, contexts, family, p, kind, split):
    f, ml, lo = refs(family, p)
    d = run(pds, f, family, kind, ctx=contexts[split])
    check(d, f, ml, lo, family, p, kind, np.float64, f"{family} p={p} {kind} {split}")


# ------------------------------------------------------------------------------------------------- 2. optimality
def _optimality(f, family, beta, alpha):
    """max_j |sum_i r_i x_ij| / sum_i |r_i x_ij| and max_g |sum_{i in g} r_i| / sum_i |r_i| at (beta, alpha), in long double"""
    rep = wr.report_at(f["X"], f["y"], f["codes"], family, beta, alpha, "se", f["pw"], f["o"])
    sx, r, g = rep["score_x"], rep["score_r"], rep["g_used"]
    by_feature = float(np.max(np.abs(sx.sum(axis=0)) / np.abs(sx).sum(axis=0)))
    sums = np.zeros(int(g.max()) + 1, dtype=np.longdouble)
    np.add.at(sums, g, r)
    return by_feature, float(np.max(np.abs(sums)) / np.abs(r).sum())


@pytest.mark.parametrize("split", ["whole", "cut"])
@pytest.mark.parametrize("p", wc.WIDTHS)
@pytest.mark.parametrize("family", wc.FAMILIES)
def test_optimality_at_the_device_output(pds, contexts, family, p, split):
    f, ml, lo = refs(family, p)
    d = run(pds, f, family, "se", ctx=contexts[split])
    got = _optimality(f, family, np_(d["beta"]), np_(d["effects"]))
    own = _optimality(f, family, lo["beta"], lo["alpha"])  # the float64 restatement's own residual scores
    print(f"{family} p={p} {split}: score sums by feature {got[0]:.2g} (reference {own[0]:.2g}), by group {got[1]:.2g} (reference {own[1]:.2g})")
    for err, spread in zip(got, own):
        assert err <= sr.budget(spread, np.float64)


# ------------------------------------------------------------------------------------------------- 3. device against device
def _small_frame(family, seed=77):
    """12 groups, 3 features, positive weights (no group is dropped by the weights): the dummy design has 15 columns"""
    rng = np.random.default_rng(seed)
    sizes = (5, 9, 70, 130, 20, 33, 3, 64, 12, 7, 40, 15)
    G, n = len(sizes), sum(sizes)
    codes = np.repeat(np.arange(G, dtype=np.int64), sizes)
    X = rng.standard_normal((n, 3))
    beta = np.array([0.4, -0.3, 0.2])
    alpha = 0.5 * rng.standard_normal(G)
    eta = X @ beta + 0.2 + alpha[codes]
    y = eta + rng.standard_normal(n) if family == "gaussian" else rng.poisson(np.exp(eta)).astype(np.float64)
    D = (codes[:, None] == np.arange(G)[None, :]).astype(np.float64)
    return {"X": X, "y": y, "pw": rng.integers(1, 4, n).astype(np.float64), "o": np.zeros(n), "codes": codes, "D": D,
            "off": np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)}


def _route_budgets(f, family, weights):
    """the budget of each route against the long double MLE, from the float64 restatement of that route"""
    pw = f["pw"] if weights else None
    ml = wr.dummy_mle(f["X"], f["y"], f["codes"], family, pw, None)
    lo_w = wr.fit(f["X"], f["y"], f["codes"], family, pw, None, tol=1e-14, dtype=np.float64)
    lo_d = wr.dummy_mle(f["X"], f["y"], f["codes"], family, pw, None, dtype=np.float64)
    return sr.budget(dist(lo_w["beta"], ml["beta"])) + sr.budget(dist(lo_d["beta"], ml["beta"]))


def test_gaussian_weighted_against_lin_reg_report_on_dummies(pds):
    f = _small_frame("gaussian")
    d = run(pds, f, "gaussian", "se", offset=False)
    lin = pds.lin_reg_report(*cols(f["X"]), *cols(f["D"][:, 1:]), target=f["y"], add_bias=True, weights=f["pw"])
    bar = _route_budgets(f, "gaussian", True)
    eb, es = dist(np_(d["beta"]), np_(lin["beta"])[:3]), dist(np_(d["std_err"]), np_(lin["std_err"])[:3])
    print(f"gaussian with weights vs lin_reg_report on features + dummies + bias: beta {eb:.3g} std_err {es:.3g} (bar {bar:.3g})")
    assert d["n_iter"] == 2 and d["converged"]  # (the gaussian working response does not depend on the start: the second step moves nothing)
    assert eb <= bar and es <= bar


@pytest.mark.parametrize("kind", KINDS)
def test_gaussian_unweighted_against_lin_reg_report_absorb(pds, kind):
    f = _small_frame("gaussian")
    d = run(pds, f, "gaussian", kind, weights=False, offset=False)
    lin = pds.lin_reg_report(*cols(f["X"]), target=f["y"], absorb_offsets=f["off"], std_err=kind, return_effects=True, return_pred=True)
    bar = _route_budgets(f, "gaussian", False)
    errs = {"beta": dist(np_(d["beta"]), np_(lin["beta"])), "std_err": dist(np_(d["std_err"]), np_(lin[LIN_SE[kind]])),
            "effects": dist(np_(d["effects"]), np_(lin["effects"])), "pred": dist(np_(d["pred"]), np_(lin["pred"]))}
    print(f"gaussian without weights vs lin_reg_report(absorb=) {kind}: " + "  ".join(f"{k} {v:.3g}" for k, v in errs.items()) + f" (bar {bar:.3g})")
    assert d["n_groups"] == lin["n_groups"]
    for k, v in errs.items():
        assert v <= bar, k


def test_poisson_against_glm_report_on_dummies(pds):
    f = _small_frame("poisson")
    # (tol = 1e-14 as everywhere in this file: glm_report forms its information AT its coefficients, the fixed-effects report at the
    # last iteration's weights -- one step earlier, a step that has to be below the rounding the bar measures.  The standard error,
    # the deviance and chi2 are smooth in (beta, alpha) with a relative sensitivity of order one on this frame: the bar of the
    # coefficients serves them too.)
    d = run(pds, f, "poisson", "se", offset=False)
    full = pds.glm_report(*cols(f["X"]), *cols(f["D"]), target=f["y"], family="poisson", weights=f["pw"], tol=1e-13, max_iter=100)
    bar = _route_budgets(f, "poisson", True)
    errs = {"beta": dist(np_(d["beta"]), np_(full["beta"])[:3]), "effects": dist(np_(d["effects"]), np_(full["beta"])[3:]),
            "std_err": dist(np_(d["std_err"]), np_(full["std_err"])[:3]), "deviance": dist(d["deviance"], full["deviance"]),
            "pearson_chi2": dist(d["pearson_chi2"], full["pearson_chi2"])}
    print("poisson vs glm_report on features + dummies: " + "  ".join(f"{k} {v:.3g}" for k, v in errs.items()) + f" (bar {bar:.3g})")
    assert d["df_resid"] == int(full["df_resid"]) and d["n_groups_dropped"] == 0
    for k, v in errs.items():
        assert v <= bar, k


# ------------------------------------------------------------------------------------------------- 4. f32 frame and report
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("p", wc.WIDTHS)
@pytest.mark.parametrize("family", wc.FAMILIES)
def test_f32_frame(pds, family, p, kind):
    f, ml, lo = refs(family, p, np.float32)
    f32 = {k: (v.astype(np.float32) if k in ("X", "y", "pw", "o") else v) for k, v in f.items()}
    d = run(pds, f32, family, kind, dtype=np.float32)
    check(d, f, ml, lo, family, p, kind, np.float32, f"f32 {family} p={p} {kind}")


# ------------------------------------------------------------------------------------------------- 5 .. 9. the same bits
BIT_FIELDS = ("beta", "std_err", "z", "p>|z|", "0.025", "0.975", "cov", "deviance", "pearson_chi2", "dispersion", "effects", "pred")


def same_bits(a, b, what, fields=BIT_FIELDS):
    for k in fields:
        x, y = np_(a[k]), np_(b[k])
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), f"{what}: {k} differs"
    for k in ("n_groups", "n_groups_dropped", "n_rows_used", "df_resid", "n_iter", "converged"):
        assert a[k] == b[k], f"{what}: {k}"


def _torch_frame(f):
    import torch

    t = {k: torch.as_tensor(v).cuda() for k, v in f.items() if k != "beta" and k != "alpha"}
    return t


def trun(pds, t, family, kind, by="offsets", ctx=None, **kw):
    groups = {"absorb_offsets": t["off"]} if by == "offsets" else {"absorb": t["codes"]}
    return pds.glm_report(*[t["X"][:, j].contiguous() for j in range(t["X"].shape[1])], target=t["y"], family=family, std_err=kind, ctx=ctx,
                          weights=t["pw"], offset=t["o"], return_effects=True, return_pred=True, return_cov=True, tol=1e-14, **groups, **kw)


@pytest.mark.parametrize("family,p", [("poisson", 7), ("binomial", 16)])
def test_host_frame_gives_the_device_frame_bits(pds, contexts, family, p):
    f, _, _ = refs(family, p)
    for split in ("whole", "cut"):
        host = run(pds, f, family, "cluster", ctx=contexts[split])
        dev = trun(pds, _torch_frame(f), family, "cluster", ctx=contexts[split])
        assert isinstance(host["pred"], np.ndarray) and dev["pred"].is_cuda and dev["effects"].is_cuda
        same_bits(host, dev, f"{family} p={p} {split}: host against device frame")


@pytest.mark.parametrize("family,p", [("poisson", 7), ("binomial", 1), ("gamma", 16)])
def test_by_key(pds, contexts, family, p):
    import torch

    f, _, _ = refs(family, p)
    want = run(pds, f, family, "cluster")
    # ordered keys: the bits of the offsets form; the keys negative and sparse
    keys = -1000 + 37 * f["codes"]
    got = run(pds, dict(f, codes=keys), family, "cluster", by="key")
    same_bits(want, got, "ordered keys")
    assert np.array_equal(np_(got["effect_keys"]), -1000 + 37 * np.arange(len(wc.SIZES)))
    # shuffled rows: the bits of the offsets form on the key-ordered frame (a stable order), per-row outputs in frame order
    perm = np.random.default_rng(5).permutation(len(keys))
    sh = {k: (v[perm] if k in ("X", "y", "pw", "o") else v) for k, v in f.items()}
    sh["codes"] = keys[perm]
    order = np.argsort(sh["codes"], kind="stable")
    ordered = {k: (v[order] if k in ("X", "y", "pw", "o") else v) for k, v in sh.items()}
    ordered["off"] = f["off"]
    for split in ("whole", "cut"):
        want_o = run(pds, ordered, family, "cluster", ctx=contexts[split])
        got_s = run(pds, sh, family, "cluster", by="key", ctx=contexts[split])
        same_bits(want_o, got_s, f"shuffled keys {split}", fields=[k for k in BIT_FIELDS if k != "pred"])
        assert np_(got_s["pred"])[order].tobytes() == np_(want_o["pred"]).tobytes(), "pred comes back in frame order"
        # CUDA tensors, the key among them
        t = _torch_frame(sh)
        got_t = trun(pds, t, family, "cluster", by="key", ctx=contexts[split])
        assert got_t["pred"].is_cuda and torch.equal(got_t["effect_keys"].cpu(), torch.as_tensor(np_(got_s["effect_keys"])))
        same_bits(got_s, got_t, f"CUDA tensors {split}")


def test_empty_groups_change_no_bit(pds, contexts):
    f, _, _ = refs("poisson", 7)
    off = f["off"]
    wide = np.concatenate([[0, 0], off[:5], [off[4]] * 3, off[5:], [off[-1]] * 2]).astype(np.int64)
    at = np.flatnonzero(np.diff(wide) > 0)
    for split in ("whole", "cut"):
        for kind in ("se", "cluster"):
            want = run(pds, f, "poisson", kind, ctx=contexts[split])
            got = run(pds, dict(f, off=wide), "poisson", kind, ctx=contexts[split])
            same_bits(want, got, f"empty groups {split} {kind}", fields=[k for k in BIT_FIELDS if k != "effects"])
            eff = np_(got["effects"])
            assert len(eff) == len(wide) - 1 and eff[at].tobytes() == np_(want["effects"]).tobytes()
            empty = np.ones(len(eff), dtype=bool)
            empty[at] = False
            assert np.isnan(eff[empty]).all()


@pytest.mark.parametrize("family", wc.FAMILIES)
def test_unit_weights_and_zero_offset_are_the_plain_call(pds, contexts, family):
    f, _, _ = refs(family, 7)
    one = dict(f, pw=np.ones_like(f["pw"]), o=np.zeros_like(f["o"]))
    for split in ("whole", "cut"):
        plain = run(pds, one, family, "cluster", ctx=contexts[split], weights=False, offset=False)
        both = run(pds, one, family, "cluster", ctx=contexts[split])
        same_bits(plain, both, f"{family} {split}: unit weights and a zero offset")
        same_bits(plain, run(pds, one, family, "cluster", ctx=contexts[split], offset=False), f"{family} {split}: unit weights")


@pytest.mark.parametrize("family,p", [("poisson", 16), ("gamma", 7)])
def test_two_calls_give_equal_bits(pds, contexts, family, p):
    f, _, _ = refs(family, p)
    for split in ("whole", "cut"):
        for by in ("offsets", "key"):
            a = run(pds, f, family, "cluster", ctx=contexts[split], by=by)
            b = run(pds, f, family, "cluster", ctx=contexts[split], by=by)
            same_bits(a, b, f"{family} p={p} {split} {by}: two calls")


# ------------------------------------------------------------------------------------------------- 10. refusals
def test_refusals_leave_the_context_usable(pds):
    f, ml, lo = refs("poisson", 7)
    ctx = pds.Context(0)
    try:
        from polars_ds_extension_amd._lib import PdsError

        def refused(code, match, frame, kind="se", **kw):
            with pytest.raises(PdsError, match=match) as e:
                run(pds, frame, "poisson", kind, ctx=ctx, **kw)
            assert e.value.code == ERR[code], (e.value.code, str(e.value))

        # a feature that is constant inside every group: refused by its index
        X = f["X"].copy()
        X[:, 4] = f["codes"] * 0.25
        refused("numeric", "feature column 4 is constant inside every group", dict(f, X=X))
        # df_resid <= 0: two groups of two counting rows and seven features
        small = {k: (v[5:9] if k in ("X", "y", "pw", "o") else v) for k, v in f.items()}
        small.update(off=np.array([0, 2, 4]), codes=np.array([0, 0, 1, 1]), pw=np.ones(4), y=np.array([1.0, 2.0, 0.0, 3.0]))
        refused("too_few", "No conclusive result", small)
        # one kept group with a cluster kind
        refused("invalid", "at least two kept groups", dict(f, off=np.array([0, wc.N_ROWS])), kind="cluster")
        # a negative weight
        pw = f["pw"].copy()
        pw[100] = -1.0
        refused("invalid", "a weight is negative or not finite", dict(f, pw=pw))
        # 17 features
        refused("unsupported", "up to 16 feature columns", dict(f, X=np.tile(f["X"], (1, 3))[:, :17]))
        # ... and the context still answers, with the bits of a fresh call
        same_bits(run(pds, f, "poisson", "cluster", ctx=ctx), run(pds, f, "poisson", "cluster"), "after the refusals")
    finally:
        ctx.close()
