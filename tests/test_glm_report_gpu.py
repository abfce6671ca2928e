"""
The grouped GLM report on the device (lstsq.glm_report_by / glm_report_by_key: pds_glm_report_grouped_* / _by_key_*,
csrc/grouped_glm_report.hip) against tests/glm_report_reference.py.

Frames (tests/glm_cases.family_frame with ragged_sizes, default_rng(7)): 150 groups of 4 (p + 1) .. 400 rows, the four families x
widths {1, 8, 16} x bias on / off, tol 1e-10.  On the CPU (float64 restatement at longdouble Newton coefficients) none of the 24
configurations has a null or non-converged group, cond(X'WX) <= 53 except gamma (1.2e3 at p = 16 with a bias), and the float64
restatement is within 3.1e-15 of the longdouble one (gamma: 7.2e-14 in se, 1.4e-13 in cov).

Budget of the accuracy tests: per configuration and quantity 64 x the distance between the float64 and the longdouble restatement
on the same frame at the same coefficients (64: the different summation order of the matrix instructions over up to 400 rows); the
tests print spread and error before they assert.  The covariance matrices are compared on the correlation scale
(glm_report_reference.cov_err).  A test that may skip groups asserts that it skips at most 2 % of them.

Measured on an MI355X: the largest error-to-spread ratio of any configuration and quantity is 7.6 (null_deviance,
the device's closed form against the restatement's direct sum), 5.7 for se / cov, against the budget's 64; se at the independent
longdouble Newton fit <= 3.3e-14 relative (bound 1e-8).
"""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import glm_cases as gc  # noqa: E402
import glm_report_reference as rr  # noqa: E402

pytestmark = pytest.mark.gpu

G = 150
TOL, MAX_ITER = 1e-10, 100
WIDTHS = (1, 8, 16)
CONFIGS = [(f, p, b) for f in gc.FAMILIES for p in WIDTHS for b in (True, False)]
COEF = ("std_err", "z", "p>|z|", "0.025", "0.975")
GROUP = ("deviance", "null_deviance", "pearson_chi2", "dispersion")
REF_NAME = {"std_err": "std_err", "z": "z", "p>|z|": "p", "0.025": "lo", "0.975": "hi"}


@pytest.fixture(scope="module")
def pds():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import polars_ds_extension_amd as m

    return m


def dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def np_(v):
    return v.cpu().numpy() if hasattr(v, "cpu") else (v if isinstance(v, list) else np.asarray(v))


def cols_of(X, space):
    cs = [np.ascontiguousarray(X[:, j]) for j in range(X.shape[1])]
    return [dev(c) for c in cs] if space == "device" else cs


def report_by(pds, X, y, off, family, bias, space="device", tol=TOL, ctx=None, cov=True):
    put = dev if space == "device" else (lambda a: a)
    r = pds.glm_report_by(*cols_of(X, space), target=put(y), group_offsets=put(off), family=family, add_bias=bias, tol=tol,
                          max_iter=MAX_ITER, return_cov=cov, ctx=ctx)
    return {k: np_(v) for k, v in r.items()}


def report_by_key(pds, X, y, key, family, bias, space="device"):
    put = dev if space == "device" else (lambda a: a)
    r = pds.glm_report_by_key(*cols_of(X, space), target=put(y), key=put(key), family=family, add_bias=bias, tol=TOL, max_iter=MAX_ITER,
                              return_cov=True)
    return {k: np_(v) for k, v in r.items()}


_FRAMES, _DEVICE = {}, {}


def config_frame(family, p):
    if (family, p) not in _FRAMES:
        rng = np.random.default_rng(7)
        sizes = gc.ragged_sizes(rng, G, p)
        _FRAMES[family, p] = gc.family_frame(rng, family, sizes, p)
    return _FRAMES[family, p]


def device_report(pds, family, p, bias):
    """the device's report of a configuration, computed once and left unchanged"""
    if (family, p, bias) not in _DEVICE:
        X, y, off = config_frame(family, p)
        _DEVICE[family, p, bias] = report_by(pds, X, y, off, family, bias)
    return _DEVICE[family, p, bias]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def usable_groups(d, what, cap=0.02):
    """groups the accuracy tests look at: fitted, converged, reported; at most `cap` of the groups may be left out"""
    ok = (d["is_null"] == 0) & (d["report_null"] == 0) & (d["n_iter"] < MAX_ITER)
    left = int((~ok).sum())
    assert left <= cap * len(ok), f"{what}: {left} of {len(ok)} groups are null or did not converge"
    return ok


def check_budget(d, X, y, off, family, bias, what, factor=64.0, ok=None):
    """(a): the device's fields against the longdouble restatement at the device's own coefficients, budget = factor x the float64
    restatement's distance from it.  Returns {quantity: (error, spread)}."""
    ok = usable_groups(d, what) if ok is None else ok
    beta = d["beta"].astype(np.float64)
    with np.errstate(all="ignore"):
        hi = rr.report_by(X, y, off, beta, family, bias, skip=~ok)
        lo = rr.report_by(X, y, off, beta, family, bias, dtype=np.float64, skip=~ok)
    assert np.isfinite(hi["std_err"][ok].astype(np.float64)).all(), f"{what}: the reference is not finite on a group the device reported"
    out = {}
    for k in ("std_err", *GROUP):
        out[k] = (rr.rel_err(d[k][ok], hi[REF_NAME.get(k, k)][ok]), rr.rel_err(lo[REF_NAME.get(k, k)][ok], hi[REF_NAME.get(k, k)][ok]))
    diag = np.arange(beta.shape[1])
    out["cov_diag"] = (rr.rel_err(d["cov"][ok][:, diag, diag], hi["cov"][ok][:, diag, diag]),
                       rr.rel_err(lo["cov"][ok][:, diag, diag], hi["cov"][ok][:, diag, diag]))
    out["cov"] = (rr.cov_err(d["cov"][ok], hi["cov"][ok]), rr.cov_err(lo["cov"][ok], hi["cov"][ok]))
    for k, (err, spread) in out.items():
        print(f"{what}: {k:14s} error {err:.3g}  spread {spread:.3g}  budget {factor * spread:.3g}")
    for k, (err, spread) in out.items():
        assert err <= factor * spread, f"{what}: {k} error {err:.3g} above {factor:g} x spread {spread:.3g}"
    # where the reference has NaN (gamma's null deviance without a bias) so has the device
    for k in GROUP:
        assert np.array_equal(np.isnan(d[k][ok]), np.isnan(hi[k][ok].astype(np.float64))), f"{what}: NaN pattern of {k}"
    # z follows from se; p: d ln p ~ z dz
    se_budget = factor * out["std_err"][1]
    z_ref, p_ref = hi["z"][ok].astype(np.float64), hi["p"][ok]
    assert rr.rel_err(d["z"][ok], hi["z"][ok]) <= se_budget + 4e-16, f"{what}: z"
    assert (np.abs(d["p>|z|"][ok] - p_ref) <= (1.0 + z_ref * z_ref) * (se_budget + 4e-16) * p_ref + 1e-300).all(), f"{what}: p"
    scale = np.abs(d["beta"][ok]) + np.abs(hi["std_err"][ok].astype(np.float64))
    for k in ("0.025", "0.975"):
        assert (np.abs(d[k][ok] - hi[REF_NAME[k]][ok].astype(np.float64)) <= (se_budget + 4e-16) * scale).all(), f"{what}: {k}"
    assert np.array_equal(d["df_resid"], hi["df_resid"])
    return out


@pytest.mark.parametrize("family,p,bias", CONFIGS)
def test_accuracy_at_the_devices_coefficients(pds, family, p, bias):
    """(a)"""
    X, y, off = config_frame(family, p)
    d = device_report(pds, family, p, bias)
    assert d["features"] == [f"x{i + 1}" for i in range(p)] + (["__bias__"] if bias else [])
    assert d["cov"].shape == (G, p + int(bias), p + int(bias)) and d["df_resid"].dtype == np.int64
    check_budget(d, X, y, off, family, bias, f"{family} p={p} bias={bias}")


@pytest.mark.parametrize("family,p,bias", CONFIGS)
def test_standard_errors_at_the_mle(pds, family, p, bias):
    """(b): se within 100 tol (relative) of the longdouble report at an independent longdouble Newton fit converged to 1e-15 -- W
    depends on beta through eta with |x| = O(1), and the device's coefficients are within tol of the MLE after a quadratically
    convergent last step."""
    X, y, off = config_frame(family, p)
    d = device_report(pds, family, p, bias)
    ok = usable_groups(d, f"mle {family} p={p} bias={bias}")
    worst = 0.0
    for g in np.nonzero(ok)[0]:
        a, e = int(off[g]), int(off[g + 1])
        with np.errstate(all="ignore"):
            b = rr.newton_fit(X[a:e], y[a:e], family, bias)
            ref = rr.report_group(X[a:e], y[a:e], b, family, bias)
        assert np.isfinite(ref["std_err"].astype(np.float64)).all()
        worst = max(worst, rr.rel_err(d["std_err"][g], ref["std_err"]))
    print(f"mle {family} p={p} bias={bias}: worst relative se error {worst:.3g} (bound {100 * TOL:.3g})")
    assert worst <= 100 * TOL


@pytest.mark.parametrize("family,p,bias", CONFIGS)
def test_fit_outputs_are_those_of_glm_by(pds, family, p, bias):
    """(c)"""
    X, y, off = config_frame(family, p)
    d = device_report(pds, family, p, bias)
    co, it, nu = (np_(v) for v in pds.glm_by(*cols_of(X, "device"), target=dev(y), group_offsets=dev(off), family=family, add_bias=bias,
                                              tol=TOL, max_iter=MAX_ITER))
    assert same_bits(d["beta"], co) and same_bits(d["n_iter"], it) and same_bits(d["is_null"], nu)


def edge_frame(family, p, bias):
    """(d): one frame with groups of n in {p' - 1, p', p' + 1, 63, 64, 65, 127, 128, 129, 257} rows"""
    pp = p + int(bias)
    sizes = np.array([pp - 1, pp, pp + 1, 63, 64, 65, 127, 128, 129, 257])
    rng = np.random.default_rng(11)
    return (*gc.family_frame(rng, family, sizes, p), sizes)


@pytest.mark.parametrize("family", gc.FAMILIES)
@pytest.mark.parametrize("p,bias", [(1, True), (8, False), (16, True)])
def test_edge_sizes(pds, family, p, bias):
    """(d)"""
    X, y, off, sizes = edge_frame(family, p, bias)
    pp = p + int(bias)
    d = report_by(pds, X, y, off, family, bias)
    what = f"edge {family} p={p} bias={bias}"
    fields = (*COEF, *GROUP)
    # n < p': null fit, null report, everything NaN
    assert d["is_null"][0] == 1 and d["report_null"][0] == 1
    assert all(np.isnan(d[k][0]).all() for k in (*fields, "cov", "beta"))
    assert set(np.unique(d["report_null"])) <= {0, 1}
    assert np.array_equal(d["df_resid"], sizes - pp)
    # n = p'
    if family in ("gaussian", "gamma"):  # (the longdouble fit of these groups is finite: checked on the CPU)
        assert d["is_null"][1] == 0 and d["report_null"][1] == 0
        assert all(np.isnan(d[k][1]).all() for k in (*COEF, "dispersion", "cov"))
        assert np.isfinite(d["deviance"][1]) and np.isfinite(d["pearson_chi2"][1])
    elif d["report_null"][1] == 0:
        assert np.isfinite(d["std_err"][1]).all() and np.isfinite(d["deviance"][1])
    # n > p': the groups the device reports are within the budget of (a), on inputs for which the reference itself is finite
    ok = (d["is_null"] == 0) & (d["report_null"] == 0) & (d["n_iter"] < MAX_ITER) & (sizes > pp)
    with np.errstate(all="ignore"):
        ref = rr.report_by(X, y, off, np.where(np.isfinite(d["beta"]), d["beta"], 0.0), family, bias, skip=~ok)
    ok &= np.isfinite(ref["std_err"].astype(np.float64)).all(axis=1)
    assert ok[3:].all(), f"{what}: the groups of 63 rows and more are all reported: {ok}"
    check_budget(d, X, y, off, family, bias, what, ok=ok)


def long_frame(family, p):
    rng = np.random.default_rng(13)
    sizes = np.concatenate([rng.integers(100, 1101, size=28), [300, 301, 1100]])
    return (*gc.family_frame(rng, family, sizes, p), sizes)


@pytest.mark.parametrize("family,p,bias", [("binomial", 8, True), ("poisson", 16, True), ("gamma", 4, True), ("gaussian", 16, False),
                                           ("gaussian", 3, True)])
def test_pieces_of_long_groups(pds, family, p, bias):
    """(e): glm_split_rows = 300 on groups of 100 .. 1 100 rows: the pieced groups stay within the budget of (a), the others keep
    their bits, two calls are bit-identical"""
    X, y, off, sizes = long_frame(family, p)
    ctx = pds.Context()
    ctx.set_option("glm_split_rows", 300)
    assert (sizes > 300).sum() >= 9 and (sizes <= 300).sum() >= 3
    d1 = report_by(pds, X, y, off, family, bias, ctx=ctx)
    d2 = report_by(pds, X, y, off, family, bias, ctx=ctx)
    for k in (*COEF, *GROUP, "cov", "beta", "n_iter", "is_null", "report_null", "df_resid"):
        assert same_bits(d1[k], d2[k]), k
    check_budget(d1, X, y, off, family, bias, f"pieces {family} p={p} bias={bias}")
    whole = report_by(pds, X, y, off, family, bias)
    small = sizes <= 300
    for k in (*COEF, *GROUP, "cov", "beta"):
        assert same_bits(d1[k][small], whole[k][small]), k


@pytest.mark.parametrize("family,p,bias", [("binomial", 8, True), ("gaussian", 16, True), ("poisson", 1, False), ("gamma", 8, True)])
def test_a_bad_group_changes_no_other_group(pds, family, p, bias):
    """(f): a group with an all-zero feature column is null (fit or report); every other group's bits are those of the frame
    without it"""
    rng = np.random.default_rng(17)
    sizes = gc.ragged_sizes(rng, 40, p)
    X, y, off = gc.family_frame(rng, family, sizes, p)
    bad = 17
    a, e = int(off[bad]), int(off[bad + 1])
    Xb = X.copy()
    Xb[a:e, p - 1] = 0.0
    d = report_by(pds, Xb, y, off, family, bias)
    assert d["is_null"][bad] == 1 or d["report_null"][bad] == 1
    assert d["report_null"][bad] == 1 and all(np.isnan(d[k][bad]).all() for k in (*COEF, *GROUP, "cov"))
    keep = np.ones(len(X), dtype=bool)
    keep[a:e] = False
    others = np.arange(40) != bad
    c = report_by(pds, X[keep], y[keep], gc.offsets(np.delete(sizes, bad)), family, bias)
    for k in (*COEF, *GROUP, "cov", "beta", "n_iter", "is_null", "report_null", "df_resid"):
        assert same_bits(d[k][others], c[k]), k


@pytest.mark.parametrize("family,p,bias", [("binomial", 8, True), ("poisson", 16, False), ("gamma", 16, True), ("gaussian", 1, True)])
def test_keys(pds, family, p, bias):
    """(g): sorted keys: bit-identical to the offsets form; shuffled rows: within 1e-12 relative"""
    X, y, off = config_frame(family, p)
    d = device_report(pds, family, p, bias)
    sizes = np.diff(off)
    key = np.repeat(np.arange(G, dtype=np.int64) * 3 - 50, sizes)
    k1 = report_by_key(pds, X, y, key, family, bias)
    assert np.array_equal(k1["keys"], np.arange(G) * 3 - 50)
    for k in (*COEF, *GROUP, "cov", "beta", "n_iter", "is_null", "report_null", "df_resid"):
        assert same_bits(k1[k], d[k]), k
    perm = np.random.default_rng(19).permutation(len(y))
    k2 = report_by_key(pds, X[perm], y[perm], key[perm], family, bias)
    assert np.array_equal(k2["keys"], k1["keys"]) and np.array_equal(k2["df_resid"], d["df_resid"])
    ok = usable_groups(d, "keys")
    for k in ("beta", *COEF[:2], "0.025", "0.975", *GROUP):
        m = np.isfinite(d[k][ok])
        scale = np.abs(d[k][ok][m])
        if k in ("beta", "z", "0.025", "0.975"):  # (a coefficient may be close to 0: its scale is its standard error's)
            scale = np.maximum(scale, np.broadcast_to(d["std_err"][ok], d[k][ok].shape)[m])
        assert (np.abs(k2[k][ok][m] - d[k][ok][m]) <= 1e-12 * scale).all(), k
    assert rr.cov_err(k2["cov"][ok], d["cov"][ok]) <= 1e-12


@pytest.mark.parametrize("family,p,bias", [("binomial", 8, True), ("poisson", 16, True), ("gamma", 1, False), ("gaussian", 16, False)])
def test_f32_frames(pds, family, p, bias):
    """(h): f32 frames: the reference on the f32-rounded frame at the returned f32 coefficients; outputs within 4 ulp of f32"""
    X, y, off = config_frame(family, p)
    X32, y32 = X.astype(np.float32), y.astype(np.float32)
    pds.config.LIN_REG_EXPR_F64 = False
    try:
        d = report_by(pds, X32, y32, off, family, bias, tol=1e-6)
    finally:
        pds.config.LIN_REG_EXPR_F64 = True
    assert all(d[k].dtype == np.float32 for k in (*COEF, *GROUP, "cov", "beta"))
    ok = usable_groups(d, "f32")
    with np.errstate(all="ignore"):
        ref = rr.report_by(X32.astype(np.float64), y32.astype(np.float64), off, d["beta"].astype(np.float64), family, bias, skip=~ok)
    ulp4 = 4 * 2.0 ** -23

    def close(a, r, scale=None):
        r = r.astype(np.float64)
        s = np.abs(r) if scale is None else scale
        return (np.abs(a.astype(np.float64) - r) <= ulp4 * s + 1e-45).all()

    for k in ("std_err", *GROUP):
        m = np.isfinite(ref[REF_NAME.get(k, k)][ok].astype(np.float64))
        assert close(d[k][ok][m], ref[REF_NAME.get(k, k)][ok][m]), k
    assert close(d["z"][ok], ref["z"][ok])
    se = ref["std_err"][ok].astype(np.float64)
    for k in ("0.025", "0.975"):
        assert close(d[k][ok], ref[REF_NAME[k]][ok], np.abs(d["beta"][ok].astype(np.float64)) + se), k
    # (below f32's normal range a value has fewer bits than an ulp bound assumes)
    assert (np.abs(d["p>|z|"][ok].astype(np.float64) - ref["p"][ok]) <= ulp4 * ref["p"][ok] + 2.0 ** -126).all()
    s = np.sqrt(np.einsum("gii->gi", ref["cov"][ok].astype(np.float64)))
    assert (np.abs(d["cov"][ok].astype(np.float64) - ref["cov"][ok].astype(np.float64)) <= ulp4 * s[:, :, None] * s[:, None, :]).all()


@pytest.mark.parametrize("family,p,bias", [("binomial", 8, True), ("gamma", 16, False)])
def test_numpy_inputs(pds, family, p, bias):
    """(i): host frames give the bits of device frames"""
    X, y, off = config_frame(family, p)
    d = device_report(pds, family, p, bias)
    h = report_by(pds, X, y, off, family, bias, space="host")
    for k in (*COEF, *GROUP, "cov", "beta", "n_iter", "is_null", "report_null", "df_resid"):
        assert isinstance(h[k], np.ndarray) and same_bits(h[k], d[k]), k
    key = np.repeat(np.arange(G, dtype=np.int64), np.diff(off))
    hk = report_by_key(pds, X, y, key, family, bias, space="host")
    for k in (*COEF, *GROUP, "cov", "beta", "n_iter", "is_null", "report_null", "df_resid"):
        assert same_bits(hk[k], d[k]), k
    # without the optional outputs
    nc = report_by(pds, X, y, off, family, bias, cov=False)
    assert "cov" not in nc and same_bits(nc["std_err"], d["std_err"])


@pytest.mark.parametrize("family,bias", [("binomial", True), ("poisson", False), ("gamma", True), ("gaussian", True)])
def test_glm_fit_with_report(pds, family, bias):
    """(j): GLM.fit(report=True) on one 5 000-row frame is the one-group call"""
    rng = np.random.default_rng(23)
    X, y, off = gc.family_frame(rng, family, np.array([5000]), 8)
    d = report_by(pds, X, y, off, family, bias, tol=1e-8)
    m = pds.linear_models.GLM(add_bias=bias, family=family, tol=1e-8).fit(X, y, report=True)
    beta = np.append(m.coeffs(), m.bias()) if bias else m.coeffs()
    assert same_bits(beta, d["beta"][0]) and m.n_iter_ == int(d["n_iter"][0])
    assert same_bits(m.std_errors_, d["std_err"][0]) and same_bits(m.z_, d["z"][0]) and same_bits(m.p_values_, d["p>|z|"][0])
    assert m.deviance_ == d["deviance"][0] and m.null_deviance_ == d["null_deviance"][0] and m.dispersion_ == d["dispersion"][0]
    assert m.df_resid_ == 5000 - 8 - int(bias)
    rep = m.report_dict()
    assert rep["features"][-1] == ("__bias__" if bias else "x8") and same_bits(rep["std_err"], d["std_err"][0])
    plain = pds.linear_models.GLM(add_bias=bias, family=family, tol=1e-8).fit(X, y)
    with pytest.raises(ValueError):
        plain.report()
    # the default path is the one-model iteration: the same estimate to its tolerance
    assert np.allclose(plain.coeffs(), m.coeffs(), rtol=0, atol=1e-6)


@pytest.mark.parametrize("p,bias", [(1, True), (8, True), (16, True), (8, False)])
def test_gaussian_against_lin_reg_report_by(pds, p, bias):
    """(k): two routes of this library: the gaussian family's se against lin_reg_report_by on the same frame, within the budget of
    (a) (the spread of the restatement on this frame; both routes are float64 evaluations of the same quantity)"""
    X, y, off = config_frame("gaussian", p)
    d = device_report(pds, "gaussian", p, bias)
    r = pds.lin_reg_report_by(*cols_of(X, "device"), target=dev(y), group_offsets=dev(off), add_bias=bias)
    se = np_(r["std_err"])
    ok = usable_groups(d, "gaussian")
    beta = d["beta"].astype(np.float64)
    hi = rr.report_by(X, y, off, beta, "gaussian", bias)
    lo = rr.report_by(X, y, off, beta, "gaussian", bias, dtype=np.float64)
    spread = rr.rel_err(lo["std_err"][ok], hi["std_err"][ok])
    err = rr.rel_err(d["std_err"][ok], se[ok])
    print(f"gaussian p={p} bias={bias}: glm report se vs lin_reg_report_by {err:.3g}, budget {64 * spread:.3g}")
    assert err <= 64 * spread


def test_argument_errors(pds):
    X, y, off = config_frame("poisson", 1)
    c = cols_of(X, "device")
    with pytest.raises(NotImplementedError):
        pds.glm_report_by(*c, target=dev(y), group_offsets=dev(off), family="poisson", l2_reg=0.1)
    with pytest.raises(NotImplementedError):
        pds.glm_report_by_key(*c, target=dev(y), key=dev(np.zeros(len(y), dtype=np.int64)), family="poisson", l1_reg=0.1)
    with pytest.raises(NotImplementedError):
        pds.glm_report_by(*(c * 17), target=dev(y), group_offsets=dev(off), family="poisson")
    with pytest.raises(ValueError):
        pds.glm_report_by(*c, target=dev(y), group_offsets=dev(off), family="poisson", max_iter=0)
    with pytest.raises(NotImplementedError):
        pds.glm_report_by(*c, target=dev(y), group_offsets=dev(off), family="tweedie")


@pytest.mark.parametrize("family,p,bias,nulls", [("binomial", 8, True, False), ("poisson", 3, False, False), ("gamma", 4, True, True)])
def test_plugin_on_host_arrow_frames(pds, family, p, bias, nulls):
    """(l): pl_glm_report_by on host Arrow frames is glm_report_by_key on the same host columns, in the long format; with nulls and
    "skip" the frame without the dropped rows"""
    import ctypes as C

    import pyarrow as pa
    from plugin_harness import call_plugin

    from polars_ds_extension_amd import _lib

    _lib.load()
    lib = C.CDLL(str(_lib.LIB_PATH))
    rng = np.random.default_rng(29)
    sizes = np.concatenate([gc.ragged_sizes(rng, 30, p), [p + int(bias) - 1]])  # (the last group is too short: a null group)
    X, y, off = gc.family_frame(rng, family, sizes, p)
    key = np.repeat(np.arange(len(sizes), dtype=np.int64) * 5 - 11, sizes)
    perm = rng.permutation(len(y))
    X, y, key = X[perm], y[perm], key[perm]
    mask = (rng.uniform(size=len(y)) < 0.03) if nulls else None
    ins = [("k", pa.array(key)), ("y", pa.array(y))] + [(f"x{j + 1}", pa.array(np.ascontiguousarray(X[:, j]), mask=mask if j == 0 else None))
                                                         for j in range(p)]
    kw = {"bias": bias, "null_policy": "skip" if nulls else "raise", "family": family, "tol": TOL, "max_iter": MAX_ITER}
    _, out = call_plugin(lib, "pl_glm_report_by", ins, kw)
    if nulls:
        X, y, key = X[~mask], y[~mask], key[~mask]
    d = report_by_key(pds, X, y, key, family, bias, space="host")
    pp, ng = p + int(bias), len(sizes)
    assert len(out) == ng * pp and out.field(0).to_pylist() == np.repeat(d["keys"], pp).tolist()
    assert out.field(1).to_pylist() == d["features"] * ng
    assert d["report_null"][-1] == 1 and d["report_null"][:-1].sum() == 0
    for i, k in enumerate(("beta", "std_err", "z", "p>|z|", "0.025", "0.975")):
        col = out.field(2 + i)
        assert col.null_count == pp, k
        got = np.asarray(col.to_numpy(zero_copy_only=False), dtype=np.float64).reshape(ng, pp)
        assert same_bits(got[:-1], d[k][:-1]), k
    for i, k in enumerate(("deviance", "null_deviance", "dispersion")):
        got = np.asarray(out.field(8 + i).to_numpy(zero_copy_only=False), dtype=np.float64).reshape(ng, pp)
        assert same_bits(got[:-1], np.repeat(d[k][:-1, None], pp, axis=1)), k
    assert out.field(11).to_pylist() == np.repeat(d["n_iter"], pp).tolist()
