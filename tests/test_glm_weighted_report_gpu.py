"""
The grouped GLM report with prior weights and an offset per row on the device (lstsq.glm_report_by / glm_report_by_key with weights= /
offset=: pds_glm_report_wo_grouped_* / _by_key_*, csrc/grouped_glm_report.hip's weighted / offset kernels; GLM.fit(report=True) with the two
columns) against the restatement of tests/glm_weighted_reference.py.

Budget (the rule of tests/test_glm_report_gpu.py): per configuration and quantity the device's error against the longdouble restatement
at the device's own coefficients is at most 64 x the float64 restatement's distance from the longdouble one on the same frame.  The
worst error-to-spread ratio of every configuration is printed.  Frames: tests/glm_weighted_cases.py, 150 ragged groups.
"""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import glm_cases as gc  # noqa: E402
import glm_report_reference as rr  # noqa: E402
import glm_weighted_cases as wc  # noqa: E402
import glm_weighted_reference as wr  # noqa: E402
from test_glm_weighted_gpu import cols_of, dev, glm_by, mode_frame, np_, pds, shapes_frame  # noqa: E402,F401  (pds: the fixture)

pytestmark = pytest.mark.gpu

TOL, MAX_ITER = 1e-10, 100
GROUP = ("deviance", "null_deviance", "pearson_chi2", "dispersion")
REF_NAME = {"0.025": "lo", "0.975": "hi"}


def report_by(pds, X, y, off, family, bias, pw, o, space="device", ctx=None):
    put = dev if space == "device" else (lambda a: a)
    d = pds.glm_report_by(*cols_of(X, space), target=put(y), group_offsets=put(off), family=family, add_bias=bias, tol=TOL, max_iter=MAX_ITER,
                          return_cov=True, ctx=ctx, weights=None if pw is None else put(pw), offset=None if o is None else put(o))
    return {k: (np_(v) if k != "features" else v) for k, v in d.items()}


def check_budget(d, X, y, off, pw, o, family, bias, what, factor=64.0, max_left=3, df0_groups=False):
    """the device's fields against the longdouble restatement at the device's own coefficients; returns the worst error / spread"""
    ok = (d["is_null"] == 0) & (d["report_null"] == 0) & (d["n_iter"] < MAX_ITER)
    assert int((~ok).sum()) <= max_left, f"{what}: {int((~ok).sum())} groups are null or did not converge"
    beta = d["beta"].astype(np.float64)
    with np.errstate(all="ignore"):
        hi = wr.report_by(X, y, off, pw, o, beta, family, bias, skip=~ok)
        lo = wr.report_by(X, y, off, pw, o, beta, family, bias, dtype=np.float64, skip=~ok)
    if df0_groups:  # (a frame with groups of n+ = p': df_resid = 0, the gaussian / gamma dispersion and the se are NaN on both sides)
        df0 = ok & (hi["df_resid"] == 0) & ~np.isfinite(hi["std_err"].astype(np.float64)).all(axis=1)
        assert np.isnan(d["std_err"][df0]).all() and np.isnan(d["dispersion"][df0]).all()
        ok = ok & ~df0
    assert np.isfinite(hi["std_err"][ok].astype(np.float64)).all(), f"{what}: the reference is not finite on a group the device reported"
    out = {}
    for k in ("std_err", *GROUP):
        out[k] = (rr.rel_err(d[k][ok], hi[k][ok]), rr.rel_err(lo[k][ok], hi[k][ok]))
    out["cov"] = (rr.cov_err(d["cov"][ok], hi["cov"][ok]), rr.cov_err(lo["cov"][ok], hi["cov"][ok]))
    worst = max((err / spread if spread > 0 else (0.0 if err == 0 else np.inf)) for err, spread in out.values())
    print(f"{what}: worst error / spread {worst:.3g}  " + "  ".join(f"{k} {e:.2g}/{s:.2g}" for k, (e, s) in out.items()))
    for k, (err, spread) in out.items():
        assert err <= factor * spread, f"{what}: {k} error {err:.3g} above {factor:g} x spread {spread:.3g}"
    for k in GROUP:
        assert np.array_equal(np.isnan(d[k][ok]), np.isnan(hi[k][ok].astype(np.float64))), f"{what}: NaN pattern of {k}"
    se_budget = factor * out["std_err"][1]
    z_ref, p_ref = hi["z"][ok].astype(np.float64), hi["p"][ok]
    assert rr.rel_err(d["z"][ok], hi["z"][ok]) <= se_budget + 4e-16, f"{what}: z"
    assert (np.abs(d["p>|z|"][ok] - p_ref) <= (1.0 + z_ref * z_ref) * (se_budget + 4e-16) * p_ref + 1e-300).all(), f"{what}: p"
    scale = np.abs(d["beta"][ok]) + np.abs(hi["std_err"][ok].astype(np.float64))
    for k in ("0.025", "0.975"):
        assert (np.abs(d[k][ok] - hi[REF_NAME[k]][ok].astype(np.float64)) <= (se_budget + 4e-16) * scale).all(), f"{what}: {k}"
    # df_resid = n+ - p' on every group that is not null by the weight rule
    assert np.array_equal(d["df_resid"][ok], hi["df_resid"][ok])
    # null_deviance is NaN exactly when an offset is given (gamma without a bias has none either way)
    if o is not None:
        assert np.isnan(d["null_deviance"]).all()
    elif not (family == "gamma" and not bias):
        assert np.isfinite(d["null_deviance"][ok]).all()
    return ok


@pytest.mark.parametrize("mode,kind", [("both", "real"), ("weights", "integer"), ("offset", "real")])
@pytest.mark.parametrize("p", wc.WIDTHS)
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("family", gc.FAMILIES)
def test_accuracy_at_the_devices_coefficients(pds, family, bias, p, mode, kind):
    X, y, off, pw, o = mode_frame(family, p, kind, mode)
    d = report_by(pds, X, y, off, family, bias, pw, o)
    check_budget(d, X, y, off, pw, o, family, bias, f"{family} p={p} bias={bias} {mode} {kind}")
    # the fit's outputs are those of glm_by on the same frame, bit for bit
    co, it, nu = glm_by(pds, X, y, off, family, bias, pw, o)
    for a, b in ((d["beta"], co), (d["n_iter"], it), (d["is_null"], nu)):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    if p == 8:
        dh = report_by(pds, X, y, off, family, bias, pw, o, space="host")
        for k in d:
            if k != "features":
                assert np.array_equal(np.ascontiguousarray(d[k]).view(np.uint8), np.ascontiguousarray(dh[k]).view(np.uint8)), k


@pytest.mark.parametrize("p", [1, 8, 16])
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("family", ["poisson", "binomial"])
def test_integer_weights_are_repeated_rows(pds, family, bias, p):
    """se and deviance of the integer-weight report against glm_report_by on the frame with row i repeated pw_i times: 100 tol relative"""
    X, y, off, pw, _ = wc.frame(family, p, "integer", with_offset=False)
    d = report_by(pds, X, y, off, family, bias, pw, None)
    Xr, yr, offr = wc.replicate(X, y, off, pw)
    r = pds.glm_report_by(*cols_of(Xr, "device"), target=dev(yr), group_offsets=dev(offr), family=family, add_bias=bias, tol=TOL,
                          max_iter=MAX_ITER)
    r = {k: (np_(v) if k != "features" else v) for k, v in r.items()}
    ok = (r["is_null"] == 0) & (r["report_null"] == 0) & (r["n_iter"] < MAX_ITER) & (d["report_null"] == 0)
    assert int((~ok).sum()) <= 2
    for k in ("std_err", "deviance", "null_deviance", "pearson_chi2"):
        err = rr.rel_err(d[k][ok], r[k][ok])
        print(f"replication {family} p={p} bias={bias}: {k} {err:.3e}")
        assert err <= 100 * TOL, k
    # (df_resid is NOT the replicated frame's: n+ - p' counts rows of positive weight, not their weights)
    n_pos = np.add.reduceat((pw > 0).astype(np.int64), off[:-1])
    assert np.array_equal(d["df_resid"][ok], n_pos[ok] - (p + int(bias)))


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("p", [1, 8, 16])
@pytest.mark.parametrize("family", ["gaussian", "poisson"])
def test_pieces_of_long_groups(pds, family, p, bias):
    """glm_split_rows = 300 on the shapes frame with groups of 301 .. 1 100 rows: the pieced groups stay within the budget, the long
    group that is null by the weight rule has a null report, the groups below 300 rows keep their bits"""
    X, y, off, pw, o, tags = shapes_frame(family, p, bias, True)
    d0 = report_by(pds, X, y, off, family, bias, pw, o)
    ctx = pds.Context()
    ctx.set_option("glm_split_rows", 300)
    d1 = report_by(pds, X, y, off, family, bias, pw, o, ctx=ctx)
    check_budget(d1, X, y, off, pw, o, family, bias, f"pieces {family} p={p} bias={bias}", max_left=5, df0_groups=True)
    small = np.diff(off) <= 300
    for k in d0:
        if k != "features":
            assert np.array_equal(np.ascontiguousarray(d0[k][small]).view(np.uint8), np.ascontiguousarray(d1[k][small]).view(np.uint8)), k
    g = tags.index("negative")
    assert d1["is_null"][g] == 1 and d1["report_null"][g] == 1 and np.isnan(d1["std_err"][g]).all() and np.isnan(d1["deviance"][g])
    # weights only on the same frame: the closed-form null deviance of the pieces' sums
    d2 = report_by(pds, X, y, off, family, bias, pw, None, ctx=ctx)
    check_budget(d2, X, y, off, pw, None, family, bias, f"pieces, weights only {family} p={p} bias={bias}", max_left=5, df0_groups=True)


def test_determinism(pds):
    X, y, off, pw, o = wc.frame("binomial", 8, "real")
    a = report_by(pds, X, y, off, "binomial", True, pw, o)
    b = report_by(pds, X, y, off, "binomial", True, pw, o)
    for k in a:
        if k != "features":
            assert np.array_equal(np.ascontiguousarray(a[k]).view(np.uint8), np.ascontiguousarray(b[k]).view(np.uint8)), k


@pytest.mark.parametrize("family,bias,p", [("poisson", True, 8), ("gamma", False, 16)])
def test_keys(pds, family, bias, p):
    """ordered keys = the offsets form bit for bit (device and host frames); shuffled rows within 1e-9 of it"""
    X, y, off, pw, o = wc.frame(family, p, "real")
    key = np.repeat(np.arange(wc.G, dtype=np.int64) * 3 - 50, np.diff(off))
    d = report_by(pds, X, y, off, family, bias, pw, o)

    def by_key(rows, space):
        put = dev if space == "device" else (lambda a: a)
        r = pds.glm_report_by_key(*cols_of(X[rows], space), target=put(y[rows]), key=put(key[rows]), family=family, add_bias=bias, tol=TOL,
                                  max_iter=MAX_ITER, return_cov=True, weights=put(pw[rows]), offset=put(o[rows]))
        return {k: (np_(v) if k != "features" else v) for k, v in r.items()}

    for space in ("device", "host"):
        r = by_key(np.arange(len(y)), space)
        for k in d:
            if k != "features":
                assert np.array_equal(np.ascontiguousarray(d[k]).view(np.uint8), np.ascontiguousarray(r[k]).view(np.uint8)), (k, space)
    r = by_key(np.random.default_rng(9).permutation(len(y)), "device")
    ok = (d["report_null"] == 0) & (d["n_iter"] < MAX_ITER)
    assert rr.rel_err(r["std_err"][ok], d["std_err"][ok]) < 1e-9 and rr.rel_err(r["deviance"][ok], d["deviance"][ok]) < 1e-9


@pytest.mark.parametrize("family,bias", [("poisson", True), ("gaussian", False)])
def test_glm_class_report(pds, family, bias):
    """GLM.fit(report=True, sample_weight=, offset=): the one-group report of lstsq.glm_report_by on the same frame"""
    from polars_ds_extension_amd.linear_models import GLM

    rng = np.random.default_rng(123)
    X, y, off, pw, o = wc.frame_for_sizes(rng, family, np.array([3000]), 5, "integer")
    m = GLM(add_bias=bias, family=family, tol=TOL, max_iter=MAX_ITER).fit(X, y, report=True, sample_weight=pw, offset=o)
    d = report_by(pds, X, y, off, family, bias, pw, o, space="host")
    assert np.array_equal(m.std_errors_, d["std_err"][0]) and m.deviance_ == d["deviance"][0] and np.isnan(m.null_deviance_)
    assert m.df_resid_ == int((pw > 0).sum()) - 5 - int(bias) and m.dispersion_ == d["dispersion"][0]
    with np.errstate(all="ignore"):
        hi = wr.report_group(X, y, pw, o, np.append(m.coeffs(), m.bias()) if bias else m.coeffs(), family, bias)
    assert rr.rel_err(m.std_errors_, hi["std_err"]) < 1e-9 and len(m.report_dict()["std_err"]) == 5 + int(bias)
    m2 = GLM(add_bias=bias, family=family, tol=TOL, max_iter=MAX_ITER).fit(X, y, report=True, sample_weight=pw)
    assert np.isfinite(m2.null_deviance_)
