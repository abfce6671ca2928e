"""
Grouped GLM fits with prior weights and an offset per row on the device (lstsq.glm_by / glm_by_key with weights= / offset=:
pds_glm_irls_wo_grouped_* / _by_key_*, the weighted / offset form of csrc/grouped_irls.hip) against the NumPy float64 restatement
of tests/glm_weighted_reference.py, and against the unweighted calls where the two must agree.

Frames: tests/glm_weighted_cases.py (default_rng(123), 150 ragged groups).  Bounds are those of tests/test_grouped_glm_gpu.py:
coefficients ||b - b_ref|| / ||b_ref|| < 1e-9 and |n_iter - it_ref| <= 1 per group at tol 1e-10, 1e-4 for f32 frames at tol 1e-6.
The restatement leaves at most 1 of 150 groups of a configuration open (binomial, p = 1), so at most 2 of 150 may be left out of a
comparison, and only those the restatement itself does not converge on.
"""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import glm_cases as gc  # noqa: E402
import glm_weighted_cases as wc  # noqa: E402
import glm_weighted_reference as wr  # noqa: E402

pytestmark = pytest.mark.gpu

TOL, MAX_ITER = 1e-10, 100
MODES = ("both", "weights", "offset")


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
    return v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)


def cols_of(X, space):
    cs = [np.ascontiguousarray(X[:, j]) for j in range(X.shape[1])]
    return [dev(c) for c in cs] if space == "device" else cs


def glm_by(pds, X, y, off, family, bias, pw=None, o=None, space="device", tol=TOL, return_pred=False, ctx=None, **kw):
    put = dev if space == "device" else (lambda a: a)
    r = pds.glm_by(*cols_of(X, space), target=put(y), group_offsets=put(off), family=family, add_bias=bias, tol=tol, max_iter=MAX_ITER,
                   return_pred=return_pred, ctx=ctx, weights=None if pw is None else put(pw), offset=None if o is None else put(o), **kw)
    return tuple(np_(v) for v in r)


def rel_err(b, bo):
    return np.linalg.norm(b - bo, axis=1) / np.linalg.norm(bo, axis=1)


def check_parity(co, it, nu, co_o, it_o, bound, what, max_open=2, check_iter=True):
    """Every group the reference converged on: not null, coefficients within `bound`, iteration count within one."""
    conv = np.isfinite(co_o).all(axis=1) & (it_o < MAX_ITER) & (it_o > 0)
    n_open = int((it_o > 0).sum()) - int(conv.sum())
    assert n_open <= max_open, f"{what}: the reference left {n_open} groups open"
    assert not nu[conv].any(), f"{what}: null groups where the reference converged: {np.nonzero(nu.astype(bool) & conv)[0][:8]}"
    err = rel_err(co[conv].astype(np.float64), co_o[conv])
    dit = np.abs(it[conv].astype(np.int64) - it_o[conv])
    print(f"{what}: groups {int(conv.sum())} (open {n_open}), worst rel err {err.max():.3e}, worst |n_iter - it_ref| {int(dit.max())}, "
          f"mean n_iter {it[conv].mean():.2f}")
    assert err.max() < bound, f"{what}: worst {err.max():.3e} at group {np.nonzero(conv)[0][int(err.argmax())]}"
    if check_iter:
        assert dit.max() <= 1, f"{what}: n_iter differs by {int(dit.max())}"
    return conv


def mode_frame(family, p, kind, mode):
    X, y, off, pw, o = wc.frame(family, p, kind, with_offset=mode != "weights")
    return X, y, off, (None if mode == "offset" else pw), (None if mode == "weights" else o)


# ------------------------------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("kind", wc.KINDS)
@pytest.mark.parametrize("p", wc.WIDTHS)
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("family", gc.FAMILIES)
def test_parity_per_group(pds, family, bias, p, kind):
    for mode in MODES:
        X, y, off, pw, o = mode_frame(family, p, kind, mode)
        co_o, it_o = wr.fit(X, y, off, pw, o, family, bias, TOL, MAX_ITER)
        for space in ("device", "host"):
            co, it, nu = glm_by(pds, X, y, off, family, bias, pw, o, space)
            assert co.shape == (wc.G, p + int(bias)) and it.dtype == np.int32 and nu.dtype == np.uint8
            check_parity(co, it, nu, co_o, it_o, 1e-9, f"{family} bias={bias} p={p} {kind} {mode} {space}")


@pytest.mark.parametrize("kind", wc.KINDS)
@pytest.mark.parametrize("p", wc.WIDTHS)
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("family", gc.FAMILIES)
def test_f32_frames(pds, family, bias, p, kind):
    """f32 frames (f64 arithmetic on f32-rounded data) against the f64 restatement on the f64 data, tol = 1e-6."""
    X, y, off, pw, o = wc.frame(family, p, kind)
    co_o, it_o = wr.fit(X, y, off, pw, o, family, bias, 1e-6, MAX_ITER)
    pds.config.LIN_REG_EXPR_F64 = False
    try:
        f = np.float32
        co, it, nu = glm_by(pds, X.astype(f), y.astype(f), off, family, bias, pw.astype(f), o.astype(f), tol=1e-6)
    finally:
        pds.config.LIN_REG_EXPR_F64 = True
    assert co.dtype == np.float32
    check_parity(co, it, nu, co_o, it_o, 1e-4, f"f32 {family} bias={bias} p={p} {kind}", check_iter=False)


# ------------------------------------------------------------------------------------------------------------- 2. replication
@pytest.mark.parametrize("family,bias,p", [("binomial", True, 8), ("poisson", False, 16), ("gamma", True, 1), ("gaussian", False, 8),
                                           ("poisson", True, 1)])
def test_integer_weights_are_repeated_rows(pds, family, bias, p):
    """the integer-weight fit = the unweighted glm_by on the frame with row i repeated pw_i times"""
    X, y, off, pw, _ = wc.frame(family, p, "integer", with_offset=False)
    co, it, nu = glm_by(pds, X, y, off, family, bias, pw)
    Xr, yr, offr = wc.replicate(X, y, off, pw)
    co_r, it_r, nu_r = glm_by(pds, Xr, yr, offr, family, bias)
    ok = ~nu_r.astype(bool) & (it_r < MAX_ITER)
    assert int((~ok).sum()) <= 2 and not nu[ok].any()
    err = rel_err(co[ok], co_r[ok])
    print(f"replication {family} bias={bias} p={p}: worst rel err {err.max():.3e}, worst |n_iter| diff {np.abs(it[ok] - it_r[ok]).max()}")
    assert err.max() < 1e-9 and np.abs(it[ok].astype(int) - it_r[ok]).max() <= 1


# ------------------------------------------------------------------------------------------ 3. unit weights and a zero offset
@pytest.mark.parametrize("family,bias,p", [("binomial", True, 8), ("poisson", True, 16), ("gamma", False, 1), ("gaussian", True, 16)])
def test_unit_weights_and_zero_offset(pds, family, bias, p):
    X, y, off, _, _ = wc.frame(family, p, "real", with_offset=False)
    base = glm_by(pds, X, y, off, family, bias, return_pred=True)
    got = glm_by(pds, X, y, off, family, bias, np.ones(len(y)), np.zeros(len(y)), return_pred=True)
    same = all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(base, got))
    print(f"unit weights, zero offset {family} bias={bias} p={p}: bit-identical to the unweighted call: {same}")
    ok = ~base[2].astype(bool) & (base[1] < MAX_ITER)
    assert not got[2][ok].any()
    assert rel_err(got[0][ok], base[0][ok]).max() < 1e-9 and np.abs(got[1][ok].astype(int) - base[1][ok]).max() <= 1


# ------------------------------------------------------------------------------------------------------------ 4. offset shift
@pytest.mark.parametrize("p", [1, 8, 16])
def test_constant_offset_moves_the_bias(pds, p):
    """poisson with a bias: a per-group constant offset c_g leaves the feature coefficients alone and takes c_g off the bias"""
    X, y, off, pw, _ = wc.frame("poisson", p, "real", with_offset=False)
    sizes = np.diff(off)
    c = np.random.default_rng(77).uniform(-1.0, 1.0, size=wc.G)
    co0, it0, nu0 = glm_by(pds, X, y, off, "poisson", True, pw)
    co, it, nu = glm_by(pds, X, y, off, "poisson", True, pw, np.repeat(c, sizes))
    ok = ~nu0.astype(bool) & (it0 < MAX_ITER)
    assert int((~ok).sum()) <= 2 and not nu[ok].any()
    moved = co.copy()
    moved[:, p] += c
    err = rel_err(moved[ok], co0[ok])
    print(f"offset shift p={p}: worst rel err {err.max():.3e}")
    assert err.max() < 1e-9 and np.abs(it[ok].astype(int) - it0[ok]).max() <= 1


# ------------------------------------------------------------------------------------------------- 5. gaussian = weighted OLS
@pytest.mark.parametrize("kind", wc.KINDS)
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("p", [1, 8, 16])
def test_gaussian_is_weighted_least_squares(pds, p, bias, kind):
    X, y, off, pw, _ = wc.frame("gaussian", p, kind, with_offset=False)
    co, it, nu = glm_by(pds, X, y, off, "gaussian", bias, pw)
    r = pds.lin_reg_report_by(*cols_of(X, "device"), target=dev(y), group_offsets=dev(off), add_bias=bias, weights=dev(pw))
    b = np_(r["beta"])
    assert not nu.any() and not np_(r["is_null"]).any()
    err = rel_err(co, b)
    print(f"gaussian against lin_reg_report_by(weights=) p={p} bias={bias} {kind}: worst rel err {err.max():.3e}")
    assert err.max() < 1e-9


# ---------------------------------------------------------------------------------------------------------------- 6. shapes
def shapes_frame(family, p, bias, long_groups):
    """Group sizes on both sides of a 64-row step and of the 128 resident rows; groups of 40 rows of which p' - 1, p', p' + 1 have a
    positive weight; a group of 150 rows whose rows 64 .. 127 all have weight 0; a group of 100 rows whose last row has weight 0;
    with `long_groups` groups of 301 .. 1 100 rows, the last of them null by the weight rule (a negative weight): with
    glm_split_rows = 300 these leave the kernel for the full-device iteration on their row range of the two columns."""
    pp = p + int(bias)
    sizes = [63, 64, 65, 127, 128, 129, 200, 40, 40, 40, 150, 100]
    tags = ["plain"] * 7 + ["npos-1", "npos", "npos+1", "zero-step", "zero-last"]
    if long_groups:
        sizes += [301, 640, 1100, 700]
        tags += ["plain"] * 3 + ["negative"]
    rng = np.random.default_rng(123)
    X, y, off, pw, o = wc.frame_for_sizes(rng, family, np.array(sizes), p, "real")
    for g, tag in enumerate(tags):
        a, b = int(off[g]), int(off[g + 1])
        if tag.startswith("npos"):
            keep = pp + {"npos-1": -1, "npos": 0, "npos+1": 1}[tag]
            live = rng.choice(b - a, size=keep, replace=False)
            pw[a:b] = 0.0
            pw[a + live] = rng.uniform(0.25, 4.0, size=keep)
        elif tag == "zero-step":
            pw[a + 64:a + 128] = 0.0
        elif tag == "zero-last":
            pw[b - 1] = 0.0
        elif tag == "negative":
            pw[a + 650] = -1.0
    return X, y, off, pw, o, tags


@pytest.mark.parametrize("long_groups", [False, True])
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("p", [1, 8, 16])
@pytest.mark.parametrize("family", ["gaussian", "poisson"])
def test_shapes(pds, family, p, bias, long_groups):
    X, y, off, pw, o, tags = shapes_frame(family, p, bias, long_groups)
    ctx = None
    if long_groups:
        ctx = pds.Context()
        ctx.set_option("glm_split_rows", 300)
    co, it, nu, pred, rn = glm_by(pds, X, y, off, family, bias, pw, o, return_pred=True, ctx=ctx)
    co_o, it_o = wr.fit(X, y, off, pw, o, family, bias, TOL, MAX_ITER)
    # (a group with exactly p' live rows is an interpolation, which the poisson family may not be able to reach: up to 2 left open)
    check_parity(co, it, nu, co_o, it_o, 1e-9, f"shapes {family} p={p} bias={bias} long={long_groups}")
    gid = np.repeat(np.arange(len(tags)), np.diff(off))
    for g, tag in enumerate(tags):
        if tag in ("npos-1", "negative"):
            assert np.isnan(co[g]).all() and it[g] == 0 and nu[g] == 1, (g, tag)
            assert (rn[gid == g] == 1).all() and np.isnan(pred[gid == g]).all()
        else:
            assert it[g] >= 1, (g, tag)
        if tag == "plain" or (family == "gaussian" and tag in ("npos", "npos+1", "zero-step", "zero-last")):
            assert nu[g] == 0 and it_o[g] < MAX_ITER, (g, tag)
    assert np.array_equal(rn, nu[gid]) and np.isfinite(pred[rn == 0]).all()


# ------------------------------------------------------------------------------------------------- 7. a bad group touches nobody
@pytest.mark.parametrize("family,bias,p", [("binomial", True, 8), ("poisson", False, 16), ("gaussian", True, 1)])
def test_bad_groups_touch_nobody(pds, family, bias, p):
    X, y, off, pw, o = wc.frame(family, p, "real", n_groups=40)
    bad = {5: "negative", 17: "nan-weight", 30: "nan-offset"}
    pw2, o2 = pw.copy(), o.copy()
    pw2[off[5] + 3] = -0.5
    pw2[off[17] + (off[18] - off[17]) - 1] = np.nan
    o2[off[30] + 7] = np.nan
    good = glm_by(pds, X, y, off, family, bias, pw, o, return_pred=True)
    got = glm_by(pds, X, y, off, family, bias, pw2, o2, return_pred=True)
    co, it, nu, pred, rn = got
    for g, kind in bad.items():
        assert nu[g] == 1 and not np.isfinite(co[g]).all(), (g, kind)
        if kind != "nan-offset":
            assert np.isnan(co[g]).all() and it[g] == 0
    others = np.array([g for g in range(40) if g not in bad])
    rows = np.isin(np.repeat(np.arange(40), np.diff(off)), others)
    assert (rn[~rows] == 1).all() and np.isnan(pred[~rows]).all()
    for a, b in zip(good[:3], got[:3]):
        assert np.array_equal(a[others].view(np.uint8), b[others].view(np.uint8))
    for a, b in zip(good[3:], got[3:]):
        assert np.array_equal(a[rows].view(np.uint8), b[rows].view(np.uint8))


# ------------------------------------------------------------------------------------------------------------------ 8. keys
@pytest.mark.parametrize("family,bias,p,kind", [("binomial", True, 8, "integer"), ("poisson", False, 16, "real"),
                                                ("gamma", True, 16, "real"), ("gaussian", True, 1, "integer")])
def test_keys(pds, family, bias, p, kind):
    """Ordered keys = the offsets form bit for bit; shuffled rows within the parity bound of it, keys ascending, pred and row_null
    at the rows' own positions."""
    X, y, off, pw, o = wc.frame(family, p, kind)
    n, sizes = len(y), np.diff(off)
    labels = np.sort(np.random.default_rng(5).choice(10 * wc.G, size=wc.G, replace=False)).astype(np.int64) - 700
    key = np.repeat(labels, sizes)
    co, it, nu, pred, rn = glm_by(pds, X, y, off, family, bias, pw, o, return_pred=True)

    def by_key(rows, space):
        put = dev if space == "device" else (lambda a: a)
        r = pds.glm_by_key(*cols_of(X[rows], space), target=put(y[rows]), key=put(key[rows]), family=family, add_bias=bias, tol=TOL,
                           max_iter=MAX_ITER, return_pred=True, weights=put(pw[rows]), offset=put(o[rows]))
        return tuple(np_(v) for v in r)

    for space in ("device", "host"):
        k1, *rest = by_key(np.arange(n), space)
        assert np.array_equal(k1, labels)
        for a, b in zip(rest, (co, it, nu, pred, rn)):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), f"ordered keys differ from the offsets form ({space})"
    ok = ~nu.astype(bool) & (it < MAX_ITER)
    gid = np.repeat(np.arange(wc.G), sizes)
    perm = np.random.default_rng(9).permutation(n)
    for space in ("device", "host"):
        k2, co2, it2, nu2, pred2, rn2 = by_key(perm, space)
        assert np.array_equal(k2, labels) and not nu2[ok].any()
        err = rel_err(co2[ok], co[ok])
        print(f"shuffled ({space}): worst rel err to the offsets form {err.max():.3e}")
        assert err.max() < 1e-9 and np.abs(it2[ok].astype(int) - it[ok]).max() <= 1
        live = ok[gid][perm]
        assert not rn2[live].any()
        assert np.allclose(pred2[live], pred[perm][live], rtol=1e-9, atol=1e-12)


# ------------------------------------------------------------------------------------------------------------------ 9. pred
@pytest.mark.parametrize("p", [1, 8, 16])
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("family", gc.FAMILIES)
def test_pred(pds, family, bias, p):
    """mu of every row = g^-1(x . beta_g + o) recomputed from the RETURNED coefficients in the kernel's order (bias first, one fused
    multiply-add per feature, then + o): 1e-12 absolute (binomial), 1e-12 relative (the other links); rows of weight 0 of a
    non-null group have a finite pred."""
    X, y, off, pw, o = wc.frame(family, p, "integer")
    co, it, nu, pred, rn = glm_by(pds, X, y, off, family, bias, pw, o, return_pred=True)
    gid = np.repeat(np.arange(wc.G), np.diff(off))
    assert np.array_equal(rn, nu[gid])
    live = rn == 0
    assert (pw[live] == 0).any() and np.isfinite(pred[live]).all()
    eta = gc.eta_in_kernel_order(X, np.where(live[:, None], co[gid], 0.0), bias) + o
    mu = gc.inv_link(family, eta[live])
    d = np.abs(pred[live] - mu)
    ok = d <= (1e-12 if family == "binomial" else 1e-12 * np.abs(mu))
    with np.errstate(all="ignore"):
        rel = np.nanmax(np.where(d == 0.0, 0.0, d if family == "binomial" else d / np.abs(mu)))
    print(f"pred {family} bias={bias} p={p}: worst {rel:.3e}")
    assert ok.all(), f"{int((~ok).sum())} rows beyond 1e-12, worst {rel:.3e}"
    assert np.isnan(pred[~live]).all()


# ---------------------------------------------------------------------------------------------------------- 10. determinism
def test_determinism(pds):
    X, y, off, pw, o = wc.frame("binomial", 8, "real")
    a = glm_by(pds, X, y, off, "binomial", True, pw, o, return_pred=True)
    b = glm_by(pds, X, y, off, "binomial", True, pw, o, return_pred=True)
    for u, v in zip(a, b):
        assert np.array_equal(u.view(np.uint8), v.view(np.uint8))


# ------------------------------------------------------------------------------------------------------- 12. Python surface
@pytest.mark.parametrize("space", ["device", "host"])
@pytest.mark.parametrize("family,bias,p", [("poisson", True, 8), ("binomial", False, 3), ("gamma", True, 16), ("gaussian", True, 20)])
def test_glm_class(pds, family, bias, p, space):
    """GLM.fit(sample_weight=, offset=) (the one-model route, 20 features: the wide build) against the restatement on the whole frame,
    predict(offset=) against g^-1(X beta + bias + o) of the fitted coefficients; the weight rule raises."""
    from polars_ds_extension_amd import _lib
    from polars_ds_extension_amd.linear_models import GLM

    rng = np.random.default_rng(123)
    X, y, off, pw, o = wc.frame_for_sizes(rng, family, np.array([5000]), p, "integer")
    put = dev if space == "device" else (lambda a: a)
    b_o, it_o = wr.fit_group(X, y, pw, o, family, bias, TOL, MAX_ITER)
    m = GLM(add_bias=bias, family=family, tol=TOL, max_iter=MAX_ITER).fit(put(X), put(y), sample_weight=put(pw), offset=put(o))
    b = np.append(m.coeffs(), m.bias()) if bias else m.coeffs()
    err = np.linalg.norm(b - b_o) / np.linalg.norm(b_o)
    print(f"GLM.fit {family} bias={bias} p={p} {space}: rel err {err:.3e}, n_iter {m.n_iter_} (restatement {it_o})")
    assert it_o < MAX_ITER and err < 1e-9 and abs(m.n_iter_ - it_o) <= 1
    mu = np_(m.predict(put(X), offset=put(o))).reshape(-1)
    want = gc.inv_link(family, X @ b[:p] + (b[p] if bias else 0.0) + o)
    assert np.allclose(mu, want, rtol=1e-9, atol=1e-12)
    assert np.allclose(np_(m.predict(put(X), linear=True, offset=put(o))).reshape(-1), X @ b[:p] + (b[p] if bias else 0.0) + o, rtol=1e-9, atol=1e-12)
    for bad, msg in ((-1.0, "finite and not negative"), (np.nan, "finite and not negative")):
        pw2 = pw.copy()
        pw2[17] = bad
        with pytest.raises(_lib.PdsError, match=msg):
            GLM(add_bias=bias, family=family).fit(put(X), put(y), sample_weight=put(pw2))
    pw3 = np.zeros(len(y))
    pw3[:p + int(bias) - 1] = 1.0
    with pytest.raises(_lib.PdsError, match="fewer rows of positive weight"):
        GLM(add_bias=bias, family=family).fit(put(X), put(y), sample_weight=put(pw3))
    with pytest.raises(NotImplementedError):
        GLM(add_bias=bias, family=family, l2_reg=0.1).fit(put(X), put(y), sample_weight=put(pw))
    # a null policy that drops rows drops them from the two columns too
    if space == "host":
        X2 = X.copy()
        X2[[5, 77], 0] = np.nan
        keep = np.ones(len(y), bool)
        keep[[5, 77]] = False
        m2 = GLM(add_bias=bias, family=family, tol=TOL, max_iter=MAX_ITER).fit(X2, y, null_policy="skip", sample_weight=pw, offset=o)
        m3 = GLM(add_bias=bias, family=family, tol=TOL, max_iter=MAX_ITER).fit(X[keep], y[keep], sample_weight=pw[keep], offset=o[keep])
        assert np.array_equal(m2.coeffs(), m3.coeffs()) and m2.bias() == m3.bias()


@pytest.mark.parametrize("family,bias,p", [("poisson", True, 8), ("binomial", True, 16)])
def test_long_route_matches_the_waves(pds, family, bias, p):
    """the same frame with the long groups on the waves (default glm_split_rows) and through the full-device iteration (300): the
    parity bound between the two, pred included; the groups below 300 rows keep their bits"""
    X, y, off, pw, o, tags = shapes_frame(family, p, bias, True)
    a = glm_by(pds, X, y, off, family, bias, pw, o, return_pred=True)
    ctx = pds.Context()
    ctx.set_option("glm_split_rows", 300)
    b = glm_by(pds, X, y, off, family, bias, pw, o, return_pred=True, ctx=ctx)
    sizes = np.diff(off)
    small = sizes <= 300
    for u, v in zip(a[:3], b[:3]):
        assert np.array_equal(u[small].view(np.uint8), v[small].view(np.uint8))
    assert np.array_equal(a[2], b[2]) and np.array_equal(a[4], b[4])
    ok = ~a[2].astype(bool) & (a[1] < MAX_ITER)
    err = rel_err(b[0][ok], a[0][ok])
    print(f"long route against the waves {family} p={p}: worst rel err {err.max():.3e}")
    assert err.max() < 1e-9 and np.abs(a[1][ok].astype(int) - b[1][ok]).max() <= 1
    live = a[4] == 0
    assert np.allclose(a[3][live], b[3][live], rtol=1e-9, atol=1e-12) and np.isnan(b[3][~live]).all()


def test_penalty_with_weights_is_refused(pds):
    import ctypes as C

    from polars_ds_extension_amd import _lib

    X, y, off, pw, o = wc.frame("poisson", 1, "real", n_groups=4)
    for kw in ({"l1_reg": 0.1}, {"l2_reg": 0.1}):
        with pytest.raises(NotImplementedError, match="weights= / offset="):
            glm_by(pds, X, y, off, "poisson", True, pw, None, **kw)
        with pytest.raises(NotImplementedError, match="weights= / offset="):
            pds.glm_by_key(dev(X[:, 0]), target=dev(y), key=dev(np.zeros(len(y), dtype=np.int64)), family="poisson", offset=dev(o), **kw)
    with pytest.raises(ValueError, match="one entry per row"):
        glm_by(pds, X, y, off, "poisson", True, pw[:-1], None)
    # both pointers null: the twin's call, the same bits
    lib, ctx = _lib.load(), pds.default_context()
    x0 = np.ascontiguousarray(X[:, 0])
    cols = (C.c_void_p * 2)(y.ctypes.data, x0.ctypes.data)
    outs = []
    for name, extra in (("pds_glm_irls_grouped_f64", ()), ("pds_glm_irls_wo_grouped_f64", (None, None))):
        co, it, nu = np.empty((4, 2)), np.empty(4, dtype=np.int32), np.empty(4, dtype=np.uint8)
        rc = getattr(lib, name)(ctx._h, cols, *extra, 1, C.c_int64(len(y)), C.c_void_p(off.ctypes.data), C.c_int64(4), _lib.PDS_HOST, 1, 1, 1,
                                C.c_double(1e-10), 100, C.c_void_p(co.ctypes.data), C.c_void_p(it.ctypes.data), C.c_void_p(nu.ctypes.data),
                                None, None)
        assert rc == 0
        outs.append((co, it, nu))
    for a, b in zip(*outs):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
