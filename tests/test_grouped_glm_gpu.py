"""
Grouped GLM fits on the device (lstsq.glm_by / glm_by_key: pds_glm_irls_grouped_* / _by_key_*, csrc/grouped_irls.hip) against
oracle.glm_irls run on every group's rows alone.

Frames (tests/glm_cases.py), seeded default_rng(123): 600 ragged groups of 4 (p + 1) .. 400 rows, the four families, bias on / off,
p in {1, 4, 8, 16}.  With the oracle at tol = 1e-10, max_iter = 100 at most one group of a configuration does not converge (a
separated binomial group) and the others take at most 11 iterations.  Bounds: coefficients ||b - b_o|| / ||b_o|| < 1e-9 and
|n_iter - it_o| <= 1 per group -- what tests/test_linear_models.py::test_glm_matches_the_oracle sets for the one-model path --
and 1e-4 for f32 frames against the f64 oracle on the f64 data (the same test's f32 bound).
"""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import glm_cases as gc  # noqa: E402

pytestmark = pytest.mark.gpu

G = 600
TOL, MAX_ITER = 1e-10, 100


@pytest.fixture(scope="module")
def pds():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import polars_ds_extension_amd as m

    return m


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle

    oracle.build()
    return oracle


def dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def np_(v):
    return v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)


def cols_of(X, space):
    cs = [np.ascontiguousarray(X[:, j]) for j in range(X.shape[1])]
    return [dev(c) for c in cs] if space == "device" else cs


def glm_by(pds, X, y, off, family, bias, space="device", tol=TOL, max_iter=MAX_ITER, return_pred=False, ctx=None):
    put = dev if space == "device" else (lambda a: a)
    r = pds.glm_by(*cols_of(X, space), target=put(y), group_offsets=put(off), family=family, add_bias=bias, tol=tol, max_iter=max_iter,
                   return_pred=return_pred, ctx=ctx)
    return tuple(np_(v) for v in r)


def glm_by_key(pds, X, y, key, family, bias, space="device", return_pred=True):
    put = dev if space == "device" else (lambda a: a)
    r = pds.glm_by_key(*cols_of(X, space), target=put(y), key=put(key), family=family, add_bias=bias, tol=TOL, max_iter=MAX_ITER,
                       return_pred=return_pred)
    return tuple(np_(v) for v in r)


def config_frame(family, p):
    rng = np.random.default_rng(123)
    sizes = gc.ragged_sizes(rng, G, p)
    return gc.family_frame(rng, family, sizes, p)


def rel_err(b, bo):
    return np.linalg.norm(b - bo, axis=1) / np.linalg.norm(bo, axis=1)


def check_parity(co, it, nu, co_o, it_o, max_iter, bound, what, max_open=0.005, check_iter=True):
    """Every group the oracle converged on: not null, coefficients within `bound`, iteration count within one."""
    conv = np.isfinite(co_o).all(axis=1) & (it_o < max_iter) & (it_o > 0)
    n_fit = int((it_o > 0).sum())
    assert (n_fit - int(conv.sum())) <= max_open * n_fit, f"{what}: the oracle left {n_fit - int(conv.sum())} of {n_fit} groups open"
    assert not nu[conv].any(), f"{what}: null groups where the oracle converged: {np.nonzero(nu.astype(bool) & conv)[0][:8]}"
    err = rel_err(co[conv].astype(np.float64), co_o[conv])
    dit = np.abs(it[conv].astype(np.int64) - it_o[conv])
    print(f"{what}: groups {int(conv.sum())}, worst rel err {err.max():.3e}, worst |n_iter - it_o| {int(dit.max())}, "
          f"mean n_iter {it[conv].mean():.2f}")
    assert err.max() < bound, f"{what}: worst {err.max():.3e} at group {np.nonzero(conv)[0][int(err.argmax())]}"
    if check_iter:
        assert dit.max() <= 1, f"{what}: n_iter differs by {int(dit.max())}"
    return conv


@pytest.mark.parametrize("p", gc.WIDTHS)
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("family", gc.FAMILIES)
def test_parity_per_group(pds, orc, family, bias, p):
    X, y, off = config_frame(family, p)
    co_o, it_o = gc.oracle_by(orc, X, y, off, family, bias, TOL, MAX_ITER)
    for space in ("device", "host"):
        co, it, nu = glm_by(pds, X, y, off, family, bias, space)
        assert co.shape == (G, p + int(bias)) and it.dtype == np.int32 and nu.dtype == np.uint8
        check_parity(co, it, nu, co_o, it_o, MAX_ITER, 1e-9, f"{family} bias={bias} p={p} {space}")


@pytest.mark.parametrize("p", gc.WIDTHS)
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("family", gc.FAMILIES)
def test_f32_frames(pds, orc, family, bias, p):
    """f32 frames (f64 arithmetic on f32-rounded data) against the f64 oracle on the f64 data, tol = 1e-6."""
    X, y, off = config_frame(family, p)
    co_o, it_o = gc.oracle_by(orc, X, y, off, family, bias, 1e-6, MAX_ITER)
    pds.config.LIN_REG_EXPR_F64 = False
    try:
        co, it, nu = glm_by(pds, X.astype(np.float32), y.astype(np.float32), off, family, bias, "device", tol=1e-6)
    finally:
        pds.config.LIN_REG_EXPR_F64 = True
    assert co.dtype == np.float32
    check_parity(co, it, nu, co_o, it_o, MAX_ITER, 1e-4, f"f32 {family} bias={bias} p={p}", check_iter=False)


@pytest.mark.parametrize("family,bias,p", [("binomial", True, 8), ("poisson", False, 16), ("gamma", True, 16), ("gaussian", True, 1)])
def test_keys(pds, orc, family, bias, p):
    """Ordered keys = the offsets form bit for bit; shuffled rows and a date-major panel within the parity bound of it, keys
    ascending, pred at the rows' own positions."""
    X, y, off = config_frame(family, p)
    n = len(y)
    sizes = np.diff(off)
    labels = np.sort(np.random.default_rng(5).choice(10 * G, size=G, replace=False)).astype(np.int64) - 3000
    key = np.repeat(labels, sizes)
    co, it, nu, pred, rn = glm_by(pds, X, y, off, family, bias, return_pred=True)
    for space in ("device", "host"):
        k1, co1, it1, nu1, pred1, rn1 = glm_by_key(pds, X, y, key, family, bias, space)
        assert np.array_equal(k1, labels)
        for a, b in ((co1, co), (it1, it), (nu1, nu), (pred1, pred), (rn1, rn)):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), f"ordered keys differ from the offsets form ({space})"
    # (a group that ran out of iterations -- a separated binomial group -- has no value to compare: its rows are left out)
    ok = ~nu.astype(bool) & (it < MAX_ITER)
    gid = np.repeat(np.arange(G), sizes)
    # shuffled rows; a date-major panel (row t of every group, then row t + 1, ...)
    rng = np.random.default_rng(9)
    within = np.arange(n) - np.repeat(off[:-1], sizes)
    for name, perm in (("shuffled", rng.permutation(n)), ("panel", np.lexsort((key, within)))):
        k2, co2, it2, nu2, pred2, rn2 = glm_by_key(pds, X[perm], y[perm], key[perm], family, bias, "device")
        assert np.array_equal(k2, labels) and not nu2[ok].any()
        err = rel_err(co2[ok], co[ok])
        print(f"{name}: worst rel err to the offsets form {err.max():.3e}")
        assert err.max() < 1e-9 and np.abs(it2[ok].astype(int) - it[ok]).max() <= 1
        live = ok[gid][perm]
        assert not rn2[live].any()
        assert np.allclose(pred2[live], pred[perm][live], rtol=1e-9, atol=1e-12)


def edge_frame(p, bias, family="binomial", scale=1):
    """Good groups with bad ones in between: short (p' - 1 rows), empty, separated, NaN / inf / 1e150, all-zero y."""
    rng = np.random.default_rng(321)
    pp = p + int(bias)
    kinds = ["good", "short", "good", "empty", "separated", "good", "nan", "inf", "huge", "good", "zeros", "good"]
    sizes = [scale * s for s in (100, 0, 130, 0, 40, 200, 50, 70, 90, 90, 80, 129)]
    sizes[1] = pp - 1
    X, y, off = gc.family_frame(rng, family, sizes, p)
    for g, kind in enumerate(kinds):
        a, b = off[g], off[g + 1]
        if kind == "separated":
            y[a:b] = (X[a:b, 0] > 0).astype(np.float64)
        elif kind == "nan":
            X[a + 3, 0] = np.nan
        elif kind == "inf":
            y[a + 5] = np.inf
        elif kind == "huge":
            X[a + 7, p - 1] = 1e150
        elif kind == "zeros":
            y[a:b] = 0.0
    return X, y, off, kinds, sizes


@pytest.mark.parametrize("split", [None, 64])
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("p", [1, 4, 16])
def test_edges(pds, orc, p, bias, split):
    """`split`: the context option glm_split_rows.  None: every group is fitted by the one-wave kernel; 64: the frame's group sizes
    are doubled and every group of more than 64 rows -- the separated, poisoned and all-zero ones among them -- takes the
    full-device iteration instead, with the same contract."""
    X, y, off, kinds, sizes = edge_frame(p, bias, scale=1 if split is None else 2)
    pp = p + int(bias)
    ctx = None
    if split is not None:
        ctx = pds.Context()
        ctx.set_option("glm_split_rows", split)
        assert sum(s > split for s in sizes) >= 9
    co, it, nu, pred, rn = glm_by(pds, X, y, off, "binomial", bias, return_pred=True, ctx=ctx)
    for g, kind in enumerate(kinds):
        short = sizes[g] < pp
        if kind in ("short", "empty"):
            assert short and nu[g] == 1 and it[g] == 0 and np.isnan(co[g]).all()
        else:
            assert nu[g] == int(not np.isfinite(co[g]).all()), (g, kind)
        if kind == "zeros":
            # the oracle drifts to max_iter with a bias near -100; without an intercept and with features of both signs an all-zero
            # target has a finite fit, which the oracle finds: then the group is held to the parity bound like any other
            a, b = off[g], off[g + 1]
            with np.errstate(all="ignore"):
                b_o, it_o = orc.glm_irls(X[a:b], y[a:b], family="binomial", add_bias=bias, tol=TOL, max_iter=MAX_ITER)
            if np.isfinite(b_o).all() and it_o < MAX_ITER:
                err = np.linalg.norm(co[g] - b_o) / np.linalg.norm(b_o)
                print(f"all-zero group p={p} bias={bias}: the oracle converges in {it_o}; rel err {err:.3e}, n_iter {it[g]}")
                assert nu[g] == 0 and err < 1e-9 and abs(int(it[g]) - it_o) <= 1
            else:
                assert nu[g] == 1 or it[g] == MAX_ITER, (it[g], co[g])
        if kind == "good":
            assert nu[g] == 0
    # every good group: the same bits as in a frame without the bad groups
    good = [g for g, k in enumerate(kinds) if k == "good"]
    rows = np.concatenate([np.arange(off[g], off[g + 1]) for g in good])
    off2 = gc.offsets([sizes[g] for g in good])
    co2, it2, nu2, pred2, rn2 = glm_by(pds, X[rows], y[rows], off2, "binomial", bias, return_pred=True, ctx=ctx)
    assert np.array_equal(co[good].view(np.uint8), co2.view(np.uint8))
    assert np.array_equal(it[good], it2) and np.array_equal(nu[good], nu2)
    assert np.array_equal(pred[rows].view(np.uint8), pred2.view(np.uint8)) and not rn[rows].any()
    # rows of null groups, and only those, are null
    gid = np.repeat(np.arange(len(sizes)), sizes)
    assert np.array_equal(rn, nu[gid]) and np.isnan(pred[rn == 1]).all() and np.isfinite(pred[rn == 0]).all()


def test_determinism(pds):
    X, y, off = config_frame("binomial", 8)
    a = glm_by(pds, X, y, off, "binomial", True, return_pred=True)
    b = glm_by(pds, X, y, off, "binomial", True, return_pred=True)
    for u, v in zip(a, b):
        assert np.array_equal(u.view(np.uint8), v.view(np.uint8))


@pytest.mark.parametrize("family,bias,p", [("binomial", True, 1), ("binomial", False, 4), ("poisson", True, 16), ("gamma", False, 8),
                                           ("gaussian", True, 4)])
def test_residency_and_split_off(pds, orc, family, bias, p):
    """One group of every size from p' to 1 100 rows (both sides of the 128 resident rows); the same frame with glm_split_rows = 300:
    the groups above it go through the full-device iteration, the ones below keep their bits.  (Configurations whose smallest
    groups the oracle fits: it leaves 0 .. 4 of these ~1 090 groups open, 0.37 % at most; binomial targets with 4 features + bias or
    with 8 features leave 0.8 - 1.0 % open -- their groups of p' .. 25 rows are mostly separated -- which is beyond (1)'s allowance.)"""
    pp = p + int(bias)
    rng = np.random.default_rng(123)
    sizes = np.arange(pp, 1101)
    X, y, off = gc.family_frame(rng, family, sizes, p)
    co_o, it_o = gc.oracle_by(orc, X, y, off, family, bias, TOL, MAX_ITER)
    co, it, nu, pred, rn = glm_by(pds, X, y, off, family, bias, return_pred=True)
    conv = check_parity(co, it, nu, co_o, it_o, MAX_ITER, 1e-9, f"sizes {family}")
    ctx = pds.Context()
    ctx.set_option("glm_split_rows", 300)
    co2, it2, nu2, pred2, rn2 = glm_by(pds, X, y, off, family, bias, return_pred=True, ctx=ctx)
    check_parity(co2, it2, nu2, co_o, it_o, MAX_ITER, 1e-9, f"sizes {family} split 300")
    small = sizes <= 300
    assert np.array_equal(co[small].view(np.uint8), co2[small].view(np.uint8)) and np.array_equal(it[small], it2[small])
    rows_small = np.repeat(small, sizes)
    assert np.array_equal(pred[rows_small].view(np.uint8), pred2[rows_small].view(np.uint8))
    big = np.nonzero(~small & conv)[0]
    gid = np.repeat(np.arange(len(sizes)), sizes)
    eta = np.einsum("ij,ij->i", X, co2[gid][:, :p]) + (co2[gid][:, p] if bias else 0.0)
    rows_big = np.isin(gid, big)
    mu = gc.inv_link(family, eta[rows_big])
    assert np.allclose(pred2[rows_big], mu, rtol=1e-12, atol=1e-12) and not rn2[rows_big].any()


@pytest.mark.parametrize("p", [1, 8, 16])
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("family", gc.FAMILIES)
def test_pred(pds, family, bias, p):
    """mu of every row = g^-1(x . beta_g) recomputed from the RETURNED coefficients: 1e-12 absolute (binomial), 1e-12 relative
    (the other links); null rows exactly those of null groups.  Identity link: mu IS the dot product, which cancels to values near
    zero, and two summation orders of it differ by rounding of its TERMS -- relative to |mu| that has no bound (1.3e-11 against an
    einsum where mu = 1e-5) -- so for the gaussian family the recomputation follows the device's order (bias first, one fused
    multiply-add per feature: glm_cases.eta_in_kernel_order) and is held to 1e-12 relative to |mu| like the other links; in
    addition the einsum form is held to 1e-12 relative to |b0| + sum |x_j b_j|, the scale of what is summed."""
    X, y, off = config_frame(family, p)
    co, it, nu, pred, rn = glm_by(pds, X, y, off, family, bias, return_pred=True)
    gid = np.repeat(np.arange(G), np.diff(off))
    assert np.array_equal(rn, nu[gid])
    live = rn == 0
    cg = co[gid]
    eta = np.einsum("ij,ij->i", X, cg[:, :p]) + (cg[:, p] if bias else 0.0)
    if family == "gaussian":
        scale = (np.einsum("ij,ij->i", np.abs(X), np.abs(cg[:, :p])) + (np.abs(cg[:, p]) if bias else 0.0))[live]
        ds = np.abs(pred[live] - eta[live]) / scale
        print(f"pred gaussian bias={bias} p={p}: einsum order, relative to the summed terms: worst {ds.max():.3e}")
        assert ds.max() < 1e-12
        eta = np.where(live, gc.eta_in_kernel_order(X, np.where(live[:, None], cg, 0.0), bias), np.nan)
    mu = gc.inv_link(family, eta[live])
    d = np.abs(pred[live] - mu)
    ok = d <= (1e-12 if family == "binomial" else 1e-12 * np.abs(mu))
    with np.errstate(all="ignore"):
        rel = np.nanmax(np.where(d == 0.0, 0.0, d if family == "binomial" else d / np.abs(mu)))
    print(f"pred {family} bias={bias} p={p}: worst {rel:.3e}")
    assert ok.all(), f"{int((~ok).sum())} rows beyond 1e-12, worst {rel:.3e}"
    assert np.isnan(pred[~live]).all()


@pytest.mark.parametrize("space", ["device", "host"])
@pytest.mark.parametrize("bias", [True, False])
def test_lstsq_logistic_reg(pds, orc, bias, space):
    """lstsq.logistic_reg (binomial IRLS on the whole frame through pds_glm_irls_*): coefficients against orc.glm_irls under the
    one-model contract (1e-9, tests/test_linear_models.py), the fitted probabilities against the sigmoid of the RETURNED
    coefficients to 1e-12 absolute."""
    rng = np.random.default_rng(123)
    X, y, _ = gc.family_frame(rng, "binomial", [5000], 6)
    put = dev if space == "device" else (lambda a: a)
    co = pds.logistic_reg(*cols_of(X, space), target=put(y), add_bias=bias, tol=1e-10, max_iter=100)
    assert isinstance(co, np.ndarray) and co.shape == (6 + int(bias),)
    b_o, _ = orc.glm_irls(X, y, family="binomial", add_bias=bias, tol=1e-10, max_iter=100)
    err = np.linalg.norm(co - b_o) / np.linalg.norm(b_o)
    pr = np_(pds.logistic_reg(*cols_of(X, space), target=put(y), add_bias=bias, tol=1e-10, max_iter=100, return_pred=True))
    want = gc.inv_link("binomial", X @ co[:6] + (co[6] if bias else 0.0))
    print(f"lstsq.logistic_reg bias={bias} {space}: coefficients {err:.3e}, pred {np.abs(pr - want).max():.3e}")
    assert err < 1e-9 and pr.shape == (5000,) and np.abs(pr - want).max() < 1e-12


def test_argument_errors(pds):
    from polars_ds_extension_amd import _lib

    X, y, off = config_frame("gaussian", 1)
    with pytest.raises(_lib.PdsError, match="Empty data"):
        pds.glm_by(dev(X[:0, 0]), target=dev(y[:0]), group_offsets=dev(off[:2]), family="gaussian")
    import ctypes as C

    ctx = pds.default_context()
    lib = _lib.load()
    cols = (C.c_void_p * 2)(y.ctypes.data, X[:, 0].copy().ctypes.data)
    co = np.empty((G, 1))
    it = np.empty(G, dtype=np.int32)
    nu = np.empty(G, dtype=np.uint8)

    def call(link=0, var=0, max_iter=10, coeffs=co):
        return lib.pds_glm_irls_grouped_f64(ctx._h, cols, 1, C.c_int64(len(y)), C.c_void_p(off.ctypes.data), C.c_int64(G), _lib.PDS_HOST, 0,
                                            link, var, C.c_double(1e-8), max_iter, C.c_void_p(coeffs.ctypes.data if coeffs is not None else None),
                                            C.c_void_p(it.ctypes.data), C.c_void_p(nu.ctypes.data), None, None)

    assert call(max_iter=0) == -1 and b"max_iter" in lib.pds_last_error()
    assert call(link=4) == -1 and b"unknown link / variance function" in lib.pds_last_error()
    assert call(coeffs=None) == -1 and b"null argument" in lib.pds_last_error()
    assert call() == 0
