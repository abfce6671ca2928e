"""Grouped weighted lin_reg_report (pds_wls_report_grouped_* / _by_key_*, lstsq.lin_reg_report_by{,_key}(weights=)) on the device,
against the oracle's per-group wls_report (pl_wls_report).

Tolerances are the project's contract as the unweighted grouped test applies it: 1e-10 up to 24 features, 1e-9 at 64, with the
propagated bounds for t, p and CI (check_group, copied from tests/test_grouped_report_gpu.py).  On such inputs the oracle alone is
within 2e-12 (beta, normwise) and 7e-13 (std_err, per element) of a long-double WLS at every width up to 64."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL = 1e-10


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


def frame(rng, sizes, p, dt=np.float64):
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n = int(off[-1])
    X = rng.normal(size=(n, p))
    beta = rng.normal(size=p)
    beta[::3] = 0.0  # true zeros: p-values away from 0
    y = X @ beta + 0.7 + 0.4 * rng.normal(size=n) * (0.5 + np.abs(X[:, 0]))
    return X.astype(dt), y.astype(dt), off


def weights_for(rng, off, pp, dt=np.float64):
    """Uniform in [0.25, 4], about 5 % exact zeros.  A group keeps at least p' + 1 rows of positive weight: with p' or fewer the
    weighted fit is exact on them, sum w e^2 and every standard error are zero in exact arithmetic, and what the oracle and the
    device return there is rounding noise of the order 1e-14, against which a relative tolerance says nothing (the bound of this
    file rests on the oracle being within 7e-13 of a long-double WLS, which holds for well-posed groups only).  A group that would
    fall below takes its positive draws back; no group is left out of the comparison."""
    n = int(off[-1])
    w = rng.uniform(0.25, 4.0, size=n)
    zero = rng.random(n) < 0.05
    for g in range(len(off) - 1):
        sl = slice(off[g], off[g + 1])
        if (off[g + 1] - off[g]) - int(zero[sl].sum()) < pp + 1:
            zero[sl] = False
    w[zero] = 0.0
    return w.astype(dt)


def ragged(rng, pp, big=2):
    return [0, 1, max(pp - 1, 0), pp, pp + 1] + list(rng.integers(2, 301, size=24)) + [5000] * big


def dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def cols_dev(X):
    return [dev(X[:, j]) for j in range(X.shape[1])]


def host(d):
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in d.items()}


def check_group(r, g, ro, dof, tol=TOL, key="std_err"):
    beta_o, se_o, t_o = np.asarray(ro["beta"]), np.asarray(ro["std_err"]), np.asarray(ro["t"])
    b = r["beta"][g]
    print(f"group {g}: beta {np.linalg.norm(b - beta_o) / np.linalg.norm(beta_o):.2e} "
          f"se {np.max(np.abs(r[key][g] - se_o) / np.abs(se_o)):.2e}")
    assert np.linalg.norm(b - beta_o) <= tol * np.linalg.norm(beta_o), g
    assert np.all(np.abs(r[key][g] - se_o) <= tol * np.abs(se_o)), g
    from scipy import stats as st

    dt_bound = tol * (np.linalg.norm(beta_o) / se_o + np.abs(t_o))
    assert np.all(np.abs(r["t"][g] - t_o) <= dt_bound), g
    dp_bound = 2.0 * st.t.pdf(np.abs(t_o), dof) * dt_bound + 1e-13 * np.asarray(ro["p"])
    assert np.all(np.abs(r["p>|t|"][g] - np.asarray(ro["p"])) <= dp_bound), g
    t_crit = st.t.ppf(0.975, dof)
    ci_bound = tol * (np.linalg.norm(beta_o) + t_crit * se_o)
    assert np.all(np.abs(r["0.025"][g] - np.asarray(ro["ci_lo"])) <= ci_bound), g
    assert np.all(np.abs(r["0.975"][g] - np.asarray(ro["ci_hi"])) <= ci_bound), g
    for k in ("r2", "adj_r2"):  # (dof 1: adj_r2 is -inf on both sides)
        assert r[k][g] == ro[k] or abs(r[k][g] - ro[k]) <= tol * max(1.0, abs(ro[k])), (g, k)


def check_all(orc, r, X, y, w, off, sizes, bias, tol):
    pp = X.shape[1] + int(bias)
    assert r["beta"].shape == (len(sizes), pp)
    assert "std_err" in r
    for g, ng in enumerate(sizes):
        if ng < pp:
            assert r["is_null"][g] == 1 and np.all(np.isnan(r["beta"][g])) and np.isnan(r["r2"][g])
            continue
        assert r["is_null"][g] == 0
        if ng == pp:
            continue  # dof 0: whatever the single report gives (NaN / inf)
        sl = slice(off[g], off[g + 1])
        Xg, yg = X[sl], y[sl]
        Xb = np.c_[Xg, np.ones(ng)] if bias else Xg
        ro = orc.wls_report(Xb, yg, w[sl], y_var=float(np.var(yg, ddof=1)))
        check_group(r, g, ro, float(ng - pp), tol)


def against_oracle(pds, orc, rng, p, bias, sizes, tol=TOL):
    X, y, off = frame(rng, sizes, p)
    w = weights_for(rng, off, p + int(bias))
    # `std_err` is ignored with weights: the column is "std_err"
    r = host(pds.lin_reg_report_by(*cols_dev(X), target=dev(y), group_offsets=dev(off), add_bias=bias, weights=dev(w), std_err="hc3"))
    check_all(orc, r, X, y, w, off, sizes, bias, tol)
    return X, y, w, off, r


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("p", [1, 3, 8, 15, 16])
def test_against_oracle(pds, orc, p, bias):
    rng = np.random.default_rng(1000 + 10 * p + bias)
    against_oracle(pds, orc, rng, p, bias, ragged(rng, p + int(bias)))


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("p", [24, 64])
def test_wide(pds, orc, p, bias):
    """17 .. 64 features; one group is longer than a piece (16384 rows), so it is cut and summed in piece order"""
    rng = np.random.default_rng(77 * p + bias)
    sizes = ragged(rng, p + int(bias), big=1) + [16384 + 3001]
    against_oracle(pds, orc, rng, p, bias, sizes, tol=1e-9 if p == 64 else TOL)


def test_long_groups(pds, orc):
    """<= 16 features: groups of several 4096-row pieces, independent of the chunking"""
    rng = np.random.default_rng(41)
    p, bias = 8, True
    sizes = [20_003, 7, 4096, 4097, 8192, 50, 0, 9, 12]
    X, y, w, off, r = against_oracle(pds, orc, rng, p, bias, sizes)
    ctx = pds.Context()
    ctx.set_option("report_chunk_groups", 3)
    same(r, host(pds.lin_reg_report_by(*cols_dev(X), target=dev(y), group_offsets=dev(off), add_bias=bias, weights=dev(w), ctx=ctx)))


@pytest.mark.parametrize("p", [3, 16])
def test_f32(pds, orc, p):
    rng = np.random.default_rng(5 + p)
    sizes = ragged(rng, p + 1)
    X, y, off = frame(rng, sizes, p)
    w = weights_for(rng, off, p + 1)
    X32, y32, w32 = X.astype(np.float32), y.astype(np.float32), w.astype(np.float32)
    pds.config.LIN_REG_EXPR_F64 = False
    try:
        r = host(pds.lin_reg_report_by(*cols_dev(X32), target=dev(y32), group_offsets=dev(off), add_bias=True, weights=dev(w32)))
    finally:
        pds.config.LIN_REG_EXPR_F64 = True
    assert r["beta"].dtype == np.float32
    for g, ng in enumerate(sizes):
        if ng < p + 1:
            assert r["is_null"][g] == 1
            continue
        if ng == p + 1:
            continue
        sl = slice(off[g], off[g + 1])
        Xg, yg, wg = X32[sl].astype(np.float64), y32[sl].astype(np.float64), w32[sl].astype(np.float64)
        ro = orc.wls_report(np.c_[Xg, np.ones(ng)], yg, wg, y_var=float(np.var(yg, ddof=1)))
        eb = np.linalg.norm(r["beta"][g] - ro["beta"]) / np.linalg.norm(ro["beta"])
        es = np.max(np.abs(r["std_err"][g] - ro["std_err"]) / np.abs(ro["std_err"]))
        print(f"f32 p={p} group {g} n={ng}: beta {eb:.2e} se {es:.2e}")
        assert eb <= 1e-4 and es <= 1e-4, g


def same(a, b):
    for k in a:
        if k == "features":
            continue
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8)), k


@pytest.mark.parametrize("p", [6, 24])
def test_forms_same_bits(pds, p):
    rng = np.random.default_rng(21 + p)
    sizes = [int(s) for s in rng.integers(0, 400, size=300)] + [5000, 40_000]
    sizes = [s for s in sizes if s > 0]
    X, y, off = frame(rng, sizes, p)
    w = weights_for(rng, off, p + 1)
    keys = np.repeat(np.sort(rng.choice(10**9, size=len(sizes), replace=False)).astype(np.int64) - 5 * 10**8, sizes)
    kw = dict(add_bias=True)
    a = host(pds.lin_reg_report_by(*cols_dev(X), target=dev(y), group_offsets=dev(off), weights=dev(w), **kw))
    b = host(pds.lin_reg_report_by(*cols_dev(X), target=dev(y), group_offsets=dev(off), weights=dev(w), **kw))
    same(a, b)  # two calls: the same bits
    hst = pds.lin_reg_report_by(*[X[:, j] for j in range(p)], target=y, group_offsets=off, weights=w, **kw)
    same(a, hst)  # host and device spaces
    ctx = pds.Context()
    ctx.set_option("report_chunk_groups", 7)
    c = host(pds.lin_reg_report_by(*cols_dev(X), target=dev(y), group_offsets=dev(off), weights=dev(w), ctx=ctx, **kw))
    same(a, c)
    # ordered keys: the offsets form
    k1 = host(pds.lin_reg_report_by_key(*cols_dev(X), target=dev(y), key=dev(keys), weights=dev(w), **kw))
    assert np.array_equal(k1.pop("keys"), np.unique(keys))
    same(a, k1)
    # shuffled: the offsets form on the frame in the order the stable key sort gives it, keys ascending
    perm = rng.permutation(len(y))
    srt = perm[np.argsort(keys[perm], kind="stable")]
    a2 = pds.lin_reg_report_by(*[X[srt, j] for j in range(p)], target=y[srt], group_offsets=off, weights=w[srt], **kw)
    for space in ("host", "device"):
        if space == "host":
            k2 = pds.lin_reg_report_by_key(*[X[perm, j] for j in range(p)], target=y[perm], key=keys[perm], weights=w[perm], **kw)
        else:
            k2 = host(pds.lin_reg_report_by_key(*cols_dev(X[perm]), target=dev(y[perm]), key=dev(keys[perm]), weights=dev(w[perm]), **kw))
        assert np.array_equal(k2.pop("keys"), np.unique(keys))
        same(a2, k2)


@pytest.mark.parametrize("p", [5, 20])
def test_isolation(pds, p):
    """A neighbour group scaled by 1e6 and holding NaN / inf values and weights changes no other group's bits."""
    rng = np.random.default_rng(3 + p)
    sizes = [60, 200, 33, 5000, 90, 17_000, 45]
    X, y, off = frame(rng, sizes, p)
    w = weights_for(rng, off, p + 1)
    a = host(pds.lin_reg_report_by(*cols_dev(X), target=dev(y), group_offsets=dev(off), add_bias=True, weights=dev(w)))
    X2, y2, w2 = X.copy(), y.copy(), w.copy()
    for g in (1, 3, 5):
        sl = slice(off[g], off[g + 1])
        X2[sl] *= 1e6
        y2[sl] *= 1e6
        w2[sl] *= 1e6
        X2[off[g] + 3, 0] = np.nan
        y2[off[g] + 5] = np.inf
        w2[off[g] + 7] = np.nan
        w2[off[g + 1] - 1] = np.inf
        w2[off[g]] = 1e150
    b = host(pds.lin_reg_report_by(*cols_dev(X2), target=dev(y2), group_offsets=dev(off), add_bias=True, weights=dev(w2)))
    keep = np.array([0, 2, 4, 6])
    for k in a:
        if k == "features":
            continue
        assert np.array_equal(np.asarray(a[k])[keep].view(np.uint8), np.asarray(b[k])[keep].view(np.uint8)), k


@pytest.mark.parametrize("p,tol", [(8, TOL), (24, TOL), (64, 1e-9)])
def test_unit_weights(pds, p, tol):
    """Unit weights give the unweighted std="se" report within the contract tolerance."""
    rng = np.random.default_rng(13 + p)
    sizes = [s for s in ragged(rng, p + 1, big=1) if s > p + 1]
    X, y, off = frame(rng, sizes, p)
    u = host(pds.lin_reg_report_by(*cols_dev(X), target=dev(y), group_offsets=dev(off), add_bias=True, std_err="se"))
    r = host(pds.lin_reg_report_by(*cols_dev(X), target=dev(y), group_offsets=dev(off), add_bias=True, weights=dev(np.ones(len(y)))))
    for g, ng in enumerate(sizes):
        ro = {"beta": u["beta"][g], "std_err": u["std_err"][g], "t": u["t"][g], "p": u["p>|t|"][g], "ci_lo": u["0.025"][g],
              "ci_hi": u["0.975"][g], "r2": u["r2"][g], "adj_r2": u["adj_r2"][g]}
        check_group(r, g, ro, float(ng - p - 1), tol)


def test_zero_weight_rows_count(pds, orc):
    """Zero weights are legal: such rows still count in n_g, in dof and in the unweighted sum e^2."""
    rng = np.random.default_rng(17)
    p, sizes = 3, [40, 9, 120]
    X, y, off = frame(rng, sizes, p)
    w = weights_for(rng, off, p + 1)
    w[off[1]:off[2]] = rng.uniform(0.25, 4.0, size=9)
    w[off[1]:off[1] + 4] = 0.0  # group 1: 9 rows, 5 of positive weight, p' = 4 -> dof stays 5
    r = host(pds.lin_reg_report_by(*cols_dev(X), target=dev(y), group_offsets=dev(off), add_bias=True, weights=dev(w)))
    check_all(orc, r, X, y, w, off, sizes, True, TOL)


def test_too_wide_and_null_weights(pds):
    import ctypes as C

    rng = np.random.default_rng(0)
    X, y, off = frame(rng, [100, 100], 65)
    w = np.ones(len(y))
    # through the C entry itself (lstsq checks the width before it calls)
    from polars_ds_extension_amd import _lib, lstsq

    ctx = lstsq.default_context()
    cols = lstsq._Cols(y, [X[:, j] for j in range(65)], w)
    outs, rep = lstsq._report_grouped_outs(cols, 2, 66)
    rc = ctx.fn("pds_wls_report_grouped")(ctx._h, cols.cols, cols.weights, 65, C.c_int64(200), C.c_void_p(off.ctypes.data), C.c_int64(2),
                                          cols.space, 1, C.c_void_p(None), C.byref(rep))
    assert rc == -5
    with pytest.raises(_lib.PdsError) as e:
        pds.lin_reg_report_by(*cols_dev(X), target=dev(y), group_offsets=dev(off), weights=dev(w))
    assert e.value.code == -5
    cols = lstsq._Cols(y, [X[:, j] for j in range(3)], w)
    outs, rep = lstsq._report_grouped_outs(cols, 2, 4)
    rc = ctx.fn("pds_wls_report_grouped")(ctx._h, cols.cols, C.c_void_p(None), 3, C.c_int64(200), C.c_void_p(off.ctypes.data), C.c_int64(2),
                                          cols.space, 1, C.c_void_p(None), C.byref(rep))
    assert rc == -1
