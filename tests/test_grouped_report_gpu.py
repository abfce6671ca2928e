"""Grouped lin_reg_report (pds_lin_reg_report_grouped_* / _by_key_*) on the device, against the oracle's per-group report."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL = 1e-10
SE_KEY = {"se": "std_err", "hc0": "hc0_se", "hc1": "hc1_se", "hc2": "hc2_se", "hc3": "hc3_se"}


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


def ragged(rng, pp, big=2):
    return [0, 1, max(pp - 1, 0), pp, pp + 1] + list(rng.integers(2, 301, size=24)) + [5000] * big


def dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def cols_dev(X):
    return [dev(X[:, j]) for j in range(X.shape[1])]


def host(d):
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in d.items()}


def check_group(r, g, ro, se, dof, tol=TOL):
    key = SE_KEY[se]
    beta_o, se_o, t_o = np.asarray(ro["beta"]), np.asarray(ro["std_err"]), np.asarray(ro["t"])
    b = r["beta"][g]
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


def against_oracle(pds, orc, rng, p, bias, se, big=2, tol=TOL):
    pp = p + int(bias)
    sizes = ragged(rng, pp, big)
    X, y, off = frame(rng, sizes, p)
    r = host(pds.lin_reg_report_by(*cols_dev(X), target=dev(y), group_offsets=dev(off), add_bias=bias, std_err=se))
    assert r["beta"].shape == (len(sizes), pp)
    for g, ng in enumerate(sizes):
        if ng < pp:
            assert r["is_null"][g] == 1 and np.all(np.isnan(r["beta"][g])) and np.isnan(r["r2"][g])
            continue
        assert r["is_null"][g] == 0
        if ng == pp:
            continue  # dof 0: whatever the single report gives (NaN / inf)
        Xg, yg = X[off[g]:off[g + 1]], y[off[g]:off[g + 1]]
        Xb = np.c_[Xg, np.ones(ng)] if bias else Xg
        ro = orc.lin_reg_report(Xb, yg, y_var=float(np.var(yg, ddof=1)), std_err=se)
        # HC2 / HC3 on groups barely above p' rows: 1 - h_i cancels (leverages near 1), which amplifies the rounding of h_i
        t = (1e-6 if pp > 64 else 1e-7) if (se in ("hc2", "hc3") and ng < 3 * pp) else tol
        check_group(r, g, ro, se, float(ng - pp), t)


@pytest.mark.parametrize("se", ["se", "hc0", "hc1", "hc2", "hc3"])
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("p", [1, 3, 8, 15, 16])
def test_against_oracle(pds, orc, p, bias, se):
    against_oracle(pds, orc, np.random.default_rng(100 * p + 10 * bias + len(se)), p, bias, se)


@pytest.mark.parametrize("se", ["se", "hc1", "hc3"])
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("p", [24, 64])
def test_wide(pds, orc, p, bias, se):
    against_oracle(pds, orc, np.random.default_rng(7 * p + bias), p, bias, se, big=1, tol=1e-9 if p == 64 else TOL)


def test_too_wide(pds):
    rng = np.random.default_rng(0)
    X, y, off = frame(rng, [100, 100], 65)
    with pytest.raises(pds._lib.PdsError) as e:
        pds.lin_reg_report_by(*cols_dev(X), target=dev(y), group_offsets=dev(off))
    assert e.value.code == -5


@pytest.mark.parametrize("se", ["se", "hc1", "hc3"])
def test_f32(pds, orc, se):
    rng = np.random.default_rng(5)
    p = 8
    sizes = [0, 5, 50, 200, 1000, 3000]
    X, y, off = frame(rng, sizes, p, np.float32)
    pds.config.LIN_REG_EXPR_F64 = False
    try:
        r = host(pds.lin_reg_report_by(*cols_dev(X), target=dev(y), group_offsets=dev(off), add_bias=True, std_err=se))
    finally:
        pds.config.LIN_REG_EXPR_F64 = True
    assert r["beta"].dtype == np.float32
    for g, ng in enumerate(sizes):
        if ng < p + 1:
            assert r["is_null"][g] == 1
            continue
        Xg, yg = X[off[g]:off[g + 1]].astype(np.float64), y[off[g]:off[g + 1]].astype(np.float64)
        ro = orc.lin_reg_report(np.c_[Xg, np.ones(ng)], yg, y_var=float(np.var(yg, ddof=1)), std_err=se)
        assert np.linalg.norm(r["beta"][g] - ro["beta"]) <= 1e-4 * np.linalg.norm(ro["beta"])
        assert np.max(np.abs(r[SE_KEY[se]][g] - ro["std_err"]) / np.abs(ro["std_err"])) <= 1e-4


def test_derived_yvar(pds):
    rng = np.random.default_rng(9)
    sizes = [40, 3, 0, 700, 5000, 129]
    X, y, off = frame(rng, sizes, 4)
    y = y + 1e4  # |mean| >> std: the shifted sums matter
    yv = np.array([np.var(y[off[g]:off[g + 1]], ddof=1) if sizes[g] > 1 else np.nan for g in range(len(sizes))])
    a = host(pds.lin_reg_report_by(*cols_dev(X), target=dev(y), group_offsets=dev(off), add_bias=True))
    b = host(pds.lin_reg_report_by(*cols_dev(X), target=dev(y), group_offsets=dev(off), add_bias=True, y_var=dev(yv)))
    ok = a["is_null"] == 0
    assert np.all(np.abs(a["r2"][ok] - b["r2"][ok]) <= 1e-12 * np.maximum(1.0, np.abs(b["r2"][ok])))
    # r2 = 1 - ssr / (var n): the derived var(y) itself
    n = np.diff(off)[ok]
    ssr_a = (1.0 - a["r2"][ok]) * n
    ssr_b = (1.0 - b["r2"][ok]) * n
    assert np.allclose(ssr_b / ssr_a, 1.0, rtol=1e-11)


def test_pvalue_grid(pds):
    from polars_ds_extension_amd import _lib

    lib = _lib.load()
    ts = np.concatenate([[0.0, 1e-8, 1e-3, 0.1, 0.5], np.linspace(1.0, 40.0, 40)])
    dofs = np.array([1, 2, 3, 4, 5, 7, 10, 17, 30, 50, 100, 300, 1e3, 3e3, 1e4, 1e5, 3e5, 1e6])
    T, D = np.meshgrid(ts, dofs)
    x, df = T.ravel(), D.ravel()
    got = pds.lstsq.student_t_sf_device(x, df)
    ref = np.array([lib.pds_student_t_sf(float(a), float(b)) for a, b in zip(x, df)])
    ok = ref > 0
    rel = np.abs(got[ok] - ref[ok]) / ref[ok]
    print("p-value grid: max rel", rel.max(), "at t, dof", x[ok][rel.argmax()], df[ok][rel.argmax()])
    # the device's exp / log may differ from the host's in the last bit, and exp's argument reaches ~800 at |t| = 40: the
    # contract is 2e-13 relative (include/pds_lstsq.h)
    assert np.all(rel <= 2e-13)
    assert np.all(np.abs(got[~ok]) <= 1e-300)


def test_ci_bitwise_and_pvalues_of_own_t(pds):
    from polars_ds_extension_amd import _lib

    lib = _lib.load()
    rng = np.random.default_rng(11)
    sizes = [30, 31, 200, 200, 1000, 4]
    X, y, off = frame(rng, sizes, 3)
    r = host(pds.lin_reg_report_by(*cols_dev(X), target=dev(y), group_offsets=dev(off), add_bias=True, std_err="hc2"))
    for g, ng in enumerate(sizes):
        if r["is_null"][g] or ng == 4:
            continue  # (null, or dof 0)
        dof = float(ng - 4)
        tc = lib.pds_student_t_ppf(0.975, dof)
        se = r["hc2_se"][g]
        assert np.array_equal(r["0.025"][g], r["beta"][g] - tc * se)
        assert np.array_equal(r["0.975"][g], r["beta"][g] + tc * se)
        p_host = np.array([2.0 * lib.pds_student_t_sf(abs(float(t)), dof) for t in r["t"][g]])
        assert np.all(np.abs(r["p>|t|"][g] - p_host) <= 1e-13 * p_host)


def same(a, b):
    for k in a:
        if k == "features":
            continue
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8)), k


@pytest.mark.parametrize("se", ["se", "hc3"])
def test_forms_same_bits(pds, se):
    rng = np.random.default_rng(21)
    p = 6
    sizes = [int(s) for s in rng.integers(0, 400, size=300)] + [5000]
    sizes = [s for s in sizes if s > 0]
    X, y, off = frame(rng, sizes, p)
    keys = np.repeat(np.sort(rng.choice(10**9, size=len(sizes), replace=False)).astype(np.int64) - 5 * 10**8, sizes)
    a = host(pds.lin_reg_report_by(*cols_dev(X), target=dev(y), group_offsets=dev(off), add_bias=True, std_err=se))
    b = host(pds.lin_reg_report_by(*cols_dev(X), target=dev(y), group_offsets=dev(off), add_bias=True, std_err=se))
    same(a, b)
    hst = pds.lin_reg_report_by(*[X[:, j] for j in range(p)], target=y, group_offsets=off, add_bias=True, std_err=se)
    same(a, hst)
    ctx = pds.Context()
    ctx.set_option("report_chunk_groups", 7)
    c = host(pds.lin_reg_report_by(*cols_dev(X), target=dev(y), group_offsets=dev(off), add_bias=True, std_err=se, ctx=ctx))
    same(a, c)
    # keys in order, then shuffled: the by-key form gives the offsets form's bits
    k1 = host(pds.lin_reg_report_by_key(*cols_dev(X), target=dev(y), key=dev(keys), add_bias=True, std_err=se))
    assert np.array_equal(k1.pop("keys"), np.unique(keys))
    same(a, k1)
    perm = rng.permutation(len(y))
    k2 = pds.lin_reg_report_by_key(*[X[perm, j] for j in range(p)], target=y[perm], key=keys[perm], add_bias=True, std_err=se)
    assert np.array_equal(k2.pop("keys"), np.unique(keys))
    # ... against the offsets form on the frame in the order the stable key sort gives it (rows of a group keep their shuffled order)
    srt = perm[np.argsort(keys[perm], kind="stable")]
    a2 = pds.lin_reg_report_by(*[X[srt, j] for j in range(p)], target=y[srt], group_offsets=off, add_bias=True, std_err=se)
    same(a2, k2)


@pytest.mark.parametrize("p,bias,se", [(8, True, "hc3"), (16, True, "hc1"), (3, False, "se"), (24, True, "hc2")])
def test_skewed_groups(pds, orc, p, bias, se):
    """Groups far longer than one wave's piece (4096 rows; 16384 beyond 16 features) are split across waves and finished in piece
    order: they match the oracle, and the result does not depend on the chunking of the groups."""
    rng = np.random.default_rng(31 + p)
    pp = p + int(bias)
    sizes = [200_003, 7, 4096, 4097, 8192, 50, 0, 70_001, pp, 12, 33_000]
    X, y, off = frame(rng, sizes, p)
    r = host(pds.lin_reg_report_by(*cols_dev(X), target=dev(y), group_offsets=dev(off), add_bias=bias, std_err=se))
    for g, ng in enumerate(sizes):
        if ng < pp:
            assert r["is_null"][g] == 1
            continue
        if ng == pp:
            continue
        Xg, yg = X[off[g]:off[g + 1]], y[off[g]:off[g + 1]]
        Xb = np.c_[Xg, np.ones(ng)] if bias else Xg
        ro = orc.lin_reg_report(Xb, yg, y_var=float(np.var(yg, ddof=1)), std_err=se)
        check_group(r, g, ro, se, float(ng - pp), (1e-7 if ng < 3 * pp and se in ("hc2", "hc3") else TOL))
    ctx = pds.Context()
    ctx.set_option("report_chunk_groups", 3)
    same(r, host(pds.lin_reg_report_by(*cols_dev(X), target=dev(y), group_offsets=dev(off), add_bias=bias, std_err=se, ctx=ctx)))


def test_size_sample(pds, orc):
    import torch

    G, m, p = 200_000, 100, 16
    gen = torch.Generator(device="cuda").manual_seed(3)
    n = G * m
    Xc = [torch.randn(n, generator=gen, device="cuda", dtype=torch.float64) for _ in range(p)]
    y = sum((0.1 * (j + 1)) * Xc[j] for j in range(p)) + torch.randn(n, generator=gen, device="cuda", dtype=torch.float64)
    off = torch.arange(0, n + 1, m, dtype=torch.int64, device="cuda")
    r = pds.lin_reg_report_by(*Xc, target=y, group_offsets=off, add_bias=True, std_err="hc1")
    assert r["beta"].shape == (G, p + 1) and not bool(r["is_null"].any())
    for g in np.random.default_rng(0).choice(G, size=12, replace=False):
        sl = slice(int(g) * m, (int(g) + 1) * m)
        Xg = np.stack([c[sl].cpu().numpy() for c in Xc], axis=1)
        yg = y[sl].cpu().numpy()
        ro = orc.lin_reg_report(np.c_[Xg, np.ones(m)], yg, y_var=float(np.var(yg, ddof=1)), std_err="hc1")
        rg = {k: (v[int(g):int(g) + 1].cpu().numpy() if hasattr(v, "cpu") else v) for k, v in r.items()}
        check_group(rg, 0, ro, "hc1", float(m - p - 1))
