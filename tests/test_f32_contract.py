"""
The f32 contract (north_star: "f32 within 1e-4"), both distances for every f32 entry point (the grouped report:
pds_lin_reg_report_grouped_f32 and pds_lin_reg_report_by_key_f32, test_grouped_report*).

For each f32 path three answers are formed on the same f32-rounded inputs:
    gpu     the HIP path (f32 symbols of the C ABI)
    orc32   the oracle's ALL-f32 arithmetic -- what "the reference's f32 path" computes
            (/root/reference/src/num_ext/linear_regression_f32.rs, lr_solvers.rs generic over f32)
    truth   the oracle in f64 on the f32-rounded inputs
and the rule is ("Next round" 1a):
    d(gpu, truth) <= 1e-4                                   the contract, or
    d(gpu, truth) <= d(orc32, truth) (+ slack for rounding order) where the reference's own f32 arithmetic is
                                                            further than 1e-4 from the truth (both are printed)
No tolerance here is looser than the contract unless the reference's own f32 error is, and then the reference's
error IS the tolerance.  d = normwise relative error on coefficient vectors (max over groups / rows where there are
many), elementwise relative with a floor for standard errors.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F32_TOL = 1e-4


@pytest.fixture(scope="module")
def pds():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import polars_ds_extension_amd as m

    return m


@pytest.fixture()
def f32(pds):
    pds.config.LIN_REG_EXPR_F64 = False
    yield
    pds.config.LIN_REG_EXPR_F64 = True


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle

    oracle.build()
    return oracle


def dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def cols_of(X):
    return [dev(X[:, j]) for j in range(X.shape[1])]


def nrel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def rowrel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.linalg.norm(a - b, axis=1) / np.maximum(np.linalg.norm(b, axis=1), 1e-300)))


def frel(a, b, floor=1e-9):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), floor)))


def hold(name, gpu, o32, truth, d=nrel, slack=1.25):
    """The contract rule of the module docstring; prints the three distances (pytest -s / on failure)."""
    dg, do, dgo = d(gpu, truth), d(o32, truth), d(gpu, o32)
    print(f"{name:46s} gpu-truth {dg:9.2e}   orc32-truth {do:9.2e}   gpu-orc32 {dgo:9.2e}")
    assert np.all(np.isfinite(np.asarray(gpu, np.float64))), name
    if dg <= F32_TOL:
        return
    assert do > F32_TOL and dg <= do * slack, (
        f"{name}: gpu is {dg:.2e} from the f64 truth (contract {F32_TOL:g}); the reference's f32 arithmetic is {do:.2e} from it")


def make_xy(rng, n, p, noise=0.01):
    X = rng.random((n, p))
    beta = np.array([(-1.0) ** j * (0.05 + 0.03 * j) for j in range(p)])
    return X, X @ beta + noise * rng.normal(size=n)


@pytest.fixture(scope="module")
def frame():
    rng = np.random.default_rng(21)
    X, y = make_xy(rng, 400_000, 8, noise=0.05)
    X32, y32 = X.astype(np.float32), y.astype(np.float32)
    return X32, y32, X32.astype(np.float64), y32.astype(np.float64)


@pytest.mark.parametrize("bias", [False, True])
def test_ols(pds, orc, f32, frame, bias):
    X32, y32, X64, y64 = frame
    b = pds.lin_reg(*cols_of(X32), target=dev(y32), add_bias=bias)
    assert b.dtype == np.float32
    hold(f"ols 4e5x8 bias={bias}", b, orc.pl_lr(X32, y32, add_bias=bias, singular_x_tol=1e-6), orc.pl_lr(X64, y64, add_bias=bias))


def test_ridge_elastic_net_nnls(pds, orc, f32, frame):
    X32, y32, X64, y64 = frame
    hold("ridge 0.1", pds.lin_reg(*cols_of(X32), target=dev(y32), l2_reg=0.1), orc.pl_lr(X32, y32, l2_reg=0.1, singular_x_tol=1e-6),
         orc.pl_lr(X64, y64, l2_reg=0.1))
    kw = dict(l1_reg=0.001, l2_reg=0.001, tol=1e-7)
    hold("elastic net", pds.lin_reg(*cols_of(X32), target=dev(y32), **kw), orc.pl_lr(X32, y32, max_iter=2000, **kw),
         orc.pl_lr(X64, y64, l1_reg=0.001, l2_reg=0.001, tol=1e-9, max_iter=2000))
    hold("nnls", pds.lin_reg(*cols_of(X32), target=dev(y32), positive=True, tol=1e-7),
         orc.pl_lr(X32, y32, positive=True, tol=1e-7, max_iter=200), orc.pl_lr(X64, y64, positive=True, tol=1e-9, max_iter=2000))


@pytest.mark.parametrize("se", ["se", "hc0", "hc1", "hc2", "hc3"])
def test_report(pds, orc, f32, frame, se):
    X32, y32, X64, y64 = frame
    r = pds.lin_reg_report(*cols_of(X32), target=dev(y32), add_bias=True, std_err=se)
    ro32 = orc.lin_reg_report(np.c_[X32, np.ones(len(y32), np.float32)], y32, std_err=se)
    ro = orc.lin_reg_report(np.c_[X64, np.ones(len(y64))], y64, std_err=se)
    key = "std_err" if se == "se" else f"{se}_se"
    hold(f"report {se}: std err", r[key], ro32["std_err"], ro["std_err"], frel)
    hold(f"report {se}: beta", r["beta"], ro32["beta"], ro["beta"])
    hold(f"report {se}: t", r["t"], ro32["t"], ro["t"], lambda a, b: frel(a, b, 1e-3))


def test_grouped(pds, orc, f32, frame):
    X32, y32, X64, y64 = frame
    NT = min(64, orc.max_threads())
    for per, bias in ((1000, False), (100, True), (100, False)):
        off = np.arange(0, 400_001, per)
        co, nu = pds.lin_reg_by(*cols_of(X32), target=dev(y32), group_offsets=off, add_bias=bias)
        c32, n32 = orc.grouped_lr([y32] + [X32[:, j] for j in range(8)], off, add_bias=bias, tol=1e-6, nthreads=NT)
        c64, n64 = orc.grouped_lr([y64] + [X64[:, j] for j in range(8)], off, add_bias=bias, nthreads=NT)
        assert not nu.cpu().numpy().any() and not n64.any()
        hold(f"grouped {len(off) - 1}x{per}x8 bias={bias}", co.cpu().numpy(), c32, c64, rowrel)
    rng = np.random.default_rng(5)
    Xn = rng.normal(size=(200_000, 8)).astype(np.float32)
    yn = (Xn @ rng.normal(size=8) + 0.1 * rng.normal(size=200_000)).astype(np.float32)
    off = np.arange(0, 200_001, 100)
    co, nu = pds.lin_reg_by(*cols_of(Xn), target=dev(yn), group_offsets=off)
    c32, _ = orc.grouped_lr([yn] + [Xn[:, j] for j in range(8)], off, tol=1e-6, nthreads=NT)
    c64, _ = orc.grouped_lr([yn.astype(np.float64)] + [Xn[:, j].astype(np.float64) for j in range(8)], off, nthreads=NT)
    hold("grouped N(0,1) 2000x100x8", co.cpu().numpy(), c32, c64, rowrel)
    # weighted groups
    w = (0.5 + rng.random(200_000)).astype(np.float32)
    co, nu = pds.lin_reg_by(*cols_of(Xn), target=dev(yn), group_offsets=off, weights=dev(w))
    sl = [slice(g * 100, (g + 1) * 100) for g in range(2000)]
    c32 = np.array([orc.weighted_lr(Xn[s_], yn[s_], w[s_]) for s_ in sl])  # faer_weighted_lr per group, all f32
    c64 = np.array([orc.weighted_lr(Xn[s_].astype(np.float64), yn[s_].astype(np.float64), w[s_].astype(np.float64)) for s_ in sl])
    hold("grouped weighted 2000x100x8", co.cpu().numpy(), c32, c64, rowrel)


@pytest.mark.parametrize("w,p", [(64, 3), (256, 8), (32, 5)])
def test_rolling(pds, orc, f32, frame, w, p):
    X32, y32, X64, y64 = frame
    n = 50_000
    co, pr, va = pds.rolling_lin_reg(*cols_of(X32[:n, :p]), target=dev(y32[:n]), window_size=w)
    assert va.cpu().numpy()[w - 1:].all()
    r32 = orc.rolling_lr(X32[:n, :p], y32[:n], w)
    r64 = orc.rolling_lr(X64[:n, :p], y64[:n], w)
    hold(f"rolling w={w} p={p} vs the f64 chain", co.cpu().numpy()[w - 1:], r32, r64, rowrel)
    # and against direct f64 window solves (the chain itself drifts)
    idx = np.arange(w - 1, n, 997)
    direct = np.array([np.linalg.lstsq(X64[i - w + 1:i + 1, :p], y64[i - w + 1:i + 1], rcond=None)[0] for i in idx])
    hold(f"rolling w={w} p={p} vs direct f64 solves", co.cpu().numpy()[idx], r32[idx - (w - 1)], direct, rowrel)


def test_recursive(pds, orc, f32, frame):
    X32, y32, X64, y64 = frame
    n = 20_000
    co, pr, va = pds.recursive_lin_reg(*cols_of(X32[:n, :3]), target=dev(y32[:n]), start_with=10)
    hold("recursive start=10 p=3", co.cpu().numpy()[9:], orc.recursive_lr(X32[:n, :3], y32[:n], 10), orc.recursive_lr(X64[:n, :3], y64[:n], 10), rowrel)


def test_coverage_paths(pds, orc, f32):
    """wide rolling (20 features + bias), grouped lasso, HC3 beyond 16 features, grouped with more than 64 features."""
    rng = np.random.default_rng(77)
    n, p, w = 3000, 20, 200
    Xw = rng.random((n, p)).astype(np.float32)
    yw = (Xw @ rng.normal(size=p) + 0.3 + 0.05 * rng.normal(size=n)).astype(np.float32)
    co, pr, va = pds.rolling_lin_reg(*cols_of(Xw), target=dev(yw), window_size=w, add_bias=True)
    Xwb = np.c_[Xw, np.ones(n, np.float32)]
    hold("wide rolling 20+bias w=200", co.cpu().numpy()[w - 1:], orc.rolling_lr(Xwb, yw, w),
         orc.rolling_lr(Xwb.astype(np.float64), yw.astype(np.float64), w), rowrel)
    G, per, q = 300, 60, 4
    Xg = rng.normal(size=(G * per, q)).astype(np.float32)
    yg = (Xg @ rng.normal(size=q) + 0.1 * rng.normal(size=G * per)).astype(np.float32)
    cl, _ = pds.lin_reg_by(*cols_of(Xg), target=dev(yg), group_offsets=np.arange(0, G * per + 1, per), l1_reg=0.01, tol=1e-7)
    sl = [slice(g * per, (g + 1) * per) for g in range(G)]
    o32 = np.array([orc.pl_lr(Xg[s], yg[s], l1_reg=0.01, tol=1e-7, max_iter=2000) for s in sl])
    o64 = np.array([orc.pl_lr(Xg[s].astype(np.float64), yg[s].astype(np.float64), l1_reg=0.01, tol=1e-10, max_iter=2000) for s in sl])
    hold("grouped lasso 300x60x4", cl.cpu().numpy(), o32, o64, rowrel)
    pw = 70
    Xh = rng.normal(size=(900, pw)).astype(np.float32)
    yh = (Xh @ rng.normal(size=pw) + 0.1 * rng.normal(size=900)).astype(np.float32)
    r = pds.lin_reg_report(*cols_of(Xh[:, :20]), target=dev(yh), std_err="hc3")
    hold("report hc3 900x20", r["hc3_se"], orc.lin_reg_report(Xh[:, :20], yh, std_err="hc3")["std_err"],
         orc.lin_reg_report(Xh[:, :20].astype(np.float64), yh.astype(np.float64), std_err="hc3")["std_err"], frel)
    cw, nw = pds.lin_reg_by(*cols_of(Xh), target=dev(yh), group_offsets=np.array([0, 400, 900]))
    assert not nw.cpu().numpy().any()
    hold("grouped > 64 features (500x70)", cw.cpu().numpy()[1], orc.pl_lr(Xh[400:], yh[400:], singular_x_tol=1e-6),
         orc.pl_lr(Xh[400:].astype(np.float64), yh[400:].astype(np.float64)))


def _grouped_report_frame(rng, p, sizes):
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    X, y = make_xy(rng, int(off[-1]), p, noise=0.05)
    return X.astype(np.float32), y.astype(np.float32), off


def _hold_grouped_report(name, r, X32, y32, off, orc, se):
    key = "std_err" if se == "se" else f"{se}_se"
    for g in range(len(off) - 1):
        sl = slice(off[g], off[g + 1])
        Xb = np.c_[X32[sl], np.ones(off[g + 1] - off[g], np.float32)]
        ro32 = orc.lin_reg_report(Xb, y32[sl], std_err=se)
        ro = orc.lin_reg_report(Xb.astype(np.float64), y32[sl].astype(np.float64), std_err=se)
        assert r["is_null"][g] == 0
        hold(f"{name} {se} g{g} ({off[g + 1] - off[g]} rows): beta", r["beta"][g], ro32["beta"], ro["beta"])
        hold(f"{name} {se} g{g}: std err", r[key][g], ro32["std_err"], ro["std_err"], frel)


@pytest.mark.parametrize("p", [3, 8, 16, 17, 32, 64])
def test_grouped_report(pds, orc, f32, p):
    """pds_lin_reg_report_grouped_f32: every standard error, groups of one piece and of several (pieces are 4096 rows up to 16
    features, 16384 beyond)."""
    rng = np.random.default_rng(900 + p)
    piece = 4096 if p <= 16 else 16384
    X32, y32, off = _grouped_report_frame(rng, p, [3 * (p + 1) + 5, 700, 2 * piece + 333])
    for se in ("se", "hc0", "hc1", "hc2", "hc3"):
        r = pds.lin_reg_report_by(*cols_of(X32), target=dev(y32), group_offsets=dev(off), add_bias=True, std_err=se)
        r = {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in r.items()}
        assert r["beta"].dtype == np.float32
        _hold_grouped_report(f"grouped report p={p}", r, X32, y32, off, orc, se)


@pytest.mark.parametrize("space", ["device", "host"])
def test_grouped_report_by_key(pds, orc, f32, space):
    """pds_lin_reg_report_by_key_f32 on shuffled keys (the sorting route), device- and host-resident."""
    rng = np.random.default_rng(950)
    p = 8
    X32, y32, off = _grouped_report_frame(rng, p, [40, 5000, 300, 9001])
    keys = np.repeat(np.array([17, -3, 40, 5], np.int64), np.diff(off))
    perm = rng.permutation(len(y32))
    if space == "device":
        r = pds.lin_reg_report_by_key(*cols_of(X32[perm]), target=dev(y32[perm]), key=dev(keys[perm]), add_bias=True, std_err="hc3")
        r = {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in r.items()}
    else:
        r = pds.lin_reg_report_by_key(*[np.ascontiguousarray(X32[perm, j]) for j in range(p)], target=y32[perm], key=keys[perm],
                                      add_bias=True, std_err="hc3")
    assert np.array_equal(r["keys"], [-3, 5, 17, 40])
    # groups in key order: the rows of each key (the rows' order within a group does not change the truth)
    order = [1, 3, 0, 2]
    Xg = np.concatenate([X32[off[g]:off[g + 1]] for g in order])
    yg = np.concatenate([y32[off[g]:off[g + 1]] for g in order])
    _hold_grouped_report(f"grouped report by key ({space})", r, Xg, yg, np.concatenate([[0], np.cumsum(np.diff(off)[order])]), orc,
                         "hc3")

