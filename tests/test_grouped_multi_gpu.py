"""
The grouped multi-target fit on the device (lstsq.lin_reg_multi_by / _by_key: pds_lr_multi_grouped_* / _by_key_*,
csrc/grouped_multi.hip and the per-target route) against oracle.solve_lr_gated run on every group's rows alone, against
lin_reg_by, and against itself under another placement, another route and another memory space.

Frames: tests/multi_cases.py -- ragged groups of {0, 1, p' - 1, p', p' + 1, 63, 64, 65, 128, 129, 200} rows x {full rank, an exactly
duplicated column, a constant column beside the intercept}; targets linear in X plus noise, the last of two or more identically
zero.  tests/test_grouped_multi_cpu.py asserts that every fitted group's gate statistic lies 1e3 below 1 / singular_x_tol and every
degenerate group's 1e3 beyond it, so no tolerance decides a null flag here.  Bounds: normwise relative error 1e-9 per group and
target against the QR oracle (what test_gpu_parity.py::test_grouped_by_key_any_row_order holds lin_reg_by_key to; the frames'
cond(X'X) stays below 1e3, so eps x cond leaves six orders), F32_TOL = 1e-4 for f32 frames (tests/test_grouped_rcond_gpu.py),
1e-12 of the row scale for pred / resid (tests/test_grouped_pred.py).
"""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import multi_cases as mc  # noqa: E402

pytestmark = pytest.mark.gpu

F64_TOL = 1e-9
F32_TOL = 1e-4
LIMIT = "grouped multi-target lin_reg: up to 16 feature columns and 15 targets"
PAIR_IDS = [f"P{p}-k{k}" for p, k in mc.PAIRS]


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


@pytest.fixture(scope="module")
def ctx(pds):
    """a context of the module's own: the route and the grid cap are set per call and put back"""
    c = pds.Context(0)
    yield c
    c.close()


def dev(a):
    import torch

    return torch.from_numpy(np.array(a, order="C")).cuda()  # (a copy: the shared frames are read-only)


def np_(v):
    return v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)


def cols_of(M, put):
    return [put(np.ascontiguousarray(M[:, j])) for j in range(M.shape[1])]


def fit(pds, ctx, f, route=1, space="device", waves=0, **kw):
    put = dev if space == "device" else (lambda a: np.array(a, order="C"))
    ctx.set_option("grouped_multi_route", route)
    ctx.set_option("grouped_multi_waves", waves)
    try:
        r = pds.lin_reg_multi_by(*cols_of(f.X, put), targets=cols_of(f.T, put), group_offsets=put(f.off), add_bias=f.bias, ctx=ctx, **kw)
    finally:
        ctx.set_option("grouped_multi_route", 0)
        ctx.set_option("grouped_multi_waves", 0)
    return tuple(np_(v) for v in r)


def single_by(pds, f, t=0, **kw):
    """lin_reg_by on target t of the same frame"""
    co, nu = pds.lin_reg_by(*cols_of(f.X, dev), target=dev(f.T[:, t]), group_offsets=dev(f.off), add_bias=f.bias, **kw)
    return np_(co), np_(nu)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else (np.uint32 if a.dtype == np.float32 else np.uint8))


def worst_nrel(co, ref, nu):
    w = 0.0
    for g in np.flatnonzero(~nu.astype(bool)):
        for t in range(co.shape[1]):
            w = max(w, mc.nrel(co[g, t], ref[g, t]))
    return w


def check_against_oracle(f, co, nu, co_o, nu_o, tol, l2=0.0):
    assert co.shape == (f.n_groups, f.k, f.pp) and nu.shape == (f.n_groups,)
    want = np.array([f.expect_null(g, l2) for g in range(f.n_groups)])
    assert np.array_equal(nu.astype(bool), want)  # the frame's construction
    assert np.array_equal(nu_o, want)             # ... which the oracle's gate sees the same way
    assert np.isnan(co[want]).all() and np.isfinite(co[~want]).all()  # null for every target or for none
    w = worst_nrel(co, co_o, nu)
    print(f"P={f.p} k={f.k} bias={f.bias} l2={l2}: worst nrel against the oracle {w:.3e}")
    assert w <= tol


# ------------------------------------------------------------------------------------------------- 1. parity, route 1
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("p,k", mc.PAIRS, ids=PAIR_IDS)
def test_parity(pds, orc, ctx, p, k, bias):
    f = mc.pair_frame(p, k, bias)
    co, nu = fit(pds, ctx, f, route=1)
    co_o, nu_o = mc.oracle_by(orc, f, key=(p, k, bias))
    check_against_oracle(f, co, nu, co_o, nu_o, F64_TOL)
    _, nu_1 = single_by(pds, f)
    assert np.array_equal(nu, nu_1)  # lin_reg_by's flags, group for group


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("p,k", [(2, 2), (8, 8), (16, 15)])
def test_ridge(pds, orc, ctx, p, k, bias):
    f = mc.pair_frame(p, k, bias)
    co, nu = fit(pds, ctx, f, route=1, l2_reg=0.1)
    co_o, nu_o = mc.oracle_by(orc, f, l2=0.1, key=(p, k, bias))
    check_against_oracle(f, co, nu, co_o, nu_o, F64_TOL, l2=0.1)
    _, nu_1 = single_by(pds, f, l2_reg=0.1)
    assert np.array_equal(nu, nu_1)


# ------------------------------------------------------------------------------------------------- 2. the two routes
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("p,k", [(1, 1), (7, 3), (8, 8), (16, 15), (8, 1)])
def test_routes_agree(pds, ctx, p, k, bias):
    f = mc.pair_frame(p, k, bias)
    co1, nu1 = fit(pds, ctx, f, route=1)
    co2, nu2 = fit(pds, ctx, f, route=2)
    co0, nu0 = fit(pds, ctx, f, route=0)
    assert np.array_equal(nu1, nu2) and np.array_equal(nu1, nu0)
    w = max(worst_nrel(co1, co2, nu1), worst_nrel(co0, co2, nu1))
    print(f"P={p} k={k} bias={bias}: worst nrel route 1 / 0 against route 2 {w:.3e}")
    assert w <= F64_TOL
    assert np.isnan(co2[nu2.astype(bool)]).all()
    if k == 1:
        co_s, nu_s = single_by(pds, f)
        assert np.array_equal(nu1, nu_s)
        assert worst_nrel(co1, co_s[:, None, :], nu1) <= F64_TOL


def test_a_nan_in_one_target_nulls_the_group(pds, ctx):
    f = mc.pair_frame(7, 3, True)
    g = next(g for g in range(f.n_groups) if f.n_of(g) == 65 and f.kinds[g] == "full")
    T = np.array(f.T)
    T[int(f.off[g]) + 3, 1] = np.nan
    f2 = mc.Frame(f.X, T, f.off, f.kinds, f.p, f.k, f.bias)
    base = fit(pds, ctx, f, route=1)
    for route in (1, 2):
        co, nu = fit(pds, ctx, f2, route=route)
        assert nu[g] == 1 and np.isnan(co[g]).all()
        others = np.arange(f.n_groups) != g
        assert np.array_equal(nu[others], base[1][others])
        if route == 1:  # a bad group never changes another group's bits
            assert np.array_equal(bits(co[others]), bits(base[0][others]))


# ------------------------------------------------------------------------------------------------- 3. placement
@pytest.mark.parametrize("p,k,bias", [(2, 2, False), (8, 8, True), (16, 15, True)])
def test_placement_does_not_change_a_bit(pds, ctx, p, k, bias):
    f = mc.pair_frame(p, k, bias)
    co, nu = fit(pds, ctx, f, route=1)
    co_again, _ = fit(pds, ctx, f, route=1)
    assert np.array_equal(bits(co), bits(co_again))
    co_r, nu_r = fit(pds, ctx, f.reversed(), route=1)  # the same groups in reversed order
    assert np.array_equal(nu_r[::-1], nu) and np.array_equal(bits(co_r[::-1]), bits(co))
    co_1, nu_1 = fit(pds, ctx, f, route=1, waves=1)    # one wave walks every group
    assert np.array_equal(nu_1, nu) and np.array_equal(bits(co_1), bits(co))


def test_more_groups_than_the_grid_holds(pds, ctx):
    """every wave of the grid walks several groups: 40 000 groups of 8 rows, each against its neighbour's bits under another grid"""
    rng = np.random.default_rng(11)
    G, n, p, k = 40_000, 8, 3, 2
    f = mc.Frame(rng.normal(size=(G * n, p)), rng.normal(size=(G * n, k)), np.arange(0, G * n + 1, n, dtype=np.int64), ["full"] * G, p, k, True)
    co, nu = fit(pds, ctx, f, route=1)
    co_c, nu_c = fit(pds, ctx, f, route=1, waves=7)
    assert not nu.any() and np.array_equal(bits(co), bits(co_c))
    for g in (0, 1, G // 2, G - 1):
        A, T = mc.design(f.X[f.rows(g)], True), f.T[f.rows(g)]
        assert mc.nrel(co[g].T, np.linalg.lstsq(A, T, rcond=None)[0]) <= 1e-8


# ------------------------------------------------------------------------------------------------- 4. the gate
@pytest.mark.parametrize("kw", [{"solver": "choleskey"}, {"singular_x_tol": 0.0}], ids=["choleskey", "gate-off"])
@pytest.mark.parametrize("route", [1, 2])
def test_gate_variants_flag_like_lin_reg_by(pds, ctx, kw, route):
    f = mc.pair_frame(7, 3, True)  # (full, dup and const groups)
    co, nu = fit(pds, ctx, f, route=route, **kw)
    flags = [single_by(pds, f, t, **kw)[1] for t in range(f.k)]
    assert np.array_equal(nu, flags[0])
    assert all(np.array_equal(nu, fl) for fl in flags)  # (the gate depends on X alone)
    ok = ~nu.astype(bool)
    for t in range(f.k):
        co_t = single_by(pds, f, t, **kw)[0]
        assert max((mc.nrel(co[g, t], co_t[g]) for g in np.flatnonzero(ok) if not f.expect_null(g)), default=0.0) <= F64_TOL
    assert np.isnan(co[~ok]).all()


# ------------------------------------------------------------------------------------------------- 5. f32 frames
@pytest.mark.parametrize("route", [1, 2])
@pytest.mark.parametrize("p,k,bias", [(2, 2, True), (8, 8, False), (16, 15, True)])
def test_f32_frames(pds, orc, ctx, p, k, bias, route):
    f = mc.pair_frame(p, k, bias)
    pds.config.LIN_REG_EXPR_F64 = False
    try:
        co, nu = fit(pds, ctx, f, route=route)
    finally:
        pds.config.LIN_REG_EXPR_F64 = True
    assert co.dtype == np.float32
    co_o, nu_o = mc.oracle_by(orc, f, dtype=np.float32, key=(p, k, bias))
    check_against_oracle(f, co, nu, co_o, nu_o, F32_TOL)


# ------------------------------------------------------------------------------------------------- 6. by key, pred / resid
def keyed(f):
    """keys 7 g - 20 of the frame's non-empty groups (ascending key order = group order), and the group of every row"""
    sizes = np.array([f.n_of(g) for g in range(f.n_groups)])
    gid = np.repeat(np.arange(f.n_groups), sizes)
    return gid * 7 - 20, gid, np.flatnonzero(sizes > 0)


def by_key(pds, ctx, f, key, rows, route, space="device", **kw):
    put = dev if space == "device" else (lambda a: np.array(a, order="C"))
    ctx.set_option("grouped_multi_route", route)
    try:
        r = pds.lin_reg_multi_by_key(*cols_of(f.X[rows], put), targets=cols_of(f.T[rows], put), key=put(key[rows]), add_bias=f.bias, ctx=ctx, **kw)
    finally:
        ctx.set_option("grouped_multi_route", 0)
    return tuple(np_(v) for v in r)


@pytest.mark.parametrize("route", [1, 2])
@pytest.mark.parametrize("p,k,bias", [(2, 2, False), (7, 3, True), (16, 15, True)])
def test_by_key_and_pred(pds, ctx, p, k, bias, route):
    f = mc.pair_frame(p, k, bias)
    key, gid, live = keyed(f)
    co, nu = fit(pds, ctx, f, route=route)
    n = len(key)
    perm = np.random.default_rng(5).permutation(n)
    for rows in (np.arange(n), perm):  # ordered keys (nothing moves), shuffled keys (sort + gather)
        ks, co_k, nu_k, pred, resid, rn = by_key(pds, ctx, f, key, rows, route, return_pred=True)
        assert np.array_equal(ks, live * 7 - 20) and np.array_equal(nu_k, nu[live])
        # (a regression does not depend on the order of a group's rows beyond rounding; ordered keys are the offsets form's frame,
        #  and route 1 gives a group the same bits wherever it stands)
        assert worst_nrel(co_k, co[live], nu_k) <= (0.0 if rows is not perm and route == 1 else F64_TOL)
        assert pred.shape == (k, n) and resid.shape == (k, n) and rn.shape == (n,)
        g_of = gid[rows]
        assert np.array_equal(rn.astype(bool), nu[g_of].astype(bool))  # row_null on the rows of null groups
        okr = ~rn.astype(bool)
        A = mc.design(f.X[rows], bias)
        for t in range(k):
            want = np.einsum("ij,ij->i", A, co[g_of, t])
            scale = np.einsum("ij,ij->i", np.abs(A), np.abs(co[g_of, t])) + np.abs(f.T[rows, t])
            assert np.all(np.abs(pred[t] - want)[okr] <= 1e-12 * scale[okr] + 1e-300)
            assert np.all(np.abs(resid[t] - (f.T[rows, t] - want))[okr] <= 1e-12 * scale[okr] + 1e-300)
            assert np.isnan(pred[t][~okr]).all() and np.isnan(resid[t][~okr]).all()
    if route == 1:  # the offsets form's own per-row outputs: the ordered by-key call's, bit for bit
        _, _, pred_o, resid_o, rn_o = fit(pds, ctx, f, route=route, return_pred=True)
        _, _, _, pred_k, resid_k, rn_k = by_key(pds, ctx, f, key, np.arange(n), route, return_pred=True)
        assert np.array_equal(bits(pred_o), bits(pred_k)) and np.array_equal(bits(resid_o), bits(resid_k)) and np.array_equal(rn_o, rn_k)


def test_by_key_max_groups(pds, ctx):
    f = mc.pair_frame(2, 2, False)
    key, _, live = keyed(f)
    rows = np.arange(len(key))
    with pytest.raises(Exception, match="more distinct keys than max_groups"):
        by_key(pds, ctx, f, key, rows, 1, max_groups=len(live) - 1)
    ks, co, nu = by_key(pds, ctx, f, key, rows, 1, max_groups=len(live))
    assert len(ks) == len(live) and co.shape == (len(live), 2, 2)


# ------------------------------------------------------------------------------------------------- 7. host against device
@pytest.mark.parametrize("route", [1, 2])
@pytest.mark.parametrize("p,k,bias", [(7, 3, True), (16, 15, False)])
def test_host_frame_same_bits(pds, ctx, p, k, bias, route):
    f = mc.pair_frame(p, k, bias)
    d = fit(pds, ctx, f, route=route, return_pred=True)
    h = fit(pds, ctx, f, route=route, space="host", return_pred=True)
    assert all(isinstance(v, np.ndarray) for v in h)
    for a, b in zip(d, h):
        assert a.shape == b.shape and np.array_equal(bits(a), bits(b))
    key, _, _ = keyed(f)
    rows = np.random.default_rng(6).permutation(len(key))
    dk = by_key(pds, ctx, f, key, rows, route, return_pred=True)
    hk = by_key(pds, ctx, f, key, rows, route, space="host", return_pred=True)
    for a, b in zip(dk, hk):
        assert a.shape == b.shape and np.array_equal(bits(a), bits(b))


# ------------------------------------------------------------------------------------------------- 8. limits and bad offsets
def test_limits(pds, ctx):
    x = dev(np.arange(12.0))
    off = dev(np.array([0, 6, 12]))
    with pytest.raises(NotImplementedError, match=LIMIT):
        pds.lin_reg_multi_by(*[x] * 17, targets=[x, x], group_offsets=off, ctx=ctx)
    with pytest.raises(NotImplementedError, match=LIMIT):
        pds.lin_reg_multi_by(x, targets=[x] * 16, group_offsets=off, ctx=ctx)
    with pytest.raises(NotImplementedError, match=LIMIT):
        pds.lin_reg_multi_by_key(*[x] * 17, targets=[x], key=dev(np.zeros(12, dtype=np.int64)), ctx=ctx)
    # the C ABI itself refuses the same way
    import ctypes as C

    from polars_ds_extension_amd import _lib

    cols = (C.c_void_p * 33)(*[int(x.data_ptr())] * 33)
    out = dev(np.zeros(2 * 16 * 17))
    nu = dev(np.zeros(2, dtype=np.uint8))
    args = (C.c_int64(12), C.c_void_p(int(off.data_ptr())), C.c_int64(2), _lib.PDS_DEVICE, 0, C.c_double(0.0), 0, C.c_double(1e-12),
            C.c_void_p(int(out.data_ptr())), C.c_void_p(int(nu.data_ptr())), None, None, None)
    for k, p in ((16, 1), (1, 17)):
        rc = ctx._lib.pds_lr_multi_grouped_f64(ctx._h, cols, k, p, *args)
        assert rc == -5 and ctx._lib.pds_last_error().decode() == LIMIT  # PDS_ERR_UNSUPPORTED


def test_offsets_that_leave_the_frame_read_nothing(pds, ctx):
    """route 1: such a group is null and the others keep their bits; a call that would walk the offsets elsewhere falls back to it"""
    f = mc.pair_frame(7, 3, True)
    co, nu = fit(pds, ctx, f, route=1)
    n = len(f.X)
    g = next(g for g in range(f.n_groups) if f.n_of(g) == 64 and f.kinds[g] == "full")
    off = np.array(f.off)
    off[g + 1:] += 10 * n  # group g now ends far past the frame, and every later group lies outside it
    f2 = mc.Frame(f.X, f.T, off, f.kinds, f.p, f.k, f.bias)
    for route in (1, 0, 2):
        co2, nu2 = fit(pds, ctx, f2, route=route)
        assert nu2[g:].all() and np.isnan(co2[g:]).all()
        assert np.array_equal(nu2[:g], nu[:g]) and np.array_equal(bits(co2[:g]), bits(co[:g]))
    with pytest.raises(Exception, match="group_offsets must be non-decreasing and inside the frame"):
        fit(pds, ctx, f2, route=1, return_pred=True)
