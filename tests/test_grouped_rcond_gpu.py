"""
Grouped lin_reg_w_rcond on the device (lstsq.lin_reg_w_rcond_by / _by_key: pds_lr_rcond_grouped_* / _by_key_*,
csrc/grouped_rcond.hip) against oracle.solve_lr_rcond and np.linalg.lstsq run on every group's rows alone.

Frames: tests/rcond_cases.py -- ragged groups of sizes {p', p' + 1, 63, 64, 65, 128, 129, 300} x {full rank, duplicated column,
constant column beside a bias, all-zero column} + one group of 5 000 rows, for every width 1 .. 16 with and without a bias.  Every
call passes rcond = 1e-6; the helper asserts on every group that kept eigenvalues are >= 10 x the cut, cut ones <= cut / 10 and the
kept condition number <= 1e4, so the bounds below leave more than an order of magnitude over eps x condition number:
F64_TOL = 1e-10 (the project's f64 parity tolerance, what test_gpu_parity.py::test_rcond holds the single-system call to), 1e-10
absolute against numpy (that test's bound from the reference's own suite), F32_TOL = 1e-4 for f32 frames.
"""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import rcond_cases as rc  # noqa: E402

pytestmark = pytest.mark.gpu

F64_TOL = 1e-10
F32_TOL = 1e-4
F32_EPS = float(np.finfo(np.float32).eps)


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

    return torch.from_numpy(np.array(a, order="C")).cuda()  # (a copy: the shared frames are read-only)


def np_(v):
    return v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)


def cols_of(X, space="device"):
    cs = [np.ascontiguousarray(X[:, j]) for j in range(X.shape[1])]
    return [dev(c) for c in cs] if space == "device" else cs


def rcond_by(pds, X, y, off, bias, space="device", l2=0.0, off_on_host=False):
    put = dev if space == "device" else (lambda a: a)
    r = pds.lin_reg_w_rcond_by(*cols_of(X, space), target=put(y), group_offsets=off if off_on_host else put(off), add_bias=bias,
                               rcond=rc.RCOND, l2_reg=l2)
    return tuple(np_(v) for v in r)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else (np.uint32 if a.dtype == np.float32 else np.uint8))


_DEVICE = {}


def width_result(pds, p, bias):
    """the device result on the every-width frame, computed once and shared"""
    if (p, bias) not in _DEVICE:
        f = rc.width_frame(p, bias)
        _DEVICE[(p, bias)] = rcond_by(pds, f.X, f.y, f.off, bias)
    return _DEVICE[(p, bias)]


# ------------------------------------------------------------------------------------------------- 1. every width
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("p", rc.WIDTHS)
def test_every_width(pds, orc, p, bias):
    f = rc.width_frame(p, bias)
    rc.frame_conditions(f)  # (the conditions on the inputs, every group)
    co, sv, nu = width_result(pds, p, bias)
    co_o, sv_o = rc.oracle_by(orc, f)
    co_n, rank_n = rc.lstsq_by(f)
    assert co.shape == (f.n_groups, f.pp) and sv.shape == (f.n_groups, f.pp) and not nu.any()
    worst = [0.0, 0.0, 0.0]
    for g in range(f.n_groups):
        worst = [max(worst[0], rc.nrel(co[g], co_o[g])), max(worst[1], rc.nrel(sv[g], sv_o[g])), max(worst[2], float(np.max(np.abs(co[g] - co_n[g]))))]
    print(f"p={p} bias={bias}: worst nrel(coeffs)={worst[0]:.3e} nrel(sv)={worst[1]:.3e} |coeffs - lstsq|={worst[2]:.3e}")
    for g in range(f.n_groups):
        tag = f"p={p} bias={bias} group {g} ({f.kinds[g]}, n={int(f.off[g + 1] - f.off[g])})"
        assert rc.nrel(co[g], co_o[g]) < F64_TOL, tag
        assert rc.nrel(sv[g], sv_o[g]) < F64_TOL, tag
        assert np.max(np.abs(co[g] - co_n[g])) < 1e-10, tag
        assert np.all(np.diff(sv[g]) <= 0), tag  # descending
        if f.kinds[g] == "full":
            continue
        n = int(f.off[g + 1] - f.off[g])
        thr = rc.rcond_g(n, f.pp) * sv[g, 0]
        assert int(np.sum(sv[g] ** 2 < thr)) == f.pp - int(rank_n[g]), tag  # (the eigenvalue against rcond * s_max)
        if f.kinds[g] == "dup" and p > 1:
            assert abs(co[g, 0] - co[g, p - 1]) < 1e-10, tag
        if f.kinds[g] == "zero":
            assert abs(co[g, p // 2]) < 1e-10, tag


# ------------------------------------------------------------------------------------------------- 2. the single-system path
def _single(pds, f, g):
    s = f.rows(g)
    return pds.lin_reg_w_rcond(*cols_of(f.X[s]), target=dev(f.y[s]), add_bias=f.bias, rcond=rc.RCOND)


def test_against_single_system_call(pds):
    """20 groups of the every-width frames through lstsq.lin_reg_w_rcond on the group's rows alone, same explicit rcond: coefficients
    and singular values within F64_TOL.  The 20 are groups whose singular values the data determines to that tolerance: full rank,
    or with an all-zero column (an exact zero in both paths).  A singular value that belongs to a CUT direction of a duplicated /
    collinear column is 0 in exact arithmetic and rounding noise of the path's own Gram matrix otherwise -- up to
    sqrt(eps * ev_max) ~ 1e-8 * s_max.  The grouped kernel and the oracle form an exactly singular Gram matrix (one summation order
    for every entry) and return ~1e-78 there; the single-system call sums per-block partials, its Gram matrix is singular only to
    rounding, and it returns ~3e-9 (measured: p = 3 + bias, "const", 4 rows: 3.45e-09 against 2.43e-78, a distance of 7.1e-10 of
    ||sv||, above F64_TOL although the grouped value is the one nearer the truth).  Those groups are compared below on what the data
    determines."""
    picks = [(1, True, 0), (1, False, 3), (2, True, 4), (2, False, 28), (3, True, 3), (3, True, 12), (5, False, 8), (7, True, 7),
             (8, True, 3), (8, False, 0), (8, True, 31), (11, False, 4), (12, True, 11), (13, True, 0), (13, False, 16), (15, True, 7),
             (16, True, 0), (16, True, 3), (16, False, 20), (16, True, 32)]
    assert len(set(picks)) == 20
    for p, bias, g in picks:
        f = rc.width_frame(p, bias)
        assert f.kinds[g] in ("full", "zero")
        co, sv, _ = width_result(pds, p, bias)
        b1, s1 = _single(pds, f, g)
        tag = f"p={p} bias={bias} group {g} ({f.kinds[g]})"
        assert rc.nrel(co[g], b1) < F64_TOL, tag
        assert rc.nrel(sv[g], s1) < F64_TOL, tag


def test_against_single_system_call_rank_deficient(pds):
    """Groups with a duplicated or collinear column against the single-system call: coefficients and KEPT singular values within
    F64_TOL; the cut singular value of either path lies below the cut (see test_against_single_system_call)."""
    picks = [(2, True, 1), (3, True, 2), (3, True, 13), (8, False, 1), (8, True, 6), (12, True, 10), (13, True, 1), (16, True, 2),
             (16, False, 1), (16, True, 29)]
    for p, bias, g in picks:
        f = rc.width_frame(p, bias)
        assert f.kinds[g] in ("dup", "const")
        co, sv, _ = width_result(pds, p, bias)
        b1, s1 = _single(pds, f, g)
        n = int(f.off[g + 1] - f.off[g])
        thr = rc.rcond_g(n, f.pp) * sv[g, 0]
        kept = sv[g] ** 2 >= thr
        tag = f"p={p} bias={bias} group {g} ({f.kinds[g]})"
        assert int((~kept).sum()) == 1 and np.array_equal(kept, s1 ** 2 >= thr), tag
        assert rc.nrel(co[g], b1) < F64_TOL, tag
        assert rc.nrel(sv[g][kept], s1[kept]) < F64_TOL, tag


# ------------------------------------------------------------------------------------------------- 3. null groups and containment
def _null_frame(p, bias):
    """healthy groups (full / dup / const / zero of 40 rows) on both sides of: n = p' - 1, a NaN in x, an inf in y, an all-zero
    group, an empty group.  Returns (X, y, sizes, bad group indices)."""
    rng = np.random.default_rng(77)
    pp = p + int(bias)
    healthy = [rc.group(rng, 40, p, bias, k) for k in ("full", "dup", "const", "zero", "full", "dup")]
    short = rc.group(rng, pp - 1, p, bias, "full")
    nan_x = rc.group(rng, 50, p, bias, "full")
    nan_x[0][17, p // 2] = np.nan
    inf_y = rc.group(rng, 70, p, bias, "full")
    inf_y[1][3] = np.inf
    zero = (np.zeros((30, p)), np.zeros(30))
    empty = (np.zeros((0, p)), np.zeros(0))
    bad = [short, nan_x, inf_y, zero, empty]
    parts, bad_idx = [], []
    for k, h in enumerate(healthy):
        parts.append(h)
        if k < len(bad):
            bad_idx.append(len(parts))
            parts.append(bad[k])
    X = np.concatenate([q[0] for q in parts])
    y = np.concatenate([q[1] for q in parts])
    return X, y, [len(q[1]) for q in parts], bad_idx, healthy


@pytest.mark.parametrize("p,bias", [(3, False), (16, False), (8, True)])
def test_null_groups_and_containment(pds, p, bias):
    """Without a bias the all-zero group is the all-zero system (the reference divides by zero: null).  With one, X'X = diag(0, n)
    and X'y = 0: the zero directions are cut and the fit is the zero vector, as in the reference -- that group is then not null."""
    X, y, sizes, bad_idx, healthy = _null_frame(p, bias)
    co, sv, nu = rcond_by(pds, X, y, rc.offsets(sizes), bias)
    zero_idx = bad_idx[3]
    expect_null = set(bad_idx)
    if bias:
        expect_null.discard(zero_idx)
        assert not nu[zero_idx] and np.all(co[zero_idx] == 0.0)
    assert set(np.flatnonzero(nu).tolist()) == expect_null
    for g in expect_null:
        assert np.isnan(co[g]).all() and np.isnan(sv[g]).all()
    good = [g for g in range(len(sizes)) if g not in bad_idx]
    Xh = np.concatenate([h[0] for h in healthy])
    yh = np.concatenate([h[1] for h in healthy])
    co_h, sv_h, nu_h = rcond_by(pds, Xh, yh, rc.offsets([len(h[1]) for h in healthy]), bias)
    assert not nu_h.any() and np.isfinite(co_h).all()
    np.testing.assert_array_equal(bits(co[good]), bits(co_h))
    np.testing.assert_array_equal(bits(sv[good]), bits(sv_h))
    # offsets that leave the frame, given as a host array to the device call: a null for that group, no error
    n = len(yh)
    off = rc.offsets([len(h[1]) for h in healthy])
    for bad_off in (np.array([0, 40, n + 5, 120, 160, 200, n]), np.array([0, 40, -3, 120, 160, 200, n])):
        co_b, sv_b, nu_b = rcond_by(pds, Xh, yh, bad_off.astype(np.int64), bias, off_on_host=True)
        leaves = [g for g in range(6) if bad_off[g] < 0 or bad_off[g + 1] < bad_off[g] or bad_off[g + 1] > n]
        assert leaves and set(np.flatnonzero(nu_b).tolist()) == set(leaves)
        for g in range(6):
            if g in leaves:
                assert np.isnan(co_b[g]).all() and np.isnan(sv_b[g]).all()
            elif bad_off[g] == off[g] and bad_off[g + 1] == off[g + 1]:
                np.testing.assert_array_equal(bits(co_b[g]), bits(co_h[g]))


def test_all_zero_system_is_null(pds):
    """p' = 1 with its only column zero: the reference divides by zero there"""
    rng = np.random.default_rng(3)
    x = np.concatenate([rng.normal(size=20), np.zeros(25), rng.normal(size=20)])
    y = rng.normal(size=65)
    co, sv, nu = rcond_by(pds, x[:, None], y, np.array([0, 20, 45, 65]), False)
    assert nu.tolist() == [0, 1, 0] and np.isnan(co[1]).all() and np.isnan(sv[1]).all() and np.isfinite(co[[0, 2]]).all()


# ------------------------------------------------------------------------------------------------- 4. determinism, position independence
def _small_groups(p, bias, n_groups, seed=11):
    rng = np.random.default_rng(seed)
    sizes = rng.integers(p + int(bias), 90, size=n_groups)
    kinds = rng.choice(rc.KINDS, size=n_groups)
    gs = [rc.group(rng, int(n), p, bias, "full" if rc.excluded(p, bias, k) else k) for n, k in zip(sizes, kinds)]
    return gs


def _run_groups(pds, gs, bias):
    X = np.concatenate([q[0] for q in gs])
    y = np.concatenate([q[1] for q in gs])
    return rcond_by(pds, X, y, rc.offsets([len(q[1]) for q in gs]), bias)


@pytest.mark.parametrize("p,bias", [(2, False), (8, True), (16, True)])
def test_determinism_and_position_independence(pds, p, bias):
    gs = _small_groups(p, bias, 3000)
    a = _run_groups(pds, gs, bias)
    b = _run_groups(pds, gs, bias)
    for u, v in zip(a, b):
        np.testing.assert_array_equal(bits(u), bits(v))
    assert not a[2].any()
    perm = np.random.default_rng(5).permutation(len(gs))
    c = _run_groups(pds, [gs[k] for k in perm], bias)
    np.testing.assert_array_equal(bits(c[0]), bits(a[0][perm]))
    np.testing.assert_array_equal(bits(c[1]), bits(a[1][perm]))
    for n_groups in (1, 2):
        d = _run_groups(pds, gs[:n_groups], bias)
        np.testing.assert_array_equal(bits(d[0]), bits(a[0][:n_groups]))
        np.testing.assert_array_equal(bits(d[1]), bits(a[1][:n_groups]))


def test_more_groups_than_the_grid_holds(pds):
    """the grid is as many workgroups as are resident at once (at most 28 per CU): 40 000 groups make every wave walk several"""
    gs = _small_groups(2, True, 3000, seed=12)
    many = (gs * 14)[:40000]
    a = _run_groups(pds, gs, True)
    m = _run_groups(pds, many, True)
    idx = np.arange(40000) % 3000
    np.testing.assert_array_equal(bits(m[0]), bits(a[0][idx]))
    np.testing.assert_array_equal(bits(m[1]), bits(a[1][idx]))


# ------------------------------------------------------------------------------------------------- 5. key form
@pytest.mark.parametrize("p,bias", [(3, True), (16, False)])
def test_key_form(pds, p, bias):
    f = rc.width_frame(p, bias)
    co, sv, nu = width_result(pds, p, bias)
    sizes = np.diff(f.off)
    labels = np.sort(np.random.default_rng(5).choice(10 * f.n_groups, size=f.n_groups, replace=False)).astype(np.int64) - 100
    key = np.repeat(labels, sizes)
    r = pds.lin_reg_w_rcond_by_key(*cols_of(f.X), target=dev(f.y), key=dev(key), add_bias=bias, rcond=rc.RCOND)
    k1, co1, sv1, nu1 = (np_(v) for v in r)
    np.testing.assert_array_equal(k1, labels)  # ascending
    np.testing.assert_array_equal(bits(co1), bits(co))  # ordered keys: the offsets form bit for bit
    np.testing.assert_array_equal(bits(sv1), bits(sv))
    assert not nu1.any()
    perm = np.random.default_rng(6).permutation(len(key))
    r = pds.lin_reg_w_rcond_by_key(*cols_of(f.X[perm]), target=dev(f.y[perm]), key=dev(key[perm]), add_bias=bias, rcond=rc.RCOND)
    k2, co2, sv2, nu2 = (np_(v) for v in r)
    np.testing.assert_array_equal(k2, labels)
    for g in range(f.n_groups):
        assert rc.nrel(co2[g], co[g]) < F64_TOL and rc.nrel(sv2[g], sv[g]) < F64_TOL, g
    # max_groups too small: PDS_ERR_INVALID, *n_groups set; the wrapper's retry succeeds
    from polars_ds_extension_amd import _lib, lstsq

    ctx = lstsq.default_context()
    cols = lstsq._Cols(dev(f.y), cols_of(f.X))
    kd = dev(key)
    cap = 5
    out_k, out_c, out_s, out_n = dev(np.zeros(cap, np.int64)), dev(np.zeros((cap, f.pp))), dev(np.zeros((cap, f.pp))), dev(np.zeros(cap, np.uint8))
    ng = C.c_int64(0)
    rcode = ctx._lib.pds_lr_rcond_by_key_f64(ctx._h, cols.cols, C.c_void_p(kd.data_ptr()), p, C.c_int64(len(key)), _lib.PDS_DEVICE, int(bias),
                                             C.c_double(0.0), C.c_double(rc.RCOND), C.c_int64(cap), C.c_void_p(out_k.data_ptr()),
                                             C.c_void_p(out_c.data_ptr()), C.c_void_p(out_s.data_ptr()), C.c_void_p(out_n.data_ptr()),
                                             C.byref(ng))
    assert rcode == -1 and ng.value == f.n_groups  # PDS_ERR_INVALID
    with pytest.raises(_lib.PdsError):
        pds.lin_reg_w_rcond_by_key(*cols_of(f.X), target=dev(f.y), key=kd, add_bias=bias, rcond=rc.RCOND, max_groups=cap)
def test_key_form_wrapper_retries(pds):
    """2^21 one-row groups: more distinct keys than the wrapper's first capacity (2^20), so its first call returns PDS_ERR_INVALID
    with the count and the second call fits.  p' = 1: x b = y, singular value |x|."""
    n = 1 << 21
    rng = np.random.default_rng(8)
    x = rng.uniform(1.0, 2.0, size=n)
    y = rng.normal(size=n)
    keys, co, sv, nu = (np_(v) for v in pds.lin_reg_w_rcond_by_key(dev(x), target=dev(y), key=dev(np.arange(n, dtype=np.int64)), rcond=rc.RCOND))
    assert len(keys) == n and co.shape == (n, 1) and not nu.any()
    np.testing.assert_array_equal(keys, np.arange(n))
    np.testing.assert_allclose(co[:, 0], y / x, rtol=1e-14)
    np.testing.assert_allclose(sv[:, 0], x, rtol=1e-14)


# ------------------------------------------------------------------------------------------------- 6. f32 frames
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("p", [1, 4, 8, 16])
def test_f32_frames(pds, orc, p, bias):
    f = rc.width_frame(p, bias)
    rc.frame_conditions(f, F32_EPS, np.float32)  # the gap conditions with the f32 cut, on the f32-rounded data
    co_o, sv_o = rc.oracle_by(orc, f, F32_EPS, np.float32)  # f64 oracle on the f32-rounded data
    pds.config.LIN_REG_EXPR_F64 = False
    try:
        co, sv, nu = rcond_by(pds, f.X.astype(np.float32), f.y.astype(np.float32), f.off, bias)
    finally:
        pds.config.LIN_REG_EXPR_F64 = True
    assert co.dtype == np.float32 and sv.dtype == np.float32 and not nu.any()
    worst = [max(rc.nrel(co[g], co_o[g]) for g in range(f.n_groups)), max(rc.nrel(sv[g], sv_o[g]) for g in range(f.n_groups))]
    print(f"f32 p={p} bias={bias}: worst nrel(coeffs)={worst[0]:.3e} nrel(sv)={worst[1]:.3e}")
    for g in range(f.n_groups):
        assert rc.nrel(co[g], co_o[g]) < F32_TOL and rc.nrel(sv[g], sv_o[g]) < F32_TOL, (p, bias, g, f.kinds[g])


# ------------------------------------------------------------------------------------------------- 7. l2_reg
@pytest.mark.parametrize("p", [3, 16])
def test_l2_reg(pds, orc, p):
    f = rc.width_frame(p, True)
    co_o, sv_o = rc.oracle_by(orc, f, l2=0.5)
    co, sv, nu = rcond_by(pds, f.X, f.y, f.off, True, l2=0.5)
    assert not nu.any()
    for g in range(f.n_groups):
        assert rc.nrel(co[g], co_o[g]) < F64_TOL and rc.nrel(sv[g], sv_o[g]) < F64_TOL, (p, g, f.kinds[g])
        if f.kinds[g] == "dup":  # the duplicated column keeps all its singular values (the penalty lifts the zero eigenvalue)
            n = int(f.off[g + 1] - f.off[g])
            assert np.all(sv[g] ** 2 >= rc.rcond_g(n, f.pp) * sv[g, 0]), (p, g)


# ------------------------------------------------------------------------------------------------- 8. host frames and the plugin
def test_host_frames_and_plugin(pds):
    import pyarrow as pa

    from plugin_harness import call_plugin
    from polars_ds_extension_amd import _lib

    p, bias = 5, True
    f = rc.build_frame(41, p, bias, sizes=(6, 7, 64, 129), long_rows=0)
    co, sv, nu = rcond_by(pds, f.X, f.y, f.off, bias)
    co_h, sv_h, nu_h = rcond_by(pds, f.X, f.y, f.off, bias, space="host")
    assert isinstance(co_h, np.ndarray)
    np.testing.assert_array_equal(bits(co_h), bits(co))
    np.testing.assert_array_equal(bits(sv_h), bits(sv))
    np.testing.assert_array_equal(nu_h, nu)
    key = np.repeat(np.arange(f.n_groups, dtype=np.int64) * 3 - 7, np.diff(f.off))
    ins = [("k", pa.array(key, type=pa.int64())), ("y", pa.array(f.y))] + [(f"x{j + 1}", pa.array(f.X[:, j])) for j in range(p)]
    kw = {"bias": bias, "null_policy": "raise", "l1_reg": 0.0, "l2_reg": 0.0, "solver": "", "tol": rc.RCOND}
    field, out = call_plugin(_lib.load(), "pl_lr_w_rcond_by", ins, kw)
    assert [q.name for q in out.type] == ["k", "coeffs", "singular_values"] and len(out) == f.n_groups
    assert out.field(0).to_pylist() == sorted(set(key.tolist()))
    np.testing.assert_array_equal(bits(np.array(out.field(1).to_pylist())), bits(co))
    np.testing.assert_array_equal(bits(np.array(out.field(2).to_pylist())), bits(sv))
