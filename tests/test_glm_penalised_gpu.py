"""
Penalised GLM fits on the device (lstsq.glm_by / glm_by_key / linear_models.GLM with l1_reg / l2_reg: pds_glm_enet_*,
csrc/grouped_irls.hip PEN = 1, csrc/capi_models.hpp) against beta*, the minimiser the NumPy restatement reaches at tol 1e-13
(tests/glm_penalised_reference.py, recorded in tests/golden/glm_penalised_refs.npz; tests/test_glm_penalised_cpu.py holds beta* to
the optimality conditions of the objective).

The tolerance rule.  No tolerance is fixed in advance: for every case the restatement's own run at the kernel's `tol` and inner
constant has a worst error against beta* and a worst KKT residual on the same data; the device must stay within 10 x each, with a
floor of 1e-12 (`cases.bound`).  The margin of 10 covers the summation order of the matrix-core Gram fed through the conditioning
of the system.  Every check prints its figures before it asserts.
"""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import glm_cases as gc  # noqa: E402
import glm_penalised_cases as pc  # noqa: E402
import glm_penalised_reference as ref  # noqa: E402

pytestmark = pytest.mark.gpu

GROUPED = [pc.name_of(f, p, b, l1, l2) for f, p, b in pc.GROUPED_CONFIGS for l1, l2 in pc.PENALTIES]
BY_KEY_CASE = pc.name_of("binomial", 8, 1, pc.L1, pc.L2)


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


def fit(pds, r, dtype=np.float64, **kw):
    """lstsq.glm_by on a case's frame with its penalties, inputs resident on the device"""
    X, y = r["X"].astype(dtype), r["y"].astype(dtype)
    out = pds.glm_by(*[dev(X[:, j]) for j in range(X.shape[1])], target=dev(y), group_offsets=dev(r["off"]), family=r["family"],
                     add_bias=r["bias"], tol=r["tol"], max_iter=pc.MAX_ITER, l1_reg=r["l1"], l2_reg=r["l2"], **kw)
    return tuple(np_(v) for v in out)


_FITS = {}


def grouped_fit(pds, name):
    if name not in _FITS:
        _FITS[name] = fit(pds, pc.reference(name))
    return _FITS[name]


def check_rule(name, r, co, what="", rows=slice(None)):
    """coefficients against beta* and their KKT residual, each within 10 x the restatement's own figure (floor 1e-12)"""
    co = np.asarray(co, dtype=np.float64)
    err = float(np.abs(co - r["star"])[rows].max())
    kk = float(ref.kkt(r["X"], r["y"], r["off"], r["family"], r["bias"], r["l1"], r["l2"], co)[rows].max())
    print(f"{name}{what}: |b - b*| {err:.3e} (restatement {r['helper_err']:.3e}, bound {pc.bound(r['helper_err']):.3e}); "
          f"KKT {kk:.3e} (restatement {r['helper_kkt']:.3e}, bound {pc.bound(r['helper_kkt']):.3e})")
    # measured on an MI355X: l1 cases |b - b*| 8.2e-12 .. 1.0e-9 and KKT 8.7e-13 .. 7.7e-11, each 1.000 x the
    # restatement's own figure; ridge-only cases <= 9.9e-14 / 4.7e-15 under the 1e-12 floor; f32 frame 1.44e-7 / 2.5e-8 against the
    # restatement's 1.40e-7 / 2.5e-8
    assert err <= pc.bound(r["helper_err"]), f"{name}{what}: coefficients {err:.3e} > {pc.bound(r['helper_err']):.3e}"
    assert kk <= pc.bound(r["helper_kkt"]), f"{name}{what}: KKT residual {kk:.3e} > {pc.bound(r['helper_kkt']):.3e}"


# ---- 1. grouped parity against beta*
@pytest.mark.parametrize("name", GROUPED)
def test_grouped_parity(pds, name):
    r = pc.reference(name)
    co, it, nu = grouped_fit(pds, name)
    assert co.shape == r["star"].shape and not nu.any() and (it < pc.MAX_ITER).all() and (it > 0).all()
    print(f"{name}: mean n_iter {it.mean():.2f} (restatement {r['n_iter'].mean():.2f}), restatement sweeps per group {r['sweeps'].mean():.0f}")
    check_rule(name, r, co)
    if r["family"] == "gaussian" and r["l1"] <= 0.0:  # the closed form (X'X + n l2 D)^-1 X'y
        p = r["p"]
        for g in range(len(co)):
            a, b = int(r["off"][g]), int(r["off"][g + 1])
            Z = np.c_[r["X"][a:b], np.ones(b - a)] if r["bias"] else r["X"][a:b]
            D = np.diag(np.r_[np.ones(p), np.zeros(Z.shape[1] - p)])
            want = np.linalg.solve(Z.T @ Z + (b - a) * r["l2"] * D, Z.T @ r["y"][a:b])
            assert np.linalg.norm(co[g] - want) <= 1e-12 * np.linalg.norm(want), (name, g)


# ---- 2. exact zeros
def test_exact_zeros(pds):
    zeros = total = 0
    for name in GROUPED:
        r = pc.reference(name)
        if r["l1"] <= 0.0:
            continue
        p = r["p"]
        co = grouped_fit(pds, name)[0]
        edge = np.abs(ref.mean_gradient(r["X"], r["y"], r["off"], r["family"], r["bias"], r["star"]) - r["l1"]) < 1e-6
        out = (edge & (r["star"][:, :p] == 0.0)).any(axis=1)  # a zero feature sits on the edge |g_j| = l1: the group is left out
        assert out.mean() <= 0.02, (name, int(out.sum()))
        assert np.array_equal((co[:, :p] == 0.0)[~out], (r["star"][:, :p] == 0.0)[~out]), name
        if r["family"] == "binomial":
            zeros += int((co[:, :p] == 0.0).sum())
            total += co[:, :p].size
    print(f"binomial l1 cases: {zeros} of {total} feature coefficients are exactly zero")
    assert 0.1 < zeros / total < 0.9


# ---- 3. zero penalty: the new symbols with (0, 0) are the old ones, bit for bit
def test_zero_penalty_is_the_unpenalised_fit(pds, monkeypatch):
    import ctypes as C

    from polars_ds_extension_amd import linear_models, lstsq

    r = pc.reference(BY_KEY_CASE)
    cols = [dev(r["X"][:, j]) for j in range(r["p"])]
    key = dev(np.repeat(np.arange(60, dtype=np.int64), np.diff(r["off"])))
    kw = dict(target=dev(r["y"]), family="binomial", add_bias=True, tol=pc.TOL, max_iter=pc.MAX_ITER)
    old = [np_(v) for v in pds.glm_by(*cols, group_offsets=dev(r["off"]), **kw)]
    old_k = [np_(v) for v in pds.glm_by_key(*cols, key=key, **kw)]
    m_old = linear_models.GLM(family="binomial", add_bias=True, tol=pc.TOL).fit(r["X"][:400], r["y"][:400])
    calls = []

    def zeros(l1, l2):
        calls.append((l1, l2))
        return (C.c_double(0.0), C.c_double(0.0))

    monkeypatch.setattr(lstsq, "_pen_args", zeros)  # (a non-empty tuple selects pds_glm_enet_*)
    new = [np_(v) for v in pds.glm_by(*cols, group_offsets=dev(r["off"]), **kw)]
    new_k = [np_(v) for v in pds.glm_by_key(*cols, key=key, **kw)]
    m_new = linear_models.GLM(family="binomial", add_bias=True, tol=pc.TOL).fit(r["X"][:400], r["y"][:400])
    assert len(calls) == 3
    for a, b in zip(old + old_k, new + new_k):
        assert a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))
    assert np.array_equal(m_old.coeffs(), m_new.coeffs()) and m_old.bias() == m_new.bias() and m_old.n_iter_ == m_new.n_iter_


# ---- 4. determinism
def test_penalised_calls_are_bit_equal(pds):
    r = pc.reference(pc.name_of("binomial", 16, 1, pc.L1, pc.L2))
    a, b = fit(pds, r, return_pred=True), fit(pds, r, return_pred=True)
    for u, v in zip(a, b):
        assert np.array_equal(u.view(np.uint8), v.view(np.uint8))


# ---- 5. separation
def test_separated_groups_have_a_ridge_fit(pds):
    """Perfectly separated groups (one feature, y = [x > 0]) with l2 = 0.1: finite, short of max_iter, within the rule of beta*.
    (The unpenalised call leaves the same groups null or at max_iter: tests/test_grouped_glm_gpu.py::test_edges.)"""
    r = pc.reference("separated")
    co, it, nu = fit(pds, r)
    assert np.isfinite(co).all() and not nu.any() and (it < pc.MAX_ITER).all()
    check_rule("separated", r, co)


# ---- 6. by key
def test_by_key_on_shuffled_rows(pds):
    r = pc.reference(BY_KEY_CASE)
    sizes = np.diff(r["off"])
    key = np.repeat(np.arange(60, dtype=np.int64) * 5 - 40, sizes)
    perm = np.random.default_rng(3).permutation(len(key))
    X, y = r["X"][perm], r["y"][perm]
    out = pds.glm_by_key(*[dev(X[:, j]) for j in range(r["p"])], target=dev(y), key=dev(key[perm]), family="binomial", add_bias=True,
                         tol=pc.TOL, max_iter=pc.MAX_ITER, l1_reg=r["l1"], l2_reg=r["l2"], return_pred=True)
    ks, co, it, nu, pred, rn = (np_(v) for v in out)
    assert np.array_equal(ks, np.arange(60) * 5 - 40) and not nu.any() and not rn.any()
    check_rule(BY_KEY_CASE, r, co, " by key")
    # 8. pred at the rows' own positions
    gid = (key[perm] + 40) // 5
    eta = gc.eta_in_kernel_order(X, co[gid], True)
    want = gc.inv_link("binomial", eta)
    assert np.abs(pred - want).max() <= 1e-13 * np.abs(want).max() and (np.abs(pred - want) <= 1e-13 * np.abs(want)).all()


# ---- 7. long groups: the one-model route
@pytest.mark.parametrize("name", [pc.name_of("binomial", 8, 1, *pen) for pen in pc.PENALTIES] + [pc.name_of("gamma", 16, 1, pc.L1, pc.L2)])
def test_long_groups_take_the_one_model_route(pds, name):
    """glm_split_rows = 300: the six 1 100-row groups leave the kernel for the one-model penalised iteration; same rule"""
    r = pc.reference(name)
    ctx = pds.Context()
    ctx.set_option("glm_split_rows", 300)
    co, it, nu, pred, rn = fit(pds, r, ctx=ctx, return_pred=True)
    long_g = np.flatnonzero(np.diff(r["off"]) > 300)
    assert len(long_g) == 6 and not nu.any() and (it < pc.MAX_ITER).all()
    check_rule(name, r, co, " split 300, long groups", rows=long_g)
    check_rule(name, r, co, " split 300, all groups")
    short = np.setdiff1d(np.arange(60), long_g)
    assert np.array_equal(co[short].view(np.uint8), grouped_fit(pds, name)[0][short].view(np.uint8))  # the others: the kernel's bits
    gid = np.repeat(np.arange(60), np.diff(r["off"]))
    want = gc.inv_link(r["family"], gc.eta_in_kernel_order(r["X"], co[gid], True))
    assert (np.abs(pred - want) <= 1e-13 * np.abs(want)).all() and not rn.any()


def test_glm_class_wide_one_model(pds):
    """GLM(family="binomial", l1_reg, l2_reg) at 20 features x 500 rows: the wide one-model route against beta*"""
    from polars_ds_extension_amd import linear_models

    r = pc.reference("wide")
    m = linear_models.GLM(family="binomial", add_bias=True, tol=pc.TOL, l1_reg=r["l1"], l2_reg=r["l2"]).fit(r["X"], r["y"])
    assert 1 < m.n_iter_ < pc.MAX_ITER
    co = np.r_[m.coeffs(), m.bias()][None, :]
    check_rule("wide", r, co)
    assert np.array_equal(co[:, :20] == 0.0, r["star"][:, :20] == 0.0) and (co[:, :20] == 0.0).any()


# ---- 8. return_pred, offsets form
def test_return_pred_offsets_form(pds):
    r = pc.reference(BY_KEY_CASE)
    co, it, nu, pred, rn = fit(pds, r, return_pred=True)
    gid = np.repeat(np.arange(60), np.diff(r["off"]))
    want = gc.inv_link("binomial", gc.eta_in_kernel_order(r["X"], co[gid], True))
    assert (np.abs(pred - want) <= 1e-13 * np.abs(want)).all() and not rn.any()
    assert np.array_equal(co.view(np.uint8), grouped_fit(pds, BY_KEY_CASE)[0].view(np.uint8))


# ---- 9. f32 frames
def test_f32_frames(pds):
    """binomial, 8 + bias, (l1, l2), f32 frame: f64 arithmetic on the f32-rounded data, coefficients returned in f32, tol 1e-6,
    against beta* of the f32-rounded data.  The bound is the same rule with the restatement's coefficients rounded to f32."""
    r = pc.reference(pc.F32_CASE)
    pds.config.LIN_REG_EXPR_F64 = False
    try:
        co, it, nu = fit(pds, r, dtype=np.float32)
    finally:
        pds.config.LIN_REG_EXPR_F64 = True
    assert co.dtype == np.float32 and not nu.any() and (it < pc.MAX_ITER).all()
    check_rule(pc.F32_CASE, r, co)


# ---- 10. the plugin
def test_plugin_calls_equal_lstsq(pds):
    import ctypes as C

    import pyarrow as pa
    from plugin_harness import call_plugin

    from polars_ds_extension_amd import _lib

    _lib.load()
    lib = C.CDLL(str(_lib.LIB_PATH))
    r = pc.reference(BY_KEY_CASE)
    rows = slice(0, int(r["off"][40]))  # (the first 40 groups)
    X, y = r["X"][rows], r["y"][rows]
    key = np.repeat(np.arange(40, dtype=np.int64) * 3 - 7, np.diff(r["off"])[:40])
    perm = np.random.default_rng(4).permutation(len(key))
    X, y, key = X[perm], y[perm], key[perm]
    ins = [("k", pa.array(key)), ("y", pa.array(y))] + [(f"x{j + 1}", pa.array(np.ascontiguousarray(X[:, j]))) for j in range(8)]
    kw = {"bias": True, "null_policy": "raise", "family": "binomial", "tol": pc.TOL, "max_iter": pc.MAX_ITER, "l1_reg": pc.L1, "l2_reg": pc.L2}
    _, out = call_plugin(lib, "pl_glm_by", ins, kw)
    _, pred = call_plugin(lib, "pl_glm_by_pred", ins, kw)
    ks, co, it, nu, pr, rn = pds.glm_by_key(*[np.ascontiguousarray(X[:, j]) for j in range(8)], target=y, key=key, family="binomial",
                                            add_bias=True, tol=pc.TOL, max_iter=pc.MAX_ITER, l1_reg=pc.L1, l2_reg=pc.L2, return_pred=True)
    assert out.field(0).to_pylist() == ks.tolist() and out.field(2).to_pylist() == it.tolist() and not nu.any()
    got = np.array([c.as_py() for c in out.field(1)])
    assert np.array_equal(got.view(np.uint8), np.ascontiguousarray(co).view(np.uint8)) and (got[:, :8] == 0.0).any()
    assert pred.null_count == 0 and np.array_equal(pred.to_numpy(zero_copy_only=False).view(np.uint8), pr.view(np.uint8))
    _, plain = call_plugin(lib, "pl_glm_by", ins, {k: v for k, v in kw.items() if not k.endswith("_reg")})
    assert not (np.array(plain.field(1)[39].as_py())[:8] == 0.0).any()  # (the 1 100-row group without the penalties: no zeros)
