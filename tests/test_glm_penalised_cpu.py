"""Penalised GLM fits without a GPU: the NumPy restatement against its own optimality conditions (and scikit-learn where it
imports), the record in tests/golden against the restatement, the public signatures, the C ABI surface, and the plugin layer on the
mock device -- penalty kwargs reach pds_glm_enet_*, and an unpenalised call never does."""
import ctypes as C
import inspect
import re
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import glm_penalised_cases as pc  # noqa: E402
import glm_penalised_reference as ref  # noqa: E402
from test_grouped_glm_cpu import CALLS, _glm_frame, _inputs, mock, orc  # noqa: E402,F401  (the mock library, old symbols bound)

ENET = ["pds_glm_enet_f64", "pds_glm_enet_f32", "pds_glm_enet_grouped_f64", "pds_glm_enet_grouped_f32", "pds_glm_enet_by_key_f64",
        "pds_glm_enet_by_key_f32"]


# ------------------------------------------------------------------------------------------------- the restatement and its record
@pytest.mark.parametrize("name", pc.ALL_CASES)
def test_recorded_star_is_optimal(name):
    """KKT(beta*) <= 1e-12 for every recorded case, from the frame in np.longdouble: no solver takes part in this check."""
    r = pc.reference(name)
    assert np.isfinite(r["star"]).all() and np.isfinite(r["helper"]).all()
    assert (r["n_iter"] < pc.MAX_ITER).all() and (r["n_iter"] > 0).all()  # no null group, none at max_iter
    k = ref.kkt(r["X"], r["y"], r["off"], r["family"], r["bias"], r["l1"], r["l2"], r["star"])
    assert k.max() <= 1e-12, f"{name}: KKT residual of beta* {k.max():.3e}"


RECOMPUTED = [pc.name_of("binomial", 1, 0, *pen) for pen in pc.PENALTIES] + [pc.name_of("gaussian", 8, 1, *pen) for pen in pc.PENALTIES] + \
             [pc.name_of("binomial", 16, 1, 0.0, pc.L2), pc.F32_CASE, "separated", "wide"]


@pytest.mark.parametrize("name", RECOMPUTED)
def test_record_is_what_the_restatement_gives(name):
    """The cases that cost well under a second, recomputed: the record is the restatement's output (1e-13: another BLAS may sum in
    another order), iteration counts to the letter."""
    got, r = pc.compute(name), pc.reference(name)
    assert np.abs(got["star"] - r["star"]).max() <= 1e-13 and np.abs(got["helper"] - r["helper"]).max() <= 1e-13
    assert np.array_equal(got["n_iter"], r["n_iter"])


def test_exact_zeros_and_supports():
    """the l1 cases zero between 10 % and 90 % of the binomial feature coefficients, and the restatement at the kernel's tolerance
    finds beta*'s support in every group"""
    zeros = total = 0
    for name in pc.ALL_CASES:
        r = pc.reference(name)
        if r["l1"] <= 0.0:
            assert not (r["star"] == 0.0).any()
            continue
        p = r["p"]
        assert np.array_equal(r["star"][:, :p] == 0.0, r["helper"][:, :p] == 0.0), name
        if r["family"] == "binomial" and name != "wide":
            zeros += int((r["star"][:, :p] == 0.0).sum())
            total += r["star"][:, :p].size
    assert 0.1 < zeros / total < 0.9


def test_first_step_inside_the_threshold_does_not_end_the_fit():
    """A group whose first step lands on beta = 0 (every feature inside the l1 threshold of the system built at the starting mu) is
    not finished: the stopping rule starts with the second iteration, and the result satisfies the optimality conditions."""
    rng = np.random.default_rng(5)
    x = rng.normal(size=(40, 1))
    y = (rng.uniform(size=40) < 0.5).astype(np.float64)
    off = np.array([0, 40])
    co, it, _ = ref.fit(x, y, off, "binomial", False, 0.5, 0.0, tol=1e-10)
    assert it[0] >= 2 and co[0, 0] == 0.0
    assert ref.kkt(x, y, off, "binomial", False, 0.5, 0.0, co).max() <= 1e-12


def test_binomial_ridge_against_sklearn():
    """l2-only binomial fits against LogisticRegression(C = 1 / (n l2), solver="newton-cholesky", tol=1e-12).  sklearn stops at a
    gradient of 1e-12 of the same objective, whose Hessian is at least l2 = 0.05 on the features: a few 1e-11 in the coefficients;
    the bound is 1e-9."""
    lm = pytest.importorskip("sklearn.linear_model")
    r = pc.reference(pc.name_of("binomial", 8, 1, 0.0, pc.L2))
    worst = 0.0
    for g in range(0, 60, 3):
        a, b = int(r["off"][g]), int(r["off"][g + 1])
        sk = lm.LogisticRegression(C=1.0 / ((b - a) * pc.L2), solver="newton-cholesky", tol=1e-12, max_iter=200).fit(r["X"][a:b], r["y"][a:b])
        worst = max(worst, float(np.abs(np.r_[sk.coef_.ravel(), sk.intercept_] - r["star"][g]).max()))
    print(f"beta* against scikit-learn: worst {worst:.3e}")
    assert worst < 1e-9


# ------------------------------------------------------------------------------------------------- signatures and the C ABI surface
def test_signatures_and_defaults():
    import polars_ds_extension_amd as pds
    from polars_ds_extension_amd import linear_models, polars_exprs

    for fn in (pds.glm_by, pds.glm_by_key, linear_models.GLM.__init__, polars_exprs.glm_by_group):
        sig = inspect.signature(fn)
        assert sig.parameters["l1_reg"].default == 0.0 and sig.parameters["l2_reg"].default == 0.0, fn
    names = list(inspect.signature(linear_models.GLM.__init__).parameters)
    assert names[-2:] == ["l1_reg", "l2_reg"]  # after the existing arguments
    m = linear_models.GLM(family="binomial", l1_reg=-1.0, l2_reg=0.3)
    assert (m.l1_reg, m.l2_reg) == (0.0, 0.3)  # a penalty <= 0 means none


def test_exported_and_declared():
    from polars_ds_extension_amd import _lib

    assert all(n in _lib.EXPORTS for n in ENET)
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "pds_lstsq.h").read_text(), flags=re.S)
    for n in ENET:
        assert len(re.findall(rf"^int\s+{n}\s*\(", text, flags=re.M)) == 1, n
    sys.path.insert(0, str(ROOT / "tests" / "mock_device"))
    try:
        import build as mock_build
    finally:
        sys.path.pop(0)
    protos = {name: [a for _, a in args] for _, name, args in mock_build.prototypes()}
    for kind in ("", "_grouped", "_by_key"):
        for sfx in ("f64", "f32"):
            old, new = protos[f"pds_glm_irls{kind}_{sfx}"], protos[f"pds_glm_enet{kind}_{sfx}"]
            at = old.index("variance") + 1
            assert new == old[:at] + ["l1_reg", "l2_reg"] + old[at:]  # the twin's list, the penalties after `variance`


# ------------------------------------------------------------------------------------------------- the plugin layer on the mock device
PEN_CALLS = []  # (entry point, l1_reg, l2_reg) of every penalised call the mock saw


@pytest.fixture(scope="module")
def pen_mock(mock):  # noqa: F811
    """the mock library with pds_glm_enet_grouped_* / _by_key_* bound to callbacks built from the restatement"""
    lib = mock
    keep = []

    def view(ptr, n, dt):
        return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(np.ctypeslib.as_ctypes_type(dt))), shape=(n,))

    def frame(cols_p, n_feat, n, dt):
        ptrs = C.cast(cols_p, C.POINTER(C.c_void_p))
        cols = [view(ptrs[c], n, dt).copy().astype(np.float64) for c in range(n_feat + 1)]
        return np.stack(cols[1:], axis=1), cols[0]

    def fill(X, y, off, bias, link, l1, l2, tol, max_iter, co_p, it_p, nu_p, pred, rnull, rows, dt):
        fam = {0: "gaussian", 1: "poisson", 2: "binomial", 3: "gamma"}[link]
        ng, pp = len(off) - 1, X.shape[1] + int(bool(bias))
        b, k, _ = ref.fit(X, y, off, fam, bool(bias), l1, l2, tol=float(tol), max_iter=int(max_iter))
        nu = (~np.isfinite(b).all(axis=1)).astype(np.uint8)
        view(co_p, ng * pp, dt).reshape(ng, pp)[:] = b
        view(it_p, ng, np.int32)[:] = k
        view(nu_p, ng, np.uint8)[:] = nu
        gid = np.repeat(np.arange(ng), np.diff(off))
        eta = np.einsum("ij,ij->i", X, b[gid, :X.shape[1]]) + (b[gid, -1] if bias else 0.0)
        if pred is not None:
            pred[rows] = np.where(nu[gid] != 0, np.nan, ref.inv_link(fam, eta))
        if rnull is not None:
            rnull[rows] = nu[gid]

    def make_grouped(dt, ct):
        def fn(ctx, cols_p, n_feat, n, off_p, ng, space, bias, link, var, l1, l2, tol, max_iter, co_p, it_p, nu_p, pred_p, rn_p):
            PEN_CALLS.append(("enet_grouped", l1, l2))
            X, y = frame(cols_p, n_feat, n, dt)
            fill(X, y, view(off_p, ng + 1, np.int64).copy(), bias, link, l1, l2, tol, max_iter, co_p, it_p, nu_p,
                 view(pred_p, n, dt) if pred_p else None, view(rn_p, n, np.uint8) if rn_p else None, np.arange(n), dt)
            return 0

        return C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, ct,
                           ct, ct, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)(fn)

    def make_by_key(dt, ct):
        def fn(ctx, cols_p, keys_p, n_feat, n, space, bias, link, var, l1, l2, tol, max_iter, max_groups, ok_p, co_p, it_p, nu_p, ng_p,
               pred_p, rn_p):
            PEN_CALLS.append(("enet_by_key", l1, l2))
            keys = view(keys_p, n, np.int64)
            order = np.argsort(keys, kind="stable")
            uniq, counts = np.unique(keys[order], return_counts=True)
            C.c_int64.from_address(ng_p).value = len(uniq)
            if len(uniq) > max_groups:
                lib.mock_set_error(b"more distinct keys than max_groups")
                return -1
            X, y = frame(cols_p, n_feat, n, dt)
            view(ok_p, len(uniq), np.int64)[:] = uniq
            fill(X[order], y[order], np.concatenate([[0], np.cumsum(counts)]), bias, link, l1, l2, tol, max_iter, co_p, it_p, nu_p,
                 view(pred_p, n, dt) if pred_p else None, view(rn_p, n, np.uint8) if rn_p else None, order, dt)
            return 0

        return C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, ct, ct, ct,
                           C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)(fn)

    for sfx, dt, ct in (("f64", np.float64, C.c_double), ("f32", np.float32, C.c_float)):
        for name, cb in ((f"pds_glm_enet_grouped_{sfx}", make_grouped(dt, ct)), (f"pds_glm_enet_by_key_{sfx}", make_by_key(dt, ct))):
            keep.append(cb)
            getattr(lib, "mock_bind_" + name)(C.cast(cb, C.c_void_p))
    lib._glm_pen_keep = keep
    return lib


GKW = {"bias": True, "null_policy": "raise", "family": "binomial", "tol": 1e-10, "max_iter": 100}


def _expected(key, X, y, family, bias, l1, l2):
    order = np.argsort(key, kind="stable")
    uniq, counts = np.unique(key[order], return_counts=True)
    off = np.concatenate([[0], np.cumsum(counts)])
    b, k, _ = ref.fit(X[order], y[order], off, family, bias, l1, l2, tol=1e-10, max_iter=100)
    return uniq, b, k, order, off


def test_plugin_penalty_kwargs_reach_the_c_abi(pen_mock):
    from plugin_harness import call_plugin

    rng = np.random.default_rng(21)
    key, X, y = _glm_frame(rng, [60, 45, 80, 50], 3)
    uniq, b, k, order, off = _expected(key, X, y, "binomial", True, 0.03125, 0.0625)
    CALLS.clear()
    PEN_CALLS.clear()
    _, out = call_plugin(pen_mock, "pl_glm_by", _inputs(key, X, y), dict(GKW, l1_reg=0.03125, l2_reg=0.0625))
    assert PEN_CALLS == [("enet_by_key", 0.03125, 0.0625)] and CALLS == []  # the values unchanged, the old symbol untouched
    assert out.field(0).to_pylist() == uniq.tolist() and out.field(2).to_pylist() == k.tolist()
    assert np.array_equal(np.array([c.as_py() for c in out.field(1)]), b)
    assert (b[:, :3] == 0.0).any()  # (the l1 term bites on this frame)
    _, pred = call_plugin(pen_mock, "pl_glm_by_pred", _inputs(key, X, y), dict(GKW, l2_reg=0.0625))
    assert PEN_CALLS[-1] == ("enet_by_key", 0.0, 0.0625) and CALLS == []
    _, b2, _, _, _ = _expected(key, X, y, "binomial", True, 0.0, 0.0625)
    gid = np.searchsorted(uniq, key)
    want = ref.inv_link("binomial", np.einsum("ij,ij->i", X, b2[gid, :3]) + b2[gid, 3])
    np.testing.assert_allclose(pred.to_numpy(zero_copy_only=False), want, rtol=1e-13, atol=0)
    # f32 frames: the penalties arrive as floats
    call_plugin(pen_mock, "pl_glm_by_f32", _inputs(key, X, y, dt=np.float32), dict(GKW, tol=1e-6, l1_reg=0.03125))
    assert PEN_CALLS[-1] == ("enet_by_key", 0.03125, 0.0)


def test_plugin_nulls_path_takes_the_penalties(pen_mock):
    """a frame with nulls is prepared on the host and goes to the offsets entry point: pds_glm_enet_grouped_* when penalised"""
    from plugin_harness import call_plugin

    rng = np.random.default_rng(22)
    key, X, y = _glm_frame(rng, [70, 60], 2)
    masks = {1: np.zeros(len(y), bool)}
    masks[1][[4, 9]] = True
    PEN_CALLS.clear()
    CALLS.clear()
    call_plugin(pen_mock, "pl_glm_by", _inputs(key, X, y, masks=masks), dict(GKW, null_policy="skip", l2_reg=0.125))
    assert PEN_CALLS == [("enet_grouped", 0.0, 0.125)] and CALLS == []
    call_plugin(pen_mock, "pl_glm_by", _inputs(key, X, y, masks=masks), dict(GKW, null_policy="skip"))
    assert len(PEN_CALLS) == 1 and [c[0] for c in CALLS] == ["grouped"]


@pytest.mark.parametrize("kw", [{}, {"l1_reg": 0.0, "l2_reg": 0.0}, {"l1_reg": -1.0}])
def test_plugin_zero_penalty_reaches_the_old_symbol(pen_mock, kw):
    from plugin_harness import call_plugin

    rng = np.random.default_rng(23)
    key, X, y = _glm_frame(rng, [60, 45], 2)
    PEN_CALLS.clear()
    CALLS.clear()
    call_plugin(pen_mock, "pl_glm_by", _inputs(key, X, y), dict(GKW, **kw))
    call_plugin(pen_mock, "pl_glm_by_pred", _inputs(key, X, y), dict(GKW, **kw))
    assert PEN_CALLS == [] and [c[0] for c in CALLS] == ["by_key", "by_key"]


def test_logistic_reg_by_serves_penalised_fits(pen_mock):
    """polars_exprs.logistic_reg(..., by=k, l2_reg=0.1) builds a pl_glm_by call that carries the penalties; without `by` the refusal
    keeps its words."""
    from test_polars_exprs import pl

    from polars_ds_extension_amd import polars_exprs as px

    px.PLUGIN_PATH = Path(pen_mock._name)
    rng = np.random.default_rng(24)
    key, X, y = _glm_frame(rng, [80, 70, 90], 2)
    df = pl.DataFrame({"k": key, "y": y, "x1": X[:, 0], "x2": X[:, 1]})
    PEN_CALLS.clear()
    res = df.select(px.logistic_reg("x1", "x2", target="y", by="k", tol=1e-10, max_iter=100, l2_reg=0.1)).unnest("glm_by")
    assert PEN_CALLS == [("enet_by_key", 0.0, 0.1)]
    uniq, b, k, _, _ = _expected(key, X, y, "binomial", True, 0.0, 0.1)
    assert res["k"].to_list() == uniq.tolist() and res["n_iter"].to_list() == k.tolist()
    assert np.array_equal(np.array(res["coeffs"].to_list()), b)
    r2 = px.glm_by_group(df, "k", "x1", "x2", target="y", family="binomial", add_bias=True, tol=1e-10, l1_reg=0.05, l2_reg=0.1)
    assert PEN_CALLS[-1] == ("enet_by_key", 0.05, 0.1) and r2.columns == ["k", "coeffs", "n_iter"]
    with pytest.raises(NotImplementedError, match="logistic_reg: l1_reg / l2_reg are not supported on this backend"):
        px.logistic_reg("x1", "x2", target="y", l2_reg=0.1)


def test_lstsq_logistic_reg_still_refuses():
    import polars_ds_extension_amd as pds

    x = np.arange(12.0)
    with pytest.raises(NotImplementedError, match="logistic_reg: l1_reg / l2_reg are not supported on this backend; use GLM"):
        pds.logistic_reg(x, target=(x > 5).astype(float), l2_reg=0.1)
