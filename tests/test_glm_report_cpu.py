"""The grouped GLM report without a GPU: the C ABI surface of pds_glm_report_grouped_* / _by_key_* (exports, header declarations, the
mock builder's view of them), the argument validation of lstsq.glm_report_by / glm_report_by_key and GLM.report(), which happens
before a device is touched, the plugin symbol pl_glm_report_by on the mock device, and the NumPy restatement the device tests measure against (tests/glm_report_reference.py) held against
closed forms."""
import math
import re
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT))

import glm_cases as gc  # noqa: E402
import glm_report_reference as rr  # noqa: E402

NEW = ["pds_glm_report_grouped_f64", "pds_glm_report_grouped_f32", "pds_glm_report_by_key_f64", "pds_glm_report_by_key_f32"]


def test_exported_and_declared():
    from polars_ds_extension_amd import _lib

    assert all(n in _lib.EXPORTS for n in NEW)
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "pds_lstsq.h").read_text(), flags=re.S)
    for n in NEW:
        assert len(re.findall(rf"^int\s+{n}\s*\(", text, flags=re.M)) == 1, n
    # the struct of output pointers: the field order the ctypes layout mirrors
    body = re.search(r"typedef struct \{([^}]*)\} pds_glm_report_out;", text, flags=re.S).group(1)
    fields = re.findall(r"\*\s*(\w+)\s*;", body)
    assert fields == [k for k, _ in _lib.GlmReportOut._fields_]
    assert fields == ["std_err", "z", "p", "ci_lower", "ci_upper", "cov", "deviance", "null_deviance", "pearson_chi2", "dispersion",
                      "df_resid", "report_null"]


def test_mock_trampolines_parse():
    sys.path.insert(0, str(ROOT / "tests" / "mock_device"))
    try:
        import build as mock_build
    finally:
        sys.path.pop(0)
    protos = {name: args for _, name, args in mock_build.prototypes()}
    irls = [a for _, a in protos["pds_glm_irls_grouped_f64"]]
    assert [a for _, a in protos["pds_glm_report_grouped_f64"]] == irls[:-2] + ["out"]  # (without pred / row_null)
    irls = [a for _, a in protos["pds_glm_irls_by_key_f32"]]
    assert [a for _, a in protos["pds_glm_report_by_key_f32"]] == irls[:-2] + ["out"]
    for n in NEW:
        assert protos[n][-1][0] == "const pds_glm_report_out*"
    assert protos["pds_glm_report_grouped_f32"][10][0] == "float" and protos["pds_glm_report_by_key_f64"][9][0] == "double"


def test_source_lists_the_kernel():
    csrc = ROOT / "polars_ds_extension_amd" / "csrc"
    assert "grouped_glm_report.hip" in (csrc / "Makefile").read_text()
    assert '#include "capi_glm_report.hpp"' in (csrc / "capi.hip").read_text()
    text = (csrc / "grouped_glm_report.hip").read_text()
    assert '#include "glm_dev.hpp"' in text and '#include "wave_tile_dev.hpp"' in text and "wave_tile_gram<P>" in text
    assert "atomicAdd(long_count" in text and text.count("atomicAdd") == 1  # (the long-group list: no atomics in any sum)


def test_public_names_and_validation_without_a_device():
    """Every one of these raises before a context is created (no GPU here: reaching the device would raise something else)."""
    import inspect

    import polars_ds_extension_amd as pds
    from polars_ds_extension_amd import lstsq

    for n in ("glm_report_by", "glm_report_by_key"):
        assert callable(getattr(pds, n)) and n in lstsq.__all__
        assert "normal distribution" in getattr(pds, n).__doc__.lower()
    x = np.arange(12.0)
    y = (x > 5).astype(float)
    off = np.array([0, 6, 12])
    key = np.zeros(12, dtype=np.int64)
    for pen in ({"l1_reg": 0.1}, {"l2_reg": 0.1}):
        with pytest.raises(NotImplementedError, match="penalised fits have no report"):
            pds.glm_report_by(x, target=y, group_offsets=off, family="binomial", **pen)
        with pytest.raises(NotImplementedError, match="penalised fits have no report"):
            pds.glm_report_by_key(x, target=y, key=key, family="binomial", **pen)
    with pytest.raises(ValueError, match="`max_iter` must be > 1."):
        pds.glm_report_by(x, target=y, group_offsets=off, max_iter=0)
    with pytest.raises(NotImplementedError, match="family"):
        pds.glm_report_by(x, target=y, group_offsets=off, family="tweedie")
    with pytest.raises(NotImplementedError, match="family"):
        pds.glm_report_by_key(x, target=y, key=key, family="tweedie")
    with pytest.raises(NotImplementedError, match="up to 16 feature columns"):
        pds.glm_report_by(*[x] * 17, target=y, group_offsets=off)
    with pytest.raises(ValueError, match="at least one feature"):
        pds.glm_report_by_key(target=y, key=key)
    sig = inspect.signature(pds.glm_report_by)
    want = {"family": "gaussian", "add_bias": False, "tol": 1e-8, "max_iter": 100, "feature_names": None, "return_cov": False, "ctx": None}
    assert {k: sig.parameters[k].default for k in want} == want
    assert "max_groups" in inspect.signature(pds.glm_report_by_key).parameters


def test_glm_report_needs_a_fit_with_report():
    from polars_ds_extension_amd.linear_models import GLM

    assert inspect_default(GLM.fit, "report") is False
    m = GLM(family="poisson", add_bias=True)
    with pytest.raises(ValueError):
        m.report()
    # the state a fit without `report` leaves behind: coefficients, no report
    m._coeffs, m._bias, m._report = np.array([0.5, -0.25]), 0.1, None
    assert m.is_fit()
    with pytest.raises(ValueError, match="report=True"):
        m.report()
    with pytest.raises(ValueError, match="report=True"):
        m.report_dict()
    with pytest.raises(NotImplementedError, match="penalised"):  # (raised before a context is created)
        GLM(family="poisson", l2_reg=0.5).fit(np.ones((8, 2)), np.ones(8), report=True)


def inspect_default(fn, name):
    import inspect

    return inspect.signature(fn).parameters[name].default


# ------------------------------------------------------------------------------------------------- the restatement against closed forms
def _frame(family, n, p, seed):
    rng = np.random.default_rng(seed)
    X, y, _ = gc.family_frame(rng, family, np.array([n]), p)
    return X, y


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("dtype", [np.longdouble, np.float64])
def test_gaussian_se_is_the_ols_se(bias, dtype):
    """the gaussian family's se = sqrt(s^2 diag (X'X)^-1), s^2 = sum e^2 / (n - p'), to 1e-12"""
    X, y = _frame("gaussian", 120, 5, 1)
    Z = np.column_stack([X, np.ones(len(y))]) if bias else X
    beta, *_ = np.linalg.lstsq(Z, y, rcond=None)
    r = rr.report_group(X, y, beta, "gaussian", bias, dtype=dtype)
    e = y - Z @ beta
    s2 = e @ e / (len(y) - Z.shape[1])
    se = np.sqrt(s2 * np.diag(np.linalg.inv(Z.T @ Z)))
    assert np.max(np.abs(r["std_err"].astype(np.float64) - se) / se) < 1e-12
    assert abs(float(r["dispersion"]) - s2) < 1e-12 * s2 and abs(float(r["deviance"]) - e @ e) < 1e-12 * (e @ e)
    assert r["df_resid"] == len(y) - Z.shape[1]
    nd = np.sum((y - y.mean()) ** 2) if bias else np.sum(y * y)
    assert abs(float(r["null_deviance"]) - nd) < 1e-12 * nd
    assert np.allclose((r["hi"] - r["lo"]).astype(np.float64), 2 * rr.Z975 * se, rtol=1e-12)


def test_binomial_null_deviance_closed_form():
    """with a bias: -2 n [ybar ln ybar + (1 - ybar) ln(1 - ybar)]; without: 2 n ln 2"""
    X, y = _frame("binomial", 200, 3, 2)
    beta = rr.newton_fit(X, y, "binomial", True)
    r = rr.report_group(X, y, beta, "binomial", True)
    n, m = len(y), y.mean()
    assert 0 < m < 1
    want = -2 * n * (m * math.log(m) + (1 - m) * math.log(1 - m))
    assert abs(float(r["null_deviance"]) - want) < 1e-12 * want
    assert float(r["dispersion"]) == 1.0 and float(r["deviance"]) < float(r["null_deviance"])
    r0 = rr.report_group(X, y, beta[:-1], "binomial", False)
    assert abs(float(r0["null_deviance"]) - 2 * n * math.log(2)) < 1e-12 * n
    g = rr.report_group(*_frame("gamma", 50, 2, 3), np.array([0.5, 0.5]), "gamma", False)
    assert np.isnan(float(g["null_deviance"])) and np.isfinite(float(g["deviance"]))


@pytest.mark.parametrize("family", gc.FAMILIES)
def test_p_is_the_two_sided_normal_tail(family):
    from scipy.stats import norm

    X, y = _frame(family, 150, 4, 4)
    beta = rr.newton_fit(X, y, family, True)
    r = rr.report_group(X, y, beta, family, True)
    z = r["z"].astype(np.float64)
    assert np.allclose(r["p"], 2 * norm.sf(np.abs(z)), rtol=1e-13, atol=0)
    # at the MLE the score vanishes, and the float64 variant of the code agrees with the longdouble one
    lo = rr.report_group(X, y, beta, family, True, dtype=np.float64)
    assert rr.rel_err(lo["std_err"], r["std_err"]) < 1e-12 and rr.cov_err(lo["cov"][None], r["cov"][None]) < 1e-12
    Z = np.column_stack([X, np.ones(len(y))]).astype(np.longdouble)
    mu = rr._inv_link(rr.FAMILY_ID[family], Z @ beta)
    score = Z.T @ ((y - mu) / (rr._var(rr.FAMILY_ID[family], mu) * rr._dlink(rr.FAMILY_ID[family], mu)))
    assert float(np.max(np.abs(score))) < 1e-10


def test_degenerate_inputs_give_nan_not_errors():
    X, y = _frame("gaussian", 6, 5, 5)
    r = rr.report_group(X, y, np.linalg.lstsq(np.column_stack([X, np.ones(6)]), y, rcond=None)[0], "gaussian", True)
    assert r["df_resid"] == 0 and np.isnan(r["std_err"].astype(np.float64)).all() and np.isfinite(float(r["deviance"]))
    Xz = X.copy()
    Xz[:, 2] = 0.0
    rz = rr.report_group(Xz, y, np.zeros(5), "gaussian", False)
    assert np.isnan(rz["cov"].astype(np.float64)).all()
    out = rr.report_by(X, y, np.array([0, 2, 6]), np.zeros((2, 6)), "gaussian", True)
    assert np.isnan(out["std_err"].astype(np.float64)).all() and list(out["df_resid"]) == [-4, -2]


# ------------------------------------------------------------------------------------------------- the plugin layer on the mock device
import ctypes as C  # noqa: E402

FAMILY_OF = {0: "gaussian", 1: "poisson", 2: "binomial", 3: "gamma"}
CALLS = []  # (entry point, n_rows, groups or max_groups) of every grouped GLM report call the mock saw
FIELDS = ["features", "beta", "std_err", "z", "p>|z|", "0.025", "0.975", "deviance", "null_deviance", "dispersion", "n_iter"]


def _reference_group(X, y, family, bias):
    """what the mock answers for one group: the float64 restatement at the longdouble Newton fit rounded to float64"""
    with np.errstate(all="ignore"):
        b = rr.newton_fit(X, y, family, bias).astype(np.float64)
        r = rr.report_group(X, y, b, family, bias, dtype=np.float64)
    return b, r


@pytest.fixture(scope="module")
def mock():
    """The mock plugin library, its grouped GLM report entry points bound to callbacks that run the reference over the groups."""
    from mock_device import device
    from polars_ds_extension_amd import _lib

    lib = device.load()
    keep = []

    def view(ptr, n, dt):
        return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(np.ctypeslib.as_ctypes_type(dt))), shape=(n,))

    def frame(cols_p, n_feat, n, dt):
        ptrs = C.cast(cols_p, C.POINTER(C.c_void_p))
        cols = [view(ptrs[c], n, dt).copy() for c in range(n_feat + 1)]
        return np.stack(cols[1:], axis=1).astype(np.float64), cols[0].astype(np.float64)

    def fill(X, y, off, bias, link, co_p, it_p, nu_p, out_p, dt):
        ng, pp = len(off) - 1, X.shape[1] + int(bool(bias))
        out = C.cast(out_p, C.POINTER(_lib.GlmReportOut)).contents
        assert not out.cov and not out.pearson_chi2 and not out.df_resid  # (the plugin does not ask for them)
        co, it, nu = view(co_p, ng * pp, dt).reshape(ng, pp), view(it_p, ng, np.int32), view(nu_p, ng, np.uint8)
        coef = {k: view(getattr(out, k), ng * pp, dt).reshape(ng, pp) for k in ("std_err", "z", "p", "ci_lower", "ci_upper")}
        grp = {k: view(getattr(out, k), ng, dt) for k in ("deviance", "null_deviance", "dispersion")}
        rnull = view(out.report_null, ng, np.uint8)
        for g in range(ng):
            s, e = int(off[g]), int(off[g + 1])
            ok = e - s >= pp
            if ok:
                b, r = _reference_group(X[s:e], y[s:e], FAMILY_OF[link], bool(bias))
                ok = bool(np.isfinite(b).all())
            if not ok:
                co[g], it[g], nu[g], rnull[g] = np.nan, 0, 1, 1
                for a in (*coef.values(), *grp.values()):
                    a[g] = np.nan
                continue
            co[g], it[g], nu[g], rnull[g] = b, 5, 0, 0
            for k, rk in (("std_err", "std_err"), ("z", "z"), ("p", "p"), ("ci_lower", "lo"), ("ci_upper", "hi")):
                coef[k][g] = r[rk]
            for k in grp:
                grp[k][g] = r[k]

    def make_grouped(dt, ct):
        def fn(ctx, cols_p, n_feat, n, off_p, ng, space, bias, link, var, tol, max_iter, co_p, it_p, nu_p, out_p):
            CALLS.append(("grouped", n, ng))
            X, y = frame(cols_p, n_feat, n, dt)
            fill(X, y, view(off_p, ng + 1, np.int64).copy(), bias, link, co_p, it_p, nu_p, out_p, dt)
            return 0

        return C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, ct,
                           C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)(fn)

    def make_by_key(dt, ct):
        def fn(ctx, cols_p, keys_p, n_feat, n, space, bias, link, var, tol, max_iter, max_groups, ok_p, co_p, it_p, nu_p, ng_p, out_p):
            CALLS.append(("by_key", n, max_groups))
            keys = view(keys_p, n, np.int64)
            order = np.argsort(keys, kind="stable")
            uniq, counts = np.unique(keys[order], return_counts=True)
            C.c_int64.from_address(ng_p).value = len(uniq)
            if len(uniq) > max_groups:
                lib.mock_set_error(b"more distinct keys than max_groups")
                return -1
            X, y = frame(cols_p, n_feat, n, dt)
            view(ok_p, len(uniq), np.int64)[:] = uniq
            fill(X[order], y[order], np.concatenate([[0], np.cumsum(counts)]), bias, link, co_p, it_p, nu_p, out_p, dt)
            return 0

        return C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, ct, C.c_int,
                           C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)(fn)

    for sfx, dt, ct in (("f64", np.float64, C.c_double), ("f32", np.float32, C.c_float)):
        for name, cb in ((f"pds_glm_report_grouped_{sfx}", make_grouped(dt, ct)), (f"pds_glm_report_by_key_{sfx}", make_by_key(dt, ct))):
            keep.append(cb)
            getattr(lib, "mock_bind_" + name)(C.cast(cb, C.c_void_p))
    lib._glm_report_keep = keep
    return lib


def _keyed_frame(rng, sizes, p, family, shuffle=True):
    X, y, _ = gc.family_frame(rng, family, sizes, p)
    key = np.repeat(np.arange(len(sizes), dtype=np.int64) * 7 - 20, sizes)
    if shuffle:
        perm = rng.permutation(len(y))
        key, X, y = key[perm], X[perm], y[perm]
    return key, X, y


def _inputs(key, X, y, key_name="k", dt=np.float64, key_mask=None, masks=None):
    import pyarrow as pa

    masks = masks or {}
    ins = [(key_name, pa.array(key, type=pa.int64(), mask=key_mask))]
    ins.append(("y", pa.array(y.astype(dt), mask=masks.get(0))))
    ins += [(f"x{j + 1}", pa.array(X[:, j].astype(dt), mask=masks.get(j + 1))) for j in range(X.shape[1])]
    return ins


GKW = {"bias": True, "null_policy": "raise", "family": "poisson", "tol": 1e-10, "max_iter": 100}


def _check_long(out, key, X, y, bias, family, null_last=None):
    """the long format: p' rows per group, keys ascending (the null key's group last), names in input order with __bias__ last, the
    per-group fields broadcast, null numeric fields for a null group"""
    p = X.shape[1]
    pp = p + int(bias)
    uniq = sorted(set(int(k) for k in key if null_last is None or k != null_last))
    groups = uniq + ([null_last] if null_last is not None else [])
    assert len(out) == len(groups) * pp
    cols = {n: out.field(i + 1).to_pylist() for i, n in enumerate(FIELDS)}
    got_keys = out.field(0).to_pylist()
    names = [f"x{j + 1}" for j in range(p)] + (["__bias__"] if bias else [])
    for gi, k in enumerate(groups):
        sl = slice(gi * pp, (gi + 1) * pp)
        assert got_keys[sl] == [None if k == null_last and null_last is not None else k] * pp
        assert cols["features"][sl] == names
        rows = np.flatnonzero(key == k)
        if len(rows) < pp:
            assert all(v is None for n in FIELDS[1:-1] for v in cols[n][sl]) and cols["n_iter"][sl] == [0] * pp
            continue
        b, r = _reference_group(X[rows], y[rows], family, bias)
        for n, ref in (("beta", b), ("std_err", r["std_err"]), ("z", r["z"]), ("p>|z|", r["p"]), ("0.025", r["lo"]), ("0.975", r["hi"])):
            np.testing.assert_allclose(np.asarray(cols[n][sl], dtype=np.float64), np.asarray(ref, dtype=np.float64), rtol=1e-12, atol=0)
        for n in ("deviance", "null_deviance", "dispersion"):
            assert cols[n][sl] == [float(r[n])] * pp
        assert cols["n_iter"][sl] == [5] * pp


def test_plugin_glm_report_by(mock):
    import pyarrow as pa
    from plugin_harness import call_plugin, output_field

    rng = np.random.default_rng(31)
    sizes = np.array([30, 2, 45, 12, 60])  # (a group of 2 rows: fewer than the 4 coefficients)
    key, X, y = _keyed_frame(rng, sizes, 3, "poisson")
    fld = output_field(mock, "pl_glm_report_by", [pa.field("k", pa.int64()), pa.field("y", pa.float64())])
    assert fld.name == "glm_report" and [f.name for f in fld.type] == ["k"] + FIELDS
    assert fld.type[0].type == pa.int64() and fld.type[1].type == pa.large_string() and fld.type[11].type == pa.int32()
    assert all(fld.type[i].type == pa.float64() for i in range(2, 11))
    f32 = output_field(mock, "pl_glm_report_by_f32")
    assert f32.type[0].name == "key" and all(f32.type[i].type == pa.float32() for i in range(2, 11))
    CALLS.clear()
    field, out = call_plugin(mock, "pl_glm_report_by", _inputs(key, X, y), GKW)
    assert field == fld and CALLS == [("by_key", len(y), len(y))]
    _check_long(out, key, X, y, True, "poisson")
    # no bias, another family, an unnamed key, f32
    key2, X2, y2 = _keyed_frame(rng, np.array([25, 40]), 2, "gaussian")
    _, out2 = call_plugin(mock, "pl_glm_report_by", _inputs(key2, X2, y2, key_name=""), dict(GKW, family="gaussian", bias=False))
    _check_long(out2, key2, X2, y2, False, "gaussian")
    f32f, out32 = call_plugin(mock, "pl_glm_report_by_f32", _inputs(key2, X2, y2, dt=np.float32), dict(GKW, family="gaussian"))
    assert out32.field(2).type == pa.float32() and len(out32) == 2 * 3


def test_plugin_glm_report_by_null_key_and_capacity_retry(mock):
    from plugin_harness import call_plugin

    rng = np.random.default_rng(32)
    key, X, y = _keyed_frame(rng, np.array([20, 30, 25]), 2, "binomial")
    mask = key == -13  # (keys -20, -13, -6: the middle group becomes the null key's)
    _, out = call_plugin(mock, "pl_glm_report_by", _inputs(key, X, y, key_mask=mask), dict(GKW, family="binomial"))
    got = out.field(0).to_pylist()
    assert got[:6] == [-20] * 3 + [-6] * 3 and got[6:] == [None] * 3  # the null key's group last
    _check_long(out, np.where(mask, 10 ** 6, key), X, y, True, "binomial", null_last=10 ** 6)
    mock.pds_plugin_debug_glm_by_first_cap(C.c_longlong(2))
    try:
        CALLS.clear()
        _, out = call_plugin(mock, "pl_glm_report_by", _inputs(key, X, y), dict(GKW, family="binomial"))
        assert [c[2] for c in CALLS] == [2, 3]  # the guess, then the device's count
        _check_long(out, key, X, y, True, "binomial")
    finally:
        mock.pds_plugin_debug_glm_by_first_cap(C.c_longlong(0))


@pytest.mark.parametrize("policy", ["skip", "zero"])
def test_plugin_glm_report_by_null_policies(mock, policy):
    """frames with nulls are prepared on the host (rows in key order, the policy row by row) and go to the offsets entry point"""
    from plugin_harness import call_plugin

    rng = np.random.default_rng(33)
    key, X, y = _keyed_frame(rng, np.array([40, 35, 50]), 3, "poisson")
    n = len(y)
    masks = {0: rng.uniform(size=n) < 0.05, 2: rng.uniform(size=n) < 0.08}
    CALLS.clear()
    _, out = call_plugin(mock, "pl_glm_report_by", _inputs(key, X, y, masks=masks), dict(GKW, null_policy=policy))
    assert [c[0] for c in CALLS] == ["grouped"]
    if policy == "skip":
        keep = ~(masks[0] | masks[2])
        Xf = X
    else:
        keep = ~masks[0]
        Xf = X.copy()
        Xf[masks[2], 1] = 0.0
    assert CALLS[0][1] == int(keep.sum())
    _check_long(out, key[keep], Xf[keep], y[keep], True, "poisson")
    with pytest.raises(Exception, match="Nulls found in data"):
        call_plugin(mock, "pl_glm_report_by", _inputs(key, X, y, masks=masks), GKW)


def test_plugin_glm_report_by_kwargs_errors(mock):
    from plugin_harness import call_plugin

    rng = np.random.default_rng(34)
    key, X, y = _keyed_frame(rng, np.array([20, 20]), 2, "poisson")
    for pen in ({"l1_reg": 0.1}, {"l2_reg": 0.1}):
        with pytest.raises(Exception, match="penalised fits have no report"):
            call_plugin(mock, "pl_glm_report_by", _inputs(key, X, y), dict(GKW, **pen))
    with pytest.raises(Exception, match="unknown GLM family"):
        call_plugin(mock, "pl_glm_report_by", _inputs(key, X, y), dict(GKW, family="tweedie"))
    with pytest.raises(Exception, match="max_iter"):
        call_plugin(mock, "pl_glm_report_by", _inputs(key, X, y), dict(GKW, max_iter=0))
    with pytest.raises(Exception, match="up to 16 feature columns"):
        call_plugin(mock, "pl_glm_report_by", _inputs(key, np.tile(X, (1, 9))[:, :17], y), GKW)
