"""pl_lin_reg_report_by / pl_wls_report_by on the product library: the long frame holds the bits of the lstsq by-key call, and the
null policies act on every group as a per-group pl_lin_reg_report call does (within the contract tolerance, DESIGN 7: 1e-10 with
the propagated bounds for t, p and CI that tests/test_grouped_report_gpu.py applies)."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT))

TOL = 1e-10
KW = {"bias": True, "null_policy": "raise", "std_err": "se", "solver": "qr", "l1_reg": 0.0, "l2_reg": 0.0, "tol": 0.0}


@pytest.fixture(scope="module")
def pds():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import polars_ds_extension_amd as m

    return m


@pytest.fixture(scope="module")
def lib(pds):
    from polars_ds_extension_amd import _lib

    return C.CDLL(str(_lib.LIB_PATH))


def _frame(rng, sizes, p):
    n = int(np.sum(sizes))
    key = np.repeat(np.arange(len(sizes), dtype=np.int64) * 7 - 20, sizes)
    X = rng.normal(size=(n, p))
    y = X @ rng.normal(size=p) + 0.3 + 0.2 * rng.normal(size=n) + 0.01 * key
    w = rng.uniform(0.25, 4.0, size=n)
    perm = rng.permutation(n)
    return key[perm], X[perm], y[perm], w[perm]


@pytest.mark.parametrize("symbol,se", [("pl_lin_reg_report_by", "se"), ("pl_lin_reg_report_by", "hc3"), ("pl_wls_report_by", "se")])
def test_plugin_holds_the_by_key_bits(pds, lib, symbol, se):
    import pyarrow as pa
    from plugin_harness import call_plugin

    rng = np.random.default_rng(3)
    sizes = [int(s) for s in rng.integers(1, 200, size=60)] + [3, 2, 5000]  # (p' = 5: null groups; one group of two pieces)
    p, pp = 4, 5
    key, X, y, w = _frame(rng, sizes, p)
    wls = symbol == "pl_wls_report_by"
    mask = key == -13  # one key's rows are null keys: one group, reported last
    ins = [("k", pa.array(key, mask=mask))] + ([("w", pa.array(w))] if wls else []) + [("y", pa.array(y))]
    ins += [(f"x{j + 1}", pa.array(X[:, j])) for j in range(p)]
    _, out = call_plugin(lib, symbol, ins, dict(KW, std_err=se))
    stand_in = int(key.max()) + 1
    k2 = np.where(mask, stand_in, key)
    r = pds.lin_reg_report_by_key(*[X[:, j] for j in range(p)], target=y, key=k2, add_bias=True, std_err=se, weights=w if wls else None)
    ng = len(r["keys"])
    assert ng == len(sizes) and len(out) == ng * pp
    keys = out.field(0)
    assert keys.null_count == pp and keys.slice(0, (ng - 1) * pp).to_pylist() == [int(k) for k in r["keys"][:-1] for _ in range(pp)]
    assert keys.slice((ng - 1) * pp).to_pylist() == [None] * pp and int(r["keys"][-1]) == stand_in
    assert out.field(1).to_pylist() == ["x1", "x2", "x3", "x4", "__bias__"] * ng
    se_name = "std_err" if (wls or se == "se") else "hc3_se"
    assert [f.name for f in out.type] == ["k", "features", "beta", se_name, "t", "p>|t|", "0.025", "0.975", "r2", "adj_r2"]
    null = np.repeat(np.asarray(r["is_null"]).astype(bool), pp)
    assert null.sum() == pp * sum(s < pp for s in sizes) >= 2 * pp
    for i, name in enumerate(["beta", se_name, "t", "p>|t|", "0.025", "0.975"]):
        a = out.field(2 + i)
        assert np.array_equal(~np.asarray(a.is_valid()), null), name
        got = a.to_numpy(zero_copy_only=False)[~null]
        want = np.asarray(r[name]).reshape(-1)[~null]
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), name
    for i, name in enumerate(["r2", "adj_r2"]):
        a = out.field(8 + i)
        assert np.array_equal(~np.asarray(a.is_valid()), null), name
        assert np.array_equal(a.to_numpy(zero_copy_only=False)[~null].view(np.uint64), np.repeat(np.asarray(r[name]), pp)[~null].view(np.uint64))


def test_plugin_capacity_retry(pds, lib):
    """A first capacity guess below the group count: one more call with the count the device returned, the same bits."""
    import pyarrow as pa
    from plugin_harness import call_plugin

    rng = np.random.default_rng(4)
    key, X, y, w = _frame(rng, [30] * 11, 2)
    ins = [("k", pa.array(key)), ("w", pa.array(w)), ("y", pa.array(y)), ("x1", pa.array(X[:, 0])), ("x2", pa.array(X[:, 1]))]
    _, a = call_plugin(lib, "pl_wls_report_by", ins, KW)
    lib.pds_plugin_debug_report_by_first_cap.argtypes = [C.c_longlong]
    lib.pds_plugin_debug_report_by_first_cap(3)
    try:
        _, b = call_plugin(lib, "pl_wls_report_by", ins, KW)
    finally:
        lib.pds_plugin_debug_report_by_first_cap(0)
    assert len(a) == 33 and a.equals(b)


def test_null_policies_equal_per_group_calls(pds, lib):
    """The by-call (grouped kernels) against one pl_lin_reg_report call per group (the single report's kernels): two computations
    that each hold the contract, compared with its tolerance and the bounds it propagates to t, p and CI."""
    from scipy import stats as st
    from test_grouped_report_polars_cpu import null_policy_equality

    def compare(want, got, se_name, dof):
        if not np.all(np.isfinite(want["beta"])):  # "ignore": the group fits on NaN
            for f in want:
                assert np.array_equal(np.isnan(want[f]), np.isnan(got[f])), f
            return
        beta_o, se_o, t_o = want["beta"], want[se_name], want["t"]
        assert np.linalg.norm(got["beta"] - beta_o) <= TOL * np.linalg.norm(beta_o)
        assert np.all(np.abs(got[se_name] - se_o) <= TOL * np.abs(se_o))
        dt_bound = TOL * (np.linalg.norm(beta_o) / se_o + np.abs(t_o))
        assert np.all(np.abs(got["t"] - t_o) <= dt_bound)
        dp_bound = 2.0 * st.t.pdf(np.abs(t_o), dof) * dt_bound + 1e-13 * want["p>|t|"]
        assert np.all(np.abs(got["p>|t|"] - want["p>|t|"]) <= dp_bound)
        ci_bound = TOL * (np.linalg.norm(beta_o) + st.t.ppf(0.975, dof) * se_o)
        assert np.all(np.abs(got["0.025"] - want["0.025"]) <= ci_bound)
        assert np.all(np.abs(got["0.975"] - want["0.975"]) <= ci_bound)
        for k in ("r2", "adj_r2"):
            assert np.all(np.abs(got[k] - want[k]) <= TOL * np.maximum(1.0, np.abs(want[k]))), k

    for se in ("se", "hc1"):
        null_policy_equality(lib, ["skip", "zero", "one", "0.5", "ignore"], compare, se=se)
