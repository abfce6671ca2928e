"""pl_lin_reg_report_cluster on the product library: the struct holds the bits of the lstsq call on the same frame (keys with a null
cluster included), and a null policy gives what lstsq gives on the rows that survive it (tests/test_grouped_report_polars_gpu.py's
arrangement: the plugin symbol through tests/plugin_harness.py, Arrow in and out)."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT))

import cluster_cases as cc  # noqa: E402

KW = {"bias": True, "null_policy": "raise", "std_err": "cluster", "solver": "qr", "l1_reg": 0.0, "l2_reg": 0.0, "tol": 0.0}
NAMES = ["beta", None, "t", "p>|t|", "0.025", "0.975", "r2", "adj_r2"]


@pytest.fixture(scope="module")
def pds():
    import polars_ds_extension_amd as m

    return m


@pytest.fixture(scope="module")
def lib(pds):
    from polars_ds_extension_amd import _lib

    return C.CDLL(str(_lib.LIB_PATH))


def _inputs(key, F, y, key_mask=None, masks=None):
    import pyarrow as pa

    masks = masks or {}
    ins = [("firm", pa.array(key, type=pa.int64(), mask=key_mask)), ("y", pa.array(y, mask=masks.get(0)))]
    return ins + [(f"x{j + 1}", pa.array(np.ascontiguousarray(F[:, j]), mask=masks.get(j + 1))) for j in range(F.shape[1])]


def _same_bits(out, r, se, p, bias=True):
    se_name = se + "_se"
    assert [f.name for f in out.type] == ["features", "beta", se_name, "t", "p>|t|", "0.025", "0.975", "r2", "adj_r2"]
    assert out.field(0).to_pylist() == [f"x{j + 1}" for j in range(p)] + (["__bias__"] if bias else [])
    for i, name in enumerate(NAMES):
        got = out.field(1 + i).to_numpy(zero_copy_only=False)
        want = np.asarray(r[name or se_name])
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), name


@pytest.mark.parametrize("se", ["cluster", "cluster0"])
def test_plugin_holds_the_lstsq_bits(pds, lib, se):
    from plugin_harness import call_plugin

    p = 4
    F, y, off, codes = cc.ragged_frame(p)
    key = codes * 7 - 200
    perm = np.random.default_rng(6).permutation(len(y))
    key, F, y = key[perm], F[perm], np.ascontiguousarray(y[perm])
    _, out = call_plugin(lib, "pl_lin_reg_report_cluster", _inputs(key, F, y), dict(KW, std_err=se))
    r = pds.lin_reg_report(*cc.columns(F), target=y, add_bias=True, std_err=se, cluster=key)
    assert r["n_clusters"] == len(off) - 1
    _same_bits(out, r, se, p)
    # the null key is its own cluster: the stand-in is a key no row uses, the largest, so the clusters are the same ones in another order
    mask = key == key.max()
    _, out_null = call_plugin(lib, "pl_lin_reg_report_cluster", _inputs(key, F, y, key_mask=mask), dict(KW, std_err=se))
    r_null = pds.lin_reg_report(*cc.columns(F), target=y, add_bias=True, std_err=se, cluster=np.where(mask, key.max() + 1, key))
    _same_bits(out_null, r_null, se, p)
    # without a bias
    _, out0 = call_plugin(lib, "pl_lin_reg_report_cluster", _inputs(key, F, y), dict(KW, std_err=se, bias=False))
    _same_bits(out0, pds.lin_reg_report(*cc.columns(F), target=y, add_bias=False, std_err=se, cluster=key), se, p, bias=False)


def test_plugin_skip_policy_equals_lstsq_on_the_kept_rows(pds, lib):
    from plugin_harness import call_plugin

    p = 4
    F, y, off, codes = cc.ragged_frame(p)
    n = len(y)
    rng = np.random.default_rng(9)
    masks = {0: rng.uniform(size=n) < 0.03, 3: rng.uniform(size=n) < 0.05}
    _, out = call_plugin(lib, "pl_lin_reg_report_cluster", _inputs(codes, F, np.ascontiguousarray(y), masks=masks), dict(KW, null_policy="skip"))
    keep = ~(masks[0] | masks[3])
    # var(y) is that of the ORIGINAL non-null target, what Polars' target.var() hands pl_lin_reg_report
    r = pds.lin_reg_report(*cc.columns(F[keep]), target=np.ascontiguousarray(y[keep]), add_bias=True, std_err="cluster", cluster=codes[keep],
                           y_var=float(np.var(y[~masks[0]], ddof=1)))
    for i, name in enumerate(NAMES):
        got = out.field(1 + i).to_numpy(zero_copy_only=False)
        want = np.asarray(r[name or "cluster_se"])
        if name in ("r2", "adj_r2"):  # (y_var: two host computations of one variance)
            assert np.all(np.abs(got - want) <= 1e-13), name
        else:
            assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), name
    with pytest.raises(Exception, match="Nulls found in data"):
        call_plugin(lib, "pl_lin_reg_report_cluster", _inputs(codes, F, np.ascontiguousarray(y), masks=masks), KW)
    with pytest.raises(Exception, match="at least two non-empty clusters"):
        call_plugin(lib, "pl_lin_reg_report_cluster", _inputs(np.zeros_like(codes), F, np.ascontiguousarray(y)), KW)
