"""
`polars_exprs.glm_report(by=)` and `glm_report_by_group`: expression -> plugin call -> `_polars_plugin_pl_glm_report_by` -> Arrow
result, with tests/mini_polars standing in for the Polars engine where no real one is importable (tests/test_polars_exprs.py's
arrangement).  CPU: the mock device behind the same plugin.cpp, its report entry points bound to the NumPy restatement
(tests/test_glm_report_cpu.py's fixture).  GPU: the product library against lstsq.glm_report_by_key.
"""
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import glm_cases as gc  # noqa: E402
from test_glm_report_cpu import FIELDS, _reference_group, mock  # noqa: E402,F401  (fixture: the mock library with the report entry points bound)
from test_polars_exprs import pl  # noqa: E402  (the real polars if importable, else tests/mini_polars)

from polars_ds_extension_amd import polars_exprs as px  # noqa: E402

SIZES = [60, 2, 45, 70]  # (key -13: 2 rows < p' = 3 -> a null group)


def _frame(seed, family):
    rng = np.random.default_rng(seed)
    X, y, _ = gc.family_frame(rng, family, np.array(SIZES), 2)
    key = np.repeat(np.arange(len(SIZES), dtype=np.int64) * 7 - 20, SIZES)
    perm = rng.permutation(len(y))
    return key[perm], X[perm], y[perm]


def _df(key, X, y, key_name="k"):
    return pl.DataFrame({key_name: key, "y": y, "x1": X[:, 0], "x2": X[:, 1]})


def _check(res, key_col, groups, rows_of, X, y, family, reference):
    """p' = 3 rows per group in the order `groups`, names x1, x2, __bias__, values from reference(rows)"""
    assert res.columns == [key_col] + FIELDS and len(res) == 3 * len(groups)
    assert res[key_col].to_list() == [g for g in groups for _ in range(3)]
    assert res["features"].to_list() == ["x1", "x2", "__bias__"] * len(groups)
    for gi, g in enumerate(groups):
        rows = rows_of(g)
        sl = slice(3 * gi, 3 * gi + 3)
        if rows.sum() < 3:
            assert all(v is None for n in FIELDS[1:-1] for v in res[n].to_list()[sl])
            continue
        ref = reference(X[rows], y[rows])
        for n in FIELDS[1:-1]:
            np.testing.assert_allclose(np.asarray(res[n].to_list()[sl], dtype=np.float64), ref[n], rtol=1e-9, atol=0, err_msg=n)


def _mock_reference(family):
    def ref(X, y):
        b, r = _reference_group(X, y, family, True)
        out = {"beta": b, "std_err": r["std_err"], "z": r["z"], "p>|z|": r["p"], "0.025": r["lo"], "0.975": r["hi"]}
        out.update({n: np.full(3, float(r[n])) for n in ("deviance", "null_deviance", "dispersion")})
        return {k: np.asarray(v, dtype=np.float64) for k, v in out.items()}

    return ref


def t_glm_report(path, family, reference):
    px.PLUGIN_PATH = path
    key, X, y = _frame(41, family)
    df = _df(key, X, y)
    res = df.select(px.glm_report("x1", "x2", target="y", by="k", family=family, add_bias=True, tol=1e-10)).unnest("glm_report")
    _check(res, "k", [-20, -13, -6, 1], lambda g: key == g, X, y, family, reference)
    res2 = px.glm_report_by_group(df, "k", "x1", "x2", target="y", family=family, add_bias=True, tol=1e-10)
    assert res2.columns == res.columns and res2["k"].to_list() == res["k"].to_list()
    # keys of another dtype: order of first appearance
    names = np.array(["oak", "elm", "ash", "fir"])[(key + 20) // 7]
    d2 = _df(names.tolist(), X, y, key_name="tree")
    r3 = px.glm_report_by_group(d2, "tree", "x1", "x2", target="y", family=family, add_bias=True, tol=1e-10)
    _check(r3, "tree", list(dict.fromkeys(names.tolist())), lambda g: names == g, X, y, family, reference)


@pytest.mark.parametrize("family", ["poisson", "gaussian"])
def test_exprs_against_the_mock_device(family, mock):  # noqa: F811
    t_glm_report(Path(mock._name), family, _mock_reference(family))


def test_builders_validate():
    with pytest.raises(NotImplementedError, match="family"):
        px.glm_report("x1", target="y", by="k", family="tweedie")
    with pytest.raises(ValueError, match="max_iter"):
        px.glm_report("x1", target="y", by="k", max_iter=0)
    assert "normal distribution" in px.glm_report.__doc__


@pytest.mark.gpu
@pytest.mark.parametrize("family", ["binomial", "gamma"])
def test_exprs_against_the_hip_library(family):
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import polars_ds_extension_amd as pds
    from polars_ds_extension_amd import _lib

    def ref(X, y):
        d = pds.glm_report_by(X[:, 0].copy(), X[:, 1].copy(), target=y, group_offsets=[0, len(y)], family=family, add_bias=True, tol=1e-10)
        out = {n: d[n][0] for n in ("beta", "std_err", "z", "p>|z|", "0.025", "0.975")}
        out.update({n: np.full(3, d[n][0]) for n in ("deviance", "null_deviance", "dispersion")})
        return out

    t_glm_report(_lib.LIB_PATH, family, ref)
