"""The fixed-effects regression without a GPU: the reference (within_reference.py) against the explicit dummy-variable regression, the
C ABI surface (exports, header declarations, the mock builder's view of them, the build lists) and the argument errors of
lstsq.lin_reg / lin_reg_report(absorb=), which are raised before any library call.

The reference is right.  In long double its beta, classical and CR0 standard errors must equal those of the regression on one dummy
column per group without an intercept, whose scores keep the dummy entries -- another formula for the same numbers (Frisch-Waugh-
Lovell; the dummy entries of a group's score are the group's residual sum, which is zero, so CR0 agrees too).  The bar is measured,
not chosen: the dummy regression is computed twice in long double, with its columns and rows in opposite orders, and the distance
between those two roundings of ONE formula -- the worst of the three fields, which all come out of one solve -- is what long double
arithmetic resolves on that frame (the dummy design carries the group levels, about 50 x the within spread, and is the worse
conditioned of the two routes).  The within reference may be 10 x that
far from the dummy regression; where the two dummy runs agree to below half an ulp of long double, 8 ulp."""
import re
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT))

import within_cases as wc  # noqa: E402
import within_reference as wr  # noqa: E402

NEW = ["pds_lin_reg_within_grouped_f64", "pds_lin_reg_within_grouped_f32", "pds_lin_reg_within_by_key_f64", "pds_lin_reg_within_by_key_f32"]


# ---- 1. the reference against the dummy-variable regression
@pytest.mark.parametrize("p", [1, 2, 4])
@pytest.mark.parametrize("g", [2, 3, 5, 9, 12])
def test_reference_equals_dummy_regression(g, p):
    assert np.finfo(np.longdouble).eps < 1e-18
    F, y, off, codes = wc.equal_frame(g, p)
    rng = np.random.default_rng(g * 10 + p)
    perm = rng.permutation(len(y))  # the reference takes codes in any order
    F, y, codes = np.asarray(F)[perm], np.asarray(y)[perm], codes[perm] * 5 - 7
    a, b = wr.dummy_report(F, y, codes), wr.dummy_report(F, y, codes, flip=True)
    ref = {se: wr.report(F, y, codes, se) for se in ("se", "cluster0")}
    got = {"beta": ref["se"]["beta"], "se": ref["se"]["std_err"], "cluster0": ref["cluster0"]["std_err"]}
    # one solve feeds all three fields, and one pair of roundings of one field can agree by luck: the frame's figure is the worst of the three
    noise = max(wr.rel(b[k], a[k]) for k in ("beta", "se", "cluster0"))
    bar = wr.budget(noise, np.longdouble)
    for k in ("beta", "se", "cluster0"):
        d = wr.rel(got[k], a[k])
        print(f"G={g} p={p} {k}: within reference vs dummy regression {d:.2e}; two long double roundings of the dummy regression {noise:.2e}; bar {bar:.2e}")
        assert d <= bar, (k, d, noise)
    assert ref["se"]["n_groups"] == g and ref["se"]["df_resid"] == len(y) - g - p and ref["cluster0"]["df_resid"] == g - 1
    # the per-row outputs hang together, in the row order given
    r = ref["se"]
    _, _, idx, _ = wr._groups(codes)
    assert wr.rel(r["alpha"][idx] + F.astype(np.longdouble) @ r["beta"] + r["resid"], y) < 1e-17
    assert wr.rel(r["pred"] + r["resid"], y) < 1e-17


def test_reference_formats_and_levels():
    """the narrower formats run the same code; the group levels dominate the frame (a fit that does not centre is nowhere near)"""
    F, y, off, codes = wc.ragged_frame(4)
    ld, f64, f32 = (wr.report(F, y, codes, "cluster", dt) for dt in (np.longdouble, np.float64, np.float32))
    assert f64["beta"].dtype == np.float64 and f32["resid"].dtype == np.float32
    assert wr.rel(f64["beta"], ld["beta"]) < 1e-11 and wr.rel(f32["beta"], ld["beta"]) < 1e-1
    pooled = np.linalg.lstsq(np.column_stack([F, np.ones(len(y))]), y, rcond=None)[0][:4]
    assert wr.rel(pooled, ld["beta"]) > 0.05  # the pooled fit is another model
    assert float(np.std(np.asarray(F)[:, 1])) > 20 * float(np.std(np.asarray(F)[:, 1] - np.repeat(
        [np.asarray(F)[off[k]:off[k + 1], 1].mean() for k in range(len(off) - 1)], np.diff(off))))
    ratio = np.asarray(ld["se_all"]["cluster"] / ld["se_all"]["se"], dtype=np.float64)
    assert np.max(np.abs(ratio - 1.0)) > 0.2  # the estimator matters on these frames
    padded, place = wc.with_empty_groups(off)
    assert len(place) == len(off) - 1 and np.array_equal(np.diff(padded)[place], np.diff(off)) and len(padded) > len(off) + 20


# ---- 2. exports, header, build lists
def test_exported_and_declared():
    from polars_ds_extension_amd import _lib

    assert all(n in _lib.EXPORTS for n in NEW)
    header = (ROOT / "include" / "pds_lstsq.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for n in NEW:
        assert len(re.findall(rf"^int\s+{n}\s*\(", text, flags=re.M)) == 1, n
    assert len(re.findall(r"\}\s*pds_within_out;", text)) == 1
    enum = re.search(r"typedef enum \{([^}]*)\} pds_se_type;", text, flags=re.S).group(1)
    assert len(re.findall(r"PDS_\w+\s*=\s*\d+", enum)) == 7  # the enum gained nothing
    assert _lib.WITHIN_SE_TYPES == {"se": 0, "cluster": 5, "cluster0": 6}
    assert [f[0] for f in _lib.WithinOut._fields_] == ["alpha", "pred", "resid", "r2_overall", "n_groups_used", "df_resid"]
    # the comment states the cluster factor as a definition and names the split option beside the cluster report's
    doc = header[header.index("pds_lin_reg_within_*: fixed-effects"):header.index("} pds_within_out;")]
    assert "DEFINITION" in doc and "no equivalence" in doc
    assert '"within_split_rows"' in header and header.index('"cluster_split_rows"') < header.index('"within_split_rows"')


def test_mock_trampolines_parse():
    sys.path.insert(0, str(ROOT / "tests" / "mock_device"))
    try:
        import build as mock_build
    finally:
        sys.path.pop(0)
    protos = {name: args for _, name, args in mock_build.prototypes()}
    assert [a for _, a in protos["pds_lin_reg_within_grouped_f64"]] == ["ctx", "cols", "n_feat", "n_rows", "group_offsets", "n_groups", "space",
                                                                       "se_type", "out", "extra"]
    assert [a for _, a in protos["pds_lin_reg_within_by_key_f32"]] == ["ctx", "cols", "keys", "n_feat", "n_rows", "space", "se_type", "max_groups",
                                                                      "out_keys", "out", "extra", "n_groups"]
    assert protos["pds_lin_reg_within_grouped_f32"][8][0] == "pds_report_f32*" and protos["pds_lin_reg_within_by_key_f64"][9][0] == "pds_report_f64*"
    assert protos["pds_lin_reg_within_by_key_f64"][10][0] == "pds_within_out*"


def test_source_lists_the_kernel():
    csrc = ROOT / "polars_ds_extension_amd" / "csrc"
    assert "within_pass.hip" in (csrc / "Makefile").read_text()
    assert '#include "capi_within.hpp"' in (csrc / "capi.hip").read_text()
    # the score / meat idiom is score_meat_dev.hpp's (shared with cluster_meat.hip), which builds on the wave tile
    text, shared = (csrc / "within_pass.hip").read_text(), (csrc / "score_meat_dev.hpp").read_text()
    assert '#include "score_meat_dev.hpp"' in text and '#include "wave_tile_dev.hpp"' in shared
    assert "__builtin_amdgcn_mfma_f64_16x16x4f64" in shared
    assert "score_rows4<P>" in text and "ScoreMeat<false>" in text and "score_long_meat_kernel<false>" in text  # (no bias entry)
    assert "launch_sum_records(" in text and "compensated=*/true" in text
    # no atomics in any sum: the pass, the shared idiom, the record sum (mixed.hip, whose one integer atomicOr is the flag word's)
    atomics = r"atomic(Add|Or|Max|Min|CAS|Exch)"
    assert not re.search(atomics, text) and not re.search(atomics, shared)
    mixed = (csrc / "mixed.hip").read_text()
    sum_text = mixed[mixed.index("template <bool COMPENSATED>"):mixed.index("template <int P>\n__global__ __launch_bounds__(64) void mixed_profile_kernel")]
    sum_text += mixed[mixed.index("int launch_sum_records("):mixed.index("int mixed_stats_blocks(")]
    assert "sum_records_kernel(" in sum_text and "two_sum(s, c, v)" in sum_text and "hipLaunchKernelGGL" in sum_text
    assert not re.search(atomics, sum_text)
    assert not re.search(r"atomic(Add|Max|Min|CAS|Exch)", mixed)


# ---- 3. argument errors, before any library call
@pytest.fixture()
def no_library(monkeypatch):
    from polars_ds_extension_amd import _lib, lstsq

    def boom(*a, **k):
        raise AssertionError("the library was called")

    monkeypatch.setattr(_lib, "load", boom)
    monkeypatch.setattr(lstsq, "default_context", boom)
    monkeypatch.setattr(lstsq, "_Cols", boom)
    return lstsq


def test_python_argument_errors(no_library):
    ls = no_library
    F, y, off, codes = wc.equal_frame(4, 2)
    cols = wc.columns(F)
    for fn in (ls.lin_reg_report, ls.lin_reg):
        with pytest.raises(ValueError, match="exactly one of `absorb` and `absorb_offsets`"):
            fn(*cols, target=y, absorb=codes, absorb_offsets=off)
        with pytest.raises(ValueError, match="the intercept is absorbed"):
            fn(*cols, target=y, absorb=codes, add_bias=True)
        with pytest.raises(NotImplementedError, match="weights"):
            fn(*cols, target=y, absorb=codes, weights=np.ones(len(y)))
        with pytest.raises(NotImplementedError, match="pyarrow"):
            import pyarrow as pa

            fn(pa.array(cols[0]), cols[1], target=y, absorb_offsets=off)
    with pytest.raises(ValueError, match='std_err="cluster" means the absorbed key'):
        ls.lin_reg_report(*cols, target=y, absorb=codes, std_err="cluster", cluster=codes)
    with pytest.raises(ValueError, match='std_err="cluster" means the absorbed key'):
        ls.lin_reg_report(*cols, target=y, absorb_offsets=off, std_err="cluster0", cluster_offsets=off)
    with pytest.raises(ValueError, match="go with `absorb`"):
        ls.lin_reg_report(*cols, target=y, return_effects=True)
    with pytest.raises(ValueError, match='std_err is "se", "cluster" or "cluster0"'):
        ls.lin_reg_report(*cols, target=y, absorb=codes, std_err="bootstrap")
    from polars_ds_extension_amd._lib import PdsError

    with pytest.raises(PdsError, match="HC0 - HC3") as e:  # refused with the library's code, without asking the library
        ls.lin_reg_report(*cols, target=y, absorb=codes, std_err="hc1")
    assert e.value.code == -5
