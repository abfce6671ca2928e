"""Fixed-effects reports with standard errors clustered on any key, without a GPU: the restatement (within_cluster_reference.py) against
the explicit dummy-variable regression with the CR0 sandwich on the full design, K and the degrees of freedom in the four relations a
cluster key can have to the absorbed keys, the C ABI surface (exports, header declarations and text, the ctypes struct and argument
counts, the build lists) and the argument errors of lstsq.lin_reg_report / fixed_effects(cluster_key=), which are raised before any
library call.

The restatement is right.  In long double its beta and its CR0 standard errors (np.add.at over the cluster codes on the PROJECTED
columns) must equal the feature block of the regression on the features and the dummies of the absorbed keys, whose scores keep the
dummy entries (Frisch-Waugh-Lovell).  The bar is the sibling files': one absorbed key -- 10 x the distance between two long double
roundings of the dummy regression of that frame (within_reference.dummy_report, columns and rows in opposite orders; 8 ulp where they
agree to below half an ulp); two absorbed keys -- 1e-15 relative, the bar of test_within2_cpu.py on these frames."""
import ctypes as C
import re
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT))

import within2_cases as c2  # noqa: E402
import within2_reference as w2r  # noqa: E402
import within_cases as wc  # noqa: E402
import within_cluster_reference as wcr  # noqa: E402
import within_reference as wr  # noqa: E402

NEW = [f"pds_lin_reg_within{two}_cl_{form}_{sfx}" for two in ("", "2") for form in ("grouped", "by_key") for sfx in ("f64", "f32")]


def _cluster_keys(k1, n, seed):
    """the relations of a cluster key to the absorbed key k1: equal, coarser and nested (levels of a cluster not adjacent), crossing"""
    rng = np.random.default_rng(seed)
    lv = np.unique(k1, return_inverse=True)[1].reshape(-1)
    g = int(lv.max()) + 1
    coarse = rng.permutation(g) % max(2, min(5, g // 2 if g > 3 else 2))
    return {"equal": np.asarray(k1) * 3 + 1, "nested": coarse[lv], "crossing": rng.integers(0, 6, size=n)}


# ---- 1. the two routes of the restatement
@pytest.mark.parametrize("kind,p,g", [("equal", 2, 5), ("equal", 4, 9), ("ragged", 4, 0)])
def test_one_key_routes_agree(kind, p, g):
    assert np.finfo(np.longdouble).eps < 1e-18
    F, y, off, codes = wc.frame(kind, p, g)
    F, y = np.asarray(F, dtype=np.float64), np.asarray(y, dtype=np.float64)
    a, b = wr.dummy_report(F, y, codes), wr.dummy_report(F, y, codes, flip=True)
    noise = max(wr.rel(b[k], a[k]) for k in ("beta", "se", "cluster0"))
    bar = wr.budget(noise, np.longdouble)
    for name, ck in _cluster_keys(codes, len(y), 10 * p + g).items():
        r = wcr.report(F, y, codes, ck, "cluster0")
        d = wcr.dummy_cluster0(F, y, codes, ck)
        dist = {"beta": wcr.rel(r["beta"], d["beta"]), "cluster0": wcr.rel(r["std_err"], d["cluster0"])}
        print(f"{kind} p={p} g={g} {name}: restatement vs dummy regression {dist}; two roundings of the dummy regression {noise:.2e}; bar {bar:.2e}")
        assert max(dist.values()) <= bar, (name, dist, bar)
        assert np.all(np.asarray(r["std_err"], dtype=np.float64) > 0)


@pytest.mark.parametrize("kind,p", [("small5", 3), ("ragged7", 4), ("balanced", 3)])
def test_two_key_routes_agree(kind, p):
    F, y, off, k1, k2 = c2.balanced_frame() if kind == "balanced" else c2.frame(kind, p)
    F, y = np.asarray(F, dtype=np.float64), np.asarray(y, dtype=np.float64)
    keys = dict(_cluster_keys(k1, len(y), p), second=np.asarray(k2))
    for name, ck in keys.items():
        r = wcr.report(F, y, (k1, k2), ck, "cluster0")
        d = wcr.dummy_cluster0(F, y, (k1, k2), ck)
        dist = {"beta": wcr.rel(r["beta"], d["beta"]), "cluster0": wcr.rel(r["std_err"], d["cluster0"])}
        print(f"{kind} p={p} {name}: restatement vs dummy regression {dist}")
        assert max(dist.values()) <= 1e-15, (name, dist)


# ---- 2. K and df_resid follow the definition
def test_parameters_and_degrees_of_freedom():
    ld = np.longdouble
    F, y, off, k1, k2 = c2.frame("small5", 3)
    F, y = np.asarray(F, dtype=np.float64), np.asarray(y, dtype=np.float64)
    n, p = F.shape
    G1, G2, Cc = w2r.components(k1, k2)
    keys = _cluster_keys(k1, n, 3)
    # (a) one absorbed key, clustered on itself: K = p + 1, the numbers of within_reference
    a = wcr.report(F, y, k1, keys["equal"], "cluster")
    old = wr.report(F, y, k1, "cluster")
    assert (a["K"], a["absorb_nested"], a["n_clusters"], a["df_resid"]) == (p + 1, (True,), G1, G1 - 1) and old["df_resid"] == G1 - 1
    assert wcr.rel(a["std_err"], old["std_err"]) < 1e-17 and np.array_equal(a["beta"], old["beta"])
    assert wcr.rel(a["t"], old["t"]) < 1e-17 and np.allclose(a["p"], old["p"], rtol=1e-13, atol=0) and a["t_crit"] == old["t_crit"]
    # (b) coarser and nested: the effects are not counted, the one intercept is
    b = wcr.report(F, y, k1, keys["nested"], "cluster")
    gc = len(np.unique(keys["nested"]))
    assert 2 <= gc < G1 and (b["K"], b["absorb_nested"], b["n_clusters"], b["df_resid"]) == (p + 1, (True,), gc, gc - 1)
    c = (ld(gc) / ld(gc - 1)) * (ld(n - 1) / ld(n - p - 1))
    assert wcr.rel(b["std_err"], b["se_all"]["cluster0"] * np.sqrt(c)) < 1e-17
    # (c) crossing: every effect is a parameter, no intercept besides
    x = wcr.report(F, y, k1, keys["crossing"], "cluster")
    gx = len(np.unique(keys["crossing"]))
    assert (x["K"], x["absorb_nested"], x["n_clusters"], x["df_resid"]) == (p + G1, (False,), gx, gx - 1)
    c = (ld(gx) / ld(gx - 1)) * (ld(n - 1) / ld(n - p - G1))
    assert wcr.rel(x["std_err"], x["se_all"]["cluster0"] * np.sqrt(c)) < 1e-17
    # two absorbed keys, no factor nested: K = p + A
    x2 = wcr.report(F, y, (k1, k2), keys["crossing"], "cluster")
    assert (x2["K"], x2["absorb_nested"]) == (p + G1 + G2 - Cc, (False, False))
    # (d) the cluster key is the SECOND absorbed key: the numbers of within2_reference with the keys swapped.  beta and the CR0 errors agree
    # to the long double floor (the sweeps run in the other order, so not bit for bit); the counts agree.  The two DEFINITIONS of K do
    # not: A_2 = G2 - C gives the components to the second key, so this call counts K = p + G1 + 1 where the swapped call counts
    # p + 1 + (A - G2) = p + G1 + 1 - C.  The "cluster" errors therefore agree once each is freed of its own (n - 1) / (n - K)
    d = wcr.report(F, y, (k1, k2), k2, "cluster")
    assert (d["K"], d["absorb_nested"], d["n_clusters"], d["df_resid"]) == (p + G1 + 1, (False, True), G2, G2 - 1)
    swapped = w2r.report(F, y, k2, k1, "cluster")
    assert (swapped["df_resid"], swapped["n_groups"]) == (G2 - 1, G2) and d["t_crit"] == swapped["t_crit"]
    assert wcr.rel(d["beta"], swapped["beta"]) < 1e-15 and wcr.rel(d["se_all"]["cluster0"], swapped["se_all"]["cluster0"]) < 1e-15
    k_swapped = p + 1 + (G1 + G2 - Cc - G2)
    assert d["K"] - k_swapped == Cc
    f_new, f_old = ld(n - 1) / ld(n - d["K"]), ld(n - 1) / ld(n - k_swapped)
    assert wcr.rel(d["std_err"] / np.sqrt(f_new), swapped["std_err"] / np.sqrt(f_old)) < 1e-15
    # two keys clustered on the FIRST: the definition of within2_reference, K = p + 1 + (A - G1)
    e = wcr.report(F, y, (k1, k2), k1, "cluster")
    first = w2r.report(F, y, k1, k2, "cluster")
    assert e["K"] == p + 1 + (G2 - Cc) and e["absorb_nested"] == (True, False)
    assert np.array_equal(e["beta"], first["beta"]) and wcr.rel(e["std_err"], first["std_err"]) < 1e-17 and e["df_resid"] == first["df_resid"]


def test_nestedness_is_decided_from_integers():
    lv = np.array([0, 0, 1, 1, 2, 2, 2])
    assert wcr.nested(lv, np.array([5, 5, 9, 9, 5, 5, 5])) and not wcr.nested(lv, np.array([5, 5, 9, 9, 5, 5, 6]))
    assert wcr.nested(lv * 7 - 3, lv) and wcr.nested(lv, np.zeros(7, dtype=np.int64))
    assert wcr.parameters(3, 12, 4, True, False) == 3 + 4 + 1 and wcr.parameters(3, 12, 4, False, False) == 3 + 16
    assert wcr.parameters(3, 12, 4, True, True) == 4 and wcr.parameters(3, 12, 0, False, False) == 15


def test_narrower_formats_run_the_same_code():
    F, y, off, codes = wc.ragged_frame(4)
    ck = _cluster_keys(codes, len(y), 1)["crossing"]
    ld, f64, f32 = (wcr.report(F, y, codes, ck, "cluster", dt) for dt in (np.longdouble, np.float64, np.float32))
    assert f64["std_err"].dtype == np.float64 and f32["std_err"].dtype == np.float32
    assert wcr.rel(f64["std_err"], ld["std_err"]) < 1e-11 and wcr.rel(f32["std_err"], ld["std_err"]) < 1e-1
    other = wr.report(F, y, codes, "cluster")  # clustering on the absorbed key is another estimator on this frame
    assert wcr.rel(other["std_err"], ld["std_err"]) > 0.05 and np.array_equal(other["beta"], ld["beta"])
    assert wcr.select(ld, "cluster0")["std_err"] is ld["se_all"]["cluster0"]


# ---- 3. exports, header, build lists
def _prototypes(text):
    out = {}
    for m in re.finditer(r"^int\s+(pds_\w+)\s*\(([^;]*?)\)\s*;", text, flags=re.M | re.S):
        out[m.group(1)] = [a.strip() for a in m.group(2).replace("\n", " ").split(",")]
    return out


def test_exported_and_declared():
    from polars_ds_extension_amd import _lib

    assert len(NEW) == 8 and all(n in _lib.EXPORTS for n in NEW)
    header = (ROOT / "include" / "pds_lstsq.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    protos = _prototypes(text)
    for n in NEW:
        assert len(re.findall(rf"^int\s+{n}\s*\(", text, flags=re.M)) == 1, n
        base = n.replace("within_cl_", "within_").replace("within2_cl_", "within2_fx_")
        assert protos[n][:-1] == protos[base] and protos[n][-1] == "pds_cluster_key* cl", n  # the base list plus the trailing struct
    assert len(re.findall(r"\}\s*pds_cluster_key;", text)) == 1
    assert [f[0] for f in _lib.ClusterKey._fields_] == ["codes", "n_levels", "n_clusters", "nested1", "nested2"]
    assert C.sizeof(_lib.ClusterKey) == 32
    doc = header[header.index("pds_lin_reg_within_cl_* / pds_lin_reg_within2_cl_*"):header.index("} pds_cluster_key;")]
    for word in ("DEFINITION", "no equivalence", "K = p + sum_f (nested_f ? 0 : A_f) + (some factor nested ? 1 : 0)", "A_2 = G2 - C",
                 "NESTED when every occupied level of it has all its rows in one cluster", "Gc - 1 degrees of freedom", "Gc < 2 PDS_ERR_INVALID",
                 "cl == NULL", "before anything is indexed by a code", "K = p + 1 + (A - G1)", "K = p + A"):
        assert word in doc, word
    capi = (ROOT / "polars_ds_extension_amd" / "csrc" / "capi_within_cluster.hpp").read_text()
    assert "DEFINITIONS" in capi and "no equivalence" in capi and "K = p + sum_f (nested_f ? 0 : A_f)" in capi


def test_signature_table_matches_the_header():
    """_lib.py gives every new symbol the argument count of its declaration (the library is loaded: its argtypes are set on load)"""
    from polars_ds_extension_amd import _lib

    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "pds_lstsq.h").read_text(), flags=re.S)
    protos = _prototypes(text)
    lib = _lib.load()
    for n in NEW:
        assert hasattr(lib, n), n
        assert len(getattr(lib, n).argtypes) == len(protos[n]), n
    assert not _lib.missing_exports()


def test_source_lists_the_kernels():
    csrc = ROOT / "polars_ds_extension_amd" / "csrc"
    assert "within_cluster.hip" in (csrc / "Makefile").read_text()
    capi = (csrc / "capi.hip").read_text()
    assert capi.index('#include "capi_within_cluster.hpp"') < capi.index('#include "capi_within.hpp"') < capi.index('#include "capi_within2.hpp"')
    text = (csrc / "within_cluster.hip").read_text()
    code = re.sub(r"//[^\n]*", "", text)
    assert '#include "within_cluster_dev.hpp"' in text and '#include "score_meat_dev.hpp"' in text
    for name in ("within_row_scores_kernel<T, P>", "cluster_gather_chunk_kernel<P>", "score_long_meat_kernel<false>", "cluster_nested_kernel"):
        assert name in code, name
    assert set(re.findall(r"atomic\w+", code)) == {"atomicOr"}  # one integer flag per factor, nothing else
    assert not re.search(r"\bwhile\s*\(", code) and "__shared__" not in code and "__syncthreads" not in code
    host = (csrc / "capi_within_cluster.hpp").read_text()
    assert "launch_within2_order(" in host and "launch_within2_level_starts(" in host and "launch_within2_range_check(" in host
    assert host.index("launch_within2_range_check(") < host.index("launch_within2_gather_codes(") < host.index("launch_within2_order(")
    import polars_ds_extension_amd as pds
    import inspect

    assert "cluster_key" in inspect.signature(pds.lstsq.lin_reg_report).parameters
    assert "cluster_key" in inspect.signature(pds.lstsq.fixed_effects).parameters
    assert "cluster_key" not in inspect.signature(pds.lstsq.lin_reg).parameters  # (it computes no errors)


# ---- 4. argument errors, before any library call
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
    F, y, off, k1, k2 = c2.frame("small5", 3)
    cols = c2.columns(F)
    ck = np.arange(len(y)) % 4
    with pytest.raises(ValueError, match="`cluster_key` goes with `absorb` or `absorb_offsets` only"):
        ls.lin_reg_report(*cols, target=y, std_err="cluster", cluster_key=ck)
    for absorb in ({"absorb": k1}, {"absorb_offsets": off}, {"absorb": [k1, k2]}):
        for se in ("se", "hc1"):
            with pytest.raises(ValueError, match='`cluster_key` goes with std_err="cluster" or "cluster0" only'):
                ls.lin_reg_report(*cols, target=y, std_err=se, cluster_key=ck, **absorb)
        with pytest.raises(ValueError, match="`cluster_key` together with `cluster` / `cluster_offsets`"):
            ls.lin_reg_report(*cols, target=y, std_err="cluster", cluster_key=ck, cluster=ck, **absorb)
        with pytest.raises(ValueError, match="`cluster_key` together with `cluster` / `cluster_offsets`"):
            ls.lin_reg_report(*cols, target=y, std_err="cluster0", cluster_key=ck, cluster_offsets=off, **absorb)
        for bad in (ck.astype(np.float64), ck.astype(np.float32), ck > 1):
            with pytest.raises(ValueError, match="`cluster_key` must be an integer column"):
                ls.lin_reg_report(*cols, target=y, std_err="cluster", cluster_key=bad, **absorb)
    with pytest.raises(ValueError, match='`cluster_key` goes with std_err="cluster" or "cluster0" only'):
        ls.fixed_effects(*cols, target=y, absorb=[k1, k2], cluster_key=ck)  # (std_err defaults to "se")
    with pytest.raises(ValueError, match="`cluster_key` must be an integer column"):
        ls.fixed_effects(*cols, target=y, absorb=[k1, k2], std_err="cluster", cluster_key=ck * 0.5)
    with pytest.raises(TypeError, match="cluster_key"):
        ls.lin_reg(*cols, target=y, absorb=k1, cluster_key=ck)
    # the old spellings keep refusing
    with pytest.raises(ValueError, match='std_err="cluster" means the absorbed key'):
        ls.lin_reg_report(*cols, target=y, absorb=k1, std_err="cluster", cluster=ck)


def test_polars_expression_points_to_lstsq():
    from polars_ds_extension_amd import polars_exprs

    with pytest.raises(NotImplementedError, match=r"lstsq\.lin_reg_report\(\.\.\., absorb=, cluster_key=\)"):
        polars_exprs.lin_reg_report("x1", target="y", absorb="firm", std_err="cluster", cluster_key="state")
