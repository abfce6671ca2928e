"""The estimated effects of the two-way fixed-effects regression and the component labelling without a GPU: the restatement
(within2_effects_reference.py) against the explicit dummy-variable regression, the normalisation, the identity, hook-and-compress
against the union-find of within2_reference.py and its round bound on a scrambled chain, the C ABI surface (exports, header
declarations, the ctypes struct, the build list) and the argument errors of lstsq.fixed_effects / absorb_components, which are raised
before any library call.

The restatement is right.  In long double (tolerance at the long double rounding floor) its effects must agree to 1e-15 relative
with the coefficients of the regression on the features, one dummy per level of key 1 and one per level of key 2 less the first
level of key 2 in every component (within2_reference.dummy_design), on four frames; measured 5e-19 .. 8e-18."""
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
import within2_effects_reference as fxr  # noqa: E402
import within2_reference as w2r  # noqa: E402

NEW = ["pds_lin_reg_within2_fx_grouped_f64", "pds_lin_reg_within2_fx_grouped_f32", "pds_lin_reg_within2_fx_by_key_f64",
       "pds_lin_reg_within2_fx_by_key_f32", "pds_absorb_components_i32"]
DUMMY_FRAMES = (("small5", 3, 1), ("blocks", 2, 3), ("panel", 4, 1), ("ragged7", 4, 1))  # frame, width, components


# ---- 1. the restatement against the dummy-variable regression; the normalisation; the identity
@pytest.mark.parametrize("kind,p,n_comp", DUMMY_FRAMES)
def test_reference_equals_dummy_coefficients(kind, p, n_comp):
    assert np.finfo(np.longdouble).eps < 1e-18
    F, y, off, k1, k2 = c2.frame(kind, p)
    F, y = np.asarray(F, dtype=np.float64), np.asarray(y, dtype=np.float64)
    r = fxr.effects(F, y, k1, k2)
    alpha, gamma, beta = fxr.dummy_effects(F, y, k1, k2)
    dist = {"effects": fxr.rel(r["effects"], alpha), "effects2": fxr.rel(r["effects2"], gamma), "beta": fxr.rel(r["beta"], beta)}
    print(kind, p, dist)
    assert max(dist.values()) <= 1e-15, dist
    assert fxr.rel(r["beta"], c2.truth(kind, p, "se")["beta"]) <= 1e-15  # the tables change nothing in the fit
    # exactly one zero gamma per component, at the lowest code of key 2 in it
    assert r["n_components"] == n_comp and int((r["effects2"] == 0).sum()) == n_comp
    for root, ref in zip(np.flatnonzero(r["component"] == np.arange(len(r["component"]))), r["reference_levels"]):
        assert r["effects2"][ref] == 0 and ref == np.flatnonzero(r["component2"] == root)[0]
    # y = alpha + gamma + x' beta + resid, at the long double floor
    i1, i2 = np.unique(k1, return_inverse=True)[1], np.unique(k2, return_inverse=True)[1]
    ld = np.longdouble
    gap = y.astype(ld) - r["effects"][i1] - r["effects2"][i2] - F.astype(ld) @ r["beta"] - r["resid"]
    scale = np.abs(y) + np.abs(r["effects"][i1]) + np.abs(r["effects2"][i2]) + np.abs(F.astype(ld) * r["beta"]).sum(axis=1)
    assert np.all(np.abs(gap) <= (3 * p + 16) * np.finfo(ld).eps * scale), float(np.max(np.abs(gap) / scale))
    assert fxr.rel(r["resid"], c2.truth(kind, p, "se")["resid"]) <= 1e-13  # (residuals cancel: relative to their own size)


def test_narrower_formats_run_the_same_code():
    F, y, off, k1, k2 = c2.frame("small5", 3)
    truth = fxr.effects(F, y, k1, k2)
    f64 = fxr.effects(F, y, k1, k2, np.float64, 1e-13)
    assert f64["effects"].dtype == np.float64 and fxr.rel(f64["effects"], truth["effects"]) < 1e-12
    assert int((f64["effects2"] == 0).sum()) == 1
    early = fxr.effects(F, y, k1, k2, np.float64, 1e-8, sweeps=f64["n_iter"] - 3)
    assert early["n_iter"] == f64["n_iter"] - 3 and fxr.rel(early["effects"], truth["effects"]) > fxr.rel(f64["effects"], truth["effects"])


# ---- 2. hook and compress
ALL_FRAMES = (("ragged7", 4), ("ragged300", 4), ("ragged7_32", 16), ("ragged300_32", 16), ("panel", 4), ("blocks", 2), ("singletons", 1),
              ("movers", 4), ("small5", 3), ("small3", 3), ("balanced", 3))


@pytest.mark.parametrize("kind,p", ALL_FRAMES)
def test_hook_compress_counts_equal_union_find(kind, p):
    assert {k for k, _ in ALL_FRAMES} == set(c2._FRAMES) | {"balanced"}  # every frame of within2_cases
    F, y, off, k1, k2 = c2.balanced_frame() if kind == "balanced" else c2.frame(kind, p)
    keys1, keys2, lab1, lab2, n_comp, rounds = fxr.components(k1, k2)
    assert (len(keys1), len(keys2), n_comp) == w2r.components(k1, k2)
    assert rounds <= fxr.round_cap(len(keys1) + len(keys2))  # (the restatement raises past the library's cap)
    # the label is the smallest level of key 1 of the component, and the labels are a partition of the cells
    i1, i2 = np.unique(k1, return_inverse=True)[1], np.unique(k2, return_inverse=True)[1]
    assert np.array_equal(lab1[i1], lab2[i2])
    for root in np.unique(lab1):
        assert root == np.flatnonzero(lab1 == root)[0]


def test_relabelled_shuffled_keys_give_the_same_partition():
    F, y, off, k1, k2 = c2.blocks_frame(2, 0, 3)
    base = fxr.components(k1, k2)
    perm = np.random.default_rng(3).permutation(len(y))
    other = fxr.components((k1 * 5 - 3)[perm], (k2 * 2 + 11)[perm])  # order-preserving relabelling
    assert np.array_equal(base[2], other[2]) and np.array_equal(base[3], other[3]) and base[4] == other[4] == 3


def test_round_cap_is_the_proved_one():
    """The trees of a component need not halve in ONE round: a root that is smaller than all its neighbours is not hooked into when
    they find a smaller one yet.  It hooks in the next round, so they halve in two, and the cap is 2 ceil(log2 nodes) + 1.  The
    restatement enforces that cap (it raises past it) like the library; the cap with one halving per round would refuse these."""
    k1, k2 = fxr.stagnant_tree()
    keys1, keys2, lab1, lab2, n_comp, rounds = fxr.components(k1, k2)
    assert (len(k1), len(keys1), len(keys2), n_comp) == (14, 8, 7, 1) == (14, 8, 7) + (w2r.components(k1, k2)[2],)
    assert rounds == 6 > fxr.ceil_log2(15) + 1 and rounds <= fxr.round_cap(15) == 9
    assert np.all(lab1 == 0) and np.all(lab2 == 0)
    k1, k2 = fxr.star(9)
    keys1, keys2, lab1, lab2, n_comp, rounds = fxr.components(k1, k2)
    assert (len(keys1), len(keys2), n_comp, rounds) == (10, 9, 1, 4) and rounds <= fxr.round_cap(19)
    # after round 2 of the star 9 of the 10 trees are left: the hooks of that round, restated
    root = np.concatenate([np.arange(10), np.arange(9)])  # round 1 hooked every code into its own level
    ru, rv = root[k1], root[10 + k2]
    hooked = np.unique(np.maximum(ru, rv)[ru != rv])
    assert list(hooked) == [9]
    # the cap is enforced: a graph is refused, not mislabelled, when the cap is lowered under its rounds
    k1, k2 = fxr.stagnant_tree()
    cap = fxr.round_cap
    try:
        fxr.round_cap = lambda n: fxr.ceil_log2(n) + 1
        with pytest.raises(fxr.RoundCapError, match="did not finish in 5 rounds"):
            fxr.components(k1, k2)
    finally:
        fxr.round_cap = cap
    # small graphs at random, trees and denser ones, every numbering: inside the cap
    rng = np.random.default_rng(11)
    worst = 0
    for _ in range(3000):
        n_a, n_b = int(rng.integers(1, 10)), int(rng.integers(1, 10))
        m = int(rng.integers(1, n_a + n_b + 3))
        i1, i2 = rng.integers(0, n_a, m), rng.integers(0, n_b, m)
        label, rounds = fxr.hook_compress(i1, i2, n_a, n_b)  # (raises past the cap)
        worst = max(worst, rounds - (fxr.ceil_log2(n_a + n_b) + 1))
        assert np.array_equal(label[i1], label[n_a + i2])
    print("rounds beyond ceil(log2 nodes) + 1, worst of 3000 random graphs:", worst)


def test_scrambled_chain_round_bound():
    """2 000 levels of key 1, each with rows in two neighbouring codes of key 2, numberings permuted: 4 001 nodes, diameter 4 000.
    On this chain hook and compress stays inside ceil(log2 nodes) + 1 rounds (the library's cap is 2 ceil(log2 nodes) + 1: the test
    above); plain label propagation needs thousands."""
    k1, k2 = fxr.scrambled_chain()
    assert len(k1) == 8000
    keys1, keys2, lab1, lab2, n_comp, rounds = fxr.components(k1, k2)
    bound = fxr.ceil_log2(len(keys1) + len(keys2)) + 1
    print("chain: rounds", rounds, "bound", bound)
    assert (len(keys1), len(keys2), n_comp, bound) == (2000, 2001, 1, 13)
    assert rounds <= bound
    assert np.all(lab1 == 0) and np.all(lab2 == 0)
    i1, i2 = np.unique(k1, return_inverse=True)[1], np.unique(k2, return_inverse=True)[1]
    assert fxr.propagate_rounds(i1, i2, 2000, 2001) > 1000
    b1, b2 = fxr.disjoint_blocks()
    assert fxr.components(b1, b2)[4] == 500 == w2r.components(b1, b2)[2]


# ---- 3. exports, header, build list
def test_exported_and_declared():
    from polars_ds_extension_amd import _lib

    assert all(n in _lib.EXPORTS for n in NEW)
    header = (ROOT / "include" / "pds_lstsq.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for n in NEW:
        assert len(re.findall(rf"^int\s+{n}\s*\(", text, flags=re.M)) == 1, n
    assert len(re.findall(r"\}\s*pds_within2_effects;", text)) == 1
    assert [f[0] for f in _lib.Within2Effects._fields_] == ["effects1", "effects2", "component1", "component2", "keys1", "cap1", "n_graph_rounds"]
    assert C.sizeof(_lib.Within2Effects) == 7 * 8
    doc = header[header.index("pds_lin_reg_within2_fx_*: pds_lin_reg_within2_*"):header.index("} pds_within2_effects;")]
    for word in ("DEFINITION", "no equivalence", "NORMALISATION", "LOWEST occupied code", "exactly 0.0", "alpha_raw[g] = a1[g][y]", "NaN"):
        assert word in doc, word
    two = header[header.index("pds_lin_reg_within2_*: fixed-effects"):header.index("} pds_within2_out;")]
    assert "union-find" not in two and "on the host" not in two and "atomicMin" in two and "component labelling did not finish" in two


def test_built_library_exports():
    from polars_ds_extension_amd import _lib

    lib = _lib.load()
    for n in NEW:
        assert hasattr(lib, n), n
    assert not _lib.missing_exports()


def test_source_lists_the_kernel():
    csrc = ROOT / "polars_ds_extension_amd" / "csrc"
    assert "within2_graph.hip" in (csrc / "Makefile").read_text()
    text = (csrc / "within2_graph.hip").read_text()
    code = re.sub(r"//[^\n]*", "", text)
    assert set(re.findall(r"atomic\w+", code)) == {"atomicMin", "atomicOr"}  # integer atomics only
    assert not re.search(r"\bwhile\s*\(", code)  # every loop is a counted for
    assert not re.search(r"atomic\w+\s*\(\s*\(?\s*(float|double)", code)
    import polars_ds_extension_amd as pds

    assert pds.fixed_effects is pds.lstsq.fixed_effects and pds.absorb_components is pds.lstsq.absorb_components


# ---- 4. without a device
def test_no_cpu_fallback_without_device():
    import torch

    import polars_ds_extension_amd as pds
    from polars_ds_extension_amd import _lib

    F, y, off, k1, k2 = c2.frame("small5", 3)
    calls = (lambda: pds.fixed_effects(*c2.columns(F), target=y, absorb=[k1, k2]), lambda: pds.absorb_components(k1, k2))
    if torch.cuda.is_available():  # (a GPU box runs this file too: there the calls go through)
        assert calls[0]()["n_components"] == 1 and calls[1]()["n_components"] == 1
        return
    for call in calls:
        with pytest.raises(_lib.PdsError) as e:
            call()
        assert e.value.code == -4  # PDS_ERR_HIP: nothing is computed on the CPU
    # the entry points themselves, handed a zeroed block in place of a context: all they read of it before the first HIP call, which
    # fails, is the device index
    from polars_ds_extension_amd.lstsq import _Cols

    lib, fake = _lib.load(), C.create_string_buffer(1 << 16)
    cs = _Cols(np.ascontiguousarray(y), c2.columns(F))
    beta = np.empty(3)
    k, codes, off = np.ascontiguousarray(k1, dtype=np.int64), np.ascontiguousarray(k2, dtype=np.int32), np.ascontiguousarray(off, dtype=np.int64)
    ng = C.c_int64(0)
    eff = np.empty(12)
    fx = _lib.Within2Effects(C.c_void_p(eff.ctypes.data), None, None, None, None, 12, 0)
    for sfx, R in (("f64", _lib.ReportF64), ("f32", _lib.ReportF32)):
        rep = R(C.c_void_p(beta.ctypes.data), None, None, None, None, None, 0.0, 0.0)
        rc = getattr(lib, "pds_lin_reg_within2_fx_grouped_" + sfx)(C.cast(fake, C.c_void_p), cs.cols, 3, C.c_int64(len(y)), C.c_void_p(off.ctypes.data),
                                                                  C.c_int64(12), C.c_void_p(codes.ctypes.data), C.c_int64(5), 0, 0, C.c_double(1e-8), 10,
                                                                  C.byref(rep), None, C.byref(fx))
        assert rc == -4, rc
        rc = getattr(lib, "pds_lin_reg_within2_fx_by_key_" + sfx)(C.cast(fake, C.c_void_p), cs.cols, C.c_void_p(k.ctypes.data), C.c_void_p(codes.ctypes.data),
                                                                 C.c_int64(5), 3, C.c_int64(len(y)), 0, 0, C.c_double(1e-8), 10, C.byref(rep), None,
                                                                 C.byref(ng), C.byref(fx))
        assert rc == -4, rc
    codes1 = np.ascontiguousarray(np.unique(k1, return_inverse=True)[1], dtype=np.int32)
    rc = lib.pds_absorb_components_i32(C.cast(fake, C.c_void_p), C.c_void_p(codes1.ctypes.data), C.c_int64(12), C.c_void_p(codes.ctypes.data),
                                       C.c_int64(5), C.c_int64(len(y)), 0, None, None, None, None, None, None)
    assert rc == -4, rc


# ---- 5. argument errors, before any library call
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
    for one in (k1, [k1], (k1,), [], ()):
        with pytest.raises(ValueError, match=r"lin_reg_report\(absorb=k, return_effects=True\)"):
            ls.fixed_effects(*cols, target=y, absorb=one)
    with pytest.raises(NotImplementedError, match="three or more absorbed keys"):
        ls.fixed_effects(*cols, target=y, absorb=[k1, k2, k1])
    with pytest.raises(NotImplementedError, match="weights"):
        ls.fixed_effects(*cols, target=y, absorb=[k1, k2], weights=np.ones(len(y)))
    with pytest.raises(ValueError, match="the intercept is absorbed"):
        ls.fixed_effects(*cols, target=y, absorb=(k1, k2), add_bias=True)
    with pytest.raises(ValueError, match='std_err is "se", "cluster" or "cluster0"'):
        ls.fixed_effects(*cols, target=y, absorb=[k1, k2], std_err="bootstrap")
    with pytest.raises(ls._lib.PdsError, match="HC0 - HC3") as e:
        ls.fixed_effects(*cols, target=y, absorb=[k1, k2], std_err="hc3")
    assert e.value.code == -5
    with pytest.raises(ValueError, match="`absorb_tol` must be > 0"):
        ls.fixed_effects(*cols, target=y, absorb=[k1, k2], absorb_tol=0.0)
    with pytest.raises(ValueError, match="`absorb_max_iter` must be >= 1"):
        ls.fixed_effects(*cols, target=y, absorb=[k1, k2], absorb_max_iter=0)
    # the report keeps refusing the effects, and says where they are
    with pytest.raises(NotImplementedError, match=r"`return_effects` with two absorbed keys.*fixed_effects"):
        ls.lin_reg_report(*cols, target=y, absorb=[k1, k2], return_effects=True)
    with pytest.raises(ValueError, match="an absorbed key must be an integer column"):
        ls.absorb_components(np.asarray(k1, dtype=np.float64), k2)
    with pytest.raises(ValueError, match="one entry per row"):
        ls.absorb_components(k1, np.asarray(k2)[:-1])
    with pytest.raises(ValueError, match="empty"):
        ls.absorb_components(np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64))
