"""The two-factor fixed-effects regression without a GPU: the reference (within2_reference.py) against the explicit dummy-variable
regression, the component count and the degrees of freedom, the sweep count of a balanced panel, the C ABI surface (exports, header
declarations, the ctypes struct, the build lists) and the argument errors of lstsq.lin_reg / lin_reg_report(absorb=[k1, k2]), which
are raised before any library call.

The reference is right.  On a frame with p = 3, G1 = 12 and G2 = 5 its long double run (tolerance at the long double rounding floor)
must agree to 1e-15 relative with the regression on the features, one dummy per level of key 1 and one per level of key 2 less one
level per component, in long double: beta, the classical standard errors (n - rank degrees of freedom) and the CR0 standard errors
clustered on key 1 (Frisch-Waugh-Lovell; the dummy entries of a cluster's score do not enter the features' block of the sandwich)."""
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

NEW = ["pds_lin_reg_within2_grouped_f64", "pds_lin_reg_within2_grouped_f32", "pds_lin_reg_within2_by_key_f64", "pds_lin_reg_within2_by_key_f32"]


# ---- 1. the reference against the dummy-variable regression
def test_reference_equals_dummy_regression():
    assert np.finfo(np.longdouble).eps < 1e-18
    F, y, off, k1, k2 = c2.frame("small5", 3)
    assert (len(np.unique(k1)), len(np.unique(k2))) == (12, 5)
    r = c2.truth("small5", 3, "se")
    assert (r["n_groups"], r["n_groups2"], r["n_components"]) == (12, 5, 1) and r["df_resid"] == len(y) - 3 - 16
    d = w2r.dummy_report(F, y, k1, k2)
    assert w2r.dummy_design(F, k1, k2).shape[1] == 3 + 12 + 4
    dist = {"beta": w2r.rel(r["beta"], d["beta"]), "se": w2r.rel(r["se_all"]["se"], d["se"]), "cluster0": w2r.rel(r["se_all"]["cluster0"], d["cluster0"])}
    print(dist)
    assert max(dist.values()) <= 1e-15, dist
    # the cluster form's factor and the degrees of freedom follow the definition
    n, p, A, G1 = len(y), 3, 16, 12
    ld = np.longdouble
    c = (ld(G1) / ld(G1 - 1)) * (ld(n - 1) / ld(n - (p + 1 + A - G1)))
    assert w2r.rel(r["se_all"]["cluster"], r["se_all"]["cluster0"] * np.sqrt(c)) < 1e-17
    assert c2.truth("small5", 3, "cluster")["df_resid"] == 11 and c2.truth("small5", 3, "cluster0")["t_dof"] == 11


def test_reference_formats_and_levels():
    """the narrower formats run the same code; the levels of BOTH factors dominate the frame"""
    import within_reference as wr

    F, y, off, k1, k2 = c2.frame("ragged7", 4)
    ld = c2.truth("ragged7", 4, "cluster")
    f64 = c2.ref("ragged7", 4, "cluster", "float64", "tight")
    assert f64["beta"].dtype == np.float64 and w2r.rel(f64["beta"], ld["beta"]) < 1e-12
    f32 = w2r.report(F, y, k1, k2, "cluster", np.float32, sweeps=f64["n_iter"])
    assert f32["beta"].dtype == np.float32 and w2r.rel(f32["beta"], ld["beta"]) < 1e-3
    for other in (wr.report(F, y, k1, "se"), wr.report(F, y, k2, "se")):  # absorbing one key alone is another model
        assert w2r.rel(other["beta"], ld["beta"]) > 0.05
    assert f64["deltas"] == sorted(f64["deltas"], reverse=True) and len(f64["deltas"]) == f64["n_iter"]
    with pytest.raises(w2r.ConvergenceError, match="did not converge"):
        w2r.report(F, y, k1, k2, "se", np.float64, 1e-13, max_iter=3)


# ---- 2. components and degrees of freedom
@pytest.mark.parametrize("blocks", [1, 2, 3])
def test_components(blocks):
    F, y, off, k1, k2 = c2.blocks_frame(2, 0, blocks)
    g2 = sum(4 + b for b in range(blocks))
    assert w2r.components(k1, k2) == (8 * blocks, g2, blocks)
    r = w2r.report(F, y, k1, k2, "se")
    A = 8 * blocks + g2 - blocks
    assert (r["n_components"], r["df_resid"]) == (blocks, len(y) - 2 - A)
    assert w2r.dummy_design(F, k1, k2).shape[1] == 2 + A  # one level of key 2 dropped per component: full column rank
    d = w2r.dummy_report(F, y, k1, k2)
    assert w2r.rel(r["beta"], d["beta"]) <= 1e-15 and w2r.rel(r["se_all"]["se"], d["se"]) <= 1e-15
    # relabelled and shuffled keys give the same counts
    rng = np.random.default_rng(blocks)
    perm = rng.permutation(len(y))
    assert w2r.components((k1 * 5 - 3)[perm], (1000 - k2)[perm]) == (8 * blocks, g2, blocks)


def test_balanced_panel_converges_in_one_sweep():
    """A complete balanced panel: ONE sweep is the whole projection.  The stopping rule sees that at the second sweep, whose delta is at
    the rounding floor -- n_iter is 2 at every tolerance above it -- and the columns after one sweep are those of the truth."""
    F, y, off, k1, k2 = c2.balanced_frame()
    Z = np.column_stack([F, y])
    truth, _, _ = w2r.demean(Z, k1, k2)
    for dt, floor in ((np.longdouble, 1e-17), (np.float64, 1e-13)):
        one, _, d1 = w2r.demean(Z, k1, k2, dt, sweeps=1)
        assert w2r.rel(one, truth) < floor
        for tol in (1e-8, floor):
            zt, n_iter, deltas = w2r.demean(Z, k1, k2, dt, tol)
            assert n_iter == 2 and deltas[0] > 0.1 and deltas[1] <= floor, (dt, tol, deltas)


# ---- 3. exports, header, build lists
def test_exported_and_declared():
    from polars_ds_extension_amd import _lib

    assert all(n in _lib.EXPORTS for n in NEW)
    header = (ROOT / "include" / "pds_lstsq.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for n in NEW:
        assert len(re.findall(rf"^int\s+{n}\s*\(", text, flags=re.M)) == 1, n
    assert len(re.findall(r"\}\s*pds_within2_out;", text)) == 1
    assert [f[0] for f in _lib.Within2Out._fields_] == ["pred", "resid", "r2_overall", "df_resid", "n_groups_used", "n_groups2_used", "n_components",
                                                        "n_iter"]
    doc = header[header.index("pds_lin_reg_within2_*: fixed-effects"):header.index("} pds_within2_out;")]
    for word in ("DEFINITION", "no equivalence", "A = G1 + G2 - C", "absorb_tol", "did not converge", "K = p + 1 + (A - G1)", "1e-10"):
        assert word in doc, word
    capi = (ROOT / "polars_ds_extension_amd" / "csrc" / "capi_within2.hpp").read_text()
    assert "DEFINITIONS" in capi and "A = G1 + G2 - C" in capi


def test_built_library_exports():
    from polars_ds_extension_amd import _lib

    lib = _lib.load()
    for n in NEW:
        assert hasattr(lib, n), n
    assert not [s for s in _lib.missing_exports() if "within2" in s]


def test_source_lists_the_kernel():
    csrc = ROOT / "polars_ds_extension_amd" / "csrc"
    assert "within2_sweep.hip" in (csrc / "Makefile").read_text()
    capi = (csrc / "capi.hip").read_text()
    assert capi.index('#include "capi_within.hpp"') < capi.index('#include "capi_within2.hpp"')
    text = (csrc / "within2_sweep.hip").read_text()
    assert not re.search(r"atomic(Add|Or|Max|Min|CAS|Exch)", text)  # every sum in a fixed order
    assert not re.search(r"\bwhile\s*\(", text)  # every device loop is a counted for
    assert "within_impl<double, R>" in (csrc / "capi_within2.hpp").read_text()  # the final stage is the one-factor fit's


# ---- 4. without a device
def test_no_cpu_fallback_without_device():
    import torch

    import polars_ds_extension_amd as pds
    from polars_ds_extension_amd import _lib

    F, y, off, k1, k2 = c2.frame("small5", 3)
    calls = (lambda: pds.lin_reg_report(*c2.columns(F), target=y, absorb=[k1, k2]), lambda: pds.lin_reg(*c2.columns(F), target=y, absorb=[k1, k2]))
    if torch.cuda.is_available():  # (a GPU box runs this file too: there the calls go through)
        assert calls[0]()["n_components"] == 1 and len(calls[1]()) == 3
        return
    for call in calls:
        with pytest.raises(_lib.PdsError) as e:
            call()
        assert e.value.code == -4  # PDS_ERR_HIP: nothing is computed on the CPU
    # the entry points themselves.  No context can be made without a device, so they are handed a zeroed block in its place: all they
    # read of it before the first HIP call, which fails, is the device index
    import ctypes as C

    from polars_ds_extension_amd.lstsq import _Cols

    lib, fake = _lib.load(), C.create_string_buffer(1 << 16)
    cs = _Cols(np.ascontiguousarray(y), c2.columns(F))
    beta = np.empty(3)
    k, codes, off = np.ascontiguousarray(k1, dtype=np.int64), np.ascontiguousarray(k2, dtype=np.int32), np.ascontiguousarray(off, dtype=np.int64)
    ng = C.c_int64(0)
    for sfx, R in (("f64", _lib.ReportF64), ("f32", _lib.ReportF32)):
        rep = R(C.c_void_p(beta.ctypes.data), None, None, None, None, None, 0.0, 0.0)
        rc = getattr(lib, "pds_lin_reg_within2_grouped_" + sfx)(C.cast(fake, C.c_void_p), cs.cols, 3, C.c_int64(len(y)), C.c_void_p(off.ctypes.data),
                                                               C.c_int64(12), C.c_void_p(codes.ctypes.data), C.c_int64(5), 0, 0, C.c_double(1e-8), 10,
                                                               C.byref(rep), None)
        assert rc == -4, rc
        rc = getattr(lib, "pds_lin_reg_within2_by_key_" + sfx)(C.cast(fake, C.c_void_p), cs.cols, C.c_void_p(k.ctypes.data), C.c_void_p(codes.ctypes.data),
                                                              C.c_int64(5), 3, C.c_int64(len(y)), 0, 0, C.c_double(1e-8), 10, C.byref(rep), None, C.byref(ng))
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
    for fn in (ls.lin_reg_report, ls.lin_reg):
        with pytest.raises(NotImplementedError, match="three or more absorbed keys"):
            fn(*cols, target=y, absorb=[k1, k2, k1])
        with pytest.raises(ValueError, match="one integer column or a list of exactly two"):
            fn(*cols, target=y, absorb=[k1])
        with pytest.raises(ValueError, match="`absorb_offsets` together with a second absorbed key"):
            fn(*cols, target=y, absorb=[k1, k2], absorb_offsets=off)
        with pytest.raises(NotImplementedError, match="weights"):
            fn(*cols, target=y, absorb=[k1, k2], weights=np.ones(len(y)))
        with pytest.raises(ValueError, match="the intercept is absorbed"):
            fn(*cols, target=y, absorb=(k1, k2), add_bias=True)
        with pytest.raises(ValueError, match="`absorb_tol` must be > 0"):
            fn(*cols, target=y, absorb=[k1, k2], absorb_tol=0.0)
        with pytest.raises(ValueError, match="`absorb_max_iter` must be >= 1"):
            fn(*cols, target=y, absorb=[k1, k2], absorb_max_iter=0)
    with pytest.raises(NotImplementedError, match="`return_effects` with two absorbed keys"):
        ls.lin_reg_report(*cols, target=y, absorb=[k1, k2], return_effects=True)
    with pytest.raises(ValueError, match='std_err="cluster" means the absorbed key'):
        ls.lin_reg_report(*cols, target=y, absorb=[k1, k2], std_err="cluster", cluster=k1)
    with pytest.raises(ValueError, match='std_err is "se", "cluster" or "cluster0"'):
        ls.lin_reg_report(*cols, target=y, absorb=[k1, k2], std_err="bootstrap")
    from polars_ds_extension_amd._lib import PdsError

    with pytest.raises(PdsError, match="HC0 - HC3") as e:  # refused with the library's code, without asking the library
        ls.lin_reg_report(*cols, target=y, absorb=[k1, k2], std_err="hc3")
    assert e.value.code == -5


def test_polars_expression_points_to_lstsq():
    pl = pytest.importorskip("polars")
    from polars_ds_extension_amd import polars_exprs as pe

    with pytest.raises(NotImplementedError, match=r"lstsq\.lin_reg_report"):
        pe.lin_reg_report("a", "b", target="y", absorb=["firm", "year"])
