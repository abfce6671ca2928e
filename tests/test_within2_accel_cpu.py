"""The accelerated (Irons-Tuck) iteration of the two-factor fixed-effects regression without a GPU: the NumPy restatement in the
device's table arithmetic (within2_accel_reference.py) against within2_reference.py, and the argument errors of `absorb_accel`, which
are raised before any library call.

  * acceleration OFF: the restatement takes exactly within2_reference.demean's sweeps on every frame -- 971 on the few-movers frame;
  * acceleration ON: the projected columns are at most 10 x as far from the long double truth as the plain float64 run's, the sweep
    count is never above the plain one, at both tolerances; on the few-movers frame (p = 4, seed 0) it is at most ONE FIFTH of the
    plain count at both tolerances (a condition: the restatement has 87 against 971 and 159 against 1 768);
  * the seeds of within2_accel_cases.py satisfy their condition (delta at the stop <= tol / 2 for the accelerated run).
"""
import re
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT))

import within2_accel_cases as ac  # noqa: E402
import within2_accel_reference as ar  # noqa: E402
import within2_cases as c2  # noqa: E402
import within2_reference as w2r  # noqa: E402

FRAMES = (("movers", 4), ("panel", 4), ("panel", 16), ("ragged300", 4), ("ragged300", 16), ("ragged7", 4), ("blocks", 4), ("singletons", 1),
          ("small5", 3), ("small3", 3))


def _z(fr):
    F, y, off, k1, k2 = fr
    return np.column_stack([np.asarray(F, dtype=np.float64), np.asarray(y, dtype=np.float64)]), k1, k2


# ---- 1. off: the plain sweeps of within2_reference, on that module's own frames (its seeds) and on this module's
@pytest.mark.parametrize("kind,p", FRAMES)
def test_off_is_the_plain_iteration(kind, p):
    for fr in (c2.frame(kind, p), ac.frame(kind, p)):
        Z, k1, k2 = _z(fr)
        for tol_name in ("default", "tight"):
            zt, n_iter, deltas = w2r.demean(Z, k1, k2, np.float64, c2.TOLS[tol_name])
            mine = ar.tables(Z, k1, k2, np.float64, c2.TOLS[tol_name], accel=False)
            assert mine[3] == n_iter, (kind, p, tol_name, mine[3], n_iter)
            assert w2r.rel(mine[0], zt) < 1e-9  # (the same projection; the tables round differently)
    if kind == "movers":
        assert ar.tables(*_z(c2.frame("movers", 4)), np.float64, 1e-8, accel=False)[3] == 971


def test_fixed_sweep_count_and_limit():
    Z, k1, k2 = _z(ac.frame("small5", 3))
    own = ar.tables(Z, k1, k2, np.float64, 1e-8)
    again = ar.tables(Z, k1, k2, np.float64, 1e-8, sweeps=own[3])
    assert again[3] == own[3] and np.array_equal(again[0], own[0]) and again[4] == own[4]
    assert ar.tables(Z, k1, k2, np.float64, 1e-8, sweeps=3)[3] == 3  # an odd count: stopped in the middle of a cycle
    with pytest.raises(w2r.ConvergenceError, match="did not converge in 3 sweeps"):
        ar.tables(Z, k1, k2, np.float64, 1e-13, max_iter=3)
    # a column whose two steps are equal (d = 0) is left alone: c_j = 0
    D = np.array([[1.0, 2.0], [3.0, 5.0]])
    assert np.array_equal(ar.coefficients(D, D, np.float64), [0.0, 0.0])
    assert np.array_equal(ar.coefficients(D, D * np.array([1.0, np.inf]), np.float64) == 0.0, [True, True])


# ---- 2. on: accuracy at the stopping rule, sweep counts
@pytest.mark.parametrize("kind,p", FRAMES)
def test_accelerated_accuracy_and_sweeps(kind, p):
    assert np.finfo(np.longdouble).eps < 1e-18
    for tol_name in ("default", "tight"):
        n_plain, _, d_plain = ac.columns_run(kind, p, tol_name, False)
        n_acc, delta, d_acc = ac.columns_run(kind, p, tol_name, True)
        print(f"{kind} p={p} {tol_name}: sweeps {n_plain} -> {n_acc}; distance from the truth plain {d_plain:.2e}, accelerated {d_acc:.2e}; "
              f"delta / tol at the stop {delta / c2.TOLS[tol_name]:.2f}")
        assert d_acc <= 10.0 * d_plain, (kind, p, tol_name, d_acc, d_plain)
        assert n_acc <= n_plain, (kind, p, tol_name, n_acc, n_plain)
        if kind == "movers":
            assert ac.seed("movers", 4) == 0 and 5 * n_acc <= n_plain, (tol_name, n_acc, n_plain)
        else:
            assert delta <= 0.5 * c2.TOLS[tol_name], (kind, p, tol_name, delta)  # the seed's condition


def test_seed_table_is_the_search():
    for kind, p in (("panel", 4), ("panel", 16), ("singletons", 1), ("small3", 3), ("ragged300_32", 16), ("one2", 2), ("many2", 4)):
        assert ac.find_seed(kind, p) == ac.seed(kind, p), (kind, p)
    F, y, off, k1, k2 = ac.frame("many2", 4)
    assert len(np.unique(k2)) > 4096 and int(np.max(k2)) + 1 == len(np.unique(k2))  # more occupied codes than the level kernel has waves
    assert len(np.unique(ac.frame("one2", 2)[4])) == 1


def test_fit_equals_the_references():
    """within2_accel_reference.fit with acceleration off is within2_reference.report and within2_effects_reference.effects"""
    import within2_effects_reference as fxr

    F, y, off, k1, k2 = ac.frame("small5", 3)
    mine = ar.fit(F, y, k1, k2, "cluster", accel=False)
    theirs, fx = w2r.report(F, y, k1, k2, "cluster"), fxr.effects(F, y, k1, k2)
    for k in w2r.FIELDS + w2r.ROW_FIELDS:
        assert w2r.rel(mine[k], theirs[k]) < 1e-16, k
    for k in ar.EFFECT_FIELDS:
        assert w2r.rel(mine[k], fx[k]) < 1e-16, k
    assert ac.truth("small5", 3, "cluster")["df_resid"] == 11


# ---- 3. the surface: header, option lists, argument errors before any library call
def test_option_is_declared():
    from polars_ds_extension_amd import lstsq

    header = (ROOT / "include" / "pds_lstsq.h").read_text()
    assert '"within2_accel"' in header[header.index("Behaviour switches of a context"):header.index("int pds_ctx_set_option(")]
    doc = header[header.index("pds_lin_reg_within2_*: fixed-effects"):header.index("} pds_within2_out;")]
    for word in ("ACCELERATION", '"within2_accel"', "Irons-Tuck", "c_j = sum Delta2 d / sum d^2", "count SWEEPS only", "a DEFINITION"):
        assert word in doc, word
    capi = (ROOT / "polars_ds_extension_amd" / "csrc" / "capi_within2.hpp").read_text()
    assert "ACCELERATION" in capi and "c_j = sum Delta2 d / sum d^2" in capi
    assert '"within2_accel"' in lstsq.Context.set_option.__doc__
    assert lstsq.ABSORB_ACCEL == {"none": 0, "irons_tuck": 1}
    from polars_ds_extension_amd import _lib

    assert "pds_ctx_get_option" in _lib.EXPORTS and hasattr(_lib.load(), "pds_ctx_get_option")  # what `absorb_accel` restores is read, not remembered
    assert len(re.findall(r"^int\s+pds_ctx_get_option\s*\(", header, flags=re.M)) == 1
    sweep = (ROOT / "polars_ds_extension_amd" / "csrc" / "within2_sweep.hip").read_text()
    for k in ("w2_level2_accel_kernel", "w2_accel_coef_kernel", "w2_accel_apply_kernel"):
        assert k in sweep, k


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
    F, y, off, k1, k2 = ac.frame("small5", 3)
    cols = ac.columns(F)
    for fn in (ls.lin_reg_report, ls.lin_reg, ls.fixed_effects):
        for bad in ("anderson", "", "Irons_Tuck", 1):
            with pytest.raises(ValueError, match='`absorb_accel` is None, "none" or "irons_tuck"'):
                fn(*cols, target=y, absorb=[k1, k2], absorb_accel=bad)
    for fn in (ls.lin_reg_report, ls.lin_reg):
        for name in ("none", "irons_tuck"):
            with pytest.raises(ValueError, match="`absorb_accel` goes with two absorbed keys"):
                fn(*cols, target=y, absorb=k1, absorb_accel=name)
            with pytest.raises(ValueError, match="`absorb_accel` goes with two absorbed keys"):
                fn(*cols, target=y, absorb_offsets=off, absorb_accel=name)
            with pytest.raises(ValueError, match="`absorb_accel` goes with two absorbed keys"):
                fn(*cols, target=y, absorb=[k1, k2], absorb_offsets=off, absorb_accel=name)
            with pytest.raises(ValueError, match="`absorb_accel` goes with two absorbed keys"):
                fn(*cols, target=y, absorb_accel=name)
        with pytest.raises(ValueError, match="`absorb_max_iter` must be >= 1"):  # the other checks still come before the library
            fn(*cols, target=y, absorb=[k1, k2], absorb_accel="irons_tuck", absorb_max_iter=0)
