"""lstsq.fixed_effects / absorb_components (pds_lin_reg_within2_fx_*, pds_absorb_components_i32) on the MI355X against the NumPy
restatement (within2_effects_reference.py): the truth is its long double run with the tolerance at the long double rounding floor.

Frames (within2_cases.py): small5 (p 3), three components (p 2), the entry/exit panel (p 4), 3 levels among 200 singletons (p 1),
60 ragged levels x 300 codes at p 16 in f64 and in f32.  Each on the default context and on one with "within_split_rows" = 128, at
absorb_tol 1e-13 and 1e-8.

Budgets (the project's standing rule, as tests/test_within2_gpu.py words it): the device may be at most 10 x as far from the truth as
the yardstick run is on that frame (8 ulp of the frame's format where that distance is below half an ulp); distance =
max |a - b| / max |b| per output.
  absorb_tol = 1e-13: the yardstick is the float64 restatement run to its own criterion.
  absorb_tol = 1e-8:  the yardstick is that run stopped ONE SWEEP EARLIER than its own criterion.
As a condition on the INPUTS the tests assert on the CPU that the float64 reference's delta at its stopping sweep is at most half the
tolerance.  The yardstick's distances are measured on the CPU inside the tests and printed before the device is looked at.
gamma at every reference level is exactly 0.0; the components equal the restatement's labels; every entry the report has is
bit-equal to lin_reg_report(absorb=[k1, k2]) on the same context; on the f64 frames, row by row,
    |y - alpha[g] - gamma[l] - sum_j x_j beta_j - resid| <= (3 p + 16) eps (|y| + |alpha| + |gamma| + sum_j |x_j beta_j|)
(the p + 3 additions of the check itself and the p + 1-term sums inside alpha and gamma).

Measured on the MI355X (effects / effects2, worst over both split settings; the yardstick's distance from the truth beside it):
                          1e-13 device        yardstick            1e-8 device          yardstick (one sweep short)
  singletons, p 1         1.8e-15 / 9.0e-16   1.3e-15 / 4.8e-16    9.9e-11 / 9.3e-11    7.1e-10 / 6.6e-10
  ragged300, p 16         6.6e-16 / 4.6e-16   9.9e-16 / 7.3e-16    2.4e-11 / 2.6e-11    2.9e-10 / 3.1e-10
  ragged300 f32, p 16     2.7e-8 / 3.2e-8     (8 ulp = 9.5e-7)     2.7e-8 / 3.2e-8      (8 ulp = 9.5e-7)
  every case passed its own frame's budget; the device's sweep count equals the reference's; 3 graph rounds (4 on singletons); the
  identity's worst row is 0.66 - 1.65 eps of the summed magnitudes over the five f64 frames, against 3 p + 16 = 19 .. 64.  The scrambled chain (8 000 rows,
  4 001 nodes, diameter 4 000): 9 rounds on the device and in the restatement, bound 13.
"""
import ctypes as C
import functools
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT))

import within2_cases as c2  # noqa: E402
import within2_effects_reference as fxr  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = (("small5", 3, "float64"), ("blocks", 2, "float64"), ("panel", 4, "float64"), ("singletons", 1, "float64"),
         ("ragged300", 16, "float64"), ("ragged300_32", 16, "float32"))
EFFECT_KEYS = ("effects", "effect_keys", "effects2", "effect_keys2", "component", "component2", "n_graph_rounds")


@pytest.fixture(scope="module")
def pds():
    import polars_ds_extension_amd as pds

    return pds


@pytest.fixture(scope="module")
def contexts(pds):
    """the default context, and one whose split threshold cuts every level above 128 rows"""
    ctxs = {"whole": pds.default_context(), "cut": pds.Context(0)}
    ctxs["cut"].set_option("within_split_rows", 128)
    yield ctxs
    ctxs["cut"].close()


@functools.lru_cache(maxsize=None)
def _ref(kind, p, dtype_name, tol_name, sweeps=None):
    """computed once per frame, arithmetic, tolerance and sweep count, never changed"""
    F, y, off, k1, k2 = c2.frame(kind, p)
    return fxr.effects(np.asarray(F, dtype=np.float64), np.asarray(y, dtype=np.float64), k1, k2, c2.DTYPES[dtype_name], c2.TOLS[tol_name],
                       sweeps=sweeps)


def _yardstick(kind, p, tol_name):
    own = _ref(kind, p, "float64", tol_name)
    return own if tol_name == "tight" else _ref(kind, p, "float64", tol_name, own["n_iter"] - 1)


def _inputs_ok(kind, p, tol_name):
    """the condition on the inputs: the float64 reference does not stop within a factor 2 of the tolerance"""
    own = c2.ref(kind, p, "se", "float64", tol_name)
    assert own["deltas"][-1] <= 0.5 * c2.TOLS[tol_name], (kind, p, tol_name, own["deltas"][-2:])
    mine = _ref(kind, p, "float64", tol_name)  # (the same sweeps with the means kept as tables)
    assert mine["deltas"][-1] <= 0.5 * c2.TOLS[tol_name] and mine["n_iter"] == own["n_iter"], (kind, p, tol_name, mine["deltas"][-2:])


def _np(v):
    return v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)


def _fixed(pds, F, y, k1, k2, ctx=None, f32=False, tol=1e-8, **kw):
    kw.setdefault("return_pred", True)
    pds.config.LIN_REG_EXPR_F64 = not f32
    try:
        return pds.fixed_effects(*c2.columns(F), target=y, absorb=[k1, k2], absorb_tol=tol, ctx=ctx, **kw)
    finally:
        pds.config.LIN_REG_EXPR_F64 = True


def _report(pds, F, y, k1, k2, ctx=None, f32=False, tol=1e-8, **kw):
    kw.setdefault("return_pred", True)
    pds.config.LIN_REG_EXPR_F64 = not f32
    try:
        return pds.lin_reg_report(*c2.columns(F), target=y, absorb=[k1, k2], absorb_tol=tol, ctx=ctx, **kw)
    finally:
        pds.config.LIN_REG_EXPR_F64 = True


def _same_bits(a, b, keys=None):
    for k in (keys if keys is not None else b.keys()):
        x, y = a[k], b[k]
        if isinstance(x, (int, float, list)):
            assert x == y, k
        else:
            assert np.array_equal(_np(x), _np(y), equal_nan=True), k


# ---- 1. accuracy, the normalisation, the components, the report's bits, the identity
@pytest.mark.parametrize("kind,p,fmt", CASES)
def test_effects(pds, contexts, kind, p, fmt):
    assert np.finfo(np.longdouble).eps < 1e-18  # the reference has to be wider than the arithmetic under test
    f32 = fmt == "float32"
    dt = c2.DTYPES[fmt]
    F, y, off, k1, k2 = c2.frame(kind, p)
    for tol_name in ("default", "tight"):
        _inputs_ok(kind, p, tol_name)
    truth = _ref(kind, p, "longdouble", "truth")
    n_comp = truth["n_components"]
    assert int((truth["effects2"] == 0).sum()) == n_comp == len(truth["reference_levels"])
    spreads = {t: {k: fxr.rel(_yardstick(kind, p, t)[k], truth[k]) for k in ("effects", "effects2")} for t in ("default", "tight")}
    print(f"{kind} p={p} {fmt}: yardstick vs truth {spreads}")  # measured first, on the CPU
    i1, i2 = np.unique(k1, return_inverse=True)[1], np.unique(k2, return_inverse=True)[1]
    for split in ("whole", "cut"):
        for tol_name in ("default", "tight"):
            got = _fixed(pds, F, y, k1, k2, ctx=contexts[split], f32=f32, tol=c2.TOLS[tol_name])
            own = _ref(kind, p, "float64", tol_name)
            assert abs(got["n_iter"] - own["n_iter"]) <= 1, (got["n_iter"], own["n_iter"])
            assert got["effects"].dtype == dt and got["effects2"].dtype == dt
            dist = {k: fxr.rel(got[k], truth[k]) for k in ("effects", "effects2")}
            bud = {k: fxr.budget(spreads[tol_name][k], dt) for k in dist}
            print(f"{split} {kind} p={p} {fmt} tol={tol_name}: sweeps {got['n_iter']} (reference {own['n_iter']}), graph rounds "
                  f"{got['n_graph_rounds']}; device vs truth {dist}; budget {bud}")
            for k in dist:
                assert dist[k] <= bud[k], (k, dist[k], spreads[tol_name][k])
            # the normalisation: gamma is exactly 0.0 at the lowest code of key 2 of every component, and nowhere else
            assert np.all(got["effects2"][truth["reference_levels"]] == 0.0) and int((got["effects2"] == 0.0).sum()) == n_comp
            # the components: the restatement's partition and labels
            assert got["component"].dtype == np.int32 and got["component2"].dtype == np.int32
            assert np.array_equal(got["component"], truth["component"]) and np.array_equal(got["component2"], truth["component2"])
            assert np.array_equal(got["effect_keys"], np.unique(k1)) and np.array_equal(got["effect_keys2"], np.unique(k2))
            assert got["n_components"] == n_comp and 1 <= got["n_graph_rounds"] <= fxr.round_cap(len(truth["effects"]) + len(truth["effects2"]))
            assert got["n_graph_rounds"] == truth["n_graph_rounds"]  # (every round's labels are minima: they do not depend on the scheduling)
            # every entry of the report, bit for bit
            rep = _report(pds, F, y, k1, k2, ctx=contexts[split], f32=f32, tol=c2.TOLS[tol_name])
            assert [k for k in got if k not in EFFECT_KEYS] == list(rep)
            _same_bits(got, rep)
            if f32:
                continue
            # the identity, row by row
            ys, a, g = np.asarray(y, dtype=np.float64), got["effects"][i1], got["effects2"][i2]
            xb = np.asarray(F, dtype=np.float64) * got["beta"][None, :]
            gap = ((ys - a) - g)
            for j in range(p):
                gap = gap - xb[:, j]
            gap = gap - got["resid"]
            scale = np.abs(ys) + np.abs(a) + np.abs(g) + np.abs(xb).sum(axis=1)
            worst = float(np.max(np.abs(gap) / scale)) / np.finfo(np.float64).eps
            print(f"    identity: worst |gap| / (eps scale) = {worst:.2f} of {3 * p + 16}")
            assert np.all(np.abs(gap) <= (3 * p + 16) * np.finfo(np.float64).eps * scale), worst


# ---- 2. the forms: the C ABI's offsets form, shuffled rows, sparse negative keys, CUDA tensors, empty groups, unused codes
def _grouped_fx_raw(ctx, F, y, off, codes2, n_levels2, se="se", tol=1e-8):
    from polars_ds_extension_amd import _lib
    from polars_ds_extension_amd.lstsq import _Cols

    cols = c2.columns(F)
    n, p, ng = len(y), len(cols), len(off) - 1
    cs = _Cols(np.ascontiguousarray(y), cols)
    outs = {k: np.empty(p) for k in ("beta", "std_err", "t", "p", "ci_lower", "ci_upper")}
    rep = _lib.ReportF64(*[C.c_void_p(o.ctypes.data) for o in outs.values()], 0.0, 0.0)
    pred, resid = np.empty(n), np.empty(n)
    extra = _lib.Within2Out(C.c_void_p(pred.ctypes.data), C.c_void_p(resid.ctypes.data), 0.0, 0, 0, 0, 0, 0)
    eff1, eff2 = np.full(ng, 7.0), np.full(n_levels2, 7.0)
    comp1, comp2 = np.full(ng, 7, dtype=np.int32), np.full(n_levels2, 7, dtype=np.int32)
    fx = _lib.Within2Effects(*[C.c_void_p(a.ctypes.data) for a in (eff1, eff2, comp1, comp2)], None, 0, 0)
    off = np.ascontiguousarray(off, dtype=np.int64)
    codes2 = np.ascontiguousarray(codes2, dtype=np.int32)
    rc = ctx._lib.pds_lin_reg_within2_fx_grouped_f64(ctx._h, cs.cols, p, C.c_int64(n), C.c_void_p(off.ctypes.data), C.c_int64(ng),
                                                     C.c_void_p(codes2.ctypes.data), C.c_int64(n_levels2), cs.space, _lib.WITHIN_SE_TYPES[se],
                                                     C.c_double(tol), 10_000, C.byref(rep), C.byref(extra), C.byref(fx))
    out = dict(outs, pred=pred, resid=resid, r2=rep.r2, adj_r2=rep.adj_r2, r2_overall=extra.r2_overall, df_resid=extra.df_resid,
               n_groups=extra.n_groups_used, n_groups2=extra.n_groups2_used, n_components=extra.n_components, n_iter=extra.n_iter,
               effects=eff1, effects2=eff2, component=comp1, component2=comp2, n_graph_rounds=fx.n_graph_rounds)
    return rc, out


def _assert_raw_equals(raw, got, row_map=None):
    for a, b in (("beta", "beta"), ("std_err", "std_err"), ("t", "t"), ("p", "p>|t|"), ("ci_lower", "0.025"), ("ci_upper", "0.975")):
        assert np.array_equal(raw[a], got[b]), a
    assert raw["r2"] == got["r2"][0] and raw["adj_r2"] == got["adj_r2"][0]
    for k in ("r2_overall", "df_resid", "n_groups", "n_groups2", "n_components", "n_iter", "n_graph_rounds"):
        assert raw[k] == got[k], k
    for k in ("effects", "effects2", "component", "component2"):
        assert np.array_equal(raw[k], _np(got[k])), k
    for k in ("pred", "resid"):
        assert np.array_equal(raw[k] if row_map is None else raw[k][row_map], _np(got[k])), k


def test_forms_agree(pds, contexts):
    import torch

    p = 4
    F, y, off, k1, k2 = c2.frame("ragged300", p)
    F, y = np.asarray(F), np.asarray(y)
    keys1, keys2 = k1 * 7 - 200, k2 * 3 - 50  # negative, sparse
    n, n2 = len(y), len(np.unique(k2))
    codes2 = np.unique(keys2, return_inverse=True)[1]
    perm = np.random.default_rng(5).permutation(n)
    by1 = np.argsort(keys1[perm], kind="stable")
    order = perm[by1]
    inv = np.empty(n, dtype=np.int64)
    inv[by1] = np.arange(n)  # row i of the shuffled frame is row inv[i] of the ordered one
    dev = torch.device("cuda", 0)
    for split in ("whole", "cut"):
        ctx = contexts[split]
        ordered = pds.fixed_effects(*c2.columns(F), target=y, absorb=[keys1, keys2], return_pred=True, ctx=ctx)
        _same_bits(pds.fixed_effects(*c2.columns(F), target=y, absorb=[keys1, keys2], return_pred=True, ctx=ctx), ordered)  # two calls
        assert np.array_equal(ordered["effect_keys"], np.unique(keys1)) and np.array_equal(ordered["effect_keys2"], np.unique(keys2))
        rc, raw = _grouped_fx_raw(ctx, F, y, off, codes2, n2)  # ordered keys move nothing: the bits of the offsets form
        assert rc == 0
        _assert_raw_equals(raw, ordered)
        # rows shuffled: the stable sort + gather brings them into the order of key 1; the effects are those of that ordered frame
        shuffled = pds.fixed_effects(*c2.columns(F[perm]), target=y[perm], absorb=[keys1[perm], keys2[perm]], return_pred=True, ctx=ctx)
        rc, on_ordered = _grouped_fx_raw(ctx, F[order], y[order], off, codes2[order], n2)
        assert rc == 0
        _assert_raw_equals(on_ordered, shuffled, row_map=inv)
        # CUDA tensors give the bits of the host frame, in device memory
        tc = [torch.from_numpy(np.array(c)).to(dev) for c in c2.columns(F[perm])]
        t_key = pds.fixed_effects(*tc, target=torch.from_numpy(y[perm]).to(dev), return_pred=True, ctx=ctx,
                                  absorb=[torch.from_numpy(keys1[perm]).to(dev), torch.from_numpy(keys2[perm]).to(dev)])
        for k in ("effects", "effects2", "component", "component2", "effect_keys", "effect_keys2", "pred", "resid"):
            assert t_key[k].is_cuda, k
        assert list(t_key) == list(shuffled)
        _same_bits(t_key, shuffled)
        # a max_groups hint that is too small is refused with the count, a sufficient one changes nothing
        with pytest.raises(pds._lib.PdsError, match="more distinct keys than max_groups"):
            pds.fixed_effects(*c2.columns(F), target=y, absorb=[keys1, keys2], max_groups=59, ctx=ctx)
        _same_bits(pds.fixed_effects(*c2.columns(F), target=y, absorb=[keys1, keys2], return_pred=True, max_groups=60, ctx=ctx), ordered)
        # empty groups of the offsets form: NaN / -1 there, the others' numbers unchanged, the components named by the caller's indices
        at = np.array([0, 0, 17, 60, 60])
        off_e = np.insert(off, at, off[at])
        kept = np.flatnonzero(np.diff(off_e) > 0)
        assert len(off_e) == len(off) + 5 and len(kept) == 60
        rc, holes = _grouped_fx_raw(ctx, F, y, off_e, codes2, n2)
        assert rc == 0 and holes["n_groups"] == 60
        empty = np.setdiff1d(np.arange(len(off_e) - 1), kept)
        assert np.all(np.isnan(holes["effects"][empty])) and np.all(holes["component"][empty] == -1)
        assert np.array_equal(holes["effects"][kept], raw["effects"]) and np.array_equal(holes["effects2"], raw["effects2"])
        assert np.array_equal(holes["component"][kept], kept[raw["component"]]) and np.array_equal(holes["component2"], kept[raw["component2"]])
        for k in ("beta", "std_err", "pred", "resid"):
            assert np.array_equal(holes[k], raw[k]), k
        # unused codes of key 2 count nowhere: NaN / -1 there, the same numbers elsewhere
        rc, spare = _grouped_fx_raw(ctx, F, y, off, codes2 * 2 + 1, 2 * n2 + 3)
        assert rc == 0 and spare["n_groups2"] == n2
        used = 2 * np.arange(n2) + 1
        unused = np.setdiff1d(np.arange(2 * n2 + 3), used)
        assert np.all(np.isnan(spare["effects2"][unused])) and np.all(spare["component2"][unused] == -1)
        assert np.array_equal(spare["effects2"][used], raw["effects2"]) and np.array_equal(spare["component2"][used], raw["component2"])
        for k in ("effects", "component", "beta", "std_err", "pred", "resid", "n_components", "n_iter"):
            assert np.array_equal(spare[k], raw[k]), k


def test_three_components_offsets_form(pds, contexts):
    """the components of the blocks frame through the C entry, with an empty group in front of every block"""
    F, y, off, k1, k2 = c2.frame("blocks", 2)
    truth = _ref("blocks", 2, "longdouble", "truth")
    rc, raw = _grouped_fx_raw(contexts["whole"], np.asarray(F), np.asarray(y), off, k2, int(k2.max()) + 1)
    assert rc == 0 and raw["n_components"] == 3
    assert np.array_equal(raw["component"], truth["component"]) and np.array_equal(raw["component2"], truth["component2"])
    assert sorted(np.unique(raw["component"])) == [0, 8, 16] and int((raw["effects2"] == 0.0).sum()) == 3
    at = np.array([0, 8, 16])
    rc, holes = _grouped_fx_raw(contexts["whole"], np.asarray(F), np.asarray(y), np.insert(off, at, off[at]), k2, int(k2.max()) + 1)
    assert rc == 0 and sorted(np.unique(holes["component"])) == [-1, 1, 10, 19]


# ---- 3. the graph pass alone
def test_absorb_components_scrambled_chain(pds):
    import torch

    k1, k2 = fxr.scrambled_chain()
    assert len(k1) == 8000
    keys1, keys2, lab1, lab2, n_comp, rounds = fxr.components(k1, k2)
    got = pds.absorb_components(k1, k2)
    print("scrambled chain: device rounds", got["n_rounds"], "restatement", rounds, "bound 13")
    assert (got["n_groups"], got["n_groups2"], got["n_components"]) == (2000, 2001, 1) and n_comp == 1
    assert got["n_rounds"] <= 13 and got["n_rounds"] == rounds
    assert np.array_equal(got["keys1"], keys1) and np.array_equal(got["keys2"], keys2)
    assert got["component1"].dtype == np.int32 and np.array_equal(got["component1"], lab1) and np.array_equal(got["component2"], lab2)
    dev = torch.device("cuda", 0)
    on_dev = pds.absorb_components(torch.from_numpy(k1).to(dev), torch.from_numpy(k2).to(dev))
    assert on_dev["component1"].is_cuda and on_dev["keys2"].is_cuda
    _same_bits(on_dev, got)
    again = pds.absorb_components(k1, k2)
    _same_bits(again, got)


def test_absorb_components_disjoint_blocks(pds):
    import torch

    k1, k2 = fxr.disjoint_blocks()
    keys1, keys2, lab1, lab2, n_comp, rounds = fxr.components(k1, k2)
    got = pds.absorb_components(k1 * 3 - 1000, 5 * k2 + 2)  # sparse, negative keys
    assert got["n_components"] == n_comp == 500 and (got["n_groups"], got["n_groups2"]) == (1500, 1500)
    assert np.array_equal(got["component1"], lab1) and np.array_equal(got["component2"], lab2) and got["n_rounds"] == rounds
    dev = torch.device("cuda", 0)
    _same_bits(pds.absorb_components(torch.from_numpy(k1 * 3 - 1000).to(dev), torch.from_numpy(5 * k2 + 2).to(dev)), got)


def test_absorb_components_c_abi(pds):
    """unused codes of either key are -1 and count nowhere; a code outside its range is refused before it is used"""
    ctx = pds.default_context()
    k1, k2 = fxr.disjoint_blocks(40)
    keys1, keys2, lab1, lab2, n_comp, rounds = fxr.components(k1, k2)

    def raw(c1, nl1, c2_, nl2):
        c1, c2_ = np.ascontiguousarray(c1, dtype=np.int32), np.ascontiguousarray(c2_, dtype=np.int32)
        comp1, comp2 = np.full(nl1, 7, dtype=np.int32), np.full(nl2, 7, dtype=np.int32)
        n1, n2, nc, nr = C.c_int64(-1), C.c_int64(-1), C.c_int64(-1), C.c_int(-1)
        rc = ctx._lib.pds_absorb_components_i32(ctx._h, C.c_void_p(c1.ctypes.data), C.c_int64(nl1), C.c_void_p(c2_.ctypes.data), C.c_int64(nl2),
                                                C.c_int64(len(c1)), 0, C.c_void_p(comp1.ctypes.data), C.c_void_p(comp2.ctypes.data), C.byref(n1),
                                                C.byref(n2), C.byref(nc), C.byref(nr))
        return rc, comp1, comp2, (n1.value, n2.value, nc.value)

    rc, comp1, comp2, counts = raw(k1, 120, k2, 120)
    assert rc == 0 and counts == (120, 120, 40) and np.array_equal(comp1, lab1) and np.array_equal(comp2, lab2)
    rc, comp1, comp2, counts = raw(2 * k1 + 1, 243, 3 * k2, 360)  # codes 2 c + 1 of key 1, 3 c of key 2
    assert rc == 0 and counts == (120, 120, 40)
    assert np.array_equal(comp1[1:241:2], 2 * lab1 + 1) and np.all(comp1[0::2] == -1)
    assert np.array_equal(comp2[0::3], 2 * lab2 + 1) and np.all(comp2[1::3] == -1) and np.all(comp2[2::3] == -1)
    for c1, nl1, c2_, nl2 in ((k1, 119, k2, 120), (k1, 120, k2, 119), (-k1 - 1, 120, k2, 120), (k1, 120, -k2 - 1, 120)):
        assert raw(c1, nl1, c2_, nl2)[0] == -1  # PDS_ERR_INVALID
    assert raw(k1, 120, k2, 120)[0] == 0  # the context is usable afterwards
    # graphs whose trees do not halve in one round (a root that neither hooks nor is hooked into): labelled, inside the cap of
    # 2 ceil(log2 nodes) + 1 rounds, in the restatement's number of rounds
    for (a, b), want_rounds in ((fxr.stagnant_tree(), 6), (fxr.star(9), 4)):
        keys1, keys2, lab1, lab2, n_comp, rounds = fxr.components(a, b)
        n1, n2 = len(keys1), len(keys2)
        c1, c2_ = np.ascontiguousarray(a, dtype=np.int32), np.ascontiguousarray(b, dtype=np.int32)
        comp1, comp2 = np.full(n1, 7, dtype=np.int32), np.full(n2, 7, dtype=np.int32)
        nc, nr = C.c_int64(-1), C.c_int(-1)
        rc = ctx._lib.pds_absorb_components_i32(ctx._h, C.c_void_p(c1.ctypes.data), C.c_int64(n1), C.c_void_p(c2_.ctypes.data), C.c_int64(n2),
                                                C.c_int64(len(c1)), 0, C.c_void_p(comp1.ctypes.data), C.c_void_p(comp2.ctypes.data), None, None,
                                                C.byref(nc), C.byref(nr))
        assert rc == 0 and nc.value == n_comp == 1 and nr.value == rounds == want_rounds <= fxr.round_cap(n1 + n2)
        assert np.array_equal(comp1, lab1) and np.array_equal(comp2, lab2)
    # ... and the regression on those cells (every row three times, so that n - p - A > 0) is fitted, not refused
    a, b = (np.tile(k, 3) for k in fxr.stagnant_tree())
    rng = np.random.default_rng(8)
    x = rng.normal(size=len(a))
    y = 0.5 * x + rng.normal(size=8)[a] + rng.normal(size=7)[b] + 0.1 * rng.normal(size=len(a))
    got = pds.fixed_effects(x, target=y, absorb=[a, b])
    assert (got["n_groups"], got["n_groups2"], got["n_components"], got["n_graph_rounds"]) == (8, 7, 1, 6) and got["df_resid"] == 42 - 1 - 14
    assert pds.lin_reg_report(x, target=y, absorb=[a, b])["n_components"] == 1
