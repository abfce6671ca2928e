"""Grouped rolling / expanding regressions: the C ABI surface, the mock trampolines of the new entry points (bound here to
callbacks that loop the oracle over the groups) and the lstsq validation -- no GPU needed."""
import ctypes as C
import re
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
NEW = [f"pds_{k}_lr_{f}_{s}" for k in ("rolling", "recursive") for f in ("grouped", "by_key") for s in ("f64", "f32")]


def test_exported_and_declared():
    from polars_ds_extension_amd import _lib

    assert all(n in _lib.EXPORTS for n in NEW)
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "pds_lstsq.h").read_text(), flags=re.S)
    for n in NEW:
        assert len(re.findall(rf"^int\s+{n}\s*\(", text, flags=re.M)) == 1, n


def _mock_build():
    sys.path.insert(0, str(ROOT / "tests" / "mock_device"))
    try:
        import build as mock_build
    finally:
        sys.path.pop(0)
    return mock_build


def test_mock_trampolines_parse():
    protos = {name: [a for _, a in args] for _, name, args in _mock_build().prototypes()}
    assert protos["pds_rolling_lr_grouped_f64"] == ["ctx", "cols", "n_feat", "n_rows", "group_offsets", "n_groups", "space", "add_bias",
                                                    "window", "min_size", "lambda", "coeffs", "pred", "valid"]
    assert protos["pds_recursive_lr_by_key_f32"] == ["ctx", "cols", "keys", "n_feat", "n_rows", "space", "add_bias", "start_with",
                                                     "lambda", "coeffs", "pred", "valid"]


def _oracle_groups(orc, kind, X, y, off, w, lam, pp):
    """What a per-group call gives: the oracle's chain on every group long enough, frame order."""
    n = len(y)
    co = np.full((n, pp), np.nan)
    va = np.zeros(n, np.uint8)
    for g in range(len(off) - 1):
        s, e = int(off[g]), int(off[g + 1])
        if e - s < w:
            continue
        ref = orc.rolling_lr(X[s:e], y[s:e], w, lam) if kind == "rolling" else orc.recursive_lr(X[s:e], y[s:e], w, lam)
        co[s + w - 1 : e] = ref
        va[s + w - 1 : e] = 1
    pred = np.einsum("ij,ij->i", X, co)
    return co, pred, va


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle

    oracle.build()
    return oracle


@pytest.fixture(scope="module")
def mock(orc):
    mb = _mock_build()
    lib = C.CDLL(str(mb.build()))
    keep = []

    def view(ptr, n, dt):
        return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(np.ctypeslib.as_ctypes_type(dt))), shape=(n,))

    def frame(cols_p, n_feat, n, dt):
        ptrs = C.cast(cols_p, C.POINTER(C.c_void_p))
        cols = [view(ptrs[c], n, dt).astype(np.float64) for c in range(n_feat + 1)]
        return np.stack(cols[1:], axis=1), cols[0]

    def make(kind, form, dt):
        def fn(ctx, cols_p, *a):
            if form == "grouped":
                n_feat, n, off_p, ng, space, bias, *rest = a
                off = view(off_p, ng + 1, np.int64).copy()
                X, y = frame(cols_p, n_feat, n, dt)
            else:
                keys_p, n_feat, n, space, bias, *rest = a
                keys = view(keys_p, n, np.int64)
                X, y = frame(cols_p, n_feat, n, dt)
                order = np.argsort(keys, kind="stable")
                _, counts = np.unique(keys[order], return_counts=True)
                off = np.concatenate([[0], np.cumsum(counts)])
            w, lam = (rest[0], rest[2]) if kind == "rolling" else (rest[0], rest[1])
            co_p, pr_p, va_p = rest[-3:]
            Xb = np.c_[X, np.ones(n)] if bias else X
            pp = Xb.shape[1]
            if form == "grouped":
                co, pr, va = _oracle_groups(orc, kind, Xb, y, off, w, lam, pp)
            else:
                co_s, pr_s, va_s = _oracle_groups(orc, kind, Xb[order], y[order], off, w, lam, pp)
                co, pr, va = np.empty_like(co_s), np.empty_like(pr_s), np.empty_like(va_s)
                co[order], pr[order], va[order] = co_s, pr_s, va_s
            view(co_p, n * pp, dt)[:] = co.ravel()
            view(pr_p, n, dt)[:] = pr
            view(va_p, n, np.uint8)[:] = va
            return 0

        real = C.c_double if dt == np.float64 else C.c_float
        if form == "grouped":
            lead = [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_int]
        else:
            lead = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_int]
        win = [C.c_int64, C.c_int64, real] if kind == "rolling" else [C.c_int64, real]
        proto = C.CFUNCTYPE(C.c_int, *lead, *win, C.c_void_p, C.c_void_p, C.c_void_p)
        cb = proto(fn)
        keep.append(cb)
        return cb

    for kind in ("rolling", "recursive"):
        for form in ("grouped", "by_key"):
            for sfx, dt in (("f64", np.float64), ("f32", np.float32)):
                getattr(lib, f"mock_bind_pds_{kind}_lr_{form}_{sfx}")(C.cast(make(kind, form, dt), C.c_void_p))
    lib._keep = keep
    return lib


@pytest.mark.parametrize("kind", ["rolling", "recursive"])
def test_trampolines_reach_the_bound_callbacks(mock, orc, kind):
    """The header's argument order (through the generated trampolines) against a per-group oracle loop: the grouped and the
    by-key forms agree, and shuffling the keys moves the rows with them."""
    rng = np.random.default_rng(1)
    sizes = [30, 0, 5, 80, 41]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n, p, w = int(off[-1]), 2, 10
    X = rng.random((n, p))
    y = X @ [0.5, -1.0] + 0.2 + 0.01 * rng.normal(size=n)
    cols = [np.ascontiguousarray(c) for c in (y, X[:, 0], X[:, 1])]
    ptrs = (C.c_void_p * 3)(*[c.ctypes.data for c in cols])

    def run(fn, *lead):
        co, pr, va = np.empty((n, 3)), np.empty(n), np.empty(n, np.uint8)
        win = (C.c_int64(w), C.c_int64(0), C.c_double(0.0)) if kind == "rolling" else (C.c_int64(w), C.c_double(0.0))
        rc = fn(None, ptrs, *lead, 1, *win, C.c_void_p(co.ctypes.data), C.c_void_p(pr.ctypes.data), C.c_void_p(va.ctypes.data))
        assert rc == 0
        return co, pr, va

    g = run(getattr(mock, f"pds_{kind}_lr_grouped_f64"), 2, C.c_int64(n), C.c_void_p(off.ctypes.data), C.c_int64(len(sizes)), 0)
    keys = np.repeat(np.arange(len(sizes), dtype=np.int64) * 5 - 7, sizes)
    k = run(getattr(mock, f"pds_{kind}_lr_by_key_f64"), C.c_void_p(keys.ctypes.data), 2, C.c_int64(n), 0)
    np.testing.assert_array_equal(g[2], k[2])
    np.testing.assert_allclose(g[0][g[2] == 1], k[0][k[2] == 1])
    expect = np.zeros(n, np.uint8)
    for s, e in zip(off[:-1], off[1:]):
        expect[s + w - 1 : e] = 1
    np.testing.assert_array_equal(g[2], expect)


def test_python_surface_and_validation():
    import polars_ds_extension_amd as pds

    x = [np.zeros(10), np.zeros(10)]
    y = np.zeros(10)
    off = np.array([0, 10], np.int64)
    for fn in (pds.rolling_lin_reg_by, pds.rolling_lin_reg_by_key, pds.recursive_lin_reg_by, pds.recursive_lin_reg_by_key):
        assert callable(fn) and fn.__name__ in pds.lstsq.__all__
    with pytest.raises(ValueError, match="window_size"):
        pds.rolling_lin_reg_by(*x, target=y, group_offsets=off, window_size=1)
    with pytest.raises(ValueError, match="features > window"):
        pds.rolling_lin_reg_by_key(*x, target=y, key=np.zeros(10, np.int64), window_size=2, add_bias=True)
    with pytest.raises(ValueError, match="min_valid_rows"):
        pds.rolling_lin_reg_by(*x, target=y, group_offsets=off, window_size=5, skip_non_finite=True, min_valid_rows=1)
    with pytest.raises(ValueError, match="initial fit"):
        pds.recursive_lin_reg_by(*x, target=y, group_offsets=off, start_with=1)
    with pytest.raises(ValueError, match="initial fit"):
        pds.recursive_lin_reg_by_key(*x, target=y, key=np.zeros(10, np.int64), start_with=2, add_bias=True)


def test_expressions_by_and_over_through_the_mock_plugin(mock, orc):
    """rolling_lin_reg(by=) / recursive_lin_reg(by=) and the _over helpers through tests/mini_polars and plugin.cpp (the mock
    device answers pds_*_lr_by_key_* with the oracle per group): row for row in frame order, string keys included."""
    sys.path.insert(0, str(ROOT / "tests" / "mini_polars"))
    sys.path.insert(0, str(ROOT / "tests"))
    import test_polars_exprs as tpe  # (the engine this suite runs the builders on: real polars if present, else mini_polars)
    from polars_ds_extension_amd import polars_exprs as px

    pl = tpe.pl
    px.PLUGIN_PATH = Path(mock._name)
    rng = np.random.default_rng(3)
    D, w = 60, 8
    names = ["pine", "oak", "birch", "elm"]
    s_key = [names[i % 4] for i in range(4 * D)]
    i_key = [[7, -3, 12, 0][i % 4] for i in range(4 * D)]
    n = len(s_key)
    X = rng.random((n, 2))
    y = X @ [0.4, -0.6] + 0.2 + 0.01 * rng.normal(size=n)
    df = pl.DataFrame({"s": s_key, "k": i_key, "y": y, "x1": X[:, 0], "x2": X[:, 1]})

    def expect(kind):
        co = [None] * n
        for name in names:
            rows = np.flatnonzero(np.array(s_key) == name)
            ref = orc.rolling_lr(X[rows], y[rows], w) if kind == "rolling" else orc.recursive_lr(X[rows], y[rows], w)
            for j, r in enumerate(rows[w - 1 :]):
                co[r] = ref[j]
        return co

    for kind, fn, over in (("rolling", px.rolling_lin_reg, px.rolling_lin_reg_over),
                           ("recursive", px.recursive_lin_reg, px.recursive_lin_reg_over)):
        kw = {"window_size": w} if kind == "rolling" else {"start_with": w}
        want = expect(kind)
        col = f"{kind}_lin_reg"
        for res in (df.with_columns(fn("x1", "x2", target="y", by="k", **kw)), over(df, "s", "x1", "x2", target="y", **kw),
                    over(df, ["s", "k"], "x1", "x2", target="y", **kw)):
            assert res["s"].to_list() == s_key and res["k"].to_list() == i_key  # the frame's own row order
            got = res.unnest(col)["coeffs"].to_list()
            for r in range(n):
                assert (got[r] is None) == (want[r] is None), (kind, r)
                if want[r] is not None:
                    np.testing.assert_allclose(got[r], want[r], rtol=1e-9, atol=1e-11)
