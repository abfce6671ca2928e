"""Grouped rolling / expanding regressions (pds_rolling_lr_grouped_* / pds_recursive_lr_grouped_* / *_by_key_*) on the device:
per-group validity, values against direct per-window solves and the oracle's per-group chain, group independence, key forms,
f32 frames, both input spaces and the argument errors."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F64_TOL = 1e-10
F32_TOL = 1e-4
LONG = 2 * 16384 + 3000  # crosses rolling (16 384) and expanding (4 096) tile anchors


@pytest.fixture(scope="module")
def pds():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import polars_ds_extension_amd as m

    return m


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle

    oracle.build()
    return oracle


def dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def nrel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def bits(a):
    a = np.ascontiguousarray(host(a))
    return a.view(np.uint64 if a.dtype == np.float64 else (np.uint32 if a.dtype == np.float32 else np.uint8))


def offsets_of(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def frame(rng, sizes, p, scale=None):
    off = offsets_of(sizes)
    n = int(off[-1])
    X = rng.random((n, p)) + 0.1 * rng.normal(size=(n, p))
    y = X @ rng.normal(size=p) + 0.3 + 0.05 * rng.normal(size=n)
    return X, y, off


def sizes_for(rng, wmin):
    s = [0, 1, 3, max(wmin - 1, 1), wmin, wmin + 1, 0] + list(rng.integers(1, 3 * wmin + 50, size=14)) + [LONG, 7]
    return [int(v) for v in s]


def call(pds, kind, X, y, off, w, bias, lam, min_size=None, on_dev=True):
    cols = [dev(X[:, j]) for j in range(X.shape[1])] if on_dev else [np.ascontiguousarray(X[:, j]) for j in range(X.shape[1])]
    t = dev(y) if on_dev else y
    o = dev(off) if on_dev else off
    if kind == "rolling":
        kw = dict(skip_non_finite=min_size is not None, min_valid_rows=min_size)
        co, pr, va = pds.rolling_lin_reg_by(*cols, target=t, group_offsets=o, window_size=w, add_bias=bias, l2_reg=lam, **kw)
    else:
        co, pr, va = pds.recursive_lin_reg_by(*cols, target=t, group_offsets=o, start_with=w, add_bias=bias, l2_reg=lam)
    return host(co), host(pr), host(va)


def spills(pds):
    from polars_ds_extension_amd import _lib

    return int(_lib.load().pds_ctx_workspace_spills(pds.default_context()._h))


def rule_valid(off, w):
    n = int(off[-1])
    v = np.zeros(n, np.uint8)
    for g in range(len(off) - 1):
        s, e = int(off[g]), int(off[g + 1])
        v[s + w - 1 : e] = 1
    return v


def direct(Xb, y, lo, r, lam):
    A, b = Xb[lo : r + 1], y[lo : r + 1]
    fin = np.isfinite(A).all(axis=1) & np.isfinite(b)
    A, b = A[fin], b[fin]
    G = A.T @ A + lam * np.eye(A.shape[1])
    return np.linalg.solve(G, A.T @ b), np.linalg.cond(G)


def sample_rows(rng, off, w):
    rows = []
    for g in range(len(off) - 1):
        s, e = int(off[g]), int(off[g + 1])
        if e - s >= w:
            rows += [s + w - 1, e - 1] + [int(v) for v in rng.integers(s + w - 1, e, size=2)]
            if e - s > 20000:  # around the tile anchors
                rows += [t + d for t in range(s - s % 4096 + 4096, e, 4096) for d in (-1, 0, 1) if s + w - 1 <= t + d < e][:40]
    return sorted(set(rows))


def check_values(kind, co, pr, X, y, off, w, bias, lam, rng, tol=F64_TOL, ref=None):
    Xb = np.c_[X, np.ones(len(y))] if bias else X
    gs = np.searchsorted(off, np.arange(len(y)), side="right") - 1
    for r in sample_rows(rng, off, w):
        s = int(off[gs[r]])
        lo = max(s, r - w + 1) if kind == "rolling" else s
        b, cond = direct(Xb, y, lo, r, lam)
        cbound = max(tol, 1e-15 * cond) if tol == F64_TOL else tol * max(1.0, cond * 1e-8)
        assert nrel(co[r], b) < cbound, (r, nrel(co[r], b), cond)
        if np.isfinite(Xb[r]).all():
            assert abs(pr[r] - Xb[r] @ b) < (1e-9 if tol == F64_TOL else 1e-3) * max(1.0, cond * 1e-6) * max(1.0, abs(Xb[r] @ b)), r


PPS = [1, 2, 3, 4, 6, 8, 9, 12, 13, 24, 64]


@pytest.mark.parametrize("pp", PPS)
def test_rolling_offsets(pds, orc, pp):
    rng = np.random.default_rng(100 + pp)
    wins = [w for w in (5, 64, 256, 300) if w >= 2 * pp]
    # (w = 256 up to 8 coefficients: where a grouped call takes the two-stream form and the ungrouped one does not)
    for i, w in enumerate([wins[0]] + ([256] if pp <= 8 else []) + [wins[-1]]):
        bias = bool((pp + i) % 2) and pp > 1
        lam = 0.1 if i == 2 or (i == 1 and pp > 8) else 0.0
        p = pp - int(bias)
        X, y, off = frame(rng, sizes_for(rng, w), p)
        co, pr, va = call(pds, "rolling", X, y, off, w, bias, lam)
        assert spills(pds) == 0  # the workspace bound of the grouped call holds
        assert co.shape == (len(y), pp)
        np.testing.assert_array_equal(va, rule_valid(off, w))
        check_values("rolling", co, pr, X, y, off, w, bias, lam, rng)
        if pp <= 8 and w >= 64:  # the reference's Woodbury chain per group, where it stays sane
            Xb = np.c_[X, np.ones(len(y))] if bias else X
            for g in range(len(off) - 1):
                s, e = int(off[g]), int(off[g + 1])
                if e - s >= w:
                    ref = orc.rolling_lr(Xb[s:e], y[s:e], w, lam)
                    err = np.linalg.norm(co[s + w - 1 : e] - ref, axis=1) / np.linalg.norm(ref, axis=1)
                    assert np.max(err[:200]) < 1e-8, (g, np.max(err))


@pytest.mark.parametrize("pp", PPS)
def test_expanding_offsets(pds, orc, pp):
    rng = np.random.default_rng(200 + pp)
    for i, n0 in enumerate((pp, max(pp, 50))):
        bias = bool((pp + i) % 2) and pp > 1
        lam = 0.1 if i else 0.0
        p = pp - int(bias)
        X, y, off = frame(rng, sizes_for(rng, max(n0, 8)), p)
        co, pr, va = call(pds, "recursive", X, y, off, n0, bias, lam)
        assert spills(pds) == 0
        np.testing.assert_array_equal(va, rule_valid(off, n0))
        check_values("recursive", co, pr, X, y, off, n0, bias, lam, rng)
        if pp <= 8 and n0 >= 50:
            Xb = np.c_[X, np.ones(len(y))] if bias else X
            for g in range(len(off) - 1):
                s, e = int(off[g]), int(off[g + 1])
                if e - s >= n0 and e - s < 5000:
                    ref = orc.recursive_lr(Xb[s:e], y[s:e], n0, lam)
                    err = np.linalg.norm(co[s + n0 - 1 : e] - ref, axis=1) / np.linalg.norm(ref, axis=1)
                    assert np.max(err) < 1e-8, (g, np.max(err))


@pytest.mark.parametrize("pp", [3, 8, 13])
def test_skipping_variant(pds, orc, pp):
    rng = np.random.default_rng(300 + pp)
    w, bias = 64, pp != 3
    p = pp - int(bias)
    X, y, off = frame(rng, sizes_for(rng, w), p)
    bad = rng.choice(len(y), size=len(y) // 20, replace=False)
    X[bad[: len(bad) // 2], 0] = np.nan
    y[bad[len(bad) // 2 :]] = np.inf
    min_size = pp + 10
    co, pr, va = call(pds, "rolling", X, y, off, w, bias, 0.0, min_size=min_size)
    Xb = np.c_[X, np.ones(len(y))] if bias else X
    for g in range(len(off) - 1):
        s, e = int(off[g]), int(off[g + 1])
        assert not va[s : min(e, s + w - 1)].any()
        if e - s >= w:
            ref, rv = orc.rolling_skipping_lr(Xb[s:e], y[s:e], w, min_size, 0.0)
            np.testing.assert_array_equal(va[s + w - 1 : e].astype(bool), rv, err_msg=f"group {g}")
    gs =np.searchsorted(off, np.arange(len(y)), side="right") - 1
    for r in [r for r in sample_rows(rng, off, w) if va[r]]:
        s = int(off[gs[r]])
        b, cond = direct(Xb, y, max(s, r - w + 1), r, 0.0)
        assert nrel(co[r], b) < max(F64_TOL, 1e-15 * cond), r


@pytest.mark.parametrize("kind,pp", [("rolling", 8), ("recursive", 8), ("rolling", 4), ("rolling", 13), ("recursive", 13)])
def test_group_independence(pds, kind, pp):
    rng = np.random.default_rng(400 + pp)
    w = 256 if kind == "rolling" else 50
    bias = True
    X, y, off = frame(rng, [300, 5000, 700, LONG, 2000, 4096, 999], pp - 1)
    a = call(pds, kind, X, y, off, w, bias, 0.0)
    again = call(pds, kind, X, y, off, w, bias, 0.0)
    for u, v in zip(a, again):
        np.testing.assert_array_equal(bits(u), bits(v))
    for g in (1, 3):
        s, e = int(off[g]), int(off[g + 1])
        X2, y2 = X.copy(), y.copy()
        X2[s:e] *= 1e6
        y2[s:e] *= 1e6
        X2[s + 10, 0] = np.nan
        y2[s + 400] = np.inf
        X2[s + 900, -1] = 1e150
        b = call(pds, kind, X2, y2, off, w, bias, 0.0)
        keep = np.ones(len(y), bool)
        keep[s:e] = False
        for u, v in zip(a, b):
            np.testing.assert_array_equal(bits(u)[keep], bits(v)[keep], err_msg=f"group {g} leaked")


def test_key_forms(pds):
    rng = np.random.default_rng(5)
    pp, w = 8, 64
    # ordered keys (negative, sparse) == the offsets form, bit for bit
    sizes = [int(v) for v in rng.integers(1, 400, size=60)] + [LONG]
    X, y, off = frame(rng, sizes, pp)
    keys = np.repeat(np.arange(len(sizes), dtype=np.int64) * 7919 - 10**6, sizes)
    cols = [dev(X[:, j]) for j in range(pp)]
    for kind, fn_by, fn_key, kw in (("rolling", pds.rolling_lin_reg_by, pds.rolling_lin_reg_by_key, dict(window_size=w)),
                                   ("recursive", pds.recursive_lin_reg_by, pds.recursive_lin_reg_by_key, dict(start_with=w))):
        ref = fn_by(*cols, target=dev(y), group_offsets=dev(off), **kw)
        got = fn_key(*cols, target=dev(y), key=dev(keys), **kw)
        for u, v in zip(ref, got):
            np.testing.assert_array_equal(bits(u), bits(v))
        one = fn_key(*cols, target=dev(y), key=dev(np.full(len(y), -3, np.int64)), **kw)
        whole = fn_by(*cols, target=dev(y), group_offsets=dev(np.array([0, len(y)], np.int64)), **kw)
        for u, v in zip(whole, one):
            np.testing.assert_array_equal(bits(u), bits(v))
    # unordered keys: a date-major panel of 200 interleaved keys == the offsets form on the stably sorted frame, scattered back
    D, K = 300, 200
    ids = rng.permutation(K).astype(np.int64) * 31 - 3000
    keys = np.tile(ids, D)
    n = D * K
    X = rng.random((n, 5))
    y = X @ rng.normal(size=5) + 0.01 * rng.normal(size=n)
    order = np.argsort(keys, kind="stable")
    _, counts = np.unique(keys[order], return_counts=True)
    off = offsets_of(counts)
    for kind, fn_by, fn_key, kw in (("rolling", pds.rolling_lin_reg_by, pds.rolling_lin_reg_by_key, dict(window_size=20, add_bias=True)),
                                   ("recursive", pds.recursive_lin_reg_by, pds.recursive_lin_reg_by_key, dict(start_with=10))):
        got = [host(t) for t in fn_key(*[dev(X[:, j]) for j in range(5)], target=dev(y), key=dev(keys), **kw)]
        srt = [host(t) for t in fn_by(*[dev(X[order, j]) for j in range(5)], target=dev(y[order]), group_offsets=dev(off), **kw)]
        for u, v in zip(srt, got):
            back = np.empty_like(u)
            back[order] = u
            np.testing.assert_array_equal(bits(back), bits(v), err_msg=kind)
        # host keys and columns give the same bits
        h = fn_key(*[np.ascontiguousarray(X[:, j]) for j in range(5)], target=y, key=keys, **kw)
        for u, v in zip(got, h):
            np.testing.assert_array_equal(bits(u), bits(v))


@pytest.mark.parametrize("kind", ["rolling", "recursive"])
def test_host_and_device_spaces(pds, kind):
    rng = np.random.default_rng(6)
    for pp in (6, 12):
        X, y, off = frame(rng, sizes_for(rng, 64), pp)
        d = call(pds, kind, X, y, off, 64, False, 0.0, on_dev=True)
        h = call(pds, kind, X, y, off, 64, False, 0.0, on_dev=False)
        for u, v in zip(d, h):
            np.testing.assert_array_equal(bits(u), bits(v))


@pytest.mark.parametrize("kind,pp", [("rolling", 4), ("recursive", 8), ("rolling", 13)])
def test_f32_frames(pds, kind, pp):
    rng = np.random.default_rng(7)
    w = 64
    X, y, off = frame(rng, sizes_for(rng, w), pp)
    X32, y32 = X.astype(np.float32), y.astype(np.float32)
    pds.config.LIN_REG_EXPR_F64 = False
    try:
        co, pr, va = call(pds, kind, X32, y32, off, w, False, 0.0)
    finally:
        pds.config.LIN_REG_EXPR_F64 = True
    assert co.dtype == np.float32
    np.testing.assert_array_equal(va, rule_valid(off, w))
    check_values(kind, co, pr, X32.astype(np.float64), y32.astype(np.float64), off, w, False, 0.0, rng, tol=F32_TOL)


def test_errors(pds):
    from polars_ds_extension_amd import _lib

    rng = np.random.default_rng(8)
    X, y, off = frame(rng, [100, 50, 80], 3)
    cols = [X[:, j].copy() for j in range(3)]
    for bad in ([1, 100, 150, 230], [0, 100, 150, 229], [0, 100, 90, 230]):
        with pytest.raises(_lib.PdsError) as e:
            pds.rolling_lin_reg_by(*cols, target=y, group_offsets=np.array(bad, np.int64), window_size=10)
        assert e.value.code == -1 and "group offsets" in e.value.msg
    wide = [rng.random(230) for _ in range(65)]
    with pytest.raises(_lib.PdsError) as e:
        pds.recursive_lin_reg_by(*wide, target=y, group_offsets=off, start_with=100)
    assert e.value.code == -5 and "64 coefficients" in e.value.msg
    with pytest.raises(_lib.PdsError) as e:
        pds.rolling_lin_reg_by_key(*wide, target=y, key=np.zeros(230, np.int64), window_size=100)
    assert e.value.code == -5
    # window / start_with < 1 straight through the C ABI
    lib = _lib.load()
    ctx = pds.default_context()
    ptrs = (C.c_void_p * 4)(*[c.ctypes.data for c in [y] + cols])
    co, pr, va = np.empty((230, 3)), np.empty(230), np.empty(230, np.uint8)
    rc = lib.pds_recursive_lr_grouped_f64(ctx._h, ptrs, 3, C.c_int64(230), C.c_void_p(off.ctypes.data), C.c_int64(3), _lib.PDS_HOST, 0,
                                          C.c_int64(0), C.c_double(0.0), C.c_void_p(co.ctypes.data), C.c_void_p(pr.ctypes.data),
                                          C.c_void_p(va.ctypes.data))
    assert rc == -1 and b"start_with" in lib.pds_last_error()
    with pytest.raises(ValueError):
        pds.rolling_lin_reg_by(*cols, target=y, group_offsets=off, window_size=1)


# ---- the Polars plugin symbols: pl_rolling_lr_by / pl_recursive_lr_by (tests/plugin_harness.py)
def _plugin_lib():
    import sys
    from pathlib import Path

    sys.path.insert(0, str(Path(__file__).resolve().parent))
    import plugin_harness as ph
    from polars_ds_extension_amd import _lib

    return ph, _lib.load()


def test_plugin_by_key_matches_per_group_calls(pds):
    import pyarrow as pa

    ph, so = _plugin_lib()
    rng = np.random.default_rng(9)
    D, K, w = 120, 7, 12
    n = D * K
    keys = np.tile(np.array([5, -2, 40, 7, 0, 11, -9], np.int64), D)
    X = rng.random((n, 2))
    y = X @ [0.7, -0.2] + 0.1 + 0.05 * rng.normal(size=n)
    key_arr = pa.array([None if k == 40 else int(k) for k in keys], type=pa.int64())  # one group of null keys
    ins = [("k", key_arr), ("y", pa.array(y)), ("x1", pa.array(X[:, 0])), ("x2", pa.array(X[:, 1]))]
    for sym, kw in (("pl_rolling_lr", {"null_policy": "raise", "n": w, "bias": True, "lambda": 0.0, "min_size": 0}),
                    ("pl_recursive_lr", {"null_policy": "raise", "n": w, "bias": True, "lambda": 0.0, "min_size": 0})):
        _, out = ph.call_plugin(so, sym + "_by", ins, kw)
        res = out.to_pylist()
        assert len(res) == n
        for k in np.unique(keys):
            rows = np.flatnonzero(keys == k)
            _, one = ph.call_plugin(so, sym, [(c, a.take(pa.array(rows))) for c, a in ins[1:]], kw)
            one = one.to_pylist()
            for j, r in enumerate(rows):
                a, b = res[r], one[j]
                assert (a["coeffs"] is None) == (b["coeffs"] is None) and (a["pred"] is None) == (b["pred"] is None), (sym, k, j)
                if b["coeffs"] is not None:
                    assert nrel(a["coeffs"], b["coeffs"]) < 1e-10 and abs(a["pred"] - b["pred"]) < 1e-9 * max(1, abs(b["pred"]))
    f = ph.output_field(so, "pl_rolling_lr_by")
    assert [c.name for c in f.type] == ["coeffs", "pred"]


def test_plugin_by_key_null_policies(pds):
    import pyarrow as pa

    ph, so = _plugin_lib()
    rng = np.random.default_rng(10)
    n, w = 600, 10
    keys = np.repeat(np.arange(3, dtype=np.int64), n // 3)[rng.permutation(n)]
    X = rng.random((n, 2))
    y = X @ [1.0, 2.0] + 0.01 * rng.normal(size=n)
    ynull = [None if i % 17 == 3 else float(v) for i, v in enumerate(y)]
    x1null = [None if i % 23 == 5 else float(v) for i, v in enumerate(X[:, 0])]
    ins = [("k", pa.array(keys)), ("y", pa.array(ynull, pa.float64())), ("x1", pa.array(x1null, pa.float64())), ("x2", pa.array(X[:, 1]))]
    kw = {"n": w, "bias": False, "lambda": 0.0, "min_size": 2}
    with pytest.raises(ph.PluginFailure, match="Nulls"):
        ph.call_plugin(so, "pl_rolling_lr_by", ins, dict(kw, null_policy="raise"))
    for pol in ("skip", "0.5"):
        for sym in ("pl_rolling_lr", "pl_recursive_lr"):
            _, out = ph.call_plugin(so, sym + "_by", ins, dict(kw, null_policy=pol))
            res = out.to_pylist()
            for k in range(3):
                rows = np.flatnonzero(keys == k)
                _, one = ph.call_plugin(so, sym, [(c, a.take(pa.array(rows))) for c, a in ins[1:]], dict(kw, null_policy=pol))
                one = one.to_pylist()
                for j, r in enumerate(rows):
                    a, b = res[r], one[j]
                    assert (a["coeffs"] is None) == (b["coeffs"] is None), (sym, pol, k, j)
                    if b["coeffs"] is not None:
                        assert nrel(a["coeffs"], b["coeffs"]) < 1e-9, (sym, pol, k, j)
