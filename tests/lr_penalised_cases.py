"""Frames and references of the lasso / elastic-net / NNLS tests (tests/test_lr_penalised_cpu.py, tests/test_lr_penalised_gpu.py).

Correlated frame of width p: X = N(0, 1) + 0.7 x (one common factor per row), 3p + 40 rows, true coefficients normal with 60 % of
them zero, y = X beta + 0.5 + 0.3 noise; seeded 77 + p (SEEDS: another seed where that one misses a frame condition).  The three frames around the prefetch border of cd_kernel (p' = 576) have 2p
rows and a factor weight of 0.3, so that the reference converges in hundreds of sweeps (13 .. 1 014).  Widths: both sides of a 64-coordinate
chunk (63, 64, 65; 128, 129), of the one-copy return of the coefficients (252, 253 without bias), of the register prefetch (575 and
576 with bias, 577 without), and 1, 8, 16, 17; bias on and off.  Penalty sets (l1, l2, positive): PENALTIES, and "nnls" (positive
alone).

Order frames: p = 80 with column 70 (another 64-coordinate chunk) or column 5 (the same chunk) an exact copy of column 3, pure
lasso: the minimiser is not unique and the iterates depend on the update order.  Saturated frames: an l1 that thresholds every
feature from the first sweep on; a target that clamps every feature under `positive`.  A frame with an all-zero column.  Grouped
frames of 40 groups, empty ones and ones with fewer rows than coefficients among them, each group with its own coefficients.

A frame on which no feature moves in the first sweep is kept out (`moves_in_the_first_sweep`): the reference stops there, before it
has set the bias, and so does the kernel -- what comes back is the reference's answer but no minimiser.

Everything here is computed on the CPU and frozen.  The long double fixed points (lr_penalised_reference.sweeps at tol 1e-17; about
90 s for a 576-wide frame) and the float64 oracle's rounding floor (its KKT residual after 20 000 sweeps at tol 1e-300) are
recorded in tests/golden/lr_penalised_refs.npz; `python tests/lr_penalised_cases.py` rewrites the record.
test_lr_penalised_cpu.py recomputes the narrow cases against it and checks every recorded fixed point against the KKT conditions
computed from the frame, which needs no solver.  The oracle's runs at the tests' settings are made when a test asks for them."""
import functools
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
for _p in (str(ROOT), str(ROOT / "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import lr_penalised_reference as ref  # noqa: E402

L = np.longdouble
GOLDEN = Path(__file__).resolve().parent / "golden" / "lr_penalised_refs.npz"
TOL, MAX_ITER = 1e-10, 5000
TOL_DEFAULT = 1e-5
TOL_F32 = 1e-6  # (an f32 frame runs under the library's own caps, 2 000 sweeps of coordinate descent and 200 of NNLS: oracle.pl_lr(f32_path=True))
STAR_TOL, STAR_CAP = 1e-17, 200_000
NNLS_STAR_TOL = 1e-17  # times max |c|: the test is on G beta - c, in the units of c
FLOOR_TOL, FLOOR_CAP = 1e-300, 20_000

PENALTIES = {"lasso": (0.05, 0.0, False), "enet": (0.03, 0.05, False), "ridge+": (0.0, 0.1, True), "lasso+": (0.02, 0.0, True)}
ALL_PENS = list(PENALTIES) + ["nnls"]
PREFETCH = [(575, True), (576, True), (577, False)]
WIDTHS = [(p, b) for p in (1, 8, 16, 17, 63, 64, 65, 128, 129) for b in (True, False)] + [(252, False), (253, False)] + PREFETCH
# width -> seed where 77 + width misses a frame condition (test_lr_penalised_cpu.py): under `positive` more than 90 % zeros, mostly
SEEDS = {16: 3093, 17: 3094, 64: 4141, 65: 1142, 128: 3205, 129: 5206, 253: 14330, 575: 14652, 577: 32654}
ORDER = {"other_chunk": 70, "same_chunk": 5}  # the column that copies column 3
ORDER_P = 80
GROUPED = [(1, True), (1, False), (16, True), (16, False), (17, True), (17, False), (65, True)]


def orc():
    from oracle import oracle

    oracle.build()
    return oracle


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def correlated(rng, rows, p, weight):
    X = rng.normal(size=(rows, p)) + weight * rng.normal(size=(rows, 1))
    b = rng.normal(size=p)
    b[rng.random(p) < 0.6] = 0.0
    y = X @ b + 0.5 + 0.3 * rng.normal(size=rows)
    return X, y, b


@functools.lru_cache(maxsize=None)
def frame(p):
    """(X, y, true coefficients) of the correlated frame of width p"""
    wide = p >= 575
    rng = np.random.default_rng(SEEDS.get(p, 77 + p))
    return _frozen(*correlated(rng, 2 * p if wide else 3 * p + 40, p, 0.3 if wide else 0.7))


@functools.lru_cache(maxsize=None)
def order_frame(kind):
    X, y, b = (a.copy() for a in frame(ORDER_P))
    X[:, ORDER[kind]] = X[:, 3]
    return _frozen(np.ascontiguousarray(X), y, b)


@functools.lru_cache(maxsize=None)
def saturated_frame(p, positive):
    """(X, y, l1): every feature is thresholded from the first sweep on, with or without a bias; `positive`: y = -X |b| on features
    of mean 1, so every x_j'y and x_j'(y - mean y) is negative and every feature is clamped at any l1"""
    rng = np.random.default_rng(900 + p)
    if positive:
        X = rng.normal(size=(3 * p + 40, p)) + 0.7 * rng.normal(size=(3 * p + 40, 1)) + 1.0
        y = -(X @ np.abs(rng.normal(size=p)))
        return _frozen(X, y) + (0.02,)
    X, y, _ = correlated(rng, 3 * p + 40, p, 0.7)
    y = y + 8.0  # (a mean well away from zero: sum y is then formed without cancellation)
    Xl, yl = X.astype(L), y.astype(L)
    n = L(len(y))
    l1 = 2 * max(np.abs(Xl.T @ yl).max(), np.abs(Xl.T @ (yl - yl.sum() / n)).max()) / n
    return _frozen(X, y) + (float(l1),)


ZERO_COLS = {8: 4, 80: 70}  # width -> the all-zero column: in the first 64-coordinate chunk, in the second


@functools.lru_cache(maxsize=None)
def zero_column_frame(p):
    """the correlated frame with column ZERO_COLS[p] all zero"""
    X, y, b = (a.copy() for a in frame(p))
    X[:, ZERO_COLS[p]] = 0.0
    return _frozen(X, y, b)


def grouped_sizes(pp):
    return np.array([0, pp - 1, pp // 2, 2 * pp + 2, 3 * pp, 4 * pp - 1, 5 * pp - 1, 5 * pp] * 5, dtype=np.int64)


def moves_in_the_first_sweep(X, y):
    """The reference's stopping rule looks at the features' moves only, and the bias is set after them: a first sweep in which every
    feature stays at zero (against a bias of zero) ends the fit, whatever the bias then does to the gradient -- the result is the
    reference's answer and the kernel's, but no minimiser, and nothing for a KKT test.  True where some x_j'y / n exceeds every l1
    of PENALTIES, so that under every penalty set, `positive` or not, a feature moves in the first sweep."""
    return len(y) > 0 and float((X.T @ y).max()) / len(y) > 2 * max(v[0] for v in PENALTIES.values())


@functools.lru_cache(maxsize=None)
def grouped_frame(p, bias):
    """(X, y, offsets): 40 groups of 0 .. 5 p' rows, every group drawn as a correlated frame with its own coefficients (drawn again
    while no feature would move in the first sweep)"""
    pp = p + int(bias)
    sizes = grouped_sizes(pp)
    rng = np.random.default_rng([31, p, int(bias)])
    parts = []
    for s in sizes:
        part = correlated(rng, int(s), p, 0.7)
        while s >= pp and not moves_in_the_first_sweep(part[0], part[1]):
            part = correlated(rng, int(s), p, 0.7)
        parts.append(part)
    X = np.ascontiguousarray(np.concatenate([a[0] for a in parts]))
    y = np.concatenate([a[1] for a in parts])
    return _frozen(X, y, np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64))


def as_f32(X, y):
    """the values an f32 frame stores, widened again"""
    return X.astype(np.float32).astype(np.float64), y.astype(np.float32).astype(np.float64)


# ---- references on a frame (X, y)
def star_of(X, y, bias, pen):
    """the long double fixed point of a frame: (beta, sweeps, converged)"""
    p = X.shape[1]
    G, c, m = ref.moments(X, y, bias)
    if pen == "nnls":
        beta, it = ref.nnls_sweeps(G, c, p, bias, NNLS_STAR_TOL * np.abs(c).max(), STAR_CAP, L)
        return beta, it, it < STAR_CAP
    l1, l2, pos = PENALTIES[pen] if isinstance(pen, str) else pen
    return ref.sweeps(G, c, m, p, bias, l1, l2, STAR_TOL, STAR_CAP, pos, L)


def oracle_of(X, y, bias, pen, tol=TOL, max_iter=MAX_ITER):
    """the float64 oracle's run on a frame: (beta, sweeps, converged); the arithmetic is the frame's dtype"""
    o = orc()
    Xb = o.with_bias(X) if bias else X
    if pen == "nnls":
        return oracle_nnls(Xb, y, bias, tol, max_iter)
    l1, l2, pos = PENALTIES[pen] if isinstance(pen, str) else pen
    return o.coordinate_descent(Xb, y, l1, l2, bias, tol, max_iter, pos, return_info=True)


def oracle_nnls(Xb, y, bias, tol, max_iter):
    """orc_nn_lr with its sweep count: (beta, sweeps, converged)"""
    import ctypes as C

    o = orc()
    Xf, yf, dt = o._prep(Xb, y)
    n, pp = Xf.shape
    beta = np.zeros(pp, dtype=dt)
    fn = getattr(o.lib(), "orc_nn_lr" + o._suf(dt))
    fn.restype = C.c_int
    it = int(fn(o._p(Xf), o._p(yf), C.c_int64(n), C.c_int(pp), C.c_int(bool(bias)), o._real(dt)(tol), C.c_int(max_iter), o._p(beta),
                C.c_int(1)))
    return beta, it, it < max_iter


def oracle_nnls_from_gram(G, c, bias, tol, max_iter):
    import ctypes as C

    o = orc()
    G = np.asfortranarray(G)
    dt = G.dtype
    c = np.ascontiguousarray(c, dtype=dt)
    beta = np.zeros(G.shape[0], dtype=dt)
    fn = getattr(o.lib(), "orc_nnls_from_gram" + o._suf(dt))
    fn.restype = C.c_int
    it = int(fn(o._p(G), o._p(c), C.c_int(G.shape[0]), C.c_int(bool(bias)), o._real(dt)(tol), C.c_int(max_iter), o._p(beta)))
    return beta, it


def kkt_of(X, y, bias, pen, beta):
    if pen == "nnls":
        return ref.nnls_kkt(X, y, bias, beta)
    l1, l2, pos = PENALTIES[pen] if isinstance(pen, str) else pen
    return ref.kkt(X, y, bias, l1, l2, beta, pos)


def floor_of(X, y, bias, pen, floor_beta=None):
    """(F, scale): the KKT residual of the oracle run to tol 1e-300 -- its rounding floor on this frame -- and the size of the terms
    its gradient is the difference of"""
    if floor_beta is None:
        floor_beta = oracle_of(X, y, bias, pen, FLOOR_TOL, FLOOR_CAP)[0]
    return kkt_of(X, y, bias, pen, floor_beta), ref.row_sums(X, y, bias, floor_beta)[1]


def kkt_bound(X, y, bias, pen, tol, floor=None):
    """(bound, parts): what a converged fit's KKT residual may be.  Coordinate descent: tol max_j sum_k |G_jk| / n -- after the last
    sweep every coordinate was optimal when visited and every other one has since moved by less than tol -- plus 10 F, F the
    rounding floor of the oracle on this frame (8 ulp of the gradient's terms where float64 does not resolve it); `floor` = (F, scale)
    where it is known already.  NNLS: tol + 10 F, the stopping test being the KKT test itself, in the units of G beta - c."""
    F, scale = floor if floor is not None else floor_of(X, y, bias, pen)
    n = X.shape[0]
    if pen == "nnls":
        first, fl = tol, ref.floor_term(F, scale * n)
    else:
        first, fl = tol * ref.row_sums(X, y, bias)[0], ref.floor_term(F, scale)
    return first + fl, {"stopping": first, "F": F, "floor": fl}


def convex(X, l2):
    return l2 > 0.0 or X.shape[0] > X.shape[1]


def split(a):
    """a long double array as its float64 value and the remainder in float32 (53 + 24 bits for the 64 of a long double): what the
    record stores"""
    hi = np.asarray(a, dtype=L).astype(np.float64)
    return hi, (np.asarray(a, dtype=L) - hi.astype(L)).astype(np.float32)


def solve(X, y, bias, pen):
    """what the record holds of a frame: the long double fixed point (split), its sweeps, the floor of the oracle (F, scale)"""
    star, it, conv = star_of(X, y, bias, pen)
    assert conv, (X.shape, bias, pen)
    hi, lo = split(star)
    return {"hi": hi, "lo": lo, "sweeps": np.int64(it), "floor": np.array(floor_of(X, y, bias, pen))}


@functools.lru_cache(maxsize=None)
def _golden():
    return dict(np.load(GOLDEN))


def recorded(key, pen, group=None):
    """one frame's entry of the record; the arrays of a key are stacked over ALL_PENS (and over the groups of a grouped frame)"""
    g = _golden()
    i = ALL_PENS.index(pen) if group is None else (ALL_PENS.index(pen), group)
    return {k: g[f"{key}:{k}"][i] for k in ("hi", "lo", "sweeps", "floor")}


def key_of(p, bias, grouped=False):
    return f"{'g' if grouped else 'w'}/{p}/{int(bias)}"


def stacked(entries):
    return {k: np.stack([e[k] for e in entries]) for k in ("hi", "lo", "sweeps", "floor")}


@functools.lru_cache(maxsize=None)
def case(p, bias, pen, fresh=False):
    """everything the tests hold the device against on the correlated frame of width p: dict with X, y, star (long double), its
    zero set, the oracle's run at TOL / MAX_ITER, its distance from star and the budget made of it, the KKT bound.  The fixed point
    and the floor run come from the record unless `fresh`."""
    X, y, _ = frame(p)
    return _case(X, y, bias, pen, solve(X, y, bias, pen) if fresh else recorded(key_of(p, bias), pen))


def _case(X, y, bias, pen, rec):
    p = X.shape[1]
    star = rec["hi"].astype(L) + rec["lo"].astype(L)
    ob, o_it, o_conv = oracle_of(X, y, bias, pen, TOL, MAX_ITER)
    bound, parts = kkt_bound(X, y, bias, pen, TOL, tuple(rec["floor"]))
    own = ref.rel(ob, star)
    n = X.shape[0]
    out = {"X": X, "y": y, "p": p, "bias": bias, "pen": pen, "star": star, "star_sweeps": int(rec["sweeps"]), "floor": tuple(float(v) for v in rec["floor"]),
           "zero": np.asarray(star[:p] == 0), "oracle": ob, "oracle_sweeps": o_it, "oracle_converged": o_conv,
           "own": own, "budget": ref.budget(own), "kkt_bound": bound, "kkt_parts": parts, "oracle_kkt": kkt_of(X, y, bias, pen, ob),
           "star_kkt": kkt_of(X, y, bias, pen, star) / (n if pen == "nnls" else 1)}
    if pen == "nnls":
        out["slack"], out["size"] = np.inf, (float(np.abs(star[:p][star[:p] != 0]).min()) if (star[:p] != 0).any() else np.inf)
    else:
        l1, l2, pos = PENALTIES[pen]
        out["slack"], out["size"] = ref.slack_and_size(X, y, bias, l1, l2, star, pos)
    return out


@functools.lru_cache(maxsize=None)
def grouped_case(p, bias, pen, fresh=False):
    """per group of the grouped frame: the dict of `_case`; None for a group with fewer rows than coefficients"""
    X, y, off = grouped_frame(p, bias)
    pp = p + int(bias)
    out = []
    for g in range(len(off) - 1):
        a, b = int(off[g]), int(off[g + 1])
        if b - a < pp:
            out.append(None)
            continue
        Xg, yg = X[a:b], y[a:b]
        out.append(_case(Xg, yg, bias, pen, solve(Xg, yg, bias, pen) if fresh else recorded(key_of(p, bias, True), pen, g)))
    return out


@functools.lru_cache(maxsize=None)
def partial(kind, p, bias, pen, n_sweeps):
    """the state after `n_sweeps` sweeps from zero: (long double, the float64 restatement's distance from it); kind: "width",
    "other_chunk", "same_chunk" """
    X, y, _ = frame(p) if kind == "width" else order_frame(kind)
    out = []
    for dt in (L, np.float64):
        G, c, m = ref.moments(X, y, bias, dt)
        if pen == "nnls":
            out.append(ref.nnls_sweeps(G, c, p, bias, TOL, n_sweeps, dt)[0])
        else:
            l1, l2, pos = PENALTIES[pen]
            beta, it, conv = ref.sweeps(G, c, m, p, bias, l1, l2, TOL, n_sweeps, pos, dt)
            assert p == 1 or (it == n_sweeps and not conv), (p, bias, pen, n_sweeps)  # (nothing has converged yet; one feature may have)
            out.append(beta)
    return out[0], ref.rel(out[1], out[0])


if __name__ == "__main__":
    import time

    rec = {k: v for k, v in np.load(GOLDEN).items() if k.startswith("w/")} if "--grouped-only" in sys.argv and GOLDEN.exists() else {}
    for p, bias in ([] if rec else WIDTHS):
        t = time.time()
        X, y, _ = frame(p)
        for k, v in stacked([solve(X, y, bias, pen) for pen in ALL_PENS]).items():
            rec[f"{key_of(p, bias)}:{k}"] = v
        print(f"p={p} bias={bias}: {time.time() - t:.1f} s", flush=True)
    for p, bias in GROUPED:
        t = time.time()
        X, y, off = grouped_frame(p, bias)
        pp = p + int(bias)
        null = {"hi": np.full(pp, np.nan), "lo": np.zeros(pp, dtype=np.float32), "sweeps": np.int64(0), "floor": np.zeros(2)}
        per_pen = [stacked([solve(X[a:b], y[a:b], bias, pen) if b - a >= pp else null for a, b in zip(off[:-1], off[1:])]) for pen in ALL_PENS]
        for k in per_pen[0]:
            rec[f"{key_of(p, bias, True)}:{k}"] = np.stack([e[k] for e in per_pen])
        print(f"grouped p={p} bias={bias}: {time.time() - t:.1f} s", flush=True)
    GOLDEN.parent.mkdir(exist_ok=True)
    np.savez_compressed(GOLDEN, **rec)
    print(GOLDEN, GOLDEN.stat().st_size, "bytes")
