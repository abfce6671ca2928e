"""Frames, input conditions and references for the grouped multi-target lin_reg tests (tests/test_grouped_multi_cpu.py,
tests/test_grouped_multi_gpu.py): seeded ragged groups of three kinds (full rank, an exactly duplicated column, a constant column
beside the intercept), k targets that are linear in X plus noise with one target identically zero, the gate statistic of every group
in NumPy (so that no tolerance decides a null flag), and the per-group oracle reference, computed once per frame and shared."""
import functools

import numpy as np

KINDS = ("full", "dup", "const")
GATE_TOL = {np.float64: 1e-12, np.float32: 1e-6}  # the dtype-aware default of singular_x_tol
# (features, targets) of the parity tests: every P of {1, 2, 7, 8, 9, 15, 16} and every k of {1, 2, 3, 8, 15}, each run with and
# without the intercept
PAIRS = ((1, 1), (2, 2), (7, 3), (8, 8), (9, 15), (15, 3), (16, 2), (16, 15), (8, 1))


def sizes_for(pp):
    """rows per group: empty, one row, one short of / exactly / one past the coefficient count, around the 64-row step of the kernel and
    its masked tail, several steps"""
    return tuple(dict.fromkeys((0, 1, pp - 1, pp, pp + 1, 63, 64, 65, 128, 129, 200)))


def offsets(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def design(X, bias):
    return np.column_stack([X, np.ones(len(X))]) if bias else X


def degenerate(kind, p, bias):
    """does the kind make X'X (with the intercept column, if any) singular?"""
    return (kind == "dup" and p >= 2) or (kind == "const" and bias)


def group(rng, n, p, k, bias, kind):
    """X [n, p], T [n, k].  n > p' + 1: standard normal features; otherwise a row-permuted identity scaled by U(1, 2) plus 0.1 N(0, 1)
    (a plain random square group can sit anywhere near the gate).  "dup": the last feature is a copy of the first; "const": the first
    feature is 2.0.  Targets: X B + 0.3 + 0.1 N(0, 1); the last of two or more targets is identically zero."""
    pp = p + int(bias)
    if n > pp + 1:
        X = rng.normal(size=(n, p))
    else:
        X = np.eye(n, p)[rng.permutation(n)] * rng.uniform(1.0, 2.0, size=(n, p)) + 0.1 * rng.normal(size=(n, p))
    if kind == "dup" and p >= 2:
        X[:, p - 1] = X[:, 0]
    elif kind == "const":
        X[:, 0] = 2.0
    T = X @ rng.uniform(-1.0, 1.0, size=(p, k)) + 0.3 + 0.1 * rng.normal(size=(n, k))
    if k >= 2:
        T[:, k - 1] = 0.0
    return X, T


class Frame:
    """One frame of ragged groups: X [n, p], T [n, k], off [G + 1], kinds [G]."""

    def __init__(self, X, T, off, kinds, p, k, bias):
        self.X, self.T, self.off, self.kinds, self.p, self.k, self.bias = X, T, off, kinds, p, k, bias
        self.pp = p + int(bias)

    @property
    def n_groups(self):
        return len(self.off) - 1

    def n_of(self, g):
        return int(self.off[g + 1] - self.off[g])

    def rows(self, g):
        return slice(int(self.off[g]), int(self.off[g + 1]))

    def expect_null(self, g, l2=0.0):
        """by construction: fewer rows than coefficients, or a singular X'X (a ridge penalty makes every kind regular)"""
        return self.n_of(g) < self.pp or (l2 == 0.0 and degenerate(self.kinds[g], self.p, self.bias))

    def reversed(self):
        """the same groups in reversed order"""
        order = range(self.n_groups - 1, -1, -1)
        idx = np.concatenate([np.arange(self.off[g], self.off[g + 1]) for g in order]) if self.n_groups else np.zeros(0, dtype=np.int64)
        return Frame(np.ascontiguousarray(self.X[idx]), np.ascontiguousarray(self.T[idx]), offsets([self.n_of(g) for g in order]),
                     [self.kinds[g] for g in order], self.p, self.k, self.bias)


def build_frame(seed, p, k, bias, sizes=None, kinds=KINDS):
    rng = np.random.default_rng(seed)
    pp = p + int(bias)
    Xs, Ts, ns, ks = [], [], [], []
    for n in (sizes_for(pp) if sizes is None else sizes):
        for kind in (kinds if n >= pp else ("full",)):  # (a group with fewer rows than coefficients is null whatever its kind)
            X, T = group(rng, n, p, k, bias, kind)
            Xs.append(X), Ts.append(T), ns.append(n), ks.append(kind)
    return Frame(np.ascontiguousarray(np.concatenate(Xs)), np.ascontiguousarray(np.concatenate(Ts)), offsets(ns), ks, p, k, bias)


@functools.lru_cache(maxsize=None)
def pair_frame(p, k, bias):
    f = build_frame(4000 + 64 * p + 2 * k + int(bias), p, k, bias)
    for a in (f.X, f.T, f.off):
        a.setflags(write=False)
    return f


def gate_statistic(A, n_feat, l2=0.0):
    """The `choleskey` gate statistic of a group in NumPy: the product of the pivot ratios G_kk / d_k of the unpivoted L D L' of
    G = A'A (+ l2 on the first n_feat diagonals) -- compared against 1 / singular_x_tol.  inf for a pivot that is not positive."""
    G = A.T @ A
    G[np.arange(n_feat), np.arange(n_feat)] += l2
    diag = np.diag(G).copy()
    prod = 1.0
    for j in range(len(G)):
        d = G[j, j]
        if not d > 0.0:
            return np.inf
        prod *= diag[j] / d
        G[j + 1:, j + 1:] -= np.outer(G[j + 1:, j], G[j, j + 1:]) / d
    return float(prod)


def frame_gate_margins(f, dtype=np.float64, l2=0.0):
    """(largest statistic of a group expected fitted, smallest statistic of a group expected null by its kind) x singular_x_tol of the
    frame type, on the data rounded to that type"""
    tol = GATE_TOL[dtype]
    fitted, gated = 0.0, np.inf
    for g in range(f.n_groups):
        if f.n_of(g) < f.pp:
            continue
        s = gate_statistic(design(f.X[f.rows(g)].astype(dtype).astype(np.float64), f.bias), f.p, l2) * tol
        if f.expect_null(g, l2):
            gated = min(gated, s)
        else:
            fitted = max(fitted, s)
    return fitted, gated


_ORACLE = {}


def oracle_by(orc, f, dtype=np.float64, l2=0.0, key=None):
    """oracle.solve_lr_gated (QR, f64) on every group's rows alone, all k targets at once: (coeffs [G, k, p'] NaN where null, is_null
    [G]); `dtype`: the frame type the device sees (the data is rounded to it first).  Cached under `key`."""
    ck = (key, np.dtype(dtype).name, l2)
    if key is not None and ck in _ORACLE:
        return _ORACLE[ck]
    co = np.full((f.n_groups, f.k, f.pp), np.nan)
    nu = np.ones(f.n_groups, dtype=bool)
    for g in range(f.n_groups):
        if f.n_of(g) < f.pp:
            continue
        A = design(f.X[f.rows(g)].astype(dtype).astype(np.float64), f.bias)
        T = f.T[f.rows(g)].astype(dtype).astype(np.float64)
        b = orc.solve_lr_gated(A, T, l2, bool(f.bias), "qr", GATE_TOL[dtype])
        if b is not None:
            co[g], nu[g] = np.asarray(b).reshape(f.pp, f.k).T, False
    if key is not None:
        _ORACLE[ck] = (co, nu)
    return co, nu


def nrel(a, b):
    """normwise relative distance ||a - b|| / ||b||; a reference that is exactly zero (the zero target) wants exactly zero"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    nb = float(np.linalg.norm(b))
    return float(np.linalg.norm(a - b)) / nb if nb > 0.0 else (0.0 if not np.any(a) else np.inf)
