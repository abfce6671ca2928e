"""Frames, input conditions and references for the grouped lin_reg_w_rcond tests (tests/test_grouped_rcond_cpu.py,
tests/test_grouped_rcond_gpu.py): seeded ragged groups of four kinds (full rank, a duplicated column, a constant column beside a bias,
an all-zero column), the conditions every group's spectrum has to meet before a comparison means anything, and the per-group
oracle / numpy references, computed once per frame and shared."""
import functools

import numpy as np

RCOND = 1e-6  # every test passes it explicitly: at the default floor an exactly collinear group's rounding noise sits next to the cut
KINDS = ("full", "dup", "const", "zero")
WIDTHS = tuple(range(1, 17))
LONG = 5000


def sizes_for(pp):
    return (pp, pp + 1, 63, 64, 65, 128, 129, 300)


def offsets(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def excluded(p, bias, kind):
    """the all-zero system (p' = 1 with its only column zero): it has its own null test"""
    return kind == "zero" and p == 1 and not bias


def group(rng, n, p, bias, kind):
    """X [n, p], y [n].  n > p' + 1: standard normal features.  n <= p' + 1: a row-permuted identity scaled by U(1, 2) plus
    0.1 N(0, 1) (plain random square groups come within 50 x of the cut).  kind: "dup" the last feature is a copy of the first,
    "const" the first feature is 2.0 (collinear with a bias), "zero" the middle feature is all zero."""
    pp = p + int(bias)
    if n > pp + 1:
        X = rng.normal(size=(n, p))
    else:
        X = np.eye(n, p)[rng.permutation(n)] * rng.uniform(1.0, 2.0, size=(n, p)) + 0.1 * rng.normal(size=(n, p))
    if kind == "dup":
        X[:, p - 1] = X[:, 0]
    elif kind == "const":
        X[:, 0] = 2.0
    elif kind == "zero":
        X[:, p // 2] = 0.0
    beta = rng.uniform(-1.0, 1.0, size=p)
    y = X @ beta + 0.3 + 0.1 * rng.normal(size=n)
    return X, y


def design(X, bias):
    return np.column_stack([X, np.ones(len(X))]) if bias else X


def rcond_g(n, pp, eps=np.finfo(np.float64).eps, rcond=RCOND):
    """the cut of a group: pl_lr_w_rcond's floor with the group's own row count"""
    return max(rcond, eps * max(n, pp))


def spectrum_gaps(A, rc, l2=0.0, n_feat=None):
    """From numpy's eigvalsh of A'A (+ l2 on the first n_feat diagonals): (smallest kept / thr, largest cut / thr, ev_max / smallest
    kept, number cut), thr = rc * sqrt(ev_max) against the EIGENVALUES, the reference's rule."""
    G = A.T @ A
    if l2:
        G[np.arange(n_feat), np.arange(n_feat)] += l2
    ev = np.linalg.eigvalsh(G)[::-1]
    thr = rc * np.sqrt(ev[0])
    kept = ev >= thr
    cut_max = float(np.max(ev[~kept])) if (~kept).any() else 0.0
    return float(ev[kept].min() / thr), cut_max / thr, float(ev[0] / ev[kept].min()), int((~kept).sum())


def check_conditions(A, rc, l2=0.0, n_feat=None):
    """The conditions on the inputs (not measurements): every kept eigenvalue >= 10 thr, every cut one <= thr / 10,
    ev_max / ev_min_kept <= 1e4.  Returns the gaps."""
    kept, cut, cond, n_cut = spectrum_gaps(A, rc, l2, n_feat)
    assert kept >= 10.0, ("a kept eigenvalue within 10 x of the cut", kept)
    assert cut <= 0.1, ("a cut eigenvalue within 10 x of the cut", cut)
    assert cond <= 1e4, ("kept-subspace condition number", cond)
    return kept, cut, cond, n_cut


class Frame:
    """One frame of ragged groups: X [n, p], y [n], off [G + 1], kinds [G]."""

    def __init__(self, X, y, off, kinds, p, bias):
        self.X, self.y, self.off, self.kinds, self.p, self.bias = X, y, off, kinds, p, bias
        self.pp = p + int(bias)

    @property
    def n_groups(self):
        return len(self.off) - 1

    def rows(self, g):
        return slice(int(self.off[g]), int(self.off[g + 1]))

    def design(self, g, dtype=np.float64):
        s = self.rows(g)
        return design(self.X[s].astype(dtype).astype(np.float64), self.bias), self.y[s].astype(dtype).astype(np.float64)


def build_frame(seed, p, bias, sizes=None, kinds=KINDS, long_rows=LONG):
    rng = np.random.default_rng(seed)
    pp = p + int(bias)
    Xs, ys, ns, ks = [], [], [], []
    for n in (sizes_for(pp) if sizes is None else sizes):
        for kind in kinds:
            if excluded(p, bias, kind):
                continue
            X, y = group(rng, n, p, bias, kind)
            Xs.append(X), ys.append(y), ns.append(n), ks.append(kind)
    if long_rows:
        X, y = group(rng, long_rows, p, bias, "full")
        Xs.append(X), ys.append(y), ns.append(long_rows), ks.append("full")
    return Frame(np.ascontiguousarray(np.concatenate(Xs)), np.ascontiguousarray(np.concatenate(ys)), offsets(ns), ks, p, bias)


@functools.lru_cache(maxsize=None)
def width_frame(p, bias):
    """the frame of the every-width test: sizes {p', p' + 1, 63, 64, 65, 128, 129, 300} x the four kinds + one group of 5 000 rows"""
    f = build_frame(1000 + 2 * p + int(bias), p, bias)
    for a in (f.X, f.y, f.off):
        a.setflags(write=False)
    return f


def frame_conditions(f, eps=np.finfo(np.float64).eps, dtype=np.float64, l2=0.0):
    """check_conditions on EVERY group of the frame; returns the worst (kept / thr, cut / thr, condition number)"""
    worst = [np.inf, 0.0, 0.0]
    for g in range(f.n_groups):
        A, _ = f.design(g, dtype)
        kept, cut, cond, _ = check_conditions(A, rcond_g(len(A), f.pp, eps), l2, f.p)
        worst = [min(worst[0], kept), max(worst[1], cut), max(worst[2], cond)]
    return tuple(worst)


def oracle_by(orc, f, eps=np.finfo(np.float64).eps, dtype=np.float64, l2=0.0):
    """oracle.solve_lr_rcond (f64) on every group's rows alone with the group's cut: (coeffs [G, p'], singular_values [G, p']);
    `dtype`: the frame type the device sees (the data is rounded to it first)"""
    G = f.n_groups
    co, sv = np.full((G, f.pp), np.nan), np.full((G, f.pp), np.nan)
    for g in range(G):
        A, y = f.design(g, dtype)
        if len(A) < f.pp:
            continue
        co[g], sv[g] = orc.solve_lr_rcond(A, y, l2, bool(f.bias), rcond_g(len(A), f.pp, eps))
    return co, sv


def lstsq_by(f):
    """np.linalg.lstsq(A_g, y_g, rcond=1e-6) on every group: (coeffs [G, p'], rank [G])"""
    co = np.full((f.n_groups, f.pp), np.nan)
    rank = np.zeros(f.n_groups, dtype=np.int64)
    for g in range(f.n_groups):
        A, y = f.design(g)
        co[g], _, rank[g], _ = np.linalg.lstsq(A, y, rcond=RCOND)
    return co, rank


def nrel(a, b):
    """normwise relative distance ||a - b|| / ||b|| (the parity measure of tests/test_gpu_parity.py), here per group"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))
