"""
The estimated effects of the two-way fixed-effects regression and the component labelling, restated in NumPy (TEST INFRASTRUCTURE
ONLY): the definitions of include/pds_lstsq.h (pds_lin_reg_within2_fx_*, pds_absorb_components_i32), line by line, for any dtype.

    hook_compress(i1, i2, n_a, n_b) -> (label [n_a + n_b], rounds)
        Nodes: n_a levels of key 1, then n_b codes of key 2; row r is the edge (i1[r], n_a + i2[r]).  label[v] = v to start; a round
        hooks -- for every edge whose ends have roots ru != rv, label[max(ru, rv)] = min(label[max(ru, rv)], min(ru, rv)), the roots
        read from the labelling the round started with -- and compresses, label = label[label] until nothing moves.  The rounds end
        with the one that finds nothing to hook; `rounds` counts it.  A parent is smaller than its child, so the final label is the
        smallest node index of the component.  round_cap(nodes) = 2 ceil(log2 nodes) + 1 is the library's cap (a root that neither
        hooks nor is hooked into in one round hooks in the next, so the trees of a component at least halve in TWO rounds;
        csrc/within2_graph.hip has the argument); a round past it raises RoundCapError, as the library refuses with PDS_ERR_NUMERIC.
    effects(F, y, codes1, codes2, dtype, tol, max_iter, sweeps) -> dict
        The sweeps of within2_reference.py with the subtracted level means KEPT as the tables a1 / a2 (every working value is formed
        from the row's original value, as on the device), in `dtype` arithmetic; beta from the projected columns; alpha', the
        one-factor effects of the projected columns (within_reference.py's alpha); then
            alpha_raw[g] = a1[g][y] - sum_j beta_j a1[g][j] + alpha'[g];    gamma_raw[l] = a2[l][y] - sum_j beta_j a2[l][j]
        and, in every component, c = gamma_raw at the lowest occupied code of key 2 in it: alpha = alpha_raw + c, gamma = gamma_raw - c.
        Levels are the distinct keys in ascending order.  "component" / "component2": the smallest level of key 1 of the component.
    dummy_effects(F, y, codes1, codes2) -> (alpha, gamma): the coefficients of within2_reference.dummy_design's regression in long
        double (gamma 0 at the dropped levels): the independent formula the restatement is checked against.
"""
from __future__ import annotations

import numpy as np

import within2_reference as w2r
import within_reference as wr

TRUTH_TOL = w2r.TRUTH_TOL
rel, budget = w2r.rel, w2r.budget


def ceil_log2(n: int) -> int:
    return int(n - 1).bit_length() if n > 1 else 0


class RoundCapError(RuntimeError):
    pass


def round_cap(n_nodes: int) -> int:
    """the rounds the library allows, the last one (which finds nothing to hook) included"""
    return 2 * ceil_log2(n_nodes) + 1


def hook_compress(i1, i2, n_a: int, n_b: int):
    i1, i2 = np.asarray(i1, dtype=np.int64), np.asarray(i2, dtype=np.int64) + n_a
    n_nodes = n_a + n_b
    label = np.arange(n_nodes, dtype=np.int64)
    for rounds in range(1, round_cap(n_nodes) + 2):
        if rounds > round_cap(n_nodes):
            raise RoundCapError(f"component labelling did not finish in {round_cap(n_nodes)} rounds")
        root = label.copy()
        assert np.array_equal(root[root], root)  # flat: every node points at its root
        ru, rv = root[i1], root[i2]
        m = ru != rv
        if not m.any():
            return label, rounds
        np.minimum.at(label, np.maximum(ru, rv)[m], np.minimum(ru, rv)[m])
        for _ in range(ceil_log2(n_nodes) + 1):
            nxt = label[label]
            if np.array_equal(nxt, label):
                break
            label = nxt
        else:
            raise AssertionError("the compression did not finish in ceil(log2 nodes) passes")


def propagate_rounds(i1, i2, n_a: int, n_b: int) -> int:
    """plain min-label propagation over the edges (no hooking of roots, no compression): the rounds it takes, the last one included"""
    i1, i2 = np.asarray(i1, dtype=np.int64), np.asarray(i2, dtype=np.int64) + n_a
    label = np.arange(n_a + n_b, dtype=np.int64)
    rounds = 0
    while True:
        rounds += 1
        before = label.copy()
        np.minimum.at(label, i1, before[i2])
        np.minimum.at(label, i2, before[i1])
        if np.array_equal(before, label):
            return rounds


def components(codes1, codes2):
    """(keys1, keys2, component1, component2, C, rounds): per distinct key, ascending, the smallest level of key 1 of its component"""
    u1, i1 = np.unique(np.asarray(codes1), return_inverse=True)
    u2, i2 = np.unique(np.asarray(codes2), return_inverse=True)
    label, rounds = hook_compress(i1.reshape(-1), i2.reshape(-1), len(u1), len(u2))
    lab1, lab2 = label[:len(u1)], label[len(u1):]
    assert np.all(lab2 < len(u1))
    return u1, u2, lab1, lab2, int((lab1 == np.arange(len(u1))).sum()), rounds


def scrambled_chain(levels: int = 2000, seed: int = 0):
    """`levels` levels of key 1, level g with rows in codes g and g + 1 of key 2 (two rows each), both numberings permuted at random
    and the rows shuffled: levels + (levels + 1) nodes, one component of diameter 2 * levels.  (k1, k2)"""
    rng = np.random.default_rng([2718, levels, seed])
    p1, p2 = rng.permutation(levels), rng.permutation(levels + 1)
    g = np.repeat(np.arange(levels), 4)
    l = g + np.tile(np.array([0, 1, 0, 1]), levels)
    rows = rng.permutation(len(g))
    return p1[g][rows].astype(np.int64), p2[l][rows].astype(np.int64)


def stagnant_tree():
    """8 levels of key 1 and 7 codes of key 2, 14 rows, one component: a tree of the levels whose numbering leaves a root that
    neither hooks nor is hooked into in round after round -- 6 rounds, one more than ceil(log2 15) + 1.  (k1, k2)"""
    k1 = np.array([0, 4, 1, 6, 2, 7, 4, 3, 3, 7, 6, 5, 5, 7], dtype=np.int64)
    k2 = np.repeat(np.arange(7, dtype=np.int64), 2)
    return k1, k2


def star(leaves: int = 9):
    """`leaves` codes of key 2, each shared by its own level of key 1 and by the LAST level of key 1, the centre.  Round 1 hooks every
    code into its own level; in round 2 the centre, the largest of leaves + 1 roots, hooks into level 0 and the other leaves neither
    hook nor are hooked into (leaves + 1 trees become leaves, not half); round 3 hooks them, round 4 finds nothing.  (k1, k2)"""
    k1 = np.stack([np.arange(leaves), np.full(leaves, leaves)], axis=1).reshape(-1).astype(np.int64)
    k2 = np.repeat(np.arange(leaves, dtype=np.int64), 2)
    return k1, k2


def disjoint_blocks(blocks: int = 500, seed: int = 0):
    """`blocks` components: block b has 3 levels of key 1 and 3 of key 2, joined in a path; numberings permuted, rows shuffled.  (k1, k2)"""
    rng = np.random.default_rng([31415, blocks, seed])
    p1, p2 = rng.permutation(3 * blocks), rng.permutation(3 * blocks)
    a = np.array([0, 0, 1, 1, 2])
    b = np.array([0, 1, 1, 2, 2])
    g = (3 * np.arange(blocks)[:, None] + a[None, :]).reshape(-1)
    l = (3 * np.arange(blocks)[:, None] + b[None, :]).reshape(-1)
    rows = rng.permutation(len(g))
    return p1[g][rows].astype(np.int64), p2[l][rows].astype(np.int64)


def tables(Z, codes1, codes2, dtype=np.longdouble, tol=TRUTH_TOL, max_iter=10_000, sweeps=None):
    """(Z~, a1, a2, n_iter, deltas): the alternating sweeps with the subtracted means kept as tables, in `dtype` arithmetic"""
    Z0 = np.array(Z, dtype=dtype)
    s = np.std(np.asarray(Z, dtype=np.longdouble), axis=0).astype(dtype)  # only a scale
    s = np.where(s > 0, s, dtype(1))
    g1, g2 = wr._groups(codes1), wr._groups(codes2)
    c1, c2 = g1[3].astype(dtype)[:, None], g2[3].astype(dtype)[:, None]
    a1, a2 = np.zeros((len(g1[1]), Z0.shape[1]), dtype=dtype), np.zeros((len(g2[1]), Z0.shape[1]), dtype=dtype)
    work = lambda: (Z0 - a1[g1[2]]) - a2[g2[2]]  # noqa: E731
    deltas = []
    for it in range(sweeps if sweeps is not None else max_iter):
        a1 = a1 + w2r._level_sums(work(), g1) / c1
        m2 = w2r._level_sums(work(), g2) / c2
        a2 = a2 + m2
        deltas.append(float(np.max(np.abs(m2) / s[None, :])))
        if sweeps is None and deltas[-1] <= tol:
            break
    else:
        if sweeps is None:
            raise w2r.ConvergenceError(f"did not converge in {max_iter} sweeps: delta = {deltas[-1]:.3e}")
    return work(), a1, a2, len(deltas), deltas


def effects(F, y, codes1, codes2, dtype=np.longdouble, tol=TRUTH_TOL, max_iter=10_000, sweeps=None) -> dict:
    X, yl = np.asarray(F).astype(dtype), np.asarray(y).astype(dtype)
    n, p = X.shape
    Zt, a1, a2, n_iter, deltas = tables(np.column_stack([X, yl]), codes1, codes2, dtype, tol, max_iter, sweeps)
    Xt, yt = Zt[:, :p], Zt[:, p]
    beta, _ = wr._solve(Xt.T @ Xt, Xt.T @ yt, dtype)
    order, starts, idx, counts = wr._groups(codes1)
    cnt = counts.astype(dtype)
    mx = np.add.reduceat(Xt[order], starts, axis=0) / cnt[:, None]
    my = np.add.reduceat(yt[order], starts) / cnt
    alpha1 = my - mx @ beta  # the one-factor effects of the projected columns
    e = (yt - my[idx]) - (Xt - mx[idx]) @ beta
    alpha_raw = a1[:, p] - a1[:, :p] @ beta + alpha1
    gamma_raw = a2[:, p] - a2[:, :p] @ beta
    keys1, keys2, lab1, lab2, n_comp, rounds = components(codes1, codes2)
    ref = np.full(len(keys1), len(keys2), dtype=np.int64)
    np.minimum.at(ref, lab2, np.arange(len(keys2)))  # the lowest occupied code of key 2 in every component, at the component's root
    c1, c2 = gamma_raw[ref[lab1]], gamma_raw[ref[lab2]]
    return {"beta": beta, "resid": e, "effects": alpha_raw + c1, "effects2": gamma_raw - c2, "effect_keys": keys1, "effect_keys2": keys2,
            "component": lab1, "component2": lab2, "reference_levels": ref[np.flatnonzero(lab1 == np.arange(len(keys1)))],
            "n_components": n_comp, "n_graph_rounds": rounds, "n_iter": n_iter, "deltas": deltas}


def dummy_effects(F, y, codes1, codes2, dtype=np.longdouble):
    """(alpha [G1], gamma [G2]) of the explicit regression on [F | a dummy per level of key 1 | a dummy per level of key 2 less the
    first level of key 2 in every component], solved by orthogonalisation, dummies first, as within2_reference.dummy_report does"""
    p = np.asarray(F).shape[1]
    D = w2r.dummy_design(F, codes1, codes2, dtype)
    g1, g2 = len(np.unique(codes1)), len(np.unique(codes2))
    X, yl = np.column_stack([D[:, p:], D[:, :p]]), np.asarray(y).astype(dtype)
    q = X.shape[1]
    Q, R = w2r._qr(X)
    b = Q.T @ yl
    coef = np.zeros(q, dtype=dtype)
    for j in range(q - 1, -1, -1):
        coef[j] = (b[j] - R[j, j + 1:] @ coef[j + 1:]) / R[j, j]
    _, _, _, lab2, _, _ = components(codes1, codes2)
    dropped = np.array([np.flatnonzero(lab2 == lab2[l])[0] == l for l in range(g2)])
    gamma = np.zeros(g2, dtype=dtype)
    gamma[~dropped] = coef[g1:q - p]
    return coef[:g1], gamma, coef[q - p:]
