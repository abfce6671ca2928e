"""
The accelerated (Irons-Tuck) iteration of the two-factor fixed-effects regression, restated in NumPy in the device's TABLE arithmetic
(TEST INFRASTRUCTURE ONLY): the definition of include/pds_lstsq.h (pds_lin_reg_within2_*, ACCELERATION), line by line, for any dtype.

    tables(Z, codes1, codes2, dtype, tol, max_iter, sweeps, accel) -> (Z~, a1, a2, n_iter, deltas)
    fit(F, y, codes1, codes2, std_err, dtype, tol, max_iter, sweeps, accel) -> dict

The state is the two tables of subtracted level means a1 / a2; a row's working value is (w - a1[g1]) - a2[g2], formed from its original
value.  A SWEEP:  a1 += mean1(work);  m2 = mean2(work);  a2 += m2;  delta = max_j max_level |m2| / s_j  -- within2_reference.demean's
sweep with the subtractions kept as tables (within2_effects_reference.tables).  accel=False runs sweeps until delta <= tol.
accel=True runs CYCLES of two sweeps:
    1. sweep, D1 = its m2; delta <= tol: stop.        2. sweep, D2 = its m2; delta <= tol: stop.
    3. per column j over the occupied levels of factor 2: d = D2 - D1, c_j = sum D2 d / sum d^2, a2[:, j] -= c_j D2[:, j];
       c_j = 0 when the denominator is 0 or a sum or the quotient is not finite.
Only a2 is extrapolated (the next sweep's factor-1 step rebuilds a1: a1 + mean1(w - a1 - a2) does not depend on the old a1); only a
sweep's delta is looked at; n_iter, max_iter and `sweeps` count sweeps and nothing else, and no extrapolation follows the last sweep
allowed.  `sweeps=k` runs exactly k sweeps whatever delta says (with the extrapolations that fall between them).
fit() is within2_reference.report and within2_effects_reference.effects on the columns and tables this iteration ends with: every
report field, pred / resid, and the effects under the library's normalisation.  The TRUTH stays within2_reference's long double
plain run at TRUTH_TOL (the projection does not depend on the road to it).
"""
from __future__ import annotations

import numpy as np

import within2_effects_reference as fxr
import within2_reference as w2r
import within_reference as wr

TRUTH_TOL = w2r.TRUTH_TOL
rel, budget = w2r.rel, w2r.budget
FIELDS, ROW_FIELDS, SE_TYPES = w2r.FIELDS, w2r.ROW_FIELDS, w2r.SE_TYPES
EFFECT_FIELDS = ("effects", "effects2")


def coefficients(D1, D2, dtype):
    """c_j of one extrapolation from the means of the two sweeps of a cycle (occupied levels x columns)"""
    d = D2 - D1
    num, den = (D2 * d).sum(axis=0), (d * d).sum(axis=0)
    with np.errstate(all="ignore"):
        c = num / den
    ok = (den != 0) & np.isfinite(num) & np.isfinite(den) & np.isfinite(c)
    return np.where(ok, c, dtype(0)).astype(dtype)


def tables(Z, codes1, codes2, dtype=np.longdouble, tol=TRUTH_TOL, max_iter=10_000, sweeps=None, accel=True):
    """(Z~, a1, a2, n_iter, deltas): the iteration in `dtype` arithmetic; a2 has one row per OCCUPIED level of factor 2, ascending"""
    Z0 = np.array(Z, dtype=dtype)
    s = np.std(np.asarray(Z, dtype=np.longdouble), axis=0).astype(dtype)  # only a scale
    s = np.where(s > 0, s, dtype(1))
    g1, g2 = wr._groups(codes1), wr._groups(codes2)
    c1, c2 = g1[3].astype(dtype)[:, None], g2[3].astype(dtype)[:, None]
    a1, a2 = np.zeros((len(g1[1]), Z0.shape[1]), dtype=dtype), np.zeros((len(g2[1]), Z0.shape[1]), dtype=dtype)
    work = lambda: (Z0 - a1[g1[2]]) - a2[g2[2]]  # noqa: E731
    limit = sweeps if sweeps is not None else max_iter
    deltas, D1 = [], None
    while len(deltas) < limit:
        a1 = a1 + w2r._level_sums(work(), g1) / c1
        m2 = w2r._level_sums(work(), g2) / c2
        a2 = a2 + m2
        deltas.append(float(np.max(np.abs(m2) / s[None, :])))
        if sweeps is None and deltas[-1] <= tol:
            break
        if accel and len(deltas) % 2 == 0 and len(deltas) < limit:
            a2 = a2 - coefficients(D1, m2, dtype)[None, :] * m2
        D1 = m2
    else:
        if sweeps is None:
            raise w2r.ConvergenceError(f"did not converge in {max_iter} sweeps: delta = {deltas[-1]:.3e}")
    return work(), a1, a2, len(deltas), deltas


def fit(F, y, codes1, codes2, std_err="se", dtype=np.longdouble, tol=TRUTH_TOL, max_iter=10_000, sweeps=None, accel=True) -> dict:
    """the report of within2_reference.report and the effects of within2_effects_reference.effects from this iteration's tables"""
    X, yl = np.asarray(F).astype(dtype), np.asarray(y).astype(dtype)
    n, p = X.shape
    Zt, a1, a2, n_iter, deltas = tables(np.column_stack([X, yl]), codes1, codes2, dtype, tol, max_iter, sweeps, accel)
    G1, G2, C = w2r.components(codes1, codes2)
    A = G1 + G2 - C
    Xt, yt = Zt[:, :p], Zt[:, p]
    beta, inv = wr._solve(Xt.T @ Xt, Xt.T @ yt, dtype)
    e = yt - Xt @ beta
    sse = (e * e).sum()
    order, starts, idx, counts = wr._groups(codes1)
    S = np.add.reduceat((Xt * e[:, None])[order], starts, axis=0)
    v0 = np.diag(inv @ (S.T @ S) @ inv)
    K = p + 1 + (A - G1)
    cf = (dtype(G1) / dtype(max(G1 - 1, 1))) * (dtype(n - 1) / dtype(n - K))
    one = dtype(1)
    r2 = one - sse / (yt * yt).sum()
    out = {"beta": beta, "se_all": {"se": np.sqrt(sse / dtype(n - p - A) * np.diag(inv)), "cluster0": np.sqrt(v0), "cluster": np.sqrt(v0 * cf)},
           "pred": yl - e, "resid": e, "sse": sse, "r2": r2, "adj_r2": one - (one - r2) * dtype(n - A) / dtype(n - A - p),
           "r2_overall": one - sse / ((yl - yl.mean()) ** 2).sum(), "n_groups": G1, "n_groups2": G2, "n_components": C, "df_se": n - p - A,
           "n_iter": n_iter, "deltas": deltas}
    # the effects (within2_effects_reference.effects, from these tables)
    cnt = counts.astype(dtype)
    mx = np.add.reduceat(Xt[order], starts, axis=0) / cnt[:, None]
    my = np.add.reduceat(yt[order], starts) / cnt
    alpha_raw = a1[:, p] - a1[:, :p] @ beta + (my - mx @ beta)
    gamma_raw = a2[:, p] - a2[:, :p] @ beta
    keys1, keys2, lab1, lab2, n_comp, rounds = fxr.components(codes1, codes2)
    ref = np.full(len(keys1), len(keys2), dtype=np.int64)
    np.minimum.at(ref, lab2, np.arange(len(keys2)))
    out["effects"], out["effects2"] = alpha_raw + gamma_raw[ref[lab1]], gamma_raw - gamma_raw[ref[lab2]]
    return w2r.select(out, std_err)
