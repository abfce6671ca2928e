"""The penalised GLM fits restated in NumPy float64 (csrc/grouped_irls.hip, PEN = 1; capi_models.hpp for one model), batched across
groups, and a solver-independent optimality check of their objective.

For a group of n rows, coefficients beta with features j < p and an optional unpenalised bias last:

    F(beta) = (1/n) sum_i l(y_i, eta_i) + (l2 / 2) sum_{j<p} beta_j^2 + l1 sum_{j<p} |beta_j|,      eta = X beta (+ bias)

with l the unit-dispersion negative log-likelihood of the family's canonical link.  `fit` is the device algorithm: the IRLS
iteration of the unpenalised fit (same start, same stopping rule), each step the minimiser of
1/2 beta'G beta - c'beta + (n l2 / 2)|beta_f|^2 + n l1 |beta_f|_1 over G = X'WX, c = X'Wz -- one solve when l1 <= 0, else a
covariance-update coordinate descent warm-started from the previous step, whose sweeps end at a largest move below `inner` * tol
or after `sweep_cap` sweeps.  `kkt` measures how far a coefficient vector is from a minimiser of F, in np.longdouble from the frame,
with no reference to any solver.  `beta_star` is `fit` driven to tol 1e-13 with inner constant 0.01: the point the device is held
against."""
import numpy as np

INNER = 0.1        # kGiCdInner
SWEEP_CAP = 1000   # kGiCdSweeps


def _link(family, mu):
    if family == "poisson":
        return np.log(mu)
    if family == "binomial":
        return np.log(mu / (1.0 - mu))
    if family == "gamma":
        return 1.0 / mu
    return mu


def _inv(family, eta):
    if family == "poisson":
        return np.exp(eta)
    if family == "binomial":
        e = np.exp(eta)
        return e / (1.0 + e)
    if family == "gamma":
        return 1.0 / eta
    return eta


def _deriv(family, mu):
    if family == "poisson":
        return 1.0 / mu
    if family == "binomial":
        return 1.0 / (mu * (1.0 - mu))
    if family == "gamma":
        return -((1.0 / mu) ** 2)
    return np.ones_like(mu)


def _var(family, mu):
    if family == "poisson":
        return mu
    if family == "binomial":
        return mu * (1.0 - mu)
    if family == "gamma":
        return mu * mu
    return np.ones_like(mu)


def _padded(X, y, off, bias):
    """[G, nmax, p'] features (+ a ones column), [G, nmax] y and the row mask; padding rows are zero"""
    off = np.asarray(off, dtype=np.int64)
    sizes = np.diff(off)
    G, nmax, p = len(sizes), int(sizes.max()), X.shape[1]
    mask = np.arange(nmax)[None, :] < sizes[:, None]
    Xp = np.zeros((G, nmax, p + int(bias)))
    yp = np.zeros((G, nmax))
    gid, pos = np.repeat(np.arange(G), sizes), np.arange(len(y)) - np.repeat(off[:-1], sizes)
    Xp[gid, pos, :p] = X
    if bias:
        Xp[gid, pos, p] = 1.0
    yp[gid, pos] = y
    return Xp, yp, mask, sizes


def _cd(Gm, c, beta, nl1, nl2, p, eps, sweep_cap, live):
    """coordinate descent on every live group's system in lockstep; a group leaves when its sweep's largest move is below eps (or is
    NaN).  Returns the sweeps each group ran."""
    pp = Gm.shape[1]
    r = c - np.einsum("gjk,gj->gk", Gm, beta)  # (row j of G for column j, as the kernel reads it)
    sweeps = np.zeros(len(beta), dtype=np.int64)
    act = live.copy()
    diag = np.einsum("gjj->gj", Gm)
    for _ in range(sweep_cap):
        if not act.any():
            break
        moved = np.zeros(len(beta))
        for j in range(pp):
            bj = beta[:, j]
            u = r[:, j] + diag[:, j] * bj
            if j < p:
                mag = np.abs(u) - nl1
                with np.errstate(all="ignore"):
                    nb = np.where(mag > 0.0, np.copysign(mag, u) / (diag[:, j] + nl2), 0.0)
            else:
                with np.errstate(all="ignore"):
                    nb = u / diag[:, j]
            delta = np.where(act, nb - bj, 0.0)
            r -= delta[:, None] * Gm[:, j, :]
            beta[:, j] = np.where(delta != 0.0, nb, bj)  # (a coordinate that does not move keeps its bits)
            d = np.abs(delta)
            moved = np.where(np.isnan(d), np.nan, np.maximum(moved, d))
        sweeps += act
        act = act & (moved >= eps)  # (False for a NaN)
    return sweeps


def fit(X, y, off, family, bias, l1=0.0, l2=0.0, tol=1e-8, max_iter=100, inner=INNER, sweep_cap=SWEEP_CAP):
    """(coeffs [G, p'] bias last, n_iter [G], inner sweeps [G]) of the penalised fit of every group; a group with fewer rows than
    coefficients is NaN with n_iter 0; a NaN coefficient ends a group at max_iter, as on the device."""
    X = np.asarray(X, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    p = X.shape[1]
    Xp, yp, mask, sizes = _padded(X, y, off, bias)
    G, pp = len(sizes), p + int(bias)
    l1, l2 = max(float(l1), 0.0), max(float(l2), 0.0)
    n = sizes.astype(np.float64)
    beta = np.zeros((G, pp))
    n_iter = np.zeros(G, dtype=np.int64)
    sweeps = np.zeros(G, dtype=np.int64)
    short = sizes < pp
    live = ~short
    ymean = yp.sum(axis=1) / np.maximum(n, 1.0)
    pen_diag = np.zeros((G, pp))
    pen_diag[:, :p] = (n * l2)[:, None]
    for it in range(1, max_iter + 1):
        if not live.any():
            break
        with np.errstate(all="ignore"):
            if it == 1:
                mu = (yp + 0.5) * 0.5 if family == "binomial" else (yp + ymean[:, None]) * 0.5
                eta = _link(family, mu)
            else:
                eta = np.einsum("gnk,gk->gn", Xp, beta)
                mu = _inv(family, eta)
            d = _deriv(family, mu)
            w = np.where(mask, 1.0 / (d * d * _var(family, mu)), 0.0)
            wz = np.where(mask, w * (eta + d * (yp - mu)), 0.0)
            Gm = np.einsum("gni,gn,gnj->gij", Xp, w, Xp)
            c = np.einsum("gni,gn->gi", Xp, wz)
            new = beta.copy()
            if l1 > 0.0:
                sweeps += _cd(Gm, c, new, (n * l1), (n * l2), p, inner * tol, sweep_cap, live)
            else:
                A = Gm + pen_diag[:, :, None] * np.eye(pp)[None]
                ok = live & np.isfinite(A).all(axis=(1, 2)) & np.isfinite(c).all(axis=1)
                sol = np.full((G, pp), np.nan)
                for g in np.flatnonzero(ok):
                    try:
                        sol[g] = np.linalg.solve(A[g], c[g])
                    except np.linalg.LinAlgError:
                        pass
                new = np.where(live[:, None], sol, beta)
        diff = np.abs(beta - new).max(axis=1)
        nanb = np.isnan(new).any(axis=1)
        beta = np.where(live[:, None], new, beta)
        n_iter[live] = it
        n_iter[live & nanb] = max_iter
        # (a penalised fit does not stop on its first step: that system is built at the starting mu, not at beta = 0)
        live = live & ~nanb & ~((diff < tol) & (it > 1 or (l1 == 0.0 and l2 == 0.0)))
    beta[short] = np.nan
    return beta, n_iter, sweeps


def beta_star(X, y, off, family, bias, l1=0.0, l2=0.0):
    """the minimiser of F the device is held against: `fit` at tol 1e-13 with inner constant 0.01"""
    return fit(X, y, off, family, bias, l1, l2, tol=1e-13, max_iter=200, inner=0.01, sweep_cap=100000)[0]


def kkt(X, y, off, family, bias, l1, l2, coeffs):
    """[G]: the largest violation of F's optimality conditions at `coeffs`, np.longdouble from the frame.  With g the mean gradient
    (1/n) X'(dl/deta):  feature, beta_j != 0: |g_j + l2 beta_j + l1 sign beta_j|;  feature, beta_j = 0: max(|g_j| - l1, 0);
    bias: |g_b|."""
    L = np.longdouble
    p = X.shape[1]
    Xp, yp, mask, sizes = _padded(np.asarray(X, dtype=np.float64), np.asarray(y, dtype=np.float64), off, bias)
    Xp, yp, b = Xp.astype(L), yp.astype(L), np.asarray(coeffs, dtype=np.float64).astype(L)
    l1, l2 = L(max(float(l1), 0.0)), L(max(float(l2), 0.0))
    eta = np.einsum("gnk,gk->gn", Xp, b)
    with np.errstate(all="ignore"):
        if family == "binomial":
            dl = 1 / (1 + np.exp(-eta)) - yp
        elif family == "poisson":
            dl = np.exp(eta) - yp
        elif family == "gamma":
            dl = yp - 1 / eta
        else:
            dl = eta - yp
    dl = np.where(mask, dl, L(0))
    g = np.einsum("gnk,gn->gk", Xp, dl) / sizes.astype(L)[:, None]
    gf, bf = g[:, :p], b[:, :p]
    res = np.where(bf != 0, np.abs(gf + l2 * bf + l1 * np.sign(bf)), np.maximum(np.abs(gf) - l1, 0))
    out = res.max(axis=1)
    if bias:
        out = np.maximum(out, np.abs(g[:, p]))
    return out.astype(np.float64)


def mean_gradient(X, y, off, family, bias, coeffs):
    """[G, p]: |g_j| of the features at `coeffs` (np.longdouble): how close a zero coefficient sits to the edge |g_j| = l1"""
    L = np.longdouble
    p = X.shape[1]
    Xp, yp, mask, sizes = _padded(np.asarray(X, dtype=np.float64), np.asarray(y, dtype=np.float64), off, bias)
    Xp, yp, b = Xp.astype(L), yp.astype(L), np.asarray(coeffs, dtype=np.float64).astype(L)
    eta = np.einsum("gnk,gk->gn", Xp, b)
    mu = {"binomial": lambda e: 1 / (1 + np.exp(-e)), "poisson": np.exp, "gamma": lambda e: 1 / e}.get(family, lambda e: e)(eta)
    dl = np.where(mask, (yp - mu) if family == "gamma" else (mu - yp), L(0))
    return np.abs(np.einsum("gnk,gn->gk", Xp, dl) / sizes.astype(L)[:, None])[:, :p].astype(np.float64)


def inv_link(family, eta):
    return _inv(family, eta)
