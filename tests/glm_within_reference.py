"""The fixed-effects GLM restated in NumPy (TEST INFRASTRUCTURE ONLY; tests/test_glm_within_cpu.py, tests/test_glm_within_gpu.py): the
definitions of include/pds_lstsq.h (pds_glm_within_*) in np.longdouble (the truth the tests measure against), or with
dtype=np.float64 / np.float32 the same code in the narrower format, whose distance from the longdouble result is what a budget is made
of.  On top of glm_report_reference.py (_inv_link, _link, _dlink, _var, unit_deviance, spd_inverse).  Nothing follows the device's
operation order.

    kept(family, y, codes, pw)                -> keys (ascending), g (row -> index into keys), drop [G], used [n]
    fit(X, y, codes, family, pw, o, tol, max_iter, dtype)
        the DEFINITION, stopping rule included: beta [p], alpha [G] (NaN for a dropped group), n_iter, converged, counts
    dummy_mle(X, y, codes, family, pw, o)     -> beta, alpha: independently, the maximum-likelihood fit of the design with one dummy
        column per kept group, in longdouble, iterated until nothing moves
    report_at(X, y, codes, family, beta, alpha, kind, pw, o, dtype)
        the report fields at coefficients the caller BRINGS.  The weights of W_xx and of the group means are taken at the brought
        (beta, alpha): at a fixed point of the iteration that is the "last W_xx" of the definition (the tests run the device to a
        tolerance at which the last step is below the rounding the budgets measure).
"""
import math

import numpy as np

import glm_report_reference as rr

KINDS = ("se", "cluster", "cluster0")


def _gsum(v, g, G):
    """sums of the rows of v over the groups g, in v's dtype (np.bincount would fall back to float64)"""
    out = np.zeros((G,) + v.shape[1:], dtype=v.dtype)
    np.add.at(out, g, v)
    return out


def kept(family, y, codes, pw=None):
    fam = rr.FAMILY_ID[family]
    y = np.asarray(y, dtype=np.float64)
    keys, g = np.unique(np.asarray(codes), return_inverse=True)
    g = g.reshape(-1)
    G = len(keys)
    cnt = np.ones(len(y), dtype=bool) if pw is None else np.asarray(pw) > 0
    has = lambda m: np.bincount(g[m], minlength=G) > 0  # noqa: E731
    drop = ~has(cnt)
    if fam == 1:
        drop |= ~has(cnt & (y != 0))
    if fam == 2:
        drop |= ~has(cnt & (y != 0)) | ~has(cnt & (y != 1))
    return keys, g, drop, cnt & ~drop[g]


def _used_frame(X, y, codes, family, pw, o, dtype):
    keys, g, drop, used = kept(family, y, codes, pw)
    Xv = np.asarray(X).astype(dtype)[used]
    yv = np.asarray(y).astype(dtype)[used]
    pv = np.ones(int(used.sum()), dtype=dtype) if pw is None else np.asarray(pw).astype(dtype)[used]
    ov = np.zeros(int(used.sum()), dtype=dtype) if o is None else np.asarray(o).astype(dtype)[used]
    kidx = np.cumsum(~drop) - 1  # group -> index among the kept groups
    return keys, g, drop, used, Xv, yv, pv, ov, kidx[g[used]], int((~drop).sum())


def _start(fam, yv, pv, dtype):
    if fam == 2:
        return (yv + dtype(0.5)) / 2
    return (yv + (pv * yv).sum() / pv.sum()) / 2


def fit(X, y, codes, family, pw=None, o=None, tol=1e-10, max_iter=100, dtype=np.longdouble):
    fam = rr.FAMILY_ID[family]
    keys, g, drop, used, Xv, yv, pv, ov, gu, Gk = _used_frame(X, y, codes, family, pw, o, dtype)
    p = Xv.shape[1]
    mu = _start(fam, yv, pv, dtype)
    eta = rr._link(fam, mu)
    beta = np.zeros(p, dtype=dtype)
    alpha_k = np.zeros(Gk, dtype=dtype)
    n_iter, converged = 0, False
    while n_iter < max_iter and not converged:
        d = rr._dlink(fam, mu)
        w = pv / (d * d * rr._var(fam, mu))
        z = (eta - ov) + d * (yv - mu)
        A = np.column_stack([Xv, z])
        m = _gsum(A * w[:, None], gu, Gk) / _gsum(w, gu, Gk)[:, None]
        Cc = A - m[gu]
        W = Cc.T @ (Cc * w[:, None])
        inv = rr.spd_inverse(W[:p, :p], dtype)
        beta_new = (inv @ W[:p, p]).astype(dtype)
        alpha_k = m[:, p] - m[:, :p] @ beta_new
        eta = alpha_k[gu] + Xv @ beta_new + ov
        mu = rr._inv_link(fam, eta)
        delta = float(np.max(np.abs(beta_new - beta)))
        beta = beta_new
        n_iter += 1
        converged = delta < tol
    alpha = np.full(len(keys), np.nan, dtype=dtype)
    alpha[~drop] = alpha_k
    return {"beta": beta, "alpha": alpha, "keys": keys, "n_iter": n_iter, "converged": converged, "n_rows_used": int(used.sum()),
            "n_groups": Gk, "n_groups_dropped": int(drop.sum()), "df_resid": int(used.sum()) - Gk - p, "drop": drop, "used": used}


def dummy_mle(X, y, codes, family, pw=None, o=None, max_iter=200, dtype=np.longdouble):
    fam = rr.FAMILY_ID[family]
    keys, g, drop, used, Xv, yv, pv, ov, gu, Gk = _used_frame(X, y, codes, family, pw, o, dtype)
    p = Xv.shape[1]
    D = np.zeros((len(yv), Gk), dtype=dtype)
    D[np.arange(len(yv)), gu] = 1
    Z = np.column_stack([Xv, D])
    mu = _start(fam, yv, pv, dtype)
    eta = rr._link(fam, mu)
    b = np.zeros(p + Gk, dtype=dtype)
    for _ in range(max_iter):
        d = rr._dlink(fam, mu)
        w = pv / (d * d * rr._var(fam, mu))
        z = (eta - ov) + d * (yv - mu)
        info = Z.T @ (Z * w[:, None])
        b_new = rr.spd_inverse(info, dtype) @ (Z.T @ (w * z))
        eta = Z @ b_new + ov
        mu = rr._inv_link(fam, eta)
        move = float(np.max(np.abs(b_new - b)))
        b = b_new
        if move < max(1e-17, 4 * float(np.finfo(dtype).eps)) * (1 + float(np.max(np.abs(b)))) or not np.isfinite(move):
            break  # (nothing moves any more, to the rounding of the format)
    alpha = np.full(len(keys), np.nan, dtype=dtype)
    alpha[~drop] = b[p:]
    return {"beta": b[:p], "alpha": alpha, "keys": keys, "drop": drop, "used": used}


def report_at(X, y, codes, family, beta, alpha, kind, pw=None, o=None, dtype=np.longdouble):
    assert kind in KINDS
    fam = rr.FAMILY_ID[family]
    keys, g, drop, used, Xv, yv, pv, ov, gu, Gk = _used_frame(X, y, codes, family, pw, o, dtype)
    n, p = Xv.shape
    b = np.asarray(beta).astype(dtype)
    a = np.asarray(alpha).astype(dtype)[~drop]
    eta = a[gu] + Xv @ b + ov
    mu = rr._inv_link(fam, eta)
    d = rr._dlink(fam, mu)
    v = rr._var(fam, mu)
    w = pv / (d * d * v)
    mx = _gsum(Xv * w[:, None], gu, Gk) / _gsum(w, gu, Gk)[:, None]
    Xc = Xv - mx[gu]
    inv = rr.spd_inverse(Xc.T @ (Xc * w[:, None]), dtype)
    deviance = (pv * rr.unit_deviance(fam, yv, mu)).sum()
    pearson = (pv * (yv - mu) ** 2 / v).sum()
    df = n - Gk - p
    phi = dtype(1) if fam in (1, 2) else pearson / dtype(df)
    r = pv * (yv - mu) / (v * d)
    if kind == "se":
        cov = phi * inv
    else:
        S = _gsum(Xc * r[:, None], gu, Gk)
        c = dtype(1) if kind == "cluster0" else (dtype(Gk) / dtype(Gk - 1)) * (dtype(n - 1) / dtype(n - p - 1))
        cov = c * (inv @ (S.T @ S) @ inv)
    cov = (cov + cov.T) / 2
    se = np.sqrt(np.diag(cov))
    z = b / se
    pval = rr._erfc(np.abs(z.astype(np.float64)) / math.sqrt(2.0))
    # mu of every row of a kept group (the zero-weight ones too), NaN on the rows of dropped groups
    Xa = np.asarray(X).astype(dtype)
    oa = np.zeros(len(Xa), dtype=dtype) if o is None else np.asarray(o).astype(dtype)
    a_all = np.asarray(alpha).astype(dtype)
    pred = np.full(len(Xa), np.nan, dtype=dtype)
    rows = ~drop[g]
    pred[rows] = rr._inv_link(fam, a_all[g[rows]] + Xa[rows] @ b + oa[rows])
    return {"std_err": se, "z": z, "p": pval, "lo": b - dtype(rr.Z975) * se, "hi": b + dtype(rr.Z975) * se, "cov": cov, "deviance": deviance,
            "pearson_chi2": pearson, "dispersion": phi, "df_resid": df, "n_rows_used": n, "n_groups": Gk, "n_groups_dropped": int(drop.sum()),
            "pred": pred, "score_x": Xv * r[:, None], "score_r": r, "g_used": gu, "drop": drop, "used": used}
