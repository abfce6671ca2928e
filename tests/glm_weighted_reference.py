"""The grouped GLM fit with prior weights and an offset per row (csrc/grouped_irls.hip, the weighted / offset form) restated in NumPy
float64, one group at a time.

    eta_i = x_i . beta + o_i,   mu_i = g^-1(eta_i),   w_i = pw_i / (g'(mu_i)^2 V(mu_i)),   z_i = (eta_i - o_i) + g'(mu_i) (y_i - mu_i)
    start: mu = (y + 0.5) / 2 (binomial), (y + ybar) / 2 otherwise with ybar = sum pw y / sum pw; eta = g(mu); beta = 0
    step:  beta_new = argmin sum_i w_i (z_i - x_i . beta)^2   (a least-squares solve of the sqrt(w)-scaled rows, not the device's
           Gram matrix + pivoted QR: the restatement shares the definition with the device, not its arithmetic)
    stop:  max_j |beta_j - beta_new_j| < tol, or max_iter iterations; a NaN coefficient ends the fit at max_iter
    null:  fewer than p' rows of positive weight, or any weight negative or not finite: NaN coefficients, 0 iterations

Rows of weight 0 are dropped before anything is computed: they contribute nothing and do not count.  From the second iteration on
the linear part of z is x . beta itself, as on the device.  `pred` is g^-1(x . beta + o) of every row, rows of weight 0 included.
"""
import numpy as np


def link(family, mu):
    if family == "poisson":
        return np.log(mu)
    if family == "binomial":
        return np.log(mu / (1.0 - mu))
    if family == "gamma":
        return 1.0 / mu
    return mu


def inv(family, eta):
    if family == "poisson":
        return np.exp(eta)
    if family == "binomial":
        e = np.exp(eta)
        return e / (1.0 + e)
    if family == "gamma":
        return 1.0 / eta
    return eta


def deriv(family, mu):
    if family == "poisson":
        return 1.0 / mu
    if family == "binomial":
        return 1.0 / (mu * (1.0 - mu))
    if family == "gamma":
        return -((1.0 / mu) ** 2)
    return np.ones_like(mu)


def var(family, mu):
    if family == "poisson":
        return mu
    if family == "binomial":
        return mu * (1.0 - mu)
    if family == "gamma":
        return mu * mu
    return np.ones_like(mu)


def is_null_by_weights(pw, pp):
    """the weight rule of a group: (null, rows of positive weight)"""
    pw = np.asarray(pw, dtype=np.float64)
    bad = bool((~np.isfinite(pw)).any() or (pw < 0).any())
    n_pos = int((pw > 0).sum()) if not bad else 0
    return bad or n_pos < pp, n_pos


def fit_group(X, y, pw, o, family, bias, tol=1e-8, max_iter=100):
    """(coefficients [p'] bias last, iterations) of one group; pw / o: arrays or None (weights 1 / offsets 0)"""
    X = np.asarray(X, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    n, p = X.shape
    pp = p + int(bool(bias))
    pw = np.ones(n) if pw is None else np.asarray(pw, dtype=np.float64)
    o = np.zeros(n) if o is None else np.asarray(o, dtype=np.float64)
    null, _ = is_null_by_weights(pw, pp)
    if null:
        return np.full(pp, np.nan), 0
    keep = pw > 0
    Z = np.column_stack([X, np.ones(n)]) if bias else X
    Z, y, pw, o = Z[keep], y[keep], pw[keep], o[keep]
    with np.errstate(all="ignore"):
        ybar = np.sum(pw * y) / np.sum(pw)
        mu = (y + 0.5) * 0.5 if family == "binomial" else (y + ybar) * 0.5
        lin = link(family, mu) - o
        beta = np.zeros(pp)
        it = 0
        while it < max_iter:
            it += 1
            if it > 1:
                lin = Z @ beta
                mu = inv(family, lin + o)
            d = deriv(family, mu)
            w = pw / (d * d * var(family, mu))
            z = lin + d * (y - mu)
            if not (np.isfinite(w).all() and np.isfinite(z).all()):
                return np.full(pp, np.nan), max_iter
            s = np.sqrt(w)
            new = np.linalg.lstsq(Z * s[:, None], z * s, rcond=None)[0]
            if np.isnan(new).any():
                return new, max_iter
            done = bool(np.max(np.abs(beta - new)) < tol)
            beta = new
            if done:
                break
    return beta, it


def fit(X, y, off, pw, o, family, bias, tol=1e-8, max_iter=100):
    """every group of the frame: (coeffs [G, p'], n_iter [G])"""
    G, pp = len(off) - 1, X.shape[1] + int(bool(bias))
    co, it = np.full((G, pp), np.nan), np.zeros(G, dtype=np.int64)
    for g in range(G):
        a, b = int(off[g]), int(off[g + 1])
        if b - a < pp:
            continue
        co[g], it[g] = fit_group(X[a:b], y[a:b], None if pw is None else pw[a:b], None if o is None else o[a:b], family, bias, tol, max_iter)
    return co, it


def score(X, y, pw, o, beta, family, bias):
    """the weighted score X' diag(pw / (g' V)) (y - mu) at beta: zero at the maximum of the weighted likelihood, whatever found it"""
    n = len(y)
    Z = np.column_stack([X, np.ones(n)]) if bias else np.asarray(X)
    pw = np.ones(n) if pw is None else pw
    o = np.zeros(n) if o is None else o
    mu = inv(family, Z @ beta + o)
    return Z.T @ (pw * (y - mu) / (deriv(family, mu) * var(family, mu)))


# --------------------------------------------------------------------------------------------------------- the weighted report
# The report of tests/glm_report_reference.py with prior weights pw and an offset o, in float64 and in longdouble (its helpers):
#   mu = g^-1(x . beta + o); I = sum pw w~ x x', w~ = 1 / (g'^2 V); pearson_chi2 = sum pw (y - mu)^2 / V; deviance = sum pw d_i;
#   df_resid = n+ - p'; dispersion 1 (poisson, binomial) or pearson_chi2 / df_resid; cov = dispersion I^-1; se, z, p, interval from
#   those; null_deviance = sum pw d(y, mu0) at mu0 = sum pw y / sum pw under a bias and g^-1(0) without -- a direct sum, not the
#   device's closed form -- and NaN whenever an offset is given.  Rows of weight 0 are dropped first.
def report_group(X, y, pw, o, beta, family, bias, dtype=np.longdouble):
    import math

    import glm_report_reference as rr

    fam = rr.FAMILY_ID[family]
    n_all = len(y)
    pw_all = np.ones(n_all) if pw is None else np.asarray(pw, dtype=np.float64)
    keep = pw_all > 0
    Z = rr._design(np.asarray(X)[keep], bias, dtype)
    yv = np.asarray(y)[keep].astype(dtype)
    w0 = pw_all[keep].astype(dtype)
    ov = np.zeros(int(keep.sum()), dtype=dtype) if o is None else np.asarray(o)[keep].astype(dtype)
    b = np.asarray(beta).astype(dtype)
    n, pp = Z.shape
    mu = rr._inv_link(fam, Z @ b + ov)
    v = rr._var(fam, mu)
    w = w0 / (rr._dlink(fam, mu) ** 2 * v)
    info = Z.T @ (Z * w[:, None])
    pearson = np.sum(w0 * (yv - mu) ** 2 / v)
    df = n - pp
    nan = dtype(np.nan)
    phi = dtype(1) if fam in (1, 2) else (pearson / df if df > 0 else nan)
    cov = phi * rr.spd_inverse(info, dtype)
    with np.errstate(invalid="ignore"):
        se = np.sqrt(np.diag(cov))
        z = b / se
    p = rr._erfc(np.abs(z.astype(np.float64)) / math.sqrt(2.0))
    if o is not None:
        null_dev = nan
    else:
        mu0 = np.full(n, np.sum(w0 * yv) / np.sum(w0) if bias else {0: 0.0, 1: 1.0, 2: 0.5, 3: np.nan}[fam], dtype=dtype)
        with np.errstate(invalid="ignore"):
            null_dev = np.sum(w0 * rr.unit_deviance(fam, yv, mu0))
    return {"std_err": se, "z": z, "p": p, "lo": b - dtype(rr.Z975) * se, "hi": b + dtype(rr.Z975) * se, "cov": cov,
            "deviance": np.sum(w0 * rr.unit_deviance(fam, yv, mu)), "null_deviance": null_dev, "pearson_chi2": pearson, "dispersion": phi,
            "df_resid": df}


REPORT_COEF = ("std_err", "z", "p", "lo", "hi")
REPORT_GROUP = ("deviance", "null_deviance", "pearson_chi2", "dispersion")


def report_by(X, y, off, pw, o, beta, family, bias, dtype=np.longdouble, skip=None):
    """report_group over the groups of a frame (NaN rows for the groups in `skip` and for groups null by the weight rule)"""
    G, pp = len(off) - 1, X.shape[1] + int(bias)
    out = {k: np.full((G, pp), np.nan, dtype=dtype) for k in REPORT_COEF}
    out["cov"] = np.full((G, pp, pp), np.nan, dtype=dtype)
    out.update({k: np.full(G, np.nan, dtype=dtype) for k in REPORT_GROUP})
    out["df_resid"] = np.zeros(G, dtype=np.int64)
    for g in range(G):
        a, e = int(off[g]), int(off[g + 1])
        pg = None if pw is None else pw[a:e]
        null, n_pos = is_null_by_weights(np.ones(e - a) if pg is None else pg, pp)
        out["df_resid"][g] = n_pos - pp
        if null or (skip is not None and skip[g]):
            continue
        r = report_group(X[a:e], y[a:e], pg, None if o is None else o[a:e], beta[g], family, bias, dtype)
        for k in (*REPORT_COEF, "cov", *REPORT_GROUP):
            out[k][g] = r[k]
    return out
