"""Row counts at which the streaming kernels of the one-model path and grouped_pred_kernel run their steady-state loop, and the
frames of tests/test_steady_state_gpu.py.

Every one of these kernels deals a fixed grid of waves contiguous ranges of units (128-row tiles, 64-row half-tiles, 128-row
chunks); the loop that prefetches unit t + 1 while unit t is consumed only turns when a wave gets a second unit.  `units_per_wave`
restates each launcher's split (the source line is beside each formula: a change there must be followed here, and
tests/test_steady_shapes_cpu.py pins the numbers at 256 CUs), `rows` picks a row count with a mean load of `units` per wave."""
import numpy as np

KINDS = ("small", "pass2", "pass2_wide", "mid", "leverage_mid", "grouped_pred")


def _es(dtype) -> int:
    es = np.dtype(dtype).itemsize
    if es not in (4, 8):
        raise ValueError("f32 or f64")
    return es


def _check(kind, dtype, p):
    es = _es(dtype)
    if kind not in KINDS:
        raise ValueError(f"unknown kind {kind!r}")
    if kind in ("small", "pass2") and not 1 <= p <= 16:
        raise ValueError(f"{kind}: 1 .. 16 features")
    if kind in ("mid", "leverage_mid") and not 17 <= p <= 64:
        raise ValueError(f"{kind}: 17 .. 64 features")
    if kind == "pass2_wide" and p <= 16:
        raise ValueError("pass2_wide: more than 16 features")
    if kind == "leverage_mid" and es != 8:
        raise ValueError("leverage_mid: f64 only (pass2.hip:436)")
    return es


def unit_rows(kind, dtype, p) -> int:
    """Rows of one unit of work."""
    es = _check(kind, dtype, p)
    rpl = 16 // es                      # rows per lane of a 16-byte load: Tile<T>::RPL, V16<T>::RPL (pass2.hip:22,27), GP16<T>::RPL
    if kind == "small":
        return 64 * rpl                 # moments.hip:50      TR = 64 * RPL
    if kind == "pass2":
        return 64 * rpl                 # pass2.hip:72        CH = 64 * RPL
    if kind == "pass2_wide":
        return 64                       # pass2.hip:260       lane = row, one row per trip of the grid-stride loop
    nblk = 2 if p <= 32 else 4          # moments_mid.hip:384-387, leverage_mid.hip:226
    if kind == "mid":
        return 1024 // (nblk * es)      # moments_mid_dev.hpp:20   HR = 1024 / (NBLK * ES)
    if kind == "leverage_mid":
        return 128 // nblk              # leverage_mid.hip:25      HR = 128 / NBLK
    return 64 * rpl                     # grouped_pred.hip:96      chunk = 64 * RPL rows


def n_waves(kind, dtype, p, n, num_cus) -> int:
    """Waves of the launch for n rows."""
    es = _check(kind, dtype, p)
    rpl = 16 // es
    cd = lambda a, b: -(-a // b)
    if kind == "small":
        ntiles = cd(n, 64 * rpl)                                # moments.hip:592
        return 4 * min(max(cd(ntiles, 4), 1), 2 * num_cus)      # moments.hip:593-594   kWaves = 4 waves per block
    if kind == "pass2":
        nvec = cd(n, rpl)                                       # pass2.hip:478
        return 4 * min(max(cd(nvec, 256), 1), 2 * num_cus)      # pass2.hip:479-481     PDS_P2_BLOCKS = 2 (pass2.hip:34)
    if kind == "pass2_wide":
        return 4 * min(max(cd(n, 256), 1), 8 * num_cus)         # pass2.hip:425
    if kind == "mid":
        return 4 * num_cus                                      # moments_mid.hip:356   kMidWavesPerCu = 4 (moments_mid_dev.hpp:10)
    if kind == "leverage_mid":
        return 4 * num_cus                                      # leverage_mid.hip:179  num_cus blocks of 256 threads
    nchunk = cd(n, 64 * rpl)                                    # grouped_pred.hip:266
    return 4 * min(max(cd(nchunk, 4), 1), 8 * num_cus)          # grouped_pred.hip:267


def units_per_wave(kind, dtype, p, n, num_cus) -> np.ndarray:
    """Trips of every wave's streaming loop for n rows (int64, one entry per wave).  A ragged tail that the kernel handles behind
    the loop (without a prefetch) is not a trip: see `tail_rows`."""
    u = unit_rows(kind, dtype, p)
    nw = n_waves(kind, dtype, p, n, num_cus)
    w = np.arange(nw + 1, dtype=object)  # (exact: nfull * wid is an __int128 product in the kernels)
    if kind == "pass2_wide":
        # pass2.hip:260   for (r = tid; r < n; r += gridDim.x * blockDim.x): wave w's first lane starts at row 64 w
        stride = 64 * nw
        return np.array([max(0, -(-(n - 64 * i) // stride)) for i in range(nw)], dtype=np.int64)
    if kind == "grouped_pred":
        nfull = -(-n // u)               # grouped_pred.hip:96-97   the ragged chunk is a trip of the loop (clamped rows)
    else:
        nfull = n // u                   # moments.hip:89, pass2.hip:75, moments_mid.hip:61, leverage_mid.hip:62
    # moments.hip:159-160, pass2.hip:76-77, moments_mid.hip:62, leverage_mid.hip:63, grouped_pred.hip:97:
    # wave w owns units [nfull w / W, nfull (w + 1) / W)
    edges = (nfull * w) // nw
    return np.diff(edges).astype(np.int64)


def tail_rows(kind, dtype, p, n) -> int:
    """Rows behind the last whole unit.  small / pass2 / mid / leverage_mid: the last wave takes them behind its loop (moments.hip:264,
    pass2.hip:181, moments_mid.hip:63,253, leverage_mid.hip:64,150); grouped_pred: the last chunk's masked lanes (grouped_pred.hip:119);
    pass2_wide: the lanes of the last wave-row that fall behind n."""
    return int(n % unit_rows(kind, dtype, p))


def one_unit_rows(kind, dtype, p, num_cus) -> int:
    """T: the row count at which the full grid is launched and every wave has exactly one unit."""
    u = unit_rows(kind, dtype, p)
    return u * n_waves(kind, dtype, p, 1 << 40, num_cus)


def second_unit_rows(kind, dtype, p, num_cus) -> int:
    """The smallest row count at which some wave's loop turns a second time.  Whole units only for the kernels that take the ragged
    tail behind the loop; one row more than T where the ragged unit is a trip of the loop."""
    t = one_unit_rows(kind, dtype, p, num_cus)
    return t + 1 if kind in ("pass2_wide", "grouped_pred") else t + unit_rows(kind, dtype, p)


def rows(kind, dtype, p, num_cus, units=2.5, tail=77) -> int:
    """A row count with a mean load of `units` units per wave (whole units), plus `tail` rows -- 77 is no multiple of any unit."""
    u = unit_rows(kind, dtype, p)
    t = one_unit_rows(kind, dtype, p, num_cus)
    return int(units * t) // u * u + tail


def boundary_rows(kind, dtype, p, num_cus):
    """[(n, expected units of every wave but the last, of the last wave, tail rows)]: T, T + one unit, T + one unit + 1 row."""
    u, t = unit_rows(kind, dtype, p), one_unit_rows(kind, dtype, p, num_cus)
    return [(t, 1, 1, 0), (t + u, 1, 2, 0), (t + u + 1, 1, 2, 1)]


# ------------------------------------------------------------------------------------------ the cases of the GPU file
SES = ("se", "hc0", "hc1", "hc2", "hc3")
F64, F32 = "float64", "float32"
SMALL_P = tuple(range(1, 17))
MID_P = (17, 24, 32, 33, 48, 49, 64)
BOUNDARY_P = (1, 2, 4, 8, 11, 16, 17, 33)
REPORT_CASES = [(p, p % 2 == 0, SES[(2 * p + k) % 5]) for p in SMALL_P for k in (0, 1)]  # (p, bias, std_err)
REPORT_F32_P = (1, 2, 4, 8, 12, 16)
WLS_CASES = [(p, F64) for p in (1, 2, 3, 4, 8, 11, 16)] + [(4, F32), (16, F32)]
FAMILIES = ("gaussian", "binomial", "poisson", "gamma")
# packings of moments_small_kernel: p = 1 | 2 | 3-4 | 5-8 | 9-15 | 16 -- each family at each of them
GLM_CASES = ([(p, FAMILIES[f], (p + f) % 2 == 0) for p in (1, 2, 16) for f in range(4)]
             + [(p, FAMILIES[(2 * p + k) % 4], (p + k) % 2 == 0) for p in (3, 4) for k in (0, 1)]
             + [(p, FAMILIES[p % 4], p % 2 == 0) for p in (5, 6, 7, 8)]
             + [(p, FAMILIES[p % 4], p % 2 == 1) for p in range(9, 16)])
GLM_F32_CASES = [(2, "gamma", True), (8, "poisson", False), (13, "binomial", True), (16, "gaussian", False)]
MID_F32_P = (20, 40)
MID_GLM_CASES = [(17, "poisson"), (40, "binomial")]
NOFUSE_CASES = [(p, se) for p in (20, 40) for se in ("hc2", "hc3")]
NOFUSE_UNITS = 2.1  # (the oracle at 1.3e6 x 41 is the slow part)
PRED_CASES = [(p, F64, b) for p in (1, 3, 16, 18) for b in (False, True)] + [(p, F32, b) for p in (3, 16) for b in (False, True)]


def nofuse_rows(p, num_cus) -> int:
    return max(rows("pass2_wide", F64, p, num_cus, units=NOFUSE_UNITS), rows("leverage_mid", F64, p, num_cus, units=NOFUSE_UNITS))


def steady_cases():
    """(kind, dtype, p, units) of every row count the GPU file takes from `rows`: what tests/test_steady_shapes_cpu.py checks."""
    out = []
    for dt in (F64, F32):
        out += [("small", dt, p, 2.5) for p in SMALL_P] + [("mid", dt, p, 2.5) for p in MID_P]
        out += [("pass2", dt, p, 2.5) for p in SMALL_P]  # (section 3 sits at rows("small"): the same count, checked there)
        out += [("grouped_pred", dt, p, 2.5) for p in sorted({c[0] for c in PRED_CASES if c[1] == dt})]
    out += [("mid", F32, p, 2.5) for p in MID_F32_P] + [("mid", F64, p, 2.5) for p, _ in MID_GLM_CASES]
    out += [(k, F64, p, NOFUSE_UNITS) for k in ("pass2_wide", "leverage_mid") for p in (20, 40)]
    return out


# ------------------------------------------------------------------------------------------ frames
def integer_frame(seed, n, p, dtype):
    """Features and target in [-3, 3], weights in {0, 1}: every product and partial sum of the Gram is an integer below 9 n."""
    rng = np.random.default_rng(seed)
    X = rng.integers(-3, 4, size=(n, p), dtype=np.int8)
    y = rng.integers(-3, 4, size=n, dtype=np.int8)
    w = rng.integers(0, 2, size=n, dtype=np.int8)
    return X.astype(dtype), y.astype(dtype), w.astype(dtype)


def integer_design(X, y):
    """Z = [X | 1 | y] in f64."""
    return np.c_[X.astype(np.float64), np.ones(len(y)), y.astype(np.float64)]


def gram_of_design(Z, w=None):
    """Z' diag(w) Z as int64.  The products run in f64 (BLAS): every partial sum is an integer below 9 n < 2^53, so they are exact in
    any order, and the cast is too."""
    assert 9 * len(Z) < 2 ** 53
    G = Z.T @ (Z if w is None else Z * w.astype(np.float64)[:, None])
    Gi = G.astype(np.int64)
    assert np.array_equal(Gi.astype(np.float64), G)
    return Gi


def integer_gram(X, y, w=None):
    """The int64 Gram of [X | 1 | y], weighted by w."""
    return gram_of_design(integer_design(X, y), w)


def report_frame(seed, n, p, bias):
    """Like test_gpu_parity.test_lin_reg_report's: U(0, 1) features, some true zero coefficients, heteroskedastic noise."""
    rng = np.random.default_rng(seed)
    X = rng.random((n, p))
    beta = np.array([(-1.0) ** j * (0.05 + 0.03 * j) for j in range(p)])
    beta[3::3] = 0.0
    if p in (2, 3):
        beta[1] = 0.0
    y = X @ beta + (0.4 if bias else 0.0) + 0.3 * rng.normal(size=n) * (0.5 + X[:, 0])
    return X, y


def wide_report_frame(seed, n, p):
    """Like test_gpu_parity.test_wide_weighted_and_hc's."""
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, p))
    y = X @ rng.normal(size=p) + 0.4 + rng.normal(size=n) * (0.5 + np.abs(X[:, 0]))
    w = rng.random(n) + 0.25
    return X, y, w


def glm_frame(seed, family, n, p, bias):
    """The four y generators of test_linear_models._glm_family_data at any width (coefficients scaled by 1 / sqrt(p)).  gamma (inverse
    link): U(0.1, 1) features and positive coefficients keep eta = 1 / mu away from zero, with or without an intercept."""
    rng = np.random.RandomState(seed)
    base = np.array([1.0, -0.5, 0.3, 0.8])
    b = np.resize(base, p) * (2.0 / np.sqrt(4.0 * p))
    if family == "gamma":
        X = rng.uniform(0.1, 1.0, size=(n, p))
        eta = X @ (0.3 + np.abs(b)) + (0.5 if bias else 0.0)
        return X, rng.gamma(shape=2.0, scale=(1.0 / eta) / 2.0)
    X = rng.randn(n, p)
    eta = X @ b + (0.2 if bias else 0.0)
    if family == "gaussian":
        y = eta + rng.randn(n) * 0.1
    elif family == "binomial":
        y = rng.binomial(1, 1.0 / (1.0 + np.exp(-eta))).astype(float)
    else:
        y = rng.poisson(np.exp(np.clip(0.5 * eta, -2.0, 2.0))).astype(float)
    return X, y


def wide_glm_frame(seed, family, n, p):
    """test_linear_models.test_glm_beyond_16_features_matches_the_oracle's frame."""
    rng = np.random.RandomState(seed)
    X = rng.randn(n, p)
    beta = rng.randn(p) * (0.6 / np.sqrt(p))
    eta = X @ beta + 0.2
    if family == "gaussian":
        y = eta + rng.randn(n) * 0.1
    elif family == "binomial":
        y = rng.binomial(1, 1.0 / (1.0 + np.exp(-eta))).astype(float)
    elif family == "poisson":
        y = rng.poisson(np.exp(np.clip(eta, -2.0, 2.0))).astype(float)
    else:
        eta = 1.5 + 0.3 * np.tanh(eta)
        y = rng.gamma(shape=2.0, scale=(1.0 / eta) / 2.0)
    return X, y


def pred_group_sizes(seed, n, pp, chunk, wave_chunks):
    """Group sizes (int64, summing to n) that mix what grouped_pred_kernel's cursor and coefficient stage have to survive: runs of
    thousands of one-row groups, groups of 2-5 rows (more than 192 / p' of them in a chunk when p' = 1: the unstaged read), runs of
    empty groups, groups of 100-300 rows, one group spanning more than three of a wave's chunks (wave_chunks = the largest number of
    chunks a wave owns), a too-small group every few hundred groups, and empty groups at the very end."""
    rng = np.random.default_rng(seed)
    parts, left = [], n
    giant = (3 * max(wave_chunks, 1) + 2) * chunk + 17
    segs = 0
    while left > 0:
        kind = segs % 5
        if kind == 0:
            s = np.ones(int(rng.integers(2000, 6000)), dtype=np.int64)
        elif kind == 1:
            s = rng.integers(2, 6, size=int(rng.integers(3000, 9000)))
        elif kind == 2:
            s = np.zeros(int(rng.integers(3, 400)), dtype=np.int64)
        elif kind == 3:
            s = rng.integers(100, 301, size=int(rng.integers(300, 900)))
            s[::257] = rng.integers(0, pp, size=len(s[::257]))  # too small: a null group
        else:
            s = np.concatenate([rng.integers(max(pp, 1) + 3, 64, size=int(rng.integers(500, 2000))), [0, 0]])
        if segs == 7:
            s = np.concatenate([s, [giant]])
        s = s.astype(np.int64)
        c = np.cumsum(s)
        if c[-1] >= left:  # cut the last segment to fit
            k = int(np.searchsorted(c, left, side="left"))
            s = s[: k + 1].copy()
            s[k] = left - (c[k - 1] if k else 0)
        parts.append(s)
        left -= int(s.sum())
        segs += 1
    assert segs > 8, "frame too short for the giant group"
    parts.append(np.zeros(5, dtype=np.int64))  # empty groups at the very end
    sizes = np.concatenate(parts)
    assert int(sizes.sum()) == n
    return sizes
