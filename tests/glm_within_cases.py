"""The frames of the fixed-effects GLM tests (TEST INFRASTRUCTURE ONLY; tests/test_glm_within_cpu.py, tests/test_glm_within_gpu.py).

The ragged frame: 14 contiguous groups of SIZES rows -- every edge of the 4-row matrix instruction (1, 3, 4, 5), of the 64-row step
(63, 64, 65) and of the 128-row residency (127, 128, 129), a group that is read twice (200) and short ones behind it -- with integer
weights in 0 .. 3 (zero-weight rows inside kept groups, and small groups whose rows all have weight 0) and an offset.  Small binomial
and poisson groups separate (all counting y equal 0, or all 1): they are dropped, which is wanted.  DROPPED states, per family and
width, how many of the 14 groups the definition drops on these frames; test_glm_within_cpu.py pins the numbers.
"""
import numpy as np

SIZES = (1, 3, 4, 5, 63, 64, 65, 127, 128, 129, 200, 2, 7, 33)
FAMILIES = ("gaussian", "binomial", "poisson", "gamma")
WIDTHS = (1, 7, 16)
OFFSETS = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)
N_ROWS = int(OFFSETS[-1])

# groups of the 14 that are dropped: no row of positive weight; poisson: every counting y is 0; binomial: all 0 or all 1
DROPPED = {("gaussian", 1): 1, ("gaussian", 7): 0, ("gaussian", 16): 0,
           ("binomial", 1): 3, ("binomial", 7): 2, ("binomial", 16): 2,
           ("poisson", 1): 2, ("poisson", 7): 0, ("poisson", 16): 0,
           ("gamma", 1): 1, ("gamma", 7): 0, ("gamma", 16): 0}


def frame(family: str, p: int) -> dict:
    """X [n, p], y, pw, o, codes (the group of every row, ascending), off (the group offsets), beta, alpha: float64 / int64"""
    rng = np.random.default_rng(900 + p)
    G, n = len(SIZES), N_ROWS
    beta = (0.3 if p == 16 else 0.5) * rng.uniform(-1.0, 1.0, p)
    alpha = 0.5 * rng.standard_normal(G)
    codes = np.repeat(np.arange(G, dtype=np.int64), SIZES)
    pw = rng.integers(0, 4, n).astype(np.float64)
    o = 0.3 * rng.standard_normal(n)
    if family == "gamma":
        X = rng.uniform(0.1, 1.0, (n, p))
        o = np.abs(o)
        eta = 0.5 + np.abs(alpha)[codes] + X @ np.abs(beta) + o
        y = rng.gamma(2.0, 1.0 / (2.0 * eta))
    else:
        X = rng.standard_normal((n, p))
        eta = X @ beta + 0.2 + alpha[codes] + o
        if family == "gaussian":
            y = eta + rng.standard_normal(n)
        elif family == "binomial":
            y = (rng.uniform(size=n) < 1.0 / (1.0 + np.exp(-eta))).astype(np.float64)
        else:
            y = rng.poisson(np.exp(eta)).astype(np.float64)
    return {"X": X, "y": y, "pw": pw, "o": o, "codes": codes, "off": OFFSETS.copy(), "beta": beta, "alpha": alpha}
