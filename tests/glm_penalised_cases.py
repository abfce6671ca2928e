"""Frames and recorded references of the penalised GLM tests (tests/test_glm_penalised_cpu.py, tests/test_glm_penalised_gpu.py).

A grouped case is (family, features, bias, l1, l2).  Its frame has 60 groups: the sizes p', p' + 1, 63, 64, 65, 127, 128, 129, 200,
1100 six times over (both sides of the kernel's 64-row step and of its 128-row residency, and a group above a lowered
`glm_split_rows`); a case without a ridge term has p' + 2 in place of p' (n = p' rows and l2 = 0 leave the fit to the l1 term
alone).  Data as tests/glm_cases.family_frame draws them (gamma: positive features and coefficients), seeded per case; the seeds
are chosen so that the NumPy restatement alone leaves no group null or at max_iter.

What the restatement (tests/glm_penalised_reference.py) gives on a case -- beta*, and its own run at the kernel's tol and inner
constant -- takes seconds to tens of seconds per case on a CPU, so it is recorded once in tests/golden/glm_penalised_refs.npz
(`python tests/glm_penalised_cases.py` rewrites it); test_glm_penalised_cpu.py recomputes some cases against the record and checks
the optimality of every recorded beta* from the frame, which needs no solver."""
import functools
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
import glm_cases as gc  # noqa: E402
import glm_penalised_reference as ref  # noqa: E402

GOLDEN = Path(__file__).resolve().parent / "golden" / "glm_penalised_refs.npz"
L1, L2 = 0.02, 0.05
PENALTIES = ((0.0, L2), (L1, 0.0), (L1, L2))
TOL, MAX_ITER = 1e-10, 100
TOL_F32 = float(np.float32(1e-6))

GROUPED_CONFIGS = [("binomial", p, b) for p, b in ((1, 0), (8, 1), (15, 1), (16, 0), (16, 1))] + \
                  [(f, p, 1) for f in ("poisson", "gamma", "gaussian") for p in (8, 16)]
SEEDS = {("binomial", 8, 1): 2}  # (seeds 0 and 1 hold a 9-row group whose ridge fit the plain Newton iteration does not reach)


def sizes_of(pp, l2):
    base = [pp if l2 > 0.0 else pp + 2, pp + 1, 63, 64, 65, 127, 128, 129, 200, 1100]
    return np.array(base * 6, dtype=np.int64)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def frame(family, p, bias, l2_on, f32=False):
    rng = np.random.default_rng([2024, SEEDS.get((family, p, bias), 0), p, bias, gc.FAMILIES.index(family)])
    X, y, off = gc.family_frame(rng, family, sizes_of(p + bias, 1.0 if l2_on else 0.0), p)
    if f32:
        X, y = X.astype(np.float32).astype(np.float64), y.astype(np.float32).astype(np.float64)
    return _frozen(X, y, off)


@functools.lru_cache(maxsize=None)
def separated_frame():
    """12 perfectly separated binomial groups of 5 .. 60 rows: one feature, y = [x > 0]"""
    rng = np.random.default_rng(77)
    sizes = np.array([5, 6, 9, 17, 33, 60] * 2, dtype=np.int64)
    x = rng.normal(size=int(sizes.sum()))
    x[np.abs(x) < 0.05] = 0.5
    off = gc.offsets(sizes)
    for g in range(len(sizes)):  # both classes in every group
        x[off[g]], x[off[g] + 1] = abs(x[off[g]]), -abs(x[off[g] + 1])
    return _frozen(x[:, None].copy(), (x > 0).astype(np.float64), off)


@functools.lru_cache(maxsize=None)
def wide_frame():
    """one binomial frame of 500 rows x 20 features: the wide one-model route"""
    rng = np.random.default_rng(78)
    X = rng.normal(size=(500, 20))
    eta = X @ (0.4 * rng.uniform(-1.0, 1.0, size=20)) + 0.2
    y = (rng.uniform(size=500) < 1.0 / (1.0 + np.exp(-eta))).astype(np.float64)
    return _frozen(X, y, np.array([0, 500], dtype=np.int64))


def case(name):
    """name -> (X, y, off, family, bias, l1, l2, tol, f32)"""
    if name == "separated":
        return (*separated_frame(), "binomial", 1, 0.0, 0.1, TOL, False)
    if name == "wide":
        return (*wide_frame(), "binomial", 1, L1, L2, TOL, False)
    family, p, bias, l1, l2, *rest = name.split("/")
    p, bias, l1, l2, f32 = int(p), int(bias), float(l1), float(l2), bool(rest)
    return (*frame(family, p, bias, l2 > 0.0, f32), family, bias, l1, l2, TOL_F32 if f32 else TOL, f32)


def name_of(family, p, bias, l1, l2, f32=False):
    return f"{family}/{p}/{bias}/{l1}/{l2}" + ("/f32" if f32 else "")


F32_CASE = name_of("binomial", 8, 1, L1, L2, True)
ALL_CASES = [name_of(f, p, b, l1, l2) for f, p, b in GROUPED_CONFIGS for l1, l2 in PENALTIES] + [F32_CASE, "separated", "wide"]


def compute(name):
    """beta* and the restatement's own run (coefficients, n_iter, inner sweeps) of a case"""
    X, y, off, family, bias, l1, l2, tol, f32 = case(name)
    star = ref.beta_star(X, y, off, family, bool(bias), l1, l2)
    co, it, sw = ref.fit(X, y, off, family, bool(bias), l1, l2, tol=tol, max_iter=MAX_ITER)
    return {"star": star, "helper": co, "n_iter": it, "sweeps": sw}


@functools.lru_cache(maxsize=None)
def _golden():
    return dict(np.load(GOLDEN))


@functools.lru_cache(maxsize=None)
def reference(name):
    """dict: the case's frame and parameters, the recorded star / helper / n_iter / sweeps, and the restatement's own figures that
    set the bounds: helper_err (worst |helper - star| over groups and coefficients; an f32 case rounds the helper's coefficients to
    f32 first) and helper_kkt (worst KKT residual of those coefficients)."""
    X, y, off, family, bias, l1, l2, tol, f32 = case(name)
    g = _golden()
    out = {k: g[f"{name}:{k}"] for k in ("star", "helper", "n_iter", "sweeps")}
    co = out["helper"].astype(np.float32).astype(np.float64) if f32 else out["helper"]
    out.update(X=X, y=y, off=off, family=family, bias=bool(bias), l1=l1, l2=l2, tol=tol, p=X.shape[1],
               helper_err=float(np.abs(co - out["star"]).max()),
               helper_kkt=float(ref.kkt(X, y, off, family, bool(bias), l1, l2, co).max()))
    return out


def bound(own):
    """the tolerance rule: 10 x the restatement's own figure on the same data, with a floor of 1e-12"""
    return max(10.0 * own, 1e-12)


if __name__ == "__main__":
    import time

    rec = {}
    for nm in ALL_CASES:
        t = time.time()
        for k, v in compute(nm).items():
            rec[f"{nm}:{k}"] = v
        print(f"{nm}: {time.time() - t:.1f} s, n_iter <= {rec[nm + ':n_iter'].max()}, sweeps <= {rec[nm + ':sweeps'].max()}", flush=True)
    GOLDEN.parent.mkdir(exist_ok=True)
    np.savez_compressed(GOLDEN, **rec)
    print(GOLDEN, GOLDEN.stat().st_size, "bytes")
