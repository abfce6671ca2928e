"""
Host Arrow frame through the plugin symbols: ONE pl_lin_reg_report_by call over the whole frame against one pl_lin_reg_report call
per group (what `group_by(key).agg(lin_reg_report(...))` makes Polars do), wall time, with tests/plugin_harness.py playing Polars'
part (its Arrow export / import is inside both timings; the per-group side is called from one thread).  A record, no target.
Usage: python tools/grouped_report_plugin_bench.py [--groups 10000] [--rows 100] [--feats 8] [--reps 5] [--weights]
"""
import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import pyarrow as pa  # noqa: E402
from plugin_harness import call_plugin  # noqa: E402

from polars_ds_extension_amd import _lib  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=10_000)
    ap.add_argument("--rows", type=int, default=100)
    ap.add_argument("--feats", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--weights", action="store_true")
    a = ap.parse_args()
    _lib.load()  # (torch's HIP runtime first, see _lib.load)
    lib = C.CDLL(str(_lib.LIB_PATH))
    rng = np.random.default_rng(3)
    G, m, p = a.groups, a.rows, a.feats
    n = G * m
    key = np.repeat(rng.permutation(G).astype(np.int64), m)
    X = rng.normal(size=(n, p))
    y = X @ rng.normal(size=p) + 0.3 + rng.normal(size=n)
    w = rng.uniform(0.25, 4.0, size=n)
    perm = rng.permutation(n)  # rows of a group are not contiguous
    key, X, y, w = key[perm], X[perm], y[perm], w[perm]
    kw = {"bias": True, "null_policy": "raise", "std_err": "se", "solver": "qr", "l1_reg": 0.0, "l2_reg": 0.0, "tol": 0.0}
    lead = [("w", pa.array(w))] if a.weights else []
    ins = [("k", pa.array(key))] + lead + [("y", pa.array(y))] + [(f"x{j + 1}", pa.array(X[:, j])) for j in range(p)]
    by_sym, one_sym = ("pl_wls_report_by", "pl_wls_report") if a.weights else ("pl_lin_reg_report_by", "pl_lin_reg_report")

    def by_call():
        return call_plugin(lib, by_sym, ins, kw)[1]

    # what Polars' group_by hands the per-group calls: every group's rows gathered, var(y) of the group in front of y
    order = np.argsort(key, kind="stable")
    groups = []
    for g in range(G):
        r = order[g * m:(g + 1) * m]
        yv = pa.array([float(np.var(y[r], ddof=1))])
        gl = [("w", pa.array(w[r]))] if a.weights else []
        groups.append(gl + [("var", yv), ("y", pa.array(y[r]))] + [(f"x{j + 1}", pa.array(X[r, j])) for j in range(p)])

    def per_group():
        return [call_plugin(lib, one_sym, gi, kw)[1] for gi in groups]

    def timed(fn, reps):
        fn()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        ts.sort()
        return ts[len(ts) // 2], ts[0], ts[-1]

    b = timed(by_call, a.reps)
    g = timed(per_group, max(1, a.reps // 2))
    out = by_call()
    assert len(out) == G * (p + 1)
    print(json.dumps({"bench": "grouped_report_plugin", "symbol": by_sym, "groups": G, "rows": n, "p": p,
                      "by_call_ms": [round(v, 2) for v in b], "per_group_calls_ms": [round(v, 1) for v in g],
                      "ratio": round(g[0] / b[0], 1), "note": "ms as median, min, max"}), flush=True)


if __name__ == "__main__":
    main()
