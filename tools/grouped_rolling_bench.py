"""Grouped rolling / expanding fits against the ungrouped call on the same frame (MI355X).

    python tools/grouped_rolling_bench.py [--rows 1e8] [--feat 8] [--window 256] [--reps 3] [--only SUBSTR]

For each shape: wall time per call (device-resident inputs and outputs, torch.cuda.synchronize around the call), the median over
--reps calls after a warm-up; the kernel time of the rolling kernels (HIP events on the context's stream, the "rolling" class of
Context.get_timing: fits, prefixes and the scatter, not the key sort / gather); and the HBM fraction of the wall time on
algorithmic bytes: N (p + 1) 8 in, N (p' + 1) 8 + N out, at 8 TB/s.  --only SUBSTR keeps the shapes whose name holds it."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import polars_ds_extension_amd as pds  # noqa: E402

HBM = 8.0e12


def timed(fn, reps):
    ctx = pds.default_context()
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    ctx.set_timing(True)
    ctx.get_timing(reset=True)
    fn()
    torch.cuda.synchronize()
    kern = ctx.get_timing(reset=True)["rolling"][0]
    ctx.set_timing(False)
    return float(np.median(ts)) * 1e3, kern


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=float, default=1e8)
    ap.add_argument("--feat", type=int, default=8)
    ap.add_argument("--window", type=int, default=256)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    n, p, w = int(a.rows), a.feat, a.window
    g = torch.Generator(device="cuda").manual_seed(0)
    cols = [torch.rand(n, device="cuda", dtype=torch.float64, generator=g) for _ in range(p)]
    y = sum(c * (0.1 * (j + 1)) for j, c in enumerate(cols)) + 1e-3 * torch.randn(n, device="cuda", dtype=torch.float64, generator=g)
    bytes_ = n * (p + 1) * 8 + n * (p + 1) * 8 + n
    res = []

    print(json.dumps({"rows": n, "feat": p, "window": w, "reps": a.reps, "statistic": "median wall ms"}), flush=True)

    def rec(name, fn):
        if a.only and a.only not in name:
            return
        ms, kern = timed(fn, a.reps)
        res.append({"shape": name, "ms": round(ms, 3), "kernel_ms": round(kern, 3), "hbm_fraction": round(bytes_ / (ms * 1e-3) / HBM, 3)})
        print(json.dumps(res[-1]), flush=True)

    rec(f"rolling ungrouped {n}x{p} w={w}", lambda: pds.rolling_lin_reg(*cols, target=y, window_size=w))
    rec(f"recursive ungrouped {n}x{p} n0={w}", lambda: pds.recursive_lin_reg(*cols, target=y, start_with=w))
    # the same two-stream kernel form on both sides (at w = 256 the ungrouped call keeps the leaving rows in registers)
    w2 = w + 44
    off1 = torch.tensor([0, n], device="cuda", dtype=torch.int64)
    rec(f"rolling ungrouped {n}x{p} w={w2}", lambda: pds.rolling_lin_reg(*cols, target=y, window_size=w2))
    rec(f"rolling offsets 1 group w={w2}", lambda: pds.rolling_lin_reg_by(*cols, target=y, group_offsets=off1, window_size=w2))
    rec(f"rolling offsets 10000x10000 w={w2}",
        lambda: pds.rolling_lin_reg_by(*cols, target=y, group_offsets=torch.arange(0, n + 1, n // 10000, device="cuda"), window_size=w2))
    for gl in (10_000, 1_000):
        ng = n // gl
        off = torch.arange(0, n + 1, gl, device="cuda", dtype=torch.int64)
        off[-1] = n
        rec(f"rolling offsets {ng}x{gl}", lambda: pds.rolling_lin_reg_by(*cols, target=y, group_offsets=off, window_size=w))
        rec(f"recursive offsets {ng}x{gl}", lambda: pds.recursive_lin_reg_by(*cols, target=y, group_offsets=off, start_with=w))
        keys = torch.repeat_interleave(torch.arange(len(off) - 1, device="cuda", dtype=torch.int64), torch.diff(off))
        rec(f"rolling ordered keys {ng}x{gl}", lambda: pds.rolling_lin_reg_by_key(*cols, target=y, key=keys, window_size=w))
        del keys
    D, K = 2500, n // 2500  # date-major panel: every date holds every key
    keys = torch.arange(K, device="cuda", dtype=torch.int64).repeat(D)[:n]
    rec(f"rolling unordered panel {D} dates x {K} keys", lambda: pds.rolling_lin_reg_by_key(*cols, target=y, key=keys, window_size=w))


if __name__ == "__main__":
    main()
