"""
The grouped multi-target fit (pds_lr_multi_grouped_* / _by_key_*, csrc/grouped_multi.hip and the per-target route) on one MI355X.
Frames: `--groups` (1e6) groups x 100 rows, f64, device resident; 8 features + bias with k in {2, 4, 8}, 16 features + bias with k in
{2, 8} (`--shapes p:k,..`).  For each frame three ways to the same k coefficient vectors per group are timed, ALTERNATING inside every
repeat (two warm-up rounds first; device events around each call, which ends in a stream synchronise):
  route1    lin_reg_multi_by, context option grouped_multi_route = 1: one kernel, one wave per group
  route2    lin_reg_multi_by, grouped_multi_route = 2: the fused grouped kernel once per target on the one staged frame
  separate  k lin_reg_by calls, one per target: the code as it stood before the grouped multi-target call (the baseline)
and the same again through the by-key forms (lin_reg_multi_by_key / k lin_reg_by_key calls, keys = the group ids in order).
Per variant: median, best and worst of `--reps` repeats (the spread), and for the two routes the ratio to `separate`.  Beside the
times stands the algorithmic byte ratio (p + k) / (k (p + 1)): the columns one call has to read over those k calls read.
`--host-groups G` (2e5; 0: skip): one host-resident pair, NumPy inputs, P = 8, k = 4: lin_reg_multi_by (route 0, what a caller gets)
against k lin_reg_by calls on the same arrays, wall clock (the frame crosses PCIe once instead of k times).
A per-kernel split comes from a separate run under `rocprofv3 --kernel-trace --stats -- python tools/grouped_multi_bench.py ...`.
"""
import argparse
import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import polars_ds_extension_amd as pds  # noqa: E402


def alternating(variants, reps, warm=2):
    """variants: {name: fn}; every repeat runs each of them once, in turn.  Returns {name: (median, best, worst)} in ms."""
    for _ in range(warm):
        for fn in variants.values():
            fn()
    s = torch.cuda.current_stream()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = {k: [] for k in variants}
    for _ in range(reps):
        for k, fn in variants.items():
            a.record(s)
            fn()
            b.record(s)
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    return {k: (sorted(v)[len(v) // 2], min(v), max(v)) for k, v in ms.items()}


def report(form, p, k, G, m, res, extra=None):
    rec = {"bench": "grouped_multi", "form": form, "groups": G, "rows_per_group": m, "p": p, "bias": True, "k": k,
           "byte_ratio_(p+k)/(k(p+1))": round((p + k) / (k * (p + 1)), 4)}
    for name, (med, best, worst) in res.items():
        rec[f"{name}_ms"] = round(med, 3)
        rec[f"{name}_ms_best"] = round(best, 3)
        rec[f"{name}_ms_worst"] = round(worst, 3)
    for name in res:
        if name != "separate":
            rec[f"{name}_over_separate"] = round(res[name][0] / res["separate"][0], 4)
    if "route1" in res and "route2" in res:
        rec["faster_route"] = 1 if res["route1"][0] < res["route2"][0] else 2
    rec.update(extra or {})
    print(json.dumps(rec), flush=True)


def with_route(ctx, route, fn):
    def run():
        ctx.set_option("grouped_multi_route", route)
        try:
            return fn()
        finally:
            ctx.set_option("grouped_multi_route", 0)

    return run


def run_shape(ctx, gen, dev, p, k, G, m, reps, by_key):
    n = G * m
    off = torch.arange(0, n + 1, m, dtype=torch.int64, device=dev)
    X = [torch.randn(n, generator=gen, device=dev, dtype=torch.float64) for _ in range(p)]
    T = []
    for t in range(k):
        y = torch.full((n,), 0.3, device=dev, dtype=torch.float64)
        for j in range(p):
            y += (0.5 * (-1) ** (j + t) * (j + 1) / p) * X[j]
        T.append(y + 0.1 * torch.randn(n, generator=gen, device=dev, dtype=torch.float64))
    multi = lambda: pds.lin_reg_multi_by(*X, targets=T, group_offsets=off, add_bias=True, ctx=ctx)  # noqa: E731
    separate = lambda: [pds.lin_reg_by(*X, target=t, group_offsets=off, add_bias=True, ctx=ctx) for t in T]  # noqa: E731
    res = alternating({"route1": with_route(ctx, 1, multi), "route2": with_route(ctx, 2, multi), "separate": separate}, reps)
    # the three agree (a timing of different answers would say nothing)
    c1 = with_route(ctx, 1, multi)()[0]
    c2 = with_route(ctx, 2, multi)()[0]
    cs = torch.stack([c for c, _ in separate()], dim=1)
    agree = max(float((c1 - cs).abs().max().item()), float((c2 - cs).abs().max().item()))
    report("offsets", p, k, G, m, res, {"max_abs_difference_of_coeffs": agree})
    if by_key:
        key = torch.arange(G, dtype=torch.int64, device=dev).repeat_interleave(m)
        multi_k = lambda: pds.lin_reg_multi_by_key(*X, targets=T, key=key, add_bias=True, max_groups=G, ctx=ctx)  # noqa: E731
        separate_k = lambda: [pds.lin_reg_by_key(*X, target=t, key=key, add_bias=True, max_groups=G, ctx=ctx) for t in T]  # noqa: E731
        res = alternating({"route1": with_route(ctx, 1, multi_k), "route2": with_route(ctx, 2, multi_k), "separate": separate_k}, reps)
        report("by_key (ordered keys)", p, k, G, m, res)


def run_host(ctx, p, k, G, m, reps):
    rng = np.random.default_rng(4)
    n = G * m
    X = [rng.standard_normal(n) for _ in range(p)]
    T = [sum((0.5 * (-1) ** (j + t) * (j + 1) / p) * X[j] for j in range(p)) + 0.3 + 0.1 * rng.standard_normal(n) for t in range(k)]
    off = np.arange(0, n + 1, m, dtype=np.int64)
    variants = {"multi": lambda: pds.lin_reg_multi_by(*X, targets=T, group_offsets=off, add_bias=True, ctx=ctx),
                "separate": lambda: [pds.lin_reg_by(*X, target=t, group_offsets=off, add_bias=True, ctx=ctx) for t in T]}
    for fn in variants.values():
        fn()
    ms = {name: [] for name in variants}
    for _ in range(reps):
        for name, fn in variants.items():
            t0 = time.perf_counter()
            fn()  # (host outputs: the call returns after its last copy)
            ms[name].append((time.perf_counter() - t0) * 1e3)
    med = {name: sorted(v)[len(v) // 2] for name, v in ms.items()}
    print(json.dumps({"bench": "grouped_multi_host_frame", "groups": G, "rows_per_group": m, "p": p, "bias": True, "k": k,
                      "frame_GB_one_call": round(n * (p + k) * 8 / 1e9, 3), "frame_GB_k_calls": round(n * k * (p + 1) * 8 / 1e9, 3),
                      "byte_ratio_(p+k)/(k(p+1))": round((p + k) / (k * (p + 1)), 4),
                      "multi_ms": round(med["multi"], 2), "multi_ms_best": round(min(ms["multi"]), 2), "multi_ms_worst": round(max(ms["multi"]), 2),
                      "separate_ms": round(med["separate"], 2), "separate_ms_best": round(min(ms["separate"]), 2),
                      "separate_ms_worst": round(max(ms["separate"]), 2), "multi_over_separate": round(med["multi"] / med["separate"], 4)}),
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="8:2,8:4,8:8,16:2,16:8")
    ap.add_argument("--groups", type=int, default=1_000_000)
    ap.add_argument("--rows", type=int, default=100)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--no-by-key", action="store_true")
    ap.add_argument("--host-groups", type=int, default=200_000)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    ctx = pds.Context(0)
    ctx.set_stream(torch.cuda.current_stream(dev))
    gen = torch.Generator(device=dev)
    gen.manual_seed(3)
    print(json.dumps({"bench": "grouped_multi", "device": torch.cuda.get_device_name(0), "reps": a.reps, "timing": "device events, alternating"}),
          flush=True)
    for shape in a.shapes.split(","):
        p, k = (int(v) for v in shape.split(":"))
        run_shape(ctx, gen, dev, p, k, a.groups, a.rows, a.reps, not a.no_by_key)
        torch.cuda.empty_cache()
    if a.host_groups > 0:
        run_host(ctx, 8, 4, a.host_groups, a.rows, max(3, a.reps // 2))


if __name__ == "__main__":
    main()
