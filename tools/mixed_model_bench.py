"""
MixedModel fits (pds_mixed_reml_grouped_*, csrc/mixed.hip) on one MI355X, inputs resident in HBM, offsets form.
Per shape: median / best / worst of `--reps` (default 7) warmed calls by device events; from one more call with the context's
timing classes on, the statistics kernels' time ("grouped_moments": both runs of the frame passes and their record sums) and the
search kernels' time ("iterative": every per-gamma reduction); the total time of the gamma search = the call minus the statistics
kernels (launches, blocking copies and host factorisations included; the two figures come from DIFFERENT calls -- the median of
the timed calls and the one extra call with timing on -- so the difference is a recorded figure, not an exact split); the
evaluation count; and frame bytes / statistics time as a share of the 8 TB/s HBM peak ("roofline_share" says "measured" when the
timing classes returned a statistics time, "not measured" otherwise -- then the share is null).  The frame passes run twice (on y, then on the residual of a first solution), and groups longer than
128 rows are read twice per run: the share is of ONE frame's bytes, so it says how far the statistics are from a single read at
peak, not what bandwidth the kernels reach.
Shapes (`--shapes`): headline = 1e6 groups x 100 rows x 8 features; wide = the same with 16; long = 1e4 groups x 1e4 rows x 8;
skewed = one 1e7-row group + 1e5 groups of 100 rows, 8 features.  `--split a,b,c` repeats the long and skewed shapes with the
context option mixed_split_rows set to each value (how the library's default was chosen).
`--sample K`: the reference's algorithm as restated in tests/mixed_reference.py (NumPy, float64, an O(n p^2) pass per evaluation)
on the first K groups of the headline frame, for scale.  No time here is a pass condition: the feature has no parent to compare
against.  Lines are appended to profiles/mixed_model_bench.txt (`--out`).
"""
import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import polars_ds_extension_amd as pds  # noqa: E402

HBM = 8.0e12
OUT = None


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if OUT is not None:
        with open(OUT, "a") as fh:
            fh.write(line + "\n")


def timed(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    s = torch.cuda.current_stream()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for _ in range(reps):
        a.record(s)
        fn()
        b.record(s)
        b.synchronize()
        ms.append(a.elapsed_time(b))
    ms.sort()
    return ms[len(ms) // 2], ms[0], ms[-1]


def make_frame(gen, dev, off, p):
    """x ~ N(3, 1), the last feature constant within groups, y = X beta + 0.7 u_g + e."""
    n, ng = int(off[-1].item()), int(off.numel()) - 1
    codes = torch.repeat_interleave(torch.arange(ng, device=dev), off[1:] - off[:-1])
    X = [torch.randn(n, generator=gen, device=dev, dtype=torch.float64) + 3.0 for _ in range(p - 1)]
    X.append((torch.randn(ng, generator=gen, device=dev, dtype=torch.float64) + 3.0)[codes])
    y = 0.7 * torch.randn(ng, generator=gen, device=dev, dtype=torch.float64)[codes]
    y += 0.5 + torch.randn(n, generator=gen, device=dev, dtype=torch.float64)
    for j in range(p):
        y += (0.5 * (-1) ** j * (j + 1) / p) * X[j]
    return X, y


def run_shape(name, ctx, gen, dev, off, p, reps, split=None):
    n, ng = int(off[-1].item()), int(off.numel()) - 1
    X, y = make_frame(gen, dev, off, p)
    ctx.set_option("mixed_split_rows", split or 0)
    call = lambda: pds.mixed_reml(*X, target=y, group_offsets=off, ctx=ctx)  # noqa: E731
    ms, best, worst = timed(call, reps)
    ctx.set_timing(True)
    ctx.get_timing()
    fit = call()
    ctx.synchronize()
    tm = ctx.get_timing()
    ctx.set_timing(False)
    stats_ms, search_kernel_ms = tm["grouped_moments"][0], tm["iterative"][0]
    frame_bytes = n * (p + 1) * 8
    emit({"bench": "mixed_model", "shape": name, "groups": ng, "rows": n, "p": p, "split_rows": split or "default",
          "ms": round(ms, 3), "ms_best": round(best, 3), "ms_worst": round(worst, 3), "stats_kernels_ms": round(stats_ms, 3),
          "search_total_ms": round(ms - stats_ms, 3), "search_kernels_ms": round(search_kernel_ms, 3), "n_eval": fit["n_eval"],
          "gamma": round(fit["gamma"], 6), "frame_GB": round(frame_bytes / 1e9, 3),
          "frame_bytes_per_stats_time_share_of_8TBps": round(frame_bytes / (stats_ms * 1e-3) / HBM, 4) if stats_ms > 0 else None,
          "roofline_share": "measured" if stats_ms > 0 else "not measured"})
    return X, y


def sample_against_reference_algorithm(X, y, m, p, k):
    """The reference's algorithm (a full pass over the rows per evaluation) in NumPy float64 on the first k groups, beside the
    library's call on the same rows."""
    import mixed_reference as mr

    Xs = [c[:k * m] for c in X]
    ys = y[:k * m]
    off = torch.arange(0, k * m + 1, m, dtype=torch.int64, device=y.device)
    F = torch.stack(Xs, dim=1).cpu().numpy()
    yh = ys.cpu().numpy()
    codes = np.repeat(np.arange(k), m)
    t0 = time.perf_counter()
    ref = mr.fit_reml(mr.design(F), yh, codes, k)
    t_ref = (time.perf_counter() - t0) * 1e3
    t = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = pds.mixed_reml(*Xs, target=ys, group_offsets=off)
        t.append((time.perf_counter() - t0) * 1e3)
    emit({"bench": "mixed_model_vs_reference_algorithm", "groups": k, "rows_per_group": m, "p": p, "numpy_reference_ms": round(t_ref, 1),
          "library_call_ms": round(float(np.median(t)), 3), "gamma_reference": round(float(ref["gamma"]), 6), "gamma_library": round(got["gamma"], 6),
          "n_eval_reference": ref["n_eval"], "n_eval_library": got["n_eval"]})


def main():
    global OUT
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="headline,wide,long,skewed")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--split", default="")
    ap.add_argument("--sample", type=int, default=1000)
    ap.add_argument("--scale", type=float, default=1.0, help="scales the group counts (a smaller rehearsal)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "mixed_model_bench.txt"))
    a = ap.parse_args()
    OUT = a.out or None
    dev = torch.device("cuda", 0)
    ctx = pds.Context(0)
    ctx.set_stream(torch.cuda.current_stream(dev))
    gen = torch.Generator(device=dev)
    gen.manual_seed(3)
    shapes = a.shapes.split(",")
    splits = [int(v) for v in a.split.split(",") if v]
    sc = a.scale
    for name, p in (("headline", 8), ("wide", 16)):
        if name in shapes:
            G, m = int(1_000_000 * sc), 100
            off = torch.arange(0, G * m + 1, m, dtype=torch.int64, device=dev)
            X, y = run_shape(name, ctx, gen, dev, off, p, a.reps)
            if name == "headline" and a.sample > 0:
                sample_against_reference_algorithm(X, y, m, p, min(a.sample, G))
            del X, y
    if "long" in shapes:
        G, m = int(10_000 * sc), 10_000
        off = torch.arange(0, G * m + 1, m, dtype=torch.int64, device=dev)
        for sp in splits or [None]:
            X, y = run_shape("long", ctx, gen, dev, off, 8, a.reps, sp)
            del X, y
    if "skewed" in shapes:
        big, G, m = int(10_000_000 * sc), int(100_000 * sc), 100
        off = torch.cat([torch.tensor([0], device=dev), torch.arange(big, big + G * m + 1, m, device=dev)]).to(torch.int64)
        for sp in splits or [None]:
            X, y = run_shape("skewed", ctx, gen, dev, off, 8, a.reps, sp)
            del X, y


if __name__ == "__main__":
    main()
