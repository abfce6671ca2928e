"""
Grouped lin_reg_w_rcond (pds_lr_rcond_grouped_*, csrc/grouped_rcond.hip) on one MI355X, inputs resident in HBM, offsets form.
Shapes: 1e6 groups x 100 rows x 8 f64 features + bias, and x 16 + bias; each once full rank and once with 0.1 % of the groups given
a duplicated column (their last feature a copy of their first).  Per shape: median / best / worst of `--reps` warmed calls by device
events, and beside it
  (a) the parent's only way: one `lstsq.lin_reg_w_rcond` call per group over the first `--sample` groups of the same frame,
      alternating with the new call on those groups; the factor per group between the two;
  (b) `lin_reg_by` on the same frame in the same process, and the ratio to it;
  (c) frame bytes / the fit kernel's own time (the context's "iterative" timing class of one more call) as a share of the 8 TB/s HBM
      peak -- the model is "one frame read + an on-chip decomposition": the share says how far the decomposition is from free.
Writes its JSON lines to stdout and to `--out` (default: profiles/grouped_rcond_bench.txt).
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

HBM = 8.0e12
RCOND = 1e-6
LINES = []


def emit(rec):
    line = json.dumps(rec)
    LINES.append(line)
    print(line, flush=True)


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


def make_frame(gen, dev, G, m, p, dup_every):
    """x ~ N(0, 1), y = x . beta + 0.2 + noise; dup_every > 0: every dup_every-th group's last feature is a copy of its first"""
    n = G * m
    X = [torch.randn(n, generator=gen, device=dev, dtype=torch.float64) for _ in range(p)]
    y = torch.full((n,), 0.2, device=dev, dtype=torch.float64)
    for j in range(p):
        y += (0.5 * (-1) ** j * (j + 1) / p) * X[j]
    y += 0.1 * torch.randn(n, generator=gen, device=dev, dtype=torch.float64)
    n_dup = 0
    if dup_every:
        first = X[0].view(G, m)
        last = X[p - 1].view(G, m)
        last[::dup_every] = first[::dup_every]
        n_dup = len(range(0, G, dup_every))
    return X, y, n_dup


def run_shape(name, ctx, gen, dev, G, m, p, dup_every, reps, sample):
    X, y, n_dup = make_frame(gen, dev, G, m, p, dup_every)
    off = torch.arange(0, G * m + 1, m, dtype=torch.int64, device=dev)
    call = lambda: pds.lin_reg_w_rcond_by(*X, target=y, group_offsets=off, add_bias=True, rcond=RCOND, ctx=ctx)  # noqa: E731
    ms, best, worst = timed(call, reps)
    ctx.set_timing(True)
    ctx.get_timing()
    co, sv, nu = call()
    ctx.synchronize()
    kernel_ms = ctx.get_timing()["iterative"][0]
    ctx.set_timing(False)
    by_ms, _, _ = timed(lambda: pds.lin_reg_by(*X, target=y, group_offsets=off, add_bias=True, ctx=ctx), reps)
    pp = p + 1
    frame_bytes = G * m * (p + 1) * 8
    thr = RCOND * sv[:, :1]
    emit({"bench": "grouped_rcond", "shape": name, "groups": G, "rows_per_group": m, "p": p, "bias": True, "rcond": RCOND,
          "groups_with_duplicated_column": n_dup, "groups_with_a_cut_singular_value": int(((sv * sv) < thr).any(dim=1).sum().item()),
          "null_groups": int(nu.sum().item()), "ms": round(ms, 3), "ms_best": round(best, 3), "ms_worst": round(worst, 3),
          "fit_kernel_ms": round(kernel_ms, 3), "us_per_group": round(ms * 1e3 / G, 4),
          "lin_reg_by_ms": round(by_ms, 3), "ratio_to_lin_reg_by": round(ms / by_ms, 2),
          "frame_GB": round(frame_bytes / 1e9, 3), "algorithmic_GB": round((frame_bytes + G * (2 * pp * 8 + 1 + 8)) / 1e9, 3),
          "frame_bytes_per_kernel_time_share_of_8TBps": round(frame_bytes / (max(kernel_ms, 1e-6) * 1e-3) / HBM, 4)})
    if sample > 0:
        k = min(sample, G)
        Xs = [c[:k * m] for c in X]
        ys = y[:k * m]
        offs = off[:k + 1]
        t_single, t_grouped = [], []
        for rep in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for g in range(k):
                pds.lin_reg_w_rcond(*[c[g * m:(g + 1) * m] for c in Xs], target=ys[g * m:(g + 1) * m], add_bias=True, rcond=RCOND, ctx=ctx)
            torch.cuda.synchronize()
            t_single.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            pds.lin_reg_w_rcond_by(*Xs, target=ys, group_offsets=offs, add_bias=True, rcond=RCOND, ctx=ctx)
            torch.cuda.synchronize()
            t_grouped.append((time.perf_counter() - t0) * 1e3)
        s, g_ = float(np.median(t_single)), float(np.median(t_grouped))
        emit({"bench": "grouped_rcond_vs_per_group_call", "shape": name, "groups": k, "rows_per_group": m, "p": p,
              "per_group_calls_ms": round(s, 2), "per_group_call_us_per_group": round(s * 1e3 / k, 2),
              "grouped_call_on_the_sample_ms": round(g_, 3), "factor_on_the_sample": round(s / g_, 1),
              "grouped_full_frame_us_per_group": round(ms * 1e3 / G, 4),
              "factor_per_group_against_the_full_frame_call": round((s / k) / (ms / G), 1)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sample", type=int, default=1000)
    ap.add_argument("--scale", type=float, default=1.0, help="scales the group count (a smaller rehearsal)")
    ap.add_argument("--widths", default="8,16")
    ap.add_argument("--out", default=str(Path(__file__).resolve().parent.parent / "profiles" / "grouped_rcond_bench.txt"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    ctx = pds.Context(0)
    ctx.set_stream(torch.cuda.current_stream(dev))
    gen = torch.Generator(device=dev)
    gen.manual_seed(3)
    G, m = int(1_000_000 * a.scale), 100
    for p in (int(v) for v in a.widths.split(",")):
        run_shape(f"p{p}_full_rank", ctx, gen, dev, G, m, p, 0, a.reps, a.sample)
        run_shape(f"p{p}_0.1pct_duplicated_column", ctx, gen, dev, G, m, p, 1000, a.reps, a.sample)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("# python tools/grouped_rcond_bench.py (one MI355X, device-resident, offsets form, median of %d warmed calls)\n" % a.reps
                               + "\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
