"""
The grouped GLM report (pds_glm_report_grouped_*, csrc/grouped_glm_report.hip) next to the fit it contains, on one MI355X, inputs
resident in HBM, offsets form.  Per shape, in one process and session: median / best / worst of `--reps` warmed calls by device
events of `glm_report_by` and of `glm_by` on the same frame (the fit is unchanged code: the baseline), alternating A / B / A / B so
that a drift of the clocks hits both alike; the ratio of the medians; and from one more call with the context's kernel timers on
the fit kernel's own time ("iterative") and the report kernel's ("pass2": nothing else of that class runs in the call).
Shapes (`--shapes`): headline = 1e6 groups x 100 rows x 8 features + bias, binomial; wide = the same with 16 features, poisson;
one = one 1e7-row group (8 features + bias, binomial) through the piece route -- there the fit is the full-device iteration.
`--scale` scales the row / group counts (a smaller rehearsal).
"""
import argparse
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch  # noqa: E402

import polars_ds_extension_amd as pds  # noqa: E402
from grouped_glm_bench import make_frame  # noqa: E402


def timed_pair(fa, fb, reps, warm=2):
    """medians (and best / worst) of fa and fb, called alternately"""
    for _ in range(warm):
        fa()
        fb()
    s = torch.cuda.current_stream()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = ([], [])
    for _ in range(reps):
        for ms, fn in zip(out, (fa, fb)):
            a.record(s)
            fn()
            b.record(s)
            b.synchronize()
            ms.append(a.elapsed_time(b))
    stats = []
    for ms in out:
        ms.sort()
        stats.append((ms[len(ms) // 2], ms[0], ms[-1]))
    return stats


def run_shape(name, ctx, gen, dev, off, p, family, reps):
    n = int(off[-1].item())
    ng = int(off.numel()) - 1
    X, y = make_frame(gen, dev, n, p, family, off)
    kw = dict(target=y, group_offsets=off, family=family, add_bias=True, tol=1e-8, max_iter=100, ctx=ctx)
    report = lambda: pds.glm_report_by(*X, **kw)  # noqa: E731
    fit = lambda: pds.glm_by(*X, **kw)  # noqa: E731
    (r_ms, r_best, r_worst), (f_ms, f_best, f_worst) = timed_pair(report, fit, reps)
    ctx.set_timing(True)
    ctx.get_timing()
    d = report()
    ctx.synchronize()
    tm = ctx.get_timing()
    ctx.set_timing(False)
    n_long = int(((off[1:] - off[:-1]) > 16384).sum().item())
    rec = {"bench": "grouped_glm_report", "shape": name, "groups": ng, "rows": n, "p": p, "family": family,
           "report_ms": round(r_ms, 3), "report_ms_best": round(r_best, 3), "report_ms_worst": round(r_worst, 3),
           "fit_ms": round(f_ms, 3), "fit_ms_best": round(f_best, 3), "fit_ms_worst": round(f_worst, 3),
           "report_over_fit": round(r_ms / f_ms, 3), "fit_kernel_ms": round(tm["iterative"][0], 3),
           "report_kernel_ms": round(tm["pass2"][0], 3), "report_kernel_over_fit_kernel": round(tm["pass2"][0] / max(tm["iterative"][0], 1e-9), 3),
           "mean_n_iter": round(float(d["n_iter"].float().mean().item()), 2), "groups_through_pieces": n_long,
           "null_reports": int(d["report_null"].sum().item())}
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="headline,wide,one")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--scale", type=float, default=1.0)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    ctx = pds.Context(0)
    ctx.set_stream(torch.cuda.current_stream(dev))
    gen = torch.Generator(device=dev)
    gen.manual_seed(3)
    shapes = a.shapes.split(",")
    G, m = int(1_000_000 * a.scale), 100
    off = torch.arange(0, G * m + 1, m, dtype=torch.int64, device=dev)
    if "headline" in shapes:
        run_shape("headline", ctx, gen, dev, off, 8, "binomial", a.reps)
    if "wide" in shapes:
        run_shape("wide", ctx, gen, dev, off, 16, "poisson", a.reps)
    if "one" in shapes:
        big = int(10_000_000 * a.scale)
        run_shape("one", ctx, gen, dev, torch.tensor([0, big], dtype=torch.int64, device=dev), 8, "binomial", max(3, a.reps // 2))


if __name__ == "__main__":
    main()
