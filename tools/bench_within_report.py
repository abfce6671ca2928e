"""
lin_reg_report(absorb=) (pds_lin_reg_within_*, csrc/within_pass.hip) on one MI355X, the frame resident in HBM.
Frame: `--rows` (default 1e8) x 16 f64 features, no bias column, y with a per-group level.  Forms (the frames of
tools/bench_cluster_report.py):
    ordered_offsets   1e6 ordered groups x 100 rows, absorb_offsets=
    long_offsets      1e4 groups x 1e4 rows, absorb_offsets=  (below the default within_split_rows of 16 384: whole groups; `--split
                      a,b` adds runs with the option set to each value, which cuts them into row chunks)
    shuffled_keys     the 1e6-group frame with its rows in random order, absorb=  (the sort + gather route)
Per form, in ONE process and alternating: the within report with std_err="se" and "cluster", and the yardstick, the cluster-robust
report of the same frame and the same groups (std_err="cluster", cluster= / cluster_offsets=, add_bias=True), whose code this feature
does not touch.  Times: median / best / worst of `--reps` (default 7) warmed calls by device events.  From one more call per form with
the context's timing classes on: the kernel time of the statistics pass ("grouped_moments": mixed.hip's kernels and their record
sums) and of the per-row pass ("pass2": the within kernels and their record sums), and frame bytes / kernel time as a share of the
8 TB/s HBM peak -- a memory bound.  The expectation to confirm or refute: the within pass costs about what the cluster pass costs
(the same stream plus p + 1 means per group).  Lines are appended to profiles/within_report_bench.txt (`--out`).  No time here is a
pass condition.
"""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
import torch  # noqa: E402

import polars_ds_extension_amd as pds  # noqa: E402
from bench_cluster_report import HBM, make_frame, timed_alternating  # noqa: E402

OUT = None


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if OUT is not None:
        with open(OUT, "a") as fh:
            fh.write(line + "\n")


def kernel_times(ctx, fn):
    ctx.set_timing(True)
    ctx.get_timing()
    rep = fn()
    ctx.synchronize()
    t = ctx.get_timing()
    ctx.set_timing(False)
    return t, rep


def run_form(name, ctx, X, y, reps, p, split=None, absorb_kw=None, cluster_kw=None):
    n = int(y.numel())
    ctx.set_option("within_split_rows", split or 0)
    fns = {
        "within_se": lambda: pds.lin_reg_report(*X, target=y, std_err="se", ctx=ctx, **absorb_kw),
        "within_cluster": lambda: pds.lin_reg_report(*X, target=y, std_err="cluster", ctx=ctx, **absorb_kw),
        "cluster_report": lambda: pds.lin_reg_report(*X, target=y, add_bias=True, std_err="cluster", ctx=ctx, **cluster_kw),
    }
    t = timed_alternating(fns, reps)
    kern = {k: kernel_times(ctx, fns[k]) for k in fns}
    frame_bytes = n * (p + 1) * 8
    rec = {"bench": "within_report", "form": name, "rows": n, "groups": kern["within_se"][1]["n_groups"], "p": p, "split_rows": split or "default",
           "frame_GB": round(frame_bytes / 1e9, 3)}
    for k in fns:
        rec[k + "_ms"] = round(t[k][0], 3)
        rec[k + "_ms_best"], rec[k + "_ms_worst"] = round(t[k][1], 3), round(t[k][2], 3)
    rec["within_cluster_over_cluster_report"] = round(t["within_cluster"][0] / t["cluster_report"][0], 4)
    for k in ("within_se", "within_cluster"):
        stats_ms, pass_ms = kern[k][0]["grouped_moments"][0], kern[k][0]["pass2"][0]
        rec[k + "_stats_pass_kernels_ms"], rec[k + "_row_pass_kernels_ms"] = round(stats_ms, 3), round(pass_ms, 3)
        for tag, ms in (("stats", stats_ms), ("row", pass_ms)):
            rec[f"{k}_{tag}_pass_share_of_8TBps"] = round(frame_bytes / (ms * 1e-3) / HBM, 4) if ms > 0 else None
    rec["cluster_report_pass_kernels_ms"] = round(kern["cluster_report"][0]["pass2"][0], 3)
    rec["cluster_report_moment_pass_kernels_ms"] = round(kern["cluster_report"][0]["moments"][0], 3)
    emit(rec)


def main():
    global OUT
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=float, default=1e8)
    ap.add_argument("--features", type=int, default=16)
    ap.add_argument("--forms", default="ordered_offsets,long_offsets,shuffled_keys")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--split", default="", help="extra runs of long_offsets with within_split_rows set to each value")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "within_report_bench.txt"))
    a = ap.parse_args()
    OUT = a.out or None
    dev = torch.device("cuda", 0)
    ctx = pds.Context(0)
    ctx.set_stream(torch.cuda.current_stream(dev))
    gen = torch.Generator(device=dev)
    gen.manual_seed(11)
    n, p = int(a.rows), a.features
    forms = a.forms.split(",")
    g_many, g_long = max(2, n // 100), max(2, n // 10_000)
    if any(f in forms for f in ("ordered_offsets", "shuffled_keys")):
        X, y, codes = make_frame(gen, dev, g_many * 100, g_many, p)
        off = torch.arange(0, g_many * 100 + 1, 100, dtype=torch.int64, device=dev)
        if "ordered_offsets" in forms:
            run_form("ordered_offsets", ctx, X, y, a.reps, p, absorb_kw={"absorb_offsets": off}, cluster_kw={"cluster_offsets": off})
        if "shuffled_keys" in forms:
            perm = torch.randperm(int(y.numel()), generator=gen, device=dev)
            X = [c[perm] for c in X]
            y, keys = y[perm], (codes * 3 - 7)[perm]
            del perm, codes
            run_form("shuffled_keys", ctx, X, y, a.reps, p, absorb_kw={"absorb": keys}, cluster_kw={"cluster": keys})
            del keys
        del X, y
    if "long_offsets" in forms:
        m = 10_000 if n >= 20_000 else n // 2
        X, y, codes = make_frame(gen, dev, g_long * m, g_long, p)
        del codes
        off = torch.arange(0, g_long * m + 1, m, dtype=torch.int64, device=dev)
        for sp in [None] + [int(v) for v in a.split.split(",") if v]:
            run_form("long_offsets", ctx, X, y, a.reps, p, split=sp, absorb_kw={"absorb_offsets": off}, cluster_kw={"cluster_offsets": off})


if __name__ == "__main__":
    main()
