"""
lin_reg_report(absorb=..., std_err="cluster", cluster_key=) (pds_lin_reg_within_cl_* / pds_lin_reg_within2_cl_*, csrc/within_cluster.hip)
on one MI355X, the frame resident in HBM.
Frames: the two-key panel of bench_within2_report.py (`--firms` x `--periods` cells less `--drop`: 1e5 x 100 less 10 % = 9.0e6 rows x 16
f64 features, rows in firm order) and the one-key frame of bench_within_report.py's ordered_offsets form (`--rows` = 1e8 rows x 16, 1e6
ordered groups of 100 rows, absorb_offsets=).  `--frames two_key,one_key` picks.
In ONE process and alternating, `--reps` (default 7) warmed calls each by device events, median / best / worst:
    yardstick   std_err="cluster" on the (first) absorbed key: the existing call, whose kernels this feature leaves as they were
    crossing    the same call with cluster_key = a key of `--crossing` (50) levels drawn at random per row
    nested      the same call with cluster_key = a key of G / 100 levels nested over the (first) absorbed key, its groups not adjacent
From one more call of each with the context's timing classes on, the split by kernel: the staging pass (within_row_scores_kernel, class
"iterative"), the ordering (iota, radix sort and level starts: class "grouped_moments" less the yardstick's, which is the statistics
pass both calls run), the gather (cluster_gather_chunk_kernel, "rolling"), the meat with its record sum (score_long_meat_kernel<false>,
"solve") and the nestedness kernels ("graph" less the yardstick's); bytes over time of the staging pass (frame read + n p 8 written)
and of the gather (n p 8 read) against the 8 TB/s HBM peak.  torch.unique of the cluster key (the dense coding inside the call:
plumbing) is timed on its own.
`--lib PATH` loads another build of the library (the parent commit's, for the A/B of the EXISTING call in a series of processes that
alternate the two builds); symbols it lacks are left out: the record then holds the yardstick alone.  `--yardstick-only` does the same
on this build.  Lines are appended to profiles/within_cluster_bench.txt (`--out`).  No time here is a pass condition.
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
from bench_within2_report import make_panel  # noqa: E402

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


def event_ms(fn):
    s = torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    fn()
    e1.record(s)
    e1.synchronize()
    return e0.elapsed_time(e1)


def run_frame(name, ctx, label, X, y, group_code, n_groups, crossing, reps, has_cl, call):
    """call(**kw) is the report on this frame; group_code: the dense level of the first absorbed key per row"""
    n, p = int(y.numel()), len(X)
    fns = {"yardstick": lambda: call()}
    keys = {}
    if has_cl:
        gen = torch.Generator(device=y.device)
        gen.manual_seed(5)
        keys["crossing"] = torch.randint(0, crossing, (n,), generator=gen, device=y.device, dtype=torch.int64)
        levels = max(2, n_groups // 100)
        keys["nested"] = (group_code * 7919) % levels  # (7919 is prime: the groups of a cluster are spread over the frame)
        for k, key in keys.items():
            fns[k] = lambda key=key: call(cluster_key=key)
    t = timed_alternating(fns, reps)
    rec = {"bench": "within_cluster", "build": label, "frame": name, "rows": n, "p": p, "groups": n_groups, "frame_GB": round(n * (p + 1) * 8 / 1e9, 3)}
    for k in fns:
        rec[k + "_ms"], rec[k + "_ms_best"], rec[k + "_ms_worst"] = (round(v, 3) for v in t[k])
    kern = {k: kernel_times(ctx, fn) for k, fn in fns.items()}
    base = kern["yardstick"][0]
    rec["yardstick_kernels_ms"] = {k: round(v[0], 3) for k, v in base.items() if v[1]}
    score_bytes = n * p * 8
    for k in keys:
        tm, rep = kern[k]
        rec[k + "_over_yardstick"] = round(t[k][0] / t["yardstick"][0], 3)
        rec[k + "_clusters"], rec[k + "_nested"] = rep["n_clusters"], list(rep["absorb_nested"])
        split = {"staging_ms": tm["iterative"][0], "ordering_ms": tm["grouped_moments"][0] - base["grouped_moments"][0], "gather_ms": tm["rolling"][0],
                 "meat_ms": tm["solve"][0], "nestedness_ms": tm["graph"][0] - base["graph"][0], "row_pass_ms": tm["pass2"][0]}
        rec[k + "_split"] = {a: round(v, 3) for a, v in split.items()}
        rec[k + "_yardstick_row_pass_ms"] = round(base["pass2"][0], 3)
        rec[k + "_staging_share_of_8TBps"] = round((n * (p + 1) * 8 + score_bytes) / (split["staging_ms"] * 1e-3) / HBM, 4)
        rec[k + "_gather_share_of_8TBps"] = round(score_bytes / (split["gather_ms"] * 1e-3) / HBM, 4)
        rec[k + "_torch_unique_of_cluster_key_ms"] = round(event_ms(lambda key=keys[k]: torch.unique(key, return_inverse=True)), 3)
    emit(rec)


def main():
    global OUT
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", default="two_key,one_key")
    ap.add_argument("--rows", type=float, default=1e8)
    ap.add_argument("--firms", type=float, default=1e5)
    ap.add_argument("--periods", type=int, default=100)
    ap.add_argument("--drop", type=float, default=0.1)
    ap.add_argument("--features", type=int, default=16)
    ap.add_argument("--crossing", type=int, default=50)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--tol", type=float, default=1e-8)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "within_cluster_bench.txt"))
    ap.add_argument("--lib", default=None, help="another build of libpds_lstsq_hip.so to measure")
    ap.add_argument("--label", default="this")
    ap.add_argument("--yardstick-only", action="store_true")
    a = ap.parse_args()
    OUT = a.out or None
    if a.lib:
        pds._lib.LIB_PATH = Path(a.lib).resolve()
    has_cl = hasattr(pds._lib.load(), "pds_lin_reg_within_cl_grouped_f64") and not a.yardstick_only
    dev = torch.device("cuda", 0)
    ctx = pds.Context(0)
    ctx.set_stream(torch.cuda.current_stream(dev))
    gen = torch.Generator(device=dev)
    gen.manual_seed(11)
    p = a.features
    frames = a.frames.split(",")
    if "two_key" in frames:
        X, y, firm, period = make_panel(gen, dev, int(a.firms), a.periods, a.drop, p)
        n_firms = int(torch.unique(firm).numel())
        code = torch.unique(firm, return_inverse=True)[1]
        run_frame(f"two keys: panel {int(a.firms)} x {a.periods} less {a.drop:.0%}, absorb_tol {a.tol:g}", ctx, a.label, X, y, code, n_firms, a.crossing,
                  a.reps, has_cl,
                  lambda **kw: pds.lin_reg_report(*X, target=y, std_err="cluster", absorb=[firm, period], absorb_tol=a.tol, ctx=ctx, **kw))
        del X, y, firm, period, code
    if "one_key" in frames:
        g = max(2, int(a.rows) // 100)
        X, y, codes = make_frame(gen, dev, g * 100, g, p)
        off = torch.arange(0, g * 100 + 1, 100, dtype=torch.int64, device=dev)
        run_frame(f"one key: {g} ordered groups x 100 rows, absorb_offsets", ctx, a.label, X, y, codes, g, a.crossing, a.reps, has_cl,
                  lambda **kw: pds.lin_reg_report(*X, target=y, std_err="cluster", absorb_offsets=off, ctx=ctx, **kw))


if __name__ == "__main__":
    main()
