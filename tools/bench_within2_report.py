"""
lin_reg_report(absorb=[k1, k2]) (pds_lin_reg_within2_*, csrc/within2_sweep.hip) on one MI355X, the frame resident in HBM.
Frame: `--firms` x `--periods` cells (default 1e5 x 100 = 1e7 rows) with `--drop` (default 10 %) of the cells dropped at random, 16 f64
features, no bias column; features and y carry a level per firm and per period.  Rows are in firm order (ordered keys: nothing is
sorted or gathered, as in the one-key bench's ordered_offsets form).
In ONE process and alternating: the two-key report (std_err="se" and "cluster") and the yardstick, the one-key report absorb=k1 of
the same frame, whose code this feature leaves bit for bit as it was.  Times: median / best / worst of `--reps` (default 7) warmed calls by
device events.  From one more call with the context's timing classes on: the sweeps used, the kernel time per sweep of the factor-1
kernels ("sweep_factor1": contiguous levels, reads the frame) and of the factor-2 kernels ("sweep_factor2": gathered chunk sums, level
sums and delta), frame bytes / sweep time against the 8 TB/s HBM peak and against the model of 2 reads of the frame per sweep, the
f64 copy + moments ("moments"), the code ordering with the final stage's statistics pass ("grouped_moments"), the projected columns
with the final stage's row pass ("pass2"), and what is left of the call: the host's pass over the codes (range, counts, components)
with the copies and the per-sweep synchronisations -- since the graph pass runs on the device (csrc/within2_graph.hip, class "graph":
level counts, hook-and-compress rounds, and the effects kernels of fixed_effects) that is the range check's and the rounds' small copies.
`fixed_effects` (the report plus the estimated effects) is timed beside the report, with the rounds the labelling took.  `--lib PATH`
loads another build of the library (an earlier commit's, for an A/B in a series of processes that alternate the two builds; symbols it
lacks are left out of the record).  One more call with absorb_max_iter=1 (it fails after one sweep) is timed by the
wall clock: everything in front of the sweeps -- the host pass among it -- and one sweep.  Lines are appended to profiles/within2_report_bench.txt
(`--out`).  No time here is a pass condition.

`--accel` measures the accelerated iteration (absorb_accel="irons_tuck": cycles of two sweeps and an extrapolation of the factor-2
table) instead, into profiles/within2_accel_bench.txt: on the panel above (at `--tol` and at 1e-13), and on a FEW-MOVERS frame at scale built with
tests/within2_cases.py::movers_frame's rule at p = 4 (`--movers WORKERS,FIRMS,MOVERS`, 6 rows per worker), the plain and the
accelerated call alternate in this one process, `--reps` warmed calls each by device events; per frame one record with both calls'
times and sweep counts, the time per sweep of each (call time / sweeps, and the sweep kernels' time / sweeps from the timing
classes; the extrapolation's two kernels are in "sweep_factor2"), and the ratios plain / accelerated of the times and of the sweeps.
"""
import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
import torch  # noqa: E402

import polars_ds_extension_amd as pds  # noqa: E402
from polars_ds_extension_amd._lib import PdsError  # noqa: E402
from bench_cluster_report import HBM, timed_alternating  # noqa: E402

OUT = None


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if OUT is not None:
        with open(OUT, "a") as fh:
            fh.write(line + "\n")


def make_panel(gen, dev, firms, periods, drop, p):
    """(X, y, firm, period): the cells of a firms x periods panel that survive, in firm order; a level per firm and per period"""
    keep = torch.rand(firms * periods, generator=gen, device=dev) >= drop
    cell = torch.nonzero(keep).reshape(-1)
    del keep
    firm, period = cell // periods, cell % periods
    del cell
    n = int(firm.numel())
    X = []
    for j in range(p):
        X.append(torch.randn(n, generator=gen, device=dev, dtype=torch.float64) + 3.0 * torch.randn(firms, generator=gen, device=dev, dtype=torch.float64)[firm]
                 + 3.0 * torch.randn(periods, generator=gen, device=dev, dtype=torch.float64)[period])
    y = (3.0 * torch.randn(firms, generator=gen, device=dev, dtype=torch.float64)[firm] + 3.0 * torch.randn(periods, generator=gen, device=dev,
                                                                                                          dtype=torch.float64)[period]
         + torch.randn(n, generator=gen, device=dev, dtype=torch.float64))
    for j in range(p):
        y += (0.5 * (-1) ** j * (j + 1) / p) * X[j]
    return X, y, firm, period


def make_movers(dev, workers, firms, movers, p=4):
    """tests/within2_cases.py::movers_frame (seed 0, 6 rows per worker) on the device: (X, y, worker, firm)"""
    sys.path.insert(0, str(ROOT / "tests"))
    import numpy as np
    import within2_cases as c2

    F, y, off, k1, k2 = c2.movers_frame(p, 0, workers, firms, 6, movers)
    X = [torch.from_numpy(np.ascontiguousarray(F[:, j])).to(dev) for j in range(p)]
    return X, torch.from_numpy(np.array(y)).to(dev), torch.from_numpy(np.array(k1)).to(dev), torch.from_numpy(np.array(k2)).to(dev)


def accel_record(ctx, name, X, y, k1, k2, tol, reps, label):
    """the plain and the accelerated report on one frame, alternating in this process"""
    fns = {m: (lambda m=m: pds.lin_reg_report(*X, target=y, std_err="se", absorb=[k1, k2], absorb_tol=tol, absorb_max_iter=100_000,
                                              absorb_accel=m, ctx=ctx)) for m in ("none", "irons_tuck")}
    t = timed_alternating(fns, reps)
    n, p = int(y.numel()), len(X)
    rec = {"bench": "within2_accel", "build": label, "frame": name, "rows": n, "p": p, "absorb_tol": tol}
    per = {}
    for m, fn in fns.items():
        ctx.set_timing(True)
        ctx.get_timing()
        r = fn()
        ctx.synchronize()
        tm = ctx.get_timing()
        ctx.set_timing(False)
        key = "plain" if m == "none" else "accel"
        sweeps = r["n_iter"]
        rec.update({"levels1": r["n_groups"], "levels2": r["n_groups2"], "components": r["n_components"]})
        rec[key + "_sweeps"] = sweeps
        rec[key + "_ms"], rec[key + "_ms_best"], rec[key + "_ms_worst"] = (round(v, 3) for v in t[m])
        rec[key + "_call_ms_per_sweep"] = round(t[m][0] / sweeps, 5)
        rec[key + "_sweep_kernels_ms_per_sweep"] = round((tm["sweep_factor1"][0] + tm["sweep_factor2"][0]) / sweeps, 5)
        rec[key + "_sweep_kernel_launches"] = tm["sweep_factor1"][1] + tm["sweep_factor2"][1]
        rec[key + "_call_less_sweep_kernels_ms"] = round(t[m][0] - (tm["sweep_factor1"][0] + tm["sweep_factor2"][0]), 3)
        per[key] = rec[key + "_sweep_kernels_ms_per_sweep"]
    rec["sweeps_plain_over_accel"] = round(rec["plain_sweeps"] / rec["accel_sweeps"], 3)
    rec["time_plain_over_accel"] = round(rec["plain_ms"] / rec["accel_ms"], 3)
    rec["call_ms_per_sweep_accel_over_plain"] = round(rec["accel_call_ms_per_sweep"] / rec["plain_call_ms_per_sweep"], 4)
    rec["sweep_kernels_ms_per_sweep_accel_over_plain"] = round(per["accel"] / per["plain"], 4)
    emit(rec)


def main():
    global OUT
    ap = argparse.ArgumentParser()
    ap.add_argument("--firms", type=float, default=1e5)
    ap.add_argument("--periods", type=int, default=100)
    ap.add_argument("--drop", type=float, default=0.1)
    ap.add_argument("--features", type=int, default=16)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--tol", type=float, default=1e-8)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "within2_report_bench.txt"))
    ap.add_argument("--lib", default=None, help="another build of libpds_lstsq_hip.so to measure")
    ap.add_argument("--label", default="this")
    ap.add_argument("--accel", action="store_true", help="the accelerated iteration against the plain one (profiles/within2_accel_bench.txt)")
    ap.add_argument("--movers", default="300000,200,15000", help="--accel: workers,firms,movers of the few-movers frame (6 rows per worker)")
    a = ap.parse_args()
    if a.accel and a.out == ap.get_default("out"):
        a.out = str(ROOT / "profiles" / "within2_accel_bench.txt")
    OUT = a.out or None
    if a.lib:
        pds._lib.LIB_PATH = Path(a.lib).resolve()
    has_fx = hasattr(pds._lib.load(), "pds_lin_reg_within2_fx_by_key_f64")
    dev = torch.device("cuda", 0)
    ctx = pds.Context(0)
    ctx.set_stream(torch.cuda.current_stream(dev))
    gen = torch.Generator(device=dev)
    gen.manual_seed(11)
    p = a.features
    X, y, firm, period = make_panel(gen, dev, int(a.firms), a.periods, a.drop, p)
    n = int(y.numel())
    if a.accel:
        for tol in sorted({a.tol, 1e-13}, reverse=True):
            accel_record(ctx, f"panel {int(a.firms)} x {a.periods} less {a.drop:.0%}", X, y, firm, period, tol, a.reps, a.label)
        del X, y, firm, period
        workers, firms, movers = (int(v) for v in a.movers.split(","))
        accel_record(ctx, f"few movers {workers} workers x 6 rows in {firms} firms, {movers} movers", *make_movers(dev, workers, firms, movers),
                     a.tol, a.reps, a.label)
        return
    fns = {
        "two_keys_se": lambda: pds.lin_reg_report(*X, target=y, std_err="se", absorb=[firm, period], absorb_tol=a.tol, ctx=ctx),
        "two_keys_cluster": lambda: pds.lin_reg_report(*X, target=y, std_err="cluster", absorb=[firm, period], absorb_tol=a.tol, ctx=ctx),
        "one_key_se": lambda: pds.lin_reg_report(*X, target=y, std_err="se", absorb=firm, ctx=ctx),
        "one_key_cluster": lambda: pds.lin_reg_report(*X, target=y, std_err="cluster", absorb=firm, ctx=ctx),
    }
    if has_fx:
        fns["fixed_effects_se"] = lambda: pds.fixed_effects(*X, target=y, std_err="se", absorb=[firm, period], absorb_tol=a.tol, ctx=ctx)
    t = timed_alternating(fns, a.reps)
    kern = {}
    for k in ("two_keys_se", "one_key_se"):
        ctx.set_timing(True)
        ctx.get_timing()
        rep = fns[k]()
        ctx.synchronize()
        kern[k] = (ctx.get_timing(), rep)
        ctx.set_timing(False)
    # the dense codes of key 2 are made by torch.unique inside the call: plumbing, timed here on its own
    s = torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    torch.unique(period, return_inverse=True)
    e1.record(s)
    e1.synchronize()
    unique_ms = e0.elapsed_time(e1)
    # the host's pass over the codes: a call that is stopped after ONE sweep has everything but the other sweeps and the final stage
    t0 = time.perf_counter()
    try:
        pds.lin_reg_report(*X, target=y, std_err="se", absorb=[firm, period], absorb_tol=1e-300, absorb_max_iter=1, ctx=ctx)
    except PdsError:
        pass
    torch.cuda.synchronize()
    one_sweep_wall_ms = (time.perf_counter() - t0) * 1e3
    tm, rep = kern["two_keys_se"]
    sweeps = rep["n_iter"]
    frame_bytes = n * (p + 1) * 8
    s1, s2 = tm["sweep_factor1"][0] / sweeps, tm["sweep_factor2"][0] / sweeps
    rec = {"bench": "within2_report", "build": a.label, "rows": n, "firms": rep["n_groups"], "periods": rep["n_groups2"], "components": rep["n_components"], "p": p,
           "absorb_tol": a.tol, "frame_GB": round(frame_bytes / 1e9, 3), "sweeps": sweeps}
    for k in fns:
        rec[k + "_ms"], rec[k + "_ms_best"], rec[k + "_ms_worst"] = (round(v, 3) for v in t[k])
    rec["two_over_one_key_se"] = round(t["two_keys_se"][0] / t["one_key_se"][0], 3)
    rec["sweep_factor1_kernels_ms_per_sweep"], rec["sweep_factor2_kernels_ms_per_sweep"] = round(s1, 4), round(s2, 4)
    rec["sweep_kernels_ms_per_sweep"] = round(s1 + s2, 4)
    rec["frame_bytes_over_sweep_time_share_of_8TBps"] = round(frame_bytes / ((s1 + s2) * 1e-3) / HBM, 4)
    rec["model_2_frame_reads_per_sweep_share_of_8TBps"] = round(2 * frame_bytes / ((s1 + s2) * 1e-3) / HBM, 4)
    rec["copy_and_moments_kernels_ms"] = round(tm["moments"][0], 3)
    rec["code_ordering_and_final_statistics_kernels_ms"] = round(tm["grouped_moments"][0], 3)
    rec["projected_columns_and_final_row_pass_kernels_ms"] = round(tm["pass2"][0], 3)
    rec["graph_pass_kernels_ms"], rec["graph_pass_launches"] = round(tm["graph"][0], 3), tm["graph"][1]
    all_kernels = sum(tm[k][0] for k in ("moments", "grouped_moments", "pass2", "sweep_factor1", "sweep_factor2", "graph"))
    rec["all_kernels_ms"] = round(all_kernels, 3)
    rec["call_less_kernels_ms"] = round(t["two_keys_se"][0] - all_kernels, 3)
    if has_fx:
        ctx.set_timing(True)
        ctx.get_timing()
        fe = fns["fixed_effects_se"]()
        ctx.synchronize()
        rec["fixed_effects_graph_rounds"] = fe["n_graph_rounds"]
        rec["fixed_effects_graph_and_effects_kernels_ms"] = round(ctx.get_timing()["graph"][0], 3)
        ctx.set_timing(False)
        rec["fixed_effects_over_report_se"] = round(t["fixed_effects_se"][0] / t["two_keys_se"][0], 3)
    rec["torch_unique_of_key2_ms"] = round(unique_ms, 3)
    rec["call_stopped_after_one_sweep_wall_ms"] = round(one_sweep_wall_ms, 3)
    one = kern["one_key_se"][0]
    rec["one_key_statistics_pass_kernels_ms"], rec["one_key_row_pass_kernels_ms"] = round(one["grouped_moments"][0], 3), round(one["pass2"][0], 3)
    rec["sweep_over_one_key_row_pass"] = round((s1 + s2) / one["pass2"][0], 3)
    emit(rec)


if __name__ == "__main__":
    main()
