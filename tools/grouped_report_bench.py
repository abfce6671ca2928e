"""
Grouped lin_reg_report (pds_lin_reg_report_grouped_*) on one MI355X, inputs resident in HBM: time per call from device events
after warm-up, the grouped fit (`lin_reg_by`) on the same frame in the same process, algorithmic bytes and the fraction of 8 TB/s.
Headline: 1e6 groups x 100 rows x 16 f64 features (and 8), for se / hc1 / hc3.  `--skewed`: one group of most of the rows beside
many small ones, against the single-frame report on the big group's rows (the case that splits groups across waves).
`--weights`: the weighted report (pds_wls_report_grouped_*, se only) on the same frame as well; its streams read one more column, so
its bytes are (p + 2) / (p + 1) of the unweighted call's.  A library without the entry point (an older build in an A/B run) says so
and times the unweighted calls only.  Every record carries the median, the best and the worst repetition.
A per-kernel split comes from a separate run under `rocprofv3 --kernel-trace --stats -- python tools/grouped_report_bench.py ...`.
Usage: python tools/grouped_report_bench.py [--groups 1000000] [--rows 100] [--feats 16,8] [--se se,hc1,hc3] [--reps 5] [--skewed]
                                            [--weights]
"""
import argparse
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch  # noqa: E402

import polars_ds_extension_amd as pds  # noqa: E402

HBM = 8.0e12


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=1_000_000)
    ap.add_argument("--rows", type=int, default=100)
    ap.add_argument("--feats", default="16,8")
    ap.add_argument("--se", default="se,hc1,hc3")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skewed", action="store_true")
    ap.add_argument("--weights", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    ctx = pds.Context(0)
    ctx.set_stream(torch.cuda.current_stream(dev))
    gen = torch.Generator(device=dev)
    gen.manual_seed(3)
    G, m = a.groups, a.rows
    n = G * m
    for p in [int(v) for v in a.feats.split(",")]:
        X = [torch.randn(n, generator=gen, device=dev, dtype=torch.float64) for _ in range(p)]
        y = sum((0.1 * (j + 1)) * X[j] for j in range(p)) + torch.randn(n, generator=gen, device=dev, dtype=torch.float64)
        if a.skewed:  # one group holds half the rows, the rest are m-row groups
            big = n // 2
            off = torch.cat([torch.tensor([0], device=dev), torch.arange(big, n + 1, m, device=dev)]).to(torch.int64)
        else:
            off = torch.arange(0, n + 1, m, dtype=torch.int64, device=dev)
        ng = int(off.numel()) - 1
        by_ms, _, _ = timed(lambda: pds.lin_reg_by(*X, target=y, group_offsets=off, add_bias=True, ctx=ctx), a.reps)
        pp = p + 1
        for se in a.se.split(","):
            ms, best, worst = timed(lambda: pds.lin_reg_report_by(*X, target=y, group_offsets=off, add_bias=True, std_err=se, ctx=ctx),
                                    a.reps)
            # the frame is read twice (Gram records, residual pass); outputs: 6 p' values + r2 / adj_r2 per group + the null byte
            nbytes = 2 * n * (p + 1) * 8 + ng * (6 * pp + 2) * 8 + ng
            rec = {"bench": "grouped_report", "shape": "skewed" if a.skewed else "uniform", "groups": ng, "rows": n, "p": p,
                   "se": se, "ms": round(ms, 3), "ms_best": round(best, 3), "ms_worst": round(worst, 3), "lin_reg_by_ms": round(by_ms, 3),
                   "ratio_to_lin_reg_by": round(ms / by_ms, 2), "algorithmic_GB": round(nbytes / 1e9, 2),
                   "fraction_of_8TBps": round(nbytes / (ms * 1e-3) / HBM, 3)}
            if a.skewed:
                bigX = [c[:big] for c in X]
                sms, _, _ = timed(lambda: pds.lin_reg_report(*bigX, target=y[:big], add_bias=True, std_err=se, ctx=ctx), a.reps)
                rec["single_report_big_group_ms"] = round(sms, 3)
            print(json.dumps(rec), flush=True)
        if a.weights and not hasattr(ctx._lib, "pds_wls_report_grouped_f64"):
            print(json.dumps({"bench": "grouped_wls_report", "p": p, "skipped": "this library has no pds_wls_report_grouped_*"}), flush=True)
        elif a.weights:
            w = 0.25 + 3.75 * torch.rand(n, generator=gen, device=dev, dtype=torch.float64)
            ms, best, worst = timed(lambda: pds.lin_reg_report_by(*X, target=y, group_offsets=off, add_bias=True, weights=w, ctx=ctx), a.reps)
            nbytes = 2 * n * (p + 2) * 8 + ng * (6 * pp + 2) * 8 + ng
            print(json.dumps({"bench": "grouped_wls_report", "shape": "skewed" if a.skewed else "uniform", "groups": ng, "rows": n, "p": p,
                              "se": "se", "ms": round(ms, 3), "ms_best": round(best, 3), "ms_worst": round(worst, 3),
                              "lin_reg_by_ms": round(by_ms, 3), "ratio_to_lin_reg_by": round(ms / by_ms, 2),
                              "algorithmic_GB": round(nbytes / 1e9, 2), "fraction_of_8TBps": round(nbytes / (ms * 1e-3) / HBM, 3)}), flush=True)
            del w
        del X, y


if __name__ == "__main__":
    main()
