"""
lin_reg_report(std_err="cluster") (pds_lin_reg_report_cluster_*, csrc/cluster_meat.hip) on one MI355X, the frame resident in HBM.
Frame: `--rows` (default 1e8) x 16 f64 features + bias, y with a per-cluster shock.  Forms:
    ordered_offsets   1e6 ordered clusters x 100 rows, cluster_offsets=
    ordered_keys      the same clusters as an ordered int64 key column, cluster=  (the order check; nothing moves)
    long_offsets      1e4 clusters x 1e4 rows, cluster_offsets=  (below the default cluster_split_rows of 16 384: whole clusters;
                      `--split a,b` adds runs with the option set to each value, which cuts them into row chunks;
                      `--waves a,b` adds runs of the two offsets forms with cluster_waves set: how the default grid was chosen)
    shuffled_keys     the 1e6-cluster frame with its rows in random order, cluster=  (the sort + gather route)
Per form, in ONE process and alternating, the existing reports of the same frame, whose code this feature does not touch and which
are therefore the yardstick: std_err="hc1" and "se".  Every call derives var(y) itself, as a user's call does.  Times: median / best
/ worst of `--reps` (default 7) warmed calls by device events.  From one more call per form with the context's timing classes on and
y_var given (so that no pass over y rides along): the kernel time of the new pass ("pass2": the cluster kernels and their record
sums) and of the moment pass, and frame bytes / kernel time as a share of the 8 TB/s HBM peak -- a memory bound: the pass needs
2 x 17 flops per element for residuals and scores, far under the matrix rate.  The expectation to confirm or refute: the ordered
forms are two streams over the frame, like HC1.  Lines are appended to profiles/cluster_report_bench.txt (`--out`).  No time here is
a pass condition.
"""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
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


def timed_alternating(fns, reps, warm=2):
    """{name: (median, best, worst) ms} of the calls in `fns`, one after the other in every repetition (device events)."""
    for _ in range(warm):
        for fn in fns.values():
            fn()
    s = torch.cuda.current_stream()
    ms = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(s)
            fn()
            b.record(s)
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    out = {}
    for k, v in ms.items():
        v.sort()
        out[k] = (v[len(v) // 2], v[0], v[-1])
    return out


def make_frame(gen, dev, n, g, p):
    """x ~ N(0, 1) plus a per-cluster component, y = 0.5 + X beta + u_g + e; clusters of n / g rows in order"""
    m = n // g
    codes = torch.arange(g, device=dev).repeat_interleave(m)
    X = []
    for j in range(p):
        X.append(torch.randn(n, generator=gen, device=dev, dtype=torch.float64) + 0.5 * torch.randn(g, generator=gen, device=dev,
                                                                                                     dtype=torch.float64)[codes])
    y = 0.5 + torch.randn(g, generator=gen, device=dev, dtype=torch.float64)[codes] + torch.randn(n, generator=gen, device=dev,
                                                                                                    dtype=torch.float64)
    for j in range(p):
        y += (0.5 * (-1) ** j * (j + 1) / p) * X[j]
    return X, y, codes


def run_form(name, ctx, X, y, reps, p, split=None, waves=None, **cluster_kw):
    n = int(y.numel())
    ctx.set_option("cluster_split_rows", split or 0)
    ctx.set_option("cluster_waves", waves or 0)
    fns = {
        "cluster": lambda: pds.lin_reg_report(*X, target=y, add_bias=True, std_err="cluster", ctx=ctx, **cluster_kw),
        "hc1": lambda: pds.lin_reg_report(*X, target=y, add_bias=True, std_err="hc1", ctx=ctx),
        "se": lambda: pds.lin_reg_report(*X, target=y, add_bias=True, std_err="se", ctx=ctx),
    }
    t = timed_alternating(fns, reps)
    y_var = float(y.var().item())
    kern = {}
    for k in ("cluster", "hc1"):
        kw = cluster_kw if k == "cluster" else {}
        ctx.set_timing(True)
        ctx.get_timing()
        rep = pds.lin_reg_report(*X, target=y, add_bias=True, std_err=k, y_var=y_var, ctx=ctx, **kw)
        ctx.synchronize()
        kern[k] = ctx.get_timing()
        ctx.set_timing(False)
        if k == "cluster":
            g = rep["n_clusters"]
    frame_bytes = n * (p + 1) * 8
    pass_ms = kern["cluster"]["pass2"][0]
    hc1_pass_ms = kern["hc1"]["moments"][0] - kern["cluster"]["moments"][0]  # HC1's second stream is a moments-class launch
    emit({"bench": "cluster_report", "form": name, "rows": n, "clusters": g, "p": p, "split_rows": split or "default", "waves": waves or "default",
          "cluster_ms": round(t["cluster"][0], 3), "cluster_ms_best": round(t["cluster"][1], 3), "cluster_ms_worst": round(t["cluster"][2], 3),
          "hc1_ms": round(t["hc1"][0], 3), "hc1_ms_best": round(t["hc1"][1], 3), "hc1_ms_worst": round(t["hc1"][2], 3),
          "se_ms": round(t["se"][0], 3), "cluster_over_hc1": round(t["cluster"][0] / t["hc1"][0], 4),
          "cluster_over_se": round(t["cluster"][0] / t["se"][0], 4), "frame_GB": round(frame_bytes / 1e9, 3),
          "cluster_pass_kernels_ms": round(pass_ms, 3), "moment_pass_kernels_ms": round(kern["cluster"]["moments"][0], 3),
          "hc1_second_pass_kernels_ms": round(hc1_pass_ms, 3),
          "cluster_pass_frame_bytes_per_time_share_of_8TBps": round(frame_bytes / (pass_ms * 1e-3) / HBM, 4) if pass_ms > 0 else None,
          "cluster_pass_TBps": round(frame_bytes / (pass_ms * 1e-3) / 1e12, 3) if pass_ms > 0 else None,
          "roofline_share": "measured" if pass_ms > 0 else "not measured"})


def main():
    global OUT
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=float, default=1e8)
    ap.add_argument("--features", type=int, default=16)
    ap.add_argument("--forms", default="ordered_offsets,ordered_keys,long_offsets,shuffled_keys")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--split", default="", help="extra runs of long_offsets with cluster_split_rows set to each value")
    ap.add_argument("--waves", default="", help="extra runs of ordered_offsets and long_offsets with cluster_waves set to each value")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "cluster_report_bench.txt"))
    a = ap.parse_args()
    OUT = a.out or None
    dev = torch.device("cuda", 0)
    ctx = pds.Context(0)
    ctx.set_stream(torch.cuda.current_stream(dev))
    gen = torch.Generator(device=dev)
    gen.manual_seed(11)
    n, p = int(a.rows), a.features
    forms = a.forms.split(",")
    waves = [None] + [int(v) for v in a.waves.split(",") if v]
    g_many, g_long = max(2, n // 100), max(2, n // 10_000)
    if any(f in forms for f in ("ordered_offsets", "ordered_keys", "shuffled_keys")):
        X, y, codes = make_frame(gen, dev, g_many * 100, g_many, p)
        off = torch.arange(0, g_many * 100 + 1, 100, dtype=torch.int64, device=dev)
        if "ordered_offsets" in forms:
            for wv in waves:
                run_form("ordered_offsets", ctx, X, y, a.reps, p, waves=wv, cluster_offsets=off)
        if "ordered_keys" in forms:
            run_form("ordered_keys", ctx, X, y, a.reps, p, cluster=codes * 3 - 7)
        if "shuffled_keys" in forms:
            perm = torch.randperm(int(y.numel()), generator=gen, device=dev)
            X = [c[perm] for c in X]
            y, keys = y[perm], (codes * 3 - 7)[perm]
            del perm, codes
            run_form("shuffled_keys", ctx, X, y, a.reps, p, cluster=keys)
            del keys
        del X, y
    if "long_offsets" in forms:
        m = 10_000 if n >= 20_000 else n // 2
        X, y, codes = make_frame(gen, dev, g_long * m, g_long, p)
        del codes
        off = torch.arange(0, g_long * m + 1, m, dtype=torch.int64, device=dev)
        for sp in [None] + [int(v) for v in a.split.split(",") if v]:
            run_form("long_offsets", ctx, X, y, a.reps, p, split=sp, cluster_offsets=off)
        for wv in waves[1:]:
            run_form("long_offsets", ctx, X, y, a.reps, p, waves=wv, cluster_offsets=off)


if __name__ == "__main__":
    main()
