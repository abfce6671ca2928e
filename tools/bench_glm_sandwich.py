"""
lstsq.glm_report(std_err="hc1" | "cluster") (pds_glm_report_robust_* / _cluster_*, csrc/glm_meat.hip) on one MI355X, the frame resident
in HBM.  Frame: `--rows` (default 1e7) x 8 f64 features + bias, poisson with an offset.  Forms:
    offsets_100       1e5 ordered clusters x 100 rows, cluster_offsets=
    offsets_10000     1e3 clusters x 1e4 rows, cluster_offsets=
    ordered_keys      the 100-row clusters as an ordered int64 key column, cluster=  (the order check; nothing moves)
    shuffled_keys     the same frame with its rows in random order, cluster=  (the sort + gather route)
Per form, in ONE process and alternating: the "hc1" and the "cluster" call, and two yardsticks on the same frame --
    plain      glm_report_by(group_offsets=[0, n]): the call the new one contains; the difference is the feature's cost
    lin        lin_reg_report(std_err="cluster") on the same columns: its cluster_meat pass is the same stream without the link
               functions, the weights and the offset
Times: median / best / worst of `--reps` (default 7) warmed calls by device events.  From one more call each with the context's timing
classes on: the kernel time of the new pass alone (the LAST "pass2" launch of the call: the meat kernels and their record sums) and of
cluster_meat's, and frame bytes / pass time (a memory bound: 8 features, y and the offset are read once).  Run it in a fresh process
per configuration; lines are appended to profiles/glm_sandwich_bench.txt (`--out`).  No time here is a pass condition.
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
TOL, MAX_ITER = 1e-8, 100


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if OUT is not None:
        with open(OUT, "a") as fh:
            fh.write(line + "\n")


def timed_alternating(fns, reps, warm=1):
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
    """x ~ 0.3 N(0, 1) with a per-cluster component, o ~ U(-1, 1), y ~ Poisson(exp(0.2 + x . beta + o + u_g)); clusters of n / g rows"""
    codes = torch.arange(g, device=dev).repeat_interleave(n // g)
    X = [0.3 * torch.randn(n, generator=gen, device=dev, dtype=torch.float64) + 0.1 * torch.randn(g, generator=gen, device=dev,
                                                                                                    dtype=torch.float64)[codes] for _ in range(p)]
    o = 2.0 * torch.rand(n, generator=gen, device=dev, dtype=torch.float64) - 1.0
    eta = 0.2 + o + 0.2 * torch.randn(g, generator=gen, device=dev, dtype=torch.float64)[codes]
    for j in range(p):
        eta += (0.5 * (-1) ** j * (j + 1) / p) * X[j]
    y = torch.poisson(torch.exp(eta), generator=gen)
    return X, y, o, codes


def last_pass_ms(ctx, call):
    """the kernel time of the last "pass2" launch of one call (device events of the context's timing classes)"""
    ctx.set_timing(True)
    ctx.get_timing()
    ctx.get_timing_samples("pass2")
    call()
    ctx.synchronize()
    samples = ctx.get_timing_samples("pass2")
    ctx.set_timing(False)
    return samples[-1] if samples else float("nan")


def run_form(name, ctx, X, y, o, reps, p, **cluster_kw):
    n = int(y.numel())
    one = torch.tensor([0, n], dtype=torch.int64, device=y.device)
    glm = dict(target=y, family="poisson", add_bias=True, tol=TOL, max_iter=MAX_ITER, offset=o, ctx=ctx)
    fns = {
        "cluster": lambda: pds.glm_report(*X, std_err="cluster", **cluster_kw, **glm),
        "hc1": lambda: pds.glm_report(*X, std_err="hc1", **glm),
        "plain": lambda: pds.glm_report_by(*X, group_offsets=one, **glm),
        "lin": lambda: pds.lin_reg_report(*X, target=y, add_bias=True, std_err="cluster", y_var=1.0, ctx=ctx, **cluster_kw),
    }
    t = timed_alternating(fns, reps)
    passes = {k: last_pass_ms(ctx, fns[k]) for k in ("cluster", "hc1", "lin")}
    g = pds.glm_report(*X, std_err="cluster", **cluster_kw, **glm)["n_clusters"]
    frame_bytes = n * (p + 2) * 8  # features, y, offset
    rec = {"bench": "glm_sandwich", "form": name, "rows": n, "clusters": g, "p": p, "family": "poisson+offset", "frame_GB": round(frame_bytes / 1e9, 3)}
    for k in fns:
        rec[f"{k}_ms"], rec[f"{k}_ms_best"], rec[f"{k}_ms_worst"] = (round(v, 3) for v in t[k])
    rec["cluster_minus_plain_ms"] = round(t["cluster"][0] - t["plain"][0], 3)
    rec["hc1_minus_plain_ms"] = round(t["hc1"][0] - t["plain"][0], 3)
    for k, v in passes.items():
        rec[f"{k}_pass_kernels_ms"] = round(v, 3)
        rec[f"{k}_pass_TBps"] = round((frame_bytes - (n * 8 if k == "lin" else 0)) / (v * 1e-3) / 1e12, 3) if v > 0 else None
    rec["cluster_pass_over_lin_pass"] = round(passes["cluster"] / passes["lin"], 3) if passes["lin"] > 0 else None
    rec["cluster_pass_share_of_8TBps"] = round(frame_bytes / (passes["cluster"] * 1e-3) / HBM, 4) if passes["cluster"] > 0 else None
    emit(rec)


def main():
    global OUT
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=float, default=1e7)
    ap.add_argument("--features", type=int, default=8)
    ap.add_argument("--forms", default="offsets_100,offsets_10000,ordered_keys,shuffled_keys")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "glm_sandwich_bench.txt"))
    a = ap.parse_args()
    OUT = a.out or None
    dev = torch.device("cuda", 0)
    ctx = pds.Context(0)
    ctx.set_stream(torch.cuda.current_stream(dev))
    gen = torch.Generator(device=dev)
    gen.manual_seed(11)
    n, p = int(a.rows), a.features
    for form in a.forms.split(","):
        m = 10_000 if form == "offsets_10000" else 100
        g = max(2, n // m)
        X, y, o, codes = make_frame(gen, dev, g * m, g, p)
        if form.startswith("offsets"):
            run_form(form, ctx, X, y, o, a.reps, p, cluster_offsets=torch.arange(0, g * m + 1, m, dtype=torch.int64, device=dev))
        elif form == "ordered_keys":
            run_form(form, ctx, X, y, o, a.reps, p, cluster=codes * 3 - 7)
        else:
            perm = torch.randperm(g * m, generator=gen, device=dev)
            run_form(form, ctx, [c[perm] for c in X], y[perm], o[perm], a.reps, p, cluster=(codes * 3 - 7)[perm])
        del X, y, o, codes


if __name__ == "__main__":
    main()
