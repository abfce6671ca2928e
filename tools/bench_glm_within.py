"""
lstsq.glm_report(absorb_offsets=) (pds_glm_within_grouped_*, csrc/glm_within.hip) on one MI355X, the frame resident in HBM.
Frame: `--rows` (default 1e7) x 8 f64 features, poisson with an offset, one level per group.  Shapes:
    groups_100        1e5 groups x 100 rows   (every group resident in the wave's LDS tile: an iteration reads the frame once)
    groups_10000      1e3 groups x 1e4 rows   (below "within_split_rows": an iteration reads the frame twice)
Per shape, in ONE process and alternating: the fixed-effects call (std_err="cluster", tol 1e-8) and two yardsticks on the same frame --
    plain      glm_report(std_err="cluster", cluster_offsets=) with a bias and without absorption: call time / n_iter is its
               per-iteration time
    lin        lin_reg_report(absorb_offsets=, std_err="cluster"): its statistics pass ("grouped_moments") and its within pass ("pass2")
Times: median / best / worst of `--reps` (default 5) warmed calls by device events.  From one more call each with the context's timing
classes on: the pre-pass ("grouped_moments"), every iteration pass ("iterative": the kernels of one iteration and its record sum) and
the final pass ("pass2") of the fixed-effects call, and the two passes of `lin`.  Bytes: an iteration needs the 8 features, y and the
offset once (groups_100) or twice (groups_10000); frame bytes x reads / pass time is reported beside the share of 8 TB/s.  The
expectation this tool confirms or refutes (not a gate): an iteration pass costs about what the linear statistics pass costs.
Run it in a fresh process per configuration; lines are appended to profiles/glm_within_bench.txt (`--out`).
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
    """x ~ 0.3 N(0, 1) with a per-group component, o ~ U(-1, 1), y ~ Poisson(exp(0.2 + x . beta + o + u_g)); groups of n / g rows"""
    f64 = dict(generator=gen, device=dev, dtype=torch.float64)
    codes = torch.arange(g, device=dev).repeat_interleave(n // g)
    X = [0.3 * torch.randn(n, **f64) + 0.1 * torch.randn(g, **f64)[codes] for _ in range(p)]
    o = 2.0 * torch.rand(n, **f64) - 1.0
    eta = 0.2 + o + 0.2 * torch.randn(g, **f64)[codes]
    for j in range(p):
        eta += (0.5 * (-1) ** j * (j + 1) / p) * X[j]
    return X, torch.poisson(torch.exp(eta), generator=gen), o


def kernel_split(ctx, call, kinds):
    """the durations (ms) the context's timing classes saw in one call: {kind: [launch, ...]}"""
    ctx.set_timing(True)
    ctx.get_timing()
    for k in kinds:
        ctx.get_timing_samples(k)
    call()
    ctx.synchronize()
    out = {k: ctx.get_timing_samples(k) for k in kinds}
    ctx.set_timing(False)
    return out


def run_shape(name, ctx, X, y, o, off, reps, p, reads):
    n = int(y.numel())
    glm = dict(target=y, family="poisson", tol=TOL, max_iter=MAX_ITER, offset=o, std_err="cluster", ctx=ctx)
    fns = {
        "within": lambda: pds.glm_report(*X, absorb_offsets=off, **glm),
        "plain": lambda: pds.glm_report(*X, add_bias=True, cluster_offsets=off, **glm),
        "lin": lambda: pds.lin_reg_report(*X, target=y, absorb_offsets=off, std_err="cluster", ctx=ctx),
    }
    t = timed_alternating(fns, reps)
    rep, plain = fns["within"](), fns["plain"]()
    ks = kernel_split(ctx, fns["within"], ("grouped_moments", "iterative", "pass2"))
    kl = kernel_split(ctx, fns["lin"], ("grouped_moments", "pass2"))
    it = sorted(ks["iterative"])
    it_med = it[len(it) // 2] if it else float("nan")
    lin_stats = sum(kl["grouped_moments"])
    frame_bytes = n * (p + 2) * 8  # features, y, offset
    plain_iters = int(plain["n_iter"])
    rec = {"bench": "glm_within", "shape": name, "rows": n, "groups": int(rep["n_groups"]), "groups_dropped": int(rep["n_groups_dropped"]), "p": p,
           "family": "poisson+offset", "frame_GB": round(frame_bytes / 1e9, 3), "n_iter": int(rep["n_iter"]), "converged": bool(rep["converged"]),
           "plain_n_iter": plain_iters}
    for k in fns:
        rec[f"{k}_ms"], rec[f"{k}_ms_best"], rec[f"{k}_ms_worst"] = (round(v, 3) for v in t[k])
    rec["within_ms_per_iter"] = round(t["within"][0] / rep["n_iter"], 3)
    rec["plain_ms_per_iter"] = round(t["plain"][0] / max(plain_iters, 1), 3)
    rec["pre_pass_ms"] = round(sum(ks["grouped_moments"]), 3)
    rec["iter_pass_ms_median"], rec["iter_pass_ms_all"] = round(it_med, 3), [round(v, 3) for v in ks["iterative"]]
    rec["final_pass_ms"] = round(sum(ks["pass2"]), 3)
    rec["lin_stats_pass_ms"], rec["lin_within_pass_ms"] = round(lin_stats, 3), round(sum(kl["pass2"]), 3)
    rec["iter_pass_over_lin_stats_pass"] = round(it_med / lin_stats, 3) if lin_stats > 0 else None
    rec["iter_over_plain_iter"] = round(rec["within_ms_per_iter"] / rec["plain_ms_per_iter"], 3) if rec["plain_ms_per_iter"] > 0 else None
    rec["iter_reads_of_frame"] = reads
    rec["iter_pass_TBps"] = round(reads * frame_bytes / (it_med * 1e-3) / 1e12, 3) if it_med > 0 else None
    rec["iter_pass_share_of_8TBps"] = round(reads * frame_bytes / (it_med * 1e-3) / HBM, 4) if it_med > 0 else None
    emit(rec)


def main():
    global OUT
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=float, default=1e7)
    ap.add_argument("--features", type=int, default=8)
    ap.add_argument("--shapes", default="groups_100,groups_10000")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "glm_within_bench.txt"))
    a = ap.parse_args()
    OUT = a.out or None
    dev = torch.device("cuda", 0)
    ctx = pds.Context(0)
    ctx.set_stream(torch.cuda.current_stream(dev))
    gen = torch.Generator(device=dev)
    gen.manual_seed(11)
    n, p = int(a.rows), a.features
    for shape in a.shapes.split(","):
        m = 10_000 if shape == "groups_10000" else 100
        g = max(2, n // m)
        X, y, o = make_frame(gen, dev, g * m, g, p)
        run_shape(shape, ctx, X, y, o, torch.arange(0, g * m + 1, m, dtype=torch.int64, device=dev), a.reps, p, 2 if m > 128 else 1)
        del X, y, o


if __name__ == "__main__":
    main()
