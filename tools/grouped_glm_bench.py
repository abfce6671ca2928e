"""
Grouped GLM fits (pds_glm_irls_grouped_*, csrc/grouped_irls.hip) on one MI355X, inputs resident in HBM, offsets form.
Per shape: median / best / worst of `--reps` warmed calls by device events, the fit kernel's own time of one more call (the
context's "iterative" timing class), the mean iteration count, `lin_reg_by` on the same frame in the same process (one read, one
solve per group) and the ratio to it, the algorithmic bytes sum n_g (p + 1) 8 + G (p' 8 + 5) and `frame bytes / kernel time` as a
share of the 8 TB/s HBM peak (the model is "one frame read + k on-chip iterations": that share is NOT a bandwidth the kernel
reaches on a second pass, it says how far the iterations are from free; left out -- null -- where groups were split off, because
the kernel's time then covers the other groups only: `groups_split_off` counts them, 16 384 rows being the library's default).
Shapes (`--shapes`): headline = 1e6 groups x 100 rows x 8 features + bias, binomial; wide = the same with 16 features, poisson;
long = 1e4 groups x 1e4 rows (beyond the 128 resident rows); skewed = one 1e7-row group beside 1e5 groups of 100 rows (the split-off
route).  `--split a,b,..` repeats the long and skewed shapes with the context option glm_split_rows set to each value.
`--sample K`: the parent's only way, `GLM.fit` per group, on the first K groups of the headline frame, alternating with the grouped
call on those K groups; the factor between the two.
`--weighted`: on the headline and wide frames, `glm_by` with prior weights (headline) / with weights and an offset (wide) against
`glm_by` without, the two calls alternating in one process: medians of `--reps` warmed calls each, their ratio, the mean iteration
counts (weights U(0.25, 4), offsets U(-0.1, 0.1): the target is not redrawn, so the counts may differ a little); and
`glm_report_by` with the columns against `glm_report_by` without, the same way.
A per-kernel split comes from a separate run under `rocprofv3 --kernel-trace --stats -- python tools/grouped_glm_bench.py ...`.
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


def make_frame(gen, dev, n, p, family, off):
    """x ~ N(0, 1) (gamma: U(0.1, 1)), one coefficient vector for the whole frame, the family's own target."""
    if family == "gamma":
        X = [0.1 + 0.9 * torch.rand(n, generator=gen, device=dev, dtype=torch.float64) for _ in range(p)]
    else:
        X = [torch.randn(n, generator=gen, device=dev, dtype=torch.float64) for _ in range(p)]
    eta = torch.full((n,), 0.2, device=dev, dtype=torch.float64)
    for j in range(p):
        eta += (0.5 * (-1) ** j * (j + 1) / p) * X[j]
    if family == "binomial":
        y = (torch.rand(n, generator=gen, device=dev, dtype=torch.float64) < torch.sigmoid(eta)).to(torch.float64)
    elif family == "poisson":
        y = torch.poisson(torch.exp(eta), generator=gen)
    else:
        y = eta + 0.5 * torch.randn(n, generator=gen, device=dev, dtype=torch.float64)
    del eta
    return X, y


def run_shape(name, ctx, gen, dev, sizes_desc, off, p, family, reps, split=None):
    n = int(off[-1].item())
    ng = int(off.numel()) - 1
    X, y = make_frame(gen, dev, n, p, family, off)
    ctx.set_option("glm_split_rows", split or 0)
    call = lambda: pds.glm_by(*X, target=y, group_offsets=off, family=family, add_bias=True, tol=1e-8, max_iter=100, ctx=ctx)  # noqa: E731
    ms, best, worst = timed(call, reps)
    ctx.set_timing(True)
    ctx.get_timing()
    co, it, nu = call()
    ctx.synchronize()
    tm = ctx.get_timing()
    ctx.set_timing(False)
    kernel_ms = tm["iterative"][0]
    by_ms, _, _ = timed(lambda: pds.lin_reg_by(*X, target=y, group_offsets=off, add_bias=True, ctx=ctx), reps)
    pp = p + 1
    # groups the kernel hands to the full-device route: its own time then covers the other groups only, and no share is derived
    n_long = int(((off[1:] - off[:-1]) > (split or 16384)).sum().item())
    frame_bytes = n * (p + 1) * 8
    alg = frame_bytes + ng * (pp * 8 + 5)
    rec = {"bench": "grouped_glm", "shape": name, "groups": ng, "rows": n, "p": p, "family": family, "split_rows": split or "default",
           "ms": round(ms, 3), "ms_best": round(best, 3), "ms_worst": round(worst, 3), "fit_kernel_ms": round(kernel_ms, 3),
           "mean_n_iter": round(float(it.float().mean().item()), 2), "null_groups": int(nu.sum().item()),
           "groups_split_off": n_long,
           "lin_reg_by_ms": round(by_ms, 3), "ratio_to_lin_reg_by": round(ms / by_ms, 2), "algorithmic_GB": round(alg / 1e9, 3),
           "frame_bytes_per_kernel_time_share_of_8TBps": None if n_long else round(frame_bytes / (max(kernel_ms, 1e-6) * 1e-3) / HBM, 4)}
    print(json.dumps(rec), flush=True)
    return X, y


def run_weighted(name, ctx, gen, dev, X, y, off, p, family, reps, with_offset):
    """`glm_by(weights= (, offset=))` against `glm_by` on the same frame, the two calls alternating."""
    n = int(y.numel())
    pw = 0.25 + 3.75 * torch.rand(n, generator=gen, device=dev, dtype=torch.float64)
    o = (0.2 * torch.rand(n, generator=gen, device=dev, dtype=torch.float64) - 0.1) if with_offset else None
    kw = dict(target=y, group_offsets=off, family=family, add_bias=True, tol=1e-8, max_iter=100, ctx=ctx)
    plain = lambda: pds.glm_by(*X, **kw)  # noqa: E731
    weighted = lambda: pds.glm_by(*X, weights=pw, offset=o, **kw)  # noqa: E731
    for _ in range(2):
        plain()
        weighted()
    s = torch.cuda.current_stream()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = {"plain": [], "weighted": []}
    for _ in range(reps):
        for k, fn in (("plain", plain), ("weighted", weighted)):
            a.record(s)
            fn()
            b.record(s)
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
    it0, itw = plain()[1], weighted()[1]
    # the report likewise: glm_report_by with the columns against glm_report_by without, alternating
    rplain = lambda: pds.glm_report_by(*X, **kw)  # noqa: E731
    rweighted = lambda: pds.glm_report_by(*X, weights=pw, offset=o, **kw)  # noqa: E731
    for _ in range(2):
        rplain()
        rweighted()
    rms = {"plain": [], "weighted": []}
    for _ in range(reps):
        for k, fn in (("plain", rplain), ("weighted", rweighted)):
            a.record(s)
            fn()
            b.record(s)
            b.synchronize()
            rms[k].append(a.elapsed_time(b))
    rmed = {k: sorted(v)[len(v) // 2] for k, v in rms.items()}
    print(json.dumps({"bench": "grouped_glm_weighted", "shape": name, "groups": int(off.numel()) - 1, "rows": n, "p": p, "family": family,
                      "columns": "weights + offset" if with_offset else "weights", "plain_ms": round(med["plain"], 3),
                      "plain_ms_best": round(min(ms["plain"]), 3), "plain_ms_worst": round(max(ms["plain"]), 3),
                      "weighted_ms": round(med["weighted"], 3), "weighted_ms_best": round(min(ms["weighted"]), 3),
                      "weighted_ms_worst": round(max(ms["weighted"]), 3), "ratio": round(med["weighted"] / med["plain"], 4),
                      "mean_n_iter_plain": round(float(it0.float().mean().item()), 2),
                      "mean_n_iter_weighted": round(float(itw.float().mean().item()), 2),
                      "report_plain_ms": round(rmed["plain"], 3), "report_weighted_ms": round(rmed["weighted"], 3),
                      "report_ratio": round(rmed["weighted"] / rmed["plain"], 4),
                      "report_weighted_over_fit_weighted": round(rmed["weighted"] / med["weighted"], 4)}), flush=True)


def sample_against_glm_fit(ctx, X, y, m, p, family, k):
    """`GLM(family).fit` per group on the first k groups (m rows each), alternating with the grouped call on those k groups."""
    from polars_ds_extension_amd.linear_models import GLM

    off = torch.arange(0, k * m + 1, m, dtype=torch.int64, device=y.device)
    Xs = [c[:k * m] for c in X]
    ys = y[:k * m]
    Xm = torch.stack(Xs, dim=1).contiguous()
    t_single, t_grouped = [], []
    for rep in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        its = 0
        for g in range(k):
            mdl = GLM(add_bias=True, family=family, max_iter=100, tol=1e-8).fit(Xm[g * m:(g + 1) * m], ys[g * m:(g + 1) * m])
            its += mdl.n_iter_
        torch.cuda.synchronize()
        t_single.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        co, it, nu = pds.glm_by(*Xs, target=ys, group_offsets=off, family=family, add_bias=True, tol=1e-8, max_iter=100, ctx=ctx)
        torch.cuda.synchronize()
        t_grouped.append((time.perf_counter() - t0) * 1e3)
    s, g_ = float(np.median(t_single)), float(np.median(t_grouped))
    print(json.dumps({"bench": "grouped_glm_vs_per_group_fit", "groups": k, "rows_per_group": m, "p": p, "family": family,
                      "glm_fit_per_group_ms": round(s, 2), "grouped_call_ms": round(g_, 3), "factor": round(s / g_, 1),
                      "iterations_per_group_single": round(its / k, 2)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="headline,wide,long,skewed")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--split", default="")
    ap.add_argument("--sample", type=int, default=1000)
    ap.add_argument("--weighted", action="store_true", help="headline / wide: the weighted (/ offset) call against the plain one")
    ap.add_argument("--scale", type=float, default=1.0, help="scales the group counts (a smaller rehearsal)")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    ctx = pds.Context(0)
    ctx.set_stream(torch.cuda.current_stream(dev))
    gen = torch.Generator(device=dev)
    gen.manual_seed(3)
    shapes = a.shapes.split(",")
    splits = [int(v) for v in a.split.split(",") if v]
    sc = a.scale
    if "headline" in shapes:
        G, m = int(1_000_000 * sc), 100
        off = torch.arange(0, G * m + 1, m, dtype=torch.int64, device=dev)
        X, y = run_shape("headline", ctx, gen, dev, None, off, 8, "binomial", a.reps)
        if a.sample > 0:
            sample_against_glm_fit(ctx, X, y, m, 8, "binomial", min(a.sample, G))
        if a.weighted:
            run_weighted("headline", ctx, gen, dev, X, y, off, 8, "binomial", a.reps, with_offset=False)
        del X, y
    if "wide" in shapes:
        G, m = int(1_000_000 * sc), 100
        off = torch.arange(0, G * m + 1, m, dtype=torch.int64, device=dev)
        X, y = run_shape("wide", ctx, gen, dev, None, off, 16, "poisson", a.reps)
        if a.weighted:
            run_weighted("wide", ctx, gen, dev, X, y, off, 16, "poisson", a.reps, with_offset=True)
        del X, y
    if "long" in shapes:
        G, m = int(10_000 * sc), 10_000
        off = torch.arange(0, G * m + 1, m, dtype=torch.int64, device=dev)
        for sp in [None] + splits:
            X, y = run_shape("long", ctx, gen, dev, None, off, 8, "binomial", max(3, a.reps // 2), sp)
            del X, y
    if "skewed" in shapes:
        big, G, m = int(10_000_000 * sc), int(100_000 * sc), 100
        off = torch.cat([torch.tensor([0], device=dev), torch.arange(big, big + G * m + 1, m, device=dev)]).to(torch.int64)
        for sp in [None] + splits:
            X, y = run_shape("skewed", ctx, gen, dev, None, off, 8, "binomial", max(3, a.reps // 2), sp)
            del X, y


if __name__ == "__main__":
    main()
