"""A/B of the fused grouped kernel's row shares on one box in one process: the share of the rows dealt to the second half of the
grid (context option "grouped_fused_late_permille"; 500 = equal shares) against the kernel's HIP-event launch time, the settings
taken in turn round after round so that drift of the box hits all of them alike.

    python tools/fused_split_ab.py [--shares 500,480,470,460,450,440] [--rounds 4] [--launches 10] [--frames p16,p8,c3]

p16 / p8: 1e6 groups x 100 rows x 16 / 8 f64 (the headline frame and `grouped_p8`); c3: the ragged C3 frame of bench.py's
`grouped_c3spec` (Poisson sizes, 0.1 % collinear groups: the marked pass runs too, outside the timed bracket of this kernel)."""
import argparse
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
import polars_ds_extension_amd as pds  # noqa: E402
import synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--shares", default="500,480,470,460,450,440")
ap.add_argument("--rounds", type=int, default=4)
ap.add_argument("--launches", type=int, default=10)
ap.add_argument("--frames", default="p16,p8,c3")
args = ap.parse_args()
shares = [int(s) for s in args.shares.split(",")]
dev = torch.device("cuda", 0)
ctx = pds.Context(0)
ctx.set_stream(torch.cuda.current_stream())


def run(name, fn):
    samples = {s: [] for s in shares}
    for s in shares:  # warm
        ctx.set_option("grouped_fused_late_permille", s)
        fn()
    ctx.get_timing(reset=True)
    ctx.get_timing_samples("grouped_moments", reset=True)
    for _ in range(args.rounds):
        for s in shares:
            ctx.set_option("grouped_fused_late_permille", s)
            ctx.set_timing(True)
            for _ in range(args.launches):
                fn()
            ctx.set_timing(False)
            got = ctx.get_timing_samples("grouped_moments", reset=True)
            ctx.get_timing(reset=True)
            # (a call that also runs the marked pass brackets its Gram build under the same class: the fused launch is the longest)
            per = len(got) // args.launches
            samples[s] += [max(got[i * per:(i + 1) * per]) for i in range(args.launches)]
    ctx.set_option("grouped_fused_late_permille", 0)
    base = float(np.median(samples[shares[0]]))
    print(f"== {name}: fused kernel ms over {args.rounds} rounds x {args.launches} launches per share (shares taken in turn)")
    print("   late share   min      median   max      median vs first")
    for s in shares:
        a = np.array(samples[s])
        print(f"   {s:4d}/1000   {a.min():.4f}   {np.median(a):.4f}   {a.max():.4f}   {100.0 * (np.median(a) / base - 1.0):+6.2f} %", flush=True)


frames = args.frames.split(",")
if "p16" in frames or "p8" in frames:
    G, R = 1_000_000, 100
    xs, y = synth.headline_frame(G, R, 16, seed=1234)
    off = torch.arange(0, G * R + 1, R, dtype=torch.int64, device=dev)
    for p in (16, 8):
        if f"p{p}" in frames:
            run(f"{G} groups x {R} rows x {p} f64", lambda: pds.lin_reg_by(*xs[:p], target=y, group_offsets=off, ctx=ctx))
    del xs, y
    torch.cuda.empty_cache()
if "c3" in frames:
    fr = synth.c3_frame(1_000_000, 8, seed=2)
    run("C3 ragged frame, 1e6 groups x 8 f64", lambda: pds.lin_reg_by(*fr["xs"], target=fr["y"], group_offsets=fr["offsets"], ctx=ctx))
