"""Development aid for the fused grouped kernel (csrc/grouped_fused.hip), two reports:

  phases  per-phase shader-clock sums of every wave             (library built with EXTRA=-DPDS_PROFILE_PHASES)
  tail    when every wave of a launch starts and ends, on the    (EXTRA=-DPDS_PROFILE_TAIL: two stamps per wave and nothing
          constant 100 MHz clock all XCDs share                   else, so the launch runs as the product kernel does; or
                                                                  -DPDS_PROFILE_PHASES, whose fences stretch the waves)

    python tools/phase_profile.py [phases] [tail] [--launches 30] [--p 16,8] [--rows 100] [--groups 1000000]
                                  [--waves W] [--late-permille S]       (context options grouped_fused_waves / _late_permille)
                                  [--frame c3]                          (tools/synth.py's ragged C3 frame, 8 features, instead)

`tail` answers: how long does the launch wait for its slowest wave?  idle share = 1 - mean(end - start) / (max end - min start),
split into the ramp (waves that start late) and the tail (waves that end early), per XCD, over >= 30 launches, next to the launch
time's own min / median / max from the context's HIP-event brackets of the same launches.  It also prints how long every wave takes
from its start to having issued its first tile load -- the two searches of the offsets sit in between -- as a distribution over
waves and as a share of the launch."""
import argparse
import ctypes as C
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np
import torch
import polars_ds_extension_amd as pds
from polars_ds_extension_amd import _lib

ap = argparse.ArgumentParser()
ap.add_argument("what", nargs="*", default=[])
ap.add_argument("--launches", type=int, default=30)
ap.add_argument("--p", default="16,8")
ap.add_argument("--rows", type=int, default=100)
ap.add_argument("--groups", type=int, default=1_000_000)
ap.add_argument("--waves", type=int, default=0)
ap.add_argument("--late-permille", type=int, default=0)
ap.add_argument("--dump", default=None, help="tail: also write the raw stamps of every launch to DUMP_p<P>.npy (launches x waves x words)")
ap.add_argument("--frame", default="equal", choices=["equal", "c3"], help="equal: --groups groups of --rows rows; c3: synth.c3_frame(--groups, 8)")
args = ap.parse_args()
what = set(args.what) or {"phases"}
G, R = args.groups, args.rows
N = G * R
PS = [int(s) for s in args.p.split(",")]
dev = torch.device("cuda", 0)
ctx = pds.Context(0)
ctx.set_stream(torch.cuda.current_stream(dev))
for name, v in (("grouped_fused_waves", args.waves), ("grouped_fused_late_permille", args.late_permille)):
    if v:
        ctx.set_option(name, v)
if args.frame == "c3":
    import synth

    PS = [8]
    fr = synth.c3_frame(G, 8, seed=2, device=dev)
    xs, y, off = fr["xs"], fr["y"], fr["offsets"]
    N = fr["n_rows"]
else:
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    xs = [torch.randn(N, dtype=torch.float64, device=dev, generator=gen) for _ in range(max(PS))]
    y = sum(x * 0.1 for x in xs) + 0.1 * torch.randn(N, dtype=torch.float64, device=dev, generator=gen)
    off = torch.arange(0, N + 1, R, dtype=torch.int64, device=dev)
so = _lib.load()


def phases(P):
    if not hasattr(so, "pds_debug_phase_cycles"):
        sys.exit("phases: the library was not built with EXTRA=-DPDS_PROFILE_PHASES")
    buf = (C.c_ulonglong * 8)()
    f = lambda: pds.lin_reg_by(*xs[:P], target=y, group_offsets=off, ctx=ctx)
    for _ in range(2):
        f()
    torch.cuda.synchronize()
    so.pds_debug_phase_cycles(buf, 1)
    K = 5
    for _ in range(K):
        f()
    torch.cuda.synchronize()
    so.pds_debug_phase_cycles(buf, 1)
    names = ["tile store (+vmcnt wait)", "next-tile load issue", "flush (acc->LDS->regs)", "solve", "consume (MFMA)", "-", "-", "wave total"]
    waves = 2048
    tot = buf[7] / K / waves
    print(f"== phases, {G} groups x {R} rows x {P} f64")
    print(f"per wave: total {tot:.0f} clk (memtime ticks); groups per wave {G / waves:.0f}; ticks per group {tot / (G / waves):.0f}")
    for k, n in enumerate(names):
        if n != "-":
            print(f"  {n:28s} {buf[k] / K / waves:12.0f}  {100.0 * buf[k] / buf[7]:5.1f} %   per group {buf[k] / K / G:8.1f}")
    print(f"  {'unaccounted':28s} {(buf[7] - sum(buf[:5])) / K / waves:12.0f}  {100.0 * (buf[7] - sum(buf[:5])) / buf[7]:5.1f} %")


def q(a, pct):
    return float(np.percentile(a, pct))


def tail(P):
    if not hasattr(so, "pds_debug_wave_stamps"):
        sys.exit("tail: the library was not built with EXTRA=-DPDS_PROFILE_TAIL (or -DPDS_PROFILE_PHASES)")
    so.pds_debug_wave_stamps.argtypes = [C.c_void_p, C.c_int]
    cap = 4096
    words = so.pds_debug_wave_stamp_words() if hasattr(so, "pds_debug_wave_stamp_words") else 4  # (5: with the first-load stamp)
    raw = np.zeros((cap, words), dtype=np.uint64)
    first_load = []  # per launch: (first load issued - start) of every live wave, us
    f = lambda: pds.lin_reg_by(*xs[:P], target=y, group_offsets=off, ctx=ctx)
    for _ in range(3):
        f()
    ctx.get_timing(reset=True)
    ctx.get_timing_samples("grouped_moments", reset=True)
    ctx.set_timing(True)
    L = args.launches
    rows = []      # per launch: span, idle, ramp, tail shares, end quantiles
    per_xcd = {}   # hardware XCD id -> list of (mean start, mean end, max end, mean busy) relative, us
    per_lbl = {}   # blockIdx % 8     -> the same
    per_half = {}  # first / second half of the grid -> the same
    per_slot = {}  # HW_ID wave slot on its SIMD   -> the same
    hist = np.zeros(12)
    edges_us = [0, 5, 10, 20, 40, 60, 80, 100, 150, 200, 300, 500, 1e9]
    n_waves = 0
    clk = []
    dumped = []
    for _ in range(L):
        f()  # (the entry point synchronises before it returns: the timing hooks are on)
        n = so.pds_debug_wave_stamps(raw.ctypes.data_as(C.c_void_p), cap)
        if n <= 0:
            sys.exit("tail: no stamps came back")
        if args.dump:
            dumped.append(raw[:n].copy())
        live = (raw[:n, 3] >> np.uint64(63)) != 0
        a = (raw[:n] & np.uint64((1 << 62) - 1)).astype(np.int64)
        st, en, mt, xcc = a[live, 0], a[live, 1], a[live, 2], a[live, 3] & 0xF
        slot = (a[live, 3] >> 8) & 0xF  # HW_REG_HW_ID bits 3:0: the wave's slot on its SIMD
        half = (np.nonzero(live)[0] >= (n - n // 2)).astype(np.int64)
        lbl = np.nonzero(live)[0] % 8
        n_waves = int(live.sum())
        t0, t1 = st.min(), en.max()
        span = (t1 - t0) / 100.0  # us (100 MHz)
        if words >= 5:
            first_load.append(np.append((a[live, 4] - st) / 100.0, span))
        busy = (en - st) / 100.0
        s_rel, e_rel = (st - t0) / 100.0, (en - t0) / 100.0
        rows.append((span, 1.0 - busy.mean() / span, s_rel.mean() / span, (span - e_rel).mean() / span, e_rel.min(), q(e_rel, 50), q(e_rel, 95),
                     e_rel.max(), s_rel.max(), q(s_rel, 50)))
        clk.append(float(np.median(mt / np.maximum(busy, 1e-9))))  # shader clocks per us
        for key, ids, store in ((xcc, np.unique(xcc), per_xcd), (lbl, np.arange(8), per_lbl), (half, np.unique(half), per_half),
                                (slot, np.unique(slot), per_slot)):
            for i in ids:
                m = key == i
                store.setdefault(int(i), []).append((s_rel[m].mean(), e_rel[m].mean(), e_rel[m].max(), busy[m].mean(), float(m.sum())))
        hist += np.histogram(span - e_rel, bins=edges_us)[0]
    ctx.set_timing(False)
    if args.dump:
        np.save(f"{args.dump}_p{P}.npy", np.stack(dumped))
    ms = np.array(sorted(ctx.get_timing_samples("grouped_moments", reset=True)))
    ctx.get_timing(reset=True)
    r = np.array(rows)
    med = lambda k: float(np.median(r[:, k]))
    print(f"== tail, {G} groups x {R} rows x {P} f64, {n_waves} waves, {L} launches" if args.frame == "equal" else
          f"== tail, C3 frame: {G} ragged groups, {N} rows x {P} f64, {n_waves} waves, {L} launches")
    print(f"launch time (HIP events), ms: min {ms.min():.4f}  median {np.median(ms):.4f}  max {ms.max():.4f}   "
          f"spread (max - min) / median {100.0 * (ms.max() - ms.min()) / np.median(ms):.2f} %   ({len(ms)} brackets)")
    print(f"first start -> last end, us:  min {r[:, 0].min():.1f}  median {med(0):.1f}  max {r[:, 0].max():.1f}      "
          f"shader clock while resident {np.median(clk) / 1e3:.3f} GHz")
    print(f"idle share 1 - mean(end - start) / (max end - min start):  min {100 * r[:, 1].min():.2f} %  median {100 * med(1):.2f} %  max {100 * r[:, 1].max():.2f} %")
    print(f"   of which ramp (mean start - first start)                 median {100 * med(2):.2f} %")
    print(f"   of which tail (last end - mean end)                      median {100 * med(3):.2f} %")
    print(f"start tick after the first start, us (median over launches): median {med(9):.1f}  max {med(8):.1f}")
    print(f"end tick after the first start, us (median over launches):   min {med(4):.1f}  median {med(5):.1f}  p95 {med(6):.1f}  max {med(7):.1f}")
    if first_load:
        fl = np.array([(q(v[:-1], 5), q(v[:-1], 50), q(v[:-1], 95), v[:-1].max(), v[:-1].mean(), v[-1]) for v in first_load])
        m = lambda k: float(np.median(fl[:, k]))
        print(f"start -> first tile load issued, us per wave (median over launches): p5 {m(0):.2f}  median {m(1):.2f}  p95 {m(2):.2f}  max {m(3):.2f}  "
              f"mean {m(4):.2f}")
        print(f"   median wave as a share of the launch (first start -> last end): {100 * float(np.median(fl[:, 1] / fl[:, 5])):.3f} %   "
              f"mean wave: {100 * float(np.median(fl[:, 4] / fl[:, 5])):.3f} %   (the 100 MHz clock resolves 0.01 us)")
    print("waves by how long before the launch's last end they ended (all launches):")
    for k in range(12):
        hi = "inf" if k == 11 else f"{edges_us[k + 1]:.0f}"
        print(f"   {edges_us[k]:4.0f} .. {hi:>4s} us  {100.0 * hist[k] / hist.sum():6.2f} %")
    for title, store in (("half of the grid (0: blocks [0, W - W/2))", per_half), ("wave slot on the SIMD (HW_ID)", per_slot),
                         ("hardware XCD id", per_xcd), ("blockIdx.x % 8", per_lbl)):
        print(f"by {title} (us after the first start, mean over launches):  waves   mean start   mean end    max end   mean busy   idle share")
        for i in sorted(store):
            v = np.array(store[i]).mean(axis=0)
            print(f"   {i:2d}   {v[4]:7.0f}   {v[0]:9.1f}   {v[1]:9.1f}   {v[2]:9.1f}   {v[3]:9.1f}   {100 * (1 - v[3] / med(0)):6.2f} %")


for P in PS:
    if "phases" in what:
        phases(P)
    if "tail" in what:
        tail(P)
