"""
Penalised grouped GLM fits (pds_glm_enet_grouped_*, csrc/grouped_irls.hip PEN = 1) beside the unpenalised call on the same frame, one
MI355X, inputs resident in HBM, offsets form: the method of tools/grouped_glm_bench.py (median / best / worst of `--reps` warmed
calls by device events).  Frames: headline = 1e6 groups x 100 rows x 8 features + bias, binomial; wide = the same with 16 features,
poisson.  Per frame one line for the unpenalised call and one per penalty pair (0, 0.05), (0.02, 0), (0.02, 0.05): time per call,
mean outer iterations, the ratio to the unpenalised call of the same run, and the mean inner sweeps per group -- the device does
not report sweeps, so that figure is the NumPy restatement's (tests/glm_penalised_reference.py, the same algorithm) on the first
`--sweep-groups` groups of the frame, copied to the host.
Comparing the unpenalised call between two builds: run tools/grouped_glm_bench.py --shapes headline,wide --sample 0 from each tree
in turn, several times over (profiles/grouped_glm_penalised_bench.txt has such a run).
"""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from grouped_glm_bench import make_frame, timed  # noqa: E402

import polars_ds_extension_amd as pds  # noqa: E402

PENALTIES = ((0.0, 0.05), (0.02, 0.0), (0.02, 0.05))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="headline,wide")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--sweep-groups", type=int, default=200)
    a = ap.parse_args()
    import glm_penalised_reference as ref

    dev = torch.device("cuda", 0)
    ctx = pds.Context(0)
    ctx.set_stream(torch.cuda.current_stream(dev))
    gen = torch.Generator(device=dev)
    gen.manual_seed(3)
    for name, p, family in (("headline", 8, "binomial"), ("wide", 16, "poisson")):
        if name not in a.shapes.split(","):
            continue
        G, m = int(1_000_000 * a.scale), 100
        off = torch.arange(0, G * m + 1, m, dtype=torch.int64, device=dev)
        X, y = make_frame(gen, dev, G * m, p, family, off)
        k = min(a.sweep_groups, G)
        Xh = torch.stack([c[:k * m] for c in X], dim=1).cpu().numpy()
        yh, offh = y[:k * m].cpu().numpy(), np.arange(0, k * m + 1, m)
        base = None
        for l1, l2 in ((0.0, 0.0),) + PENALTIES:
            call = lambda: pds.glm_by(*X, target=y, group_offsets=off, family=family, add_bias=True, tol=1e-8, max_iter=100, ctx=ctx,  # noqa: E731
                                      l1_reg=l1, l2_reg=l2)
            ms, best, worst = timed(call, a.reps)
            co, it, nu = call()
            base = ms if base is None else base
            sweeps = None
            if l1 > 0.0:
                sweeps = round(float(ref.fit(Xh, yh, offh, family, True, l1, l2, tol=1e-8, max_iter=100)[2].mean()), 1)
            zeros = float((co[:, :p] == 0).double().mean().item())
            print(json.dumps({"bench": "grouped_glm_penalised", "shape": name, "groups": G, "rows_per_group": m, "p": p, "family": family,
                              "l1_reg": l1, "l2_reg": l2, "ms": round(ms, 3), "ms_best": round(best, 3), "ms_worst": round(worst, 3),
                              "ratio_to_unpenalised": round(ms / base, 2), "mean_n_iter": round(float(it.double().mean().item()), 2),
                              "groups_at_max_iter": int((it >= 100).sum().item()), "null_groups": int(nu.sum().item()),
                              "zero_feature_coefficients": round(zeros, 4), "restatement_sweeps_per_group": sweeps}), flush=True)
        del X, y


if __name__ == "__main__":
    main()
