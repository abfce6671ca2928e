"""
bench.py's plain run and `--dump-outputs DIR`: a plain run prints the headline line only (the other legs run under `--full`), and
the dump holds what the last timed step returned -- the coefficients and null flags of a fixed, seeded sample of the groups -- on
inputs that are the same from run to run.  CPU: the dry run (PDS_BENCH_DRYRUN=1, tests/test_bench_dryrun.py) at world size 2 and
the sampling on its own; GPU: the dumped coefficients of the HIP path against the oracle on the regenerated frame.
"""
import json
import os
import socket
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent

HEADLINE_KEYS = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_KEYS = ("roofline", "gram_build", "grouped_p8", "grouped_by_key", "cpu_baseline", "parity_spot_check", "dist_step", "end_to_end",
             "other_configs", "grouped_c3spec", "scatter")
DUMP_LIMIT = 64 * 1024 * 1024


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _line(r):
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def _load_dump(d):
    files = sorted(Path(d).glob("*.npy"))
    assert sum(f.stat().st_size for f in files) <= DUMP_LIMIT
    out = {f.stem: np.load(f) for f in files}
    assert set(out) == {"coefficients", "null_flags", "group_index"}
    for a in out.values():
        assert a.dtype in (np.float32, np.float64)
    return out


@pytest.mark.timeout(600)
def test_bench_plain_run_dumps_the_same_outputs_twice(tmp_path):
    env = dict(os.environ, PDS_BENCH_DRYRUN="1", OMP_NUM_THREADS="1", MKL_NUM_THREADS="1")
    got = []
    for k in range(2):
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
               "--master-port", str(_free_port()), str(ROOT / "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1",
               "--groups", "1201", "--rows-per-group", "12", "--feats", "4", "--dump-outputs", str(tmp_path / f"run{k}")]
        d = _line(subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=540, cwd=str(ROOT)))
        assert all(k_ in d for k_ in HEADLINE_KEYS) and not any(k_ in d for k_ in FULL_KEYS)
        assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["value"] > 0
        got.append(_load_dump(tmp_path / f"run{k}"))
    a, b = got
    # rank 0's gathered result: every group of the frame (fewer than the sample size), one row of coefficients each
    assert a["coefficients"].shape == (1201, 4) and a["null_flags"].shape == (1201,)
    np.testing.assert_array_equal(a["group_index"], np.arange(1201))
    for name in a:
        np.testing.assert_array_equal(a[name], b[name])
    assert np.isfinite(a["coefficients"]).all() and not a["null_flags"].any()


def test_dump_sample_is_fixed_and_bounded(tmp_path):
    import torch

    sys.path.insert(0, str(ROOT))
    import bench

    G, P = 400_000, 16
    co = torch.arange(G * P, dtype=torch.float64).reshape(G, P)
    nu = (torch.arange(G) % 7 == 0).to(torch.uint8)
    for k in range(2):
        bench._dump_outputs(np, torch, tmp_path / f"d{k}", co, nu)
    a, b = _load_dump(tmp_path / "d0"), _load_dump(tmp_path / "d1")
    idx = a["group_index"].astype(np.int64)
    assert len(idx) == bench.DUMP_SAMPLE_GROUPS and (np.diff(idx) > 0).all() and idx[0] >= 0 and idx[-1] < G
    np.testing.assert_array_equal(a["coefficients"], co.numpy()[idx])
    np.testing.assert_array_equal(a["null_flags"], (idx % 7 == 0).astype(np.float32))
    for name in a:
        np.testing.assert_array_equal(a[name], b[name])


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_bench_dump_matches_oracle(tmp_path, orc):
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    G, R, P = 300_000, 20, 16  # more groups than the dump samples
    cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--groups", str(G),
           "--rows-per-group", str(R), "--feats", str(P), "--dump-outputs", str(tmp_path / "out")]
    d = _line(subprocess.run(cmd, capture_output=True, text=True, timeout=540, cwd=str(ROOT)))
    assert d["steps"] == 2 and d["ms_per_step"] > 0 and not any(k in d for k in FULL_KEYS)
    out = _load_dump(tmp_path / "out")
    idx = out["group_index"].astype(np.int64)
    assert out["coefficients"].shape == (len(idx), P) and len(idx) < G
    # the frame bench.py timed (tools/synth.headline_frame, seed 1234 on rank 0), the sampled groups only
    sys.path.insert(0, str(ROOT / "tools"))
    import synth

    xs, y = synth.headline_frame(G, R, P, seed=1234, device="cuda")
    rows = torch.from_numpy((idx[:, None] * R + np.arange(R)).ravel()).cuda()
    cols = [y[rows].cpu().numpy()] + [x[rows].cpu().numpy() for x in xs]
    del xs, y
    co_o, nu_o = orc.grouped_lr(cols, np.arange(0, len(idx) * R + 1, R, dtype=np.int64), add_bias=False, tol=1e-12,
                                nthreads=max(1, min(16, orc.max_threads())))
    assert not nu_o.any() and not out["null_flags"].any()
    err = np.linalg.norm(out["coefficients"] - co_o, axis=1) / np.linalg.norm(co_o, axis=1)
    assert err.max() < 1e-10, err.max()
