"""bench.py's multi-rank path on the one-GPU test box (VERDICT r03 "do this" 1).

`python bench.py --gpus N` without torchrun starts its own N ranks (torch.distributed.run as a
child process, before the parent touches the GPU).  With `--backend gloo --comm torch` every rank
shares the box's GPU, so the whole N > 1 branch runs here: the row partition of the reference's
src/rSVD.cpp:20-23 (uneven at world 3), the n-side reduce-scatter / all-gather
hooks, the barriers around the timed region, the max-over-ranks time and the self-check's
all-reduce.  The line must carry n_gpus = N and a passing self-check.
"""
import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, timeout=300):
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    out = subprocess.run([sys.executable, os.path.join(REPO, "bench.py")] + args, cwd=REPO, env=env,
                         capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-3000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_bench_plain_run_is_the_headline_alone_and_dumps_outputs(tmp_path):
    """Without --full the line carries the headline and none of the extra passes; --dump-outputs
    writes the last timed step's U, S, V (C2-sized: 4096 x 64 fp32, below the sampling bound)."""
    import numpy as np

    d = str(tmp_path / "dump")
    line = _run(["--gpus", "1", "--config", "c2", "--steps", "2", "--warmup", "1", "--dump-outputs", d])
    assert line["steps"] == 2 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["value"] > 0
    assert line["unit"] == "TFLOP/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["full"] is False
    for key in ("roofline", "cpu_baseline", "check", "lowp_intermediates", "c1"):
        assert key not in line
    U, S, V = (np.load(os.path.join(d, f + ".npy")) for f in "USV")
    assert U.dtype == S.dtype == V.dtype == np.float32
    assert U.shape == (4096, 64) and S.shape == (64,) and V.shape == (4096, 64)
    assert np.all(np.isfinite(S)) and S.min() > 0
    # orthonormal columns to fp32 rounding (64 columns of 4096 entries: well below 1e-4)
    assert np.abs(U.T.astype(np.float64) @ U - np.eye(64)).max() < 1e-4
    assert np.abs(V.T.astype(np.float64) @ V - np.eye(64)).max() < 1e-4


@pytest.mark.gpu
@pytest.mark.parametrize("world,m,n,config", [(2, 8192, 8192, "c4"), (3, 8191, 8000, "c4"), (2, 8192, 4096, "c5")])
def test_bench_self_launches_ranks(world, m, n, config):
    line = _run(["--gpus", str(world), "--backend", "gloo", "--comm", "torch", "--config", config,
                 "--m", str(m), "--n", str(n), "--steps", "2", "--warmup", "1", "--full", "--cpu-budget", "0"])
    assert line["n_gpus"] == world
    assert line["steps"] == 2 and line["value"] > 0 and line["ms_per_step"] > 0
    assert line["config"]["m"] == m and line["config"]["n"] == n
    # rank 0's share by the reference's remainder rule (rank < m % world gets one row more)
    assert line["config"]["m_per_gpu"] == m // world + (1 if m % world else 0)
    assert line["check"]["ok"], line["check"]
    assert line["cpu_baseline"] is None  # the CPU leg runs at N = 1 only
