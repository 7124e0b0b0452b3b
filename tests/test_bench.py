"""bench.py's plain run and --dump-outputs: the plain command times exactly --steps steps once and prints the headline line only;
the outputs of its last timed step are written as float32 .npy files and are the same from run to run with the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*args):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + [str(a) for a in args], capture_output=True, text=True,
                       env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_dump_outputs_sample_is_fixed_and_bounded(tmp_path):
    """above the size limit every array keeps the same seeded rows, listed in agent_index.npy (own process: importing bench
    sets HIP environment variables)"""
    code = ("import sys, numpy as np; sys.path.insert(0, sys.argv[1]); import bench\n"
            "a = {'obs': np.arange(13000, dtype=np.float32).reshape(1000, 13), 'reward': np.arange(1000.), 'done': np.ones(1000, bool)}\n"
            "for d in sys.argv[2:]: bench.dump_outputs(d, a, limit=20000)\n")
    dirs = [tmp_path / "a", tmp_path / "b"]
    subprocess.run([sys.executable, "-c", code, ROOT] + [str(d) for d in dirs], check=True, timeout=300)
    got = [{f[:-4]: np.load(d / f) for f in os.listdir(d)} for d in dirs]
    assert sorted(got[0]) == ["agent_index", "done", "obs", "reward"]
    assert sum(a.nbytes for a in got[0].values()) <= 20000
    idx = got[0]["agent_index"]
    assert idx.dtype == np.float64 and np.all(np.diff(idx) > 0) and len(idx) < 1000
    rows = idx.astype(np.int64)
    assert got[0]["obs"].dtype == np.float32 and np.array_equal(got[0]["obs"][:, 0], rows * 13)
    assert np.array_equal(got[0]["reward"], rows.astype(np.float32)) and np.all(got[0]["done"] == 1)
    for k in got[0]:
        assert np.array_equal(got[0][k], got[1][k]), k


@pytest.mark.gpu
def test_plain_run_and_dumped_outputs(tmp_path):
    N, K = 4096, 37                        # K not a multiple of the 16-step chunk: the timed region ends on a short step_n call
    lines, dumps = [], []
    for i in range(2):
        d = tmp_path / f"run{i}"
        lines.append(_bench("--gpus", 1, "--steps", K, "--warmup", 5, "--agents", N, "--dump-outputs", d))
        dumps.append({f[:-4]: np.load(d / f) for f in os.listdir(d)})
    out = lines[0]
    assert out["steps"] == K and out["warmup"] == 5 and out["timing"]["repeats"] == 1
    assert out["unit"] == "agent-steps/s" and out["higher_is_better"] is True and out["dtype"] == "f32"
    assert abs(out["value"] - N * K / (out["ms_per_step"] * 1e-3 * K)) < 1e-6 * out["value"]
    for extra in ("secondary", "cpu_baseline", "roofline", "sustained", "with_resets", "rollout_fused", "value_without_spinup"):
        assert extra not in out, extra                 # --full only
    assert sorted(dumps[0]) == ["done", "obs", "reward"]
    assert dumps[0]["obs"].shape == (N, 13) and dumps[0]["reward"].shape == (N,) and dumps[0]["done"].shape == (N,)
    for k, a in dumps[0].items():
        assert a.dtype == np.float32 and np.isfinite(a).all(), k
        assert np.array_equal(a.view(np.uint32), dumps[1][k].view(np.uint32)), f"{k} differs between two runs with the same arguments"
    assert set(np.unique(dumps[0]["done"])) <= {0.0, 1.0}
