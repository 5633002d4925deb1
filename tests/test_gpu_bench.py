"""-m gpu: a plain bench.py run on one GPU -- the headline line and nothing else, and --dump-outputs.

The run is a fresh child process (nothing here touches the GPU itself)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.timeout(600)
def test_plain_bench_prints_the_headline_and_dumps_the_last_step(tmp_path):
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "WSSDL_FORCE_DIST", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    dump = tmp_path / "out"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--workload", "resnet18_sup_b2", "--dump-outputs", str(dump)]
    p = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=540)
    out = p.stdout.decode()
    assert p.returncode == 0, out[-2000:] + p.stderr.decode()[-4000:]
    lines = [l for l in out.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out[-2000:]
    r = json.loads(lines[0])
    assert r["metric"].startswith("images/sec") and r["unit"] == "images/s" and r["higher_is_better"] is True
    assert r["dtype"] == "f32" and r["steps"] == 3 and r["warmup"] == 1 and r["n_gpus"] == 1
    assert r["ms_per_step"] > 0 and abs(r["value"] - 2 / (r["ms_per_step"] * 1e-3)) <= 0.01 * r["value"]
    for k in ("roofline", "cpu_baseline", "hot_path", "scaling_diag"):        # --full only
        assert k not in r, k
    files = sorted(os.listdir(dump))
    assert "loss.npy" in files and "rpn_cross_entropy.npy" in files
    total = 0
    for f in files:
        a = np.load(dump / f)
        assert a.dtype in (np.float32, np.float64), (f, a.dtype)
        assert np.all(np.isfinite(a)), f
        total += a.nbytes
    assert total <= 64 << 20
    assert abs(float(np.load(dump / "loss.npy")) - r["final_loss"]) <= 1e-6 * max(1.0, abs(r["final_loss"]))
    # same arguments, same inputs: a second run computes the same outputs, up to rounding
    again = tmp_path / "again"
    p = subprocess.run(cmd[:-1] + [str(again)], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=540)
    assert p.returncode == 0, p.stderr.decode()[-4000:]
    assert sorted(os.listdir(again)) == files
    for f in files:
        a, b = np.load(dump / f), np.load(again / f)
        assert np.allclose(a, b, rtol=1e-4, atol=1e-6), (f, a, b)
