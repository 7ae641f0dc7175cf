"""A plain ``bench.py`` run (no --full): the headline line and nothing else, --steps timed steps, and --dump-outputs writing
what the last timed step returned -- the same files, bit for bit, from two runs with the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_bench(dump_dir):
    env = {k: v for k, v in os.environ.items() if not k.startswith("PV_")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "16",
           "--dump-outputs", str(dump_dir)]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert r.returncode == 0 and len(lines) == 1, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return json.loads(lines[0])


@pytest.mark.timeout(1200)
def test_plain_bench_line_and_dumped_outputs(tmp_path):
    line = run_bench(tmp_path / "a")
    assert line["metric"] == "images/sec run_with_cache (all hooks) CLIP ViT-B/32 @224" and line["unit"] == "images/s"
    assert line["higher_is_better"] is True and line["dtype"] == "bf16" and line["steps"] == 3 and line["warmup"] == 1
    assert line["value"] > 0 and line["ms_per_step"] > 0 and line["ok"] is True and line["full"] is False
    assert abs(line["value"] - 16 * 1e3 / line["ms_per_step"]) <= 1e-2 * line["value"]
    for k in ("roofline", "kernels", "sae", "l14_336_pattern", "cpu_baseline"):
        assert k not in line, k
    files = sorted(os.listdir(tmp_path / "a"))
    assert len(files) == 1 + 214 and "output.npy" in files
    out = np.load(tmp_path / "a" / "output.npy")
    assert out.shape == (16, 512) and out.dtype == np.float32 and np.isfinite(out).all()
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 64 << 20
    run_bench(tmp_path / "b")
    assert sorted(os.listdir(tmp_path / "b")) == files
    for f in files:
        x, y = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert x.dtype == np.float32 and np.array_equal(x, y), f
