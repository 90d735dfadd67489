"""bench.py's plain N = 1 run (no --full): exactly K timed steps, the contract fields and nothing that takes measurements of its
own; --dump-outputs writes what the last timed step returned, and that is what the product computes on the bench's inputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_plain_line_and_dumped_outputs(tmp_path):
    B = 8
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", str(B),
           "--dump-outputs", str(tmp_path)]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [l for l in res.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, res.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["metric"] == "projector images/sec" and d["unit"] == "images/s" and d["higher_is_better"] is True
    assert d["dtype"] == "bf16" and d["steps"] == 3 and d["config"]["global_batch"] == B
    assert d["value"] > 0 and abs(d["value"] - B / (d["ms_per_step"] * 1e-3)) / d["value"] < 1e-3
    for key in ("roofline", "stages_ms", "clocks", "timing", "cpu_baseline", "eager_rocm_baseline", "sweep", "pack_ms"):
        assert key not in d, key

    files = sorted(os.listdir(tmp_path))
    assert files == ["tokens.npy"], files
    got = np.load(tmp_path / "tokens.npy")
    assert got.dtype == np.float32 and got.shape == (B, 144, 4096)

    import bench
    device = torch.device("cuda", 0)
    model = bench.build_model(4096, 2, torch.bfloat16, device)
    x, xm = bench.make_device_inputs(B, torch.bfloat16, "tower", device, seed=1234)
    with torch.no_grad():
        y = model((x, xm)).float().cpu().numpy()
    assert np.array_equal(got, y)
