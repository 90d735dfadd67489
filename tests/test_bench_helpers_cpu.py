"""bench.py's PMC side files (CPU): the traffic / sustained-clock numbers are only reported when profiles/traffic.json was stamped on
THIS kernel source — a stale or broken file must never reach the bench line, and must never break it."""
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _write(tmp_path, sha, **entry):
    os.makedirs(tmp_path / "profiles", exist_ok=True)
    doc = {"_stamp": {"tag": "t", "head": "h", "kernel_source_sha16": sha},
           "kv_layer0_B256_bf16": {"total": 4.2e9, "shader_clock_ghz": 1.8, **entry}}
    (tmp_path / "profiles" / "traffic.json").write_text(json.dumps(doc))


def test_kernel_source_digest_is_stable_and_names_every_kernel_source():
    d = bench.kernel_source_digest()
    assert d == bench.kernel_source_digest() and len(d) == 16 and int(d, 16) >= 0


def test_the_shipped_traffic_file_is_stamped_on_the_shipped_sources():
    doc = json.load(open(os.path.join(ROOT, "profiles", "traffic.json")))
    if doc["_stamp"]["kernel_source_sha16"] != bench.kernel_source_digest():
        # not a failure of the product: bench.py refuses a stale file by itself (next test); the skip is the reminder
        pytest.skip("profiles/traffic.json is stale: re-run `tools/gpu_round.sh <tag> pmc` after editing tokenpacker_amd/csrc")


def test_current_stamp_is_reported_and_stale_stamp_refused(tmp_path, monkeypatch):
    sha = bench.kernel_source_digest()
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    monkeypatch.setattr(bench, "kernel_source_digest", lambda: sha)
    _write(tmp_path, sha)
    traffic, src = bench.load_traffic(256, "bf16", "tower")
    assert traffic == 4.2e9 and src.startswith("t @")
    assert bench.load_sustained_clock(256, "bf16", "tower") == 1.8
    assert bench.load_traffic(256, "bf16", "contiguous") == (None, None)          # measured on the tower layout only
    assert bench.load_sustained_clock(32, "bf16", "tower") is None                 # no entry for this batch
    _write(tmp_path, "0" * 16)
    traffic, src = bench.load_traffic(256, "bf16", "tower")
    assert traffic is None and "stale" in src
    assert bench.load_sustained_clock(256, "bf16", "tower") is None


def test_broken_file_does_not_break_the_line(tmp_path, monkeypatch):
    sha = bench.kernel_source_digest()
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    monkeypatch.setattr(bench, "kernel_source_digest", lambda: sha)
    os.makedirs(tmp_path / "profiles")
    (tmp_path / "profiles" / "traffic.json").write_text("{not json")
    traffic, src = bench.load_traffic(256, "bf16", "tower")
    assert traffic is None and "unreadable" in src
    assert bench.load_sustained_clock(256, "bf16", "tower") is None


def test_plain_run_is_the_default_and_steps_must_be_positive(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse_args()
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse_args()
    assert a.full and a.dump_outputs == "d"
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "0"])
    with pytest.raises(SystemExit):
        bench.parse_args()


def test_dump_outputs_whole_and_sampled(tmp_path, monkeypatch):
    """--dump-outputs: a small output is written whole in float32; a larger one as a seeded sample of its rows (the same rows
    every run), their flat indices and the float64 sum of every row, within the byte budget."""
    import numpy as np
    monkeypatch.setattr(bench, "DUMP_SAMPLE_BYTES", 2 * 1024 * 4 * 16)       # 16 rows of 1024 fp32 per output
    g = torch.Generator().manual_seed(0)
    small = torch.randn(2, 3, 8, generator=g).to(torch.bfloat16)
    big = torch.randn(4, 50, 1024, generator=g).to(torch.bfloat16)
    bench.dump_outputs(str(tmp_path / "a"), {"small": small, "big": big})
    bench.dump_outputs(str(tmp_path / "b"), {"small": small, "big": big})
    a = {f: np.load(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")}
    assert sorted(a) == ["big.npy", "big_row_sum.npy", "big_rows.npy", "small.npy"]
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert np.array_equal(a["small.npy"], small.float().numpy())
    rows = a["big_rows.npy"].astype(np.int64)
    assert len(rows) == 16 and np.all(np.diff(rows) > 0) and rows.max() < 200
    assert np.array_equal(a["big.npy"], big.reshape(-1, 1024).float().numpy()[rows])
    assert a["big_row_sum.npy"].shape == (4, 50)
    assert np.allclose(a["big_row_sum.npy"], big.double().sum(-1).numpy(), rtol=0, atol=1e-9)
    for f, v in a.items():
        assert np.array_equal(v, np.load(tmp_path / "b" / f)), f
