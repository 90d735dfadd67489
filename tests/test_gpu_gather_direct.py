"""shard.DirectGather (tp_gather_*: the all-gather of projected tokens as per-peer copies + sequence flags, no collective
kernel) between PROCESSES, on the one GPU the box has: two and three ranks all driving cuda:0 through HIP IPC, uneven load,
equal and ragged shards, depth 2 and 3, every step compared bit for bit with the expectation; and bench.py's N > 1 flow
started WITHOUT a launcher (`python bench.py --gpus 2`), in both gather modes."""
import json
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _env(**kw):
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.update(kw)
    return env


@pytest.mark.parametrize("nproc,use_cus", [(2, 0), (3, 0), (2, 1)])
def test_direct_gather_between_processes(nproc, use_cus):
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nproc), "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "tests", "gather_worker.py")]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT, env=_env(TP_GATHER_USE_CUS=str(use_cus)))
    assert res.returncode == 0, (res.stdout[-1500:], res.stderr[-3000:])
    assert res.stdout.count("gather scenarios OK") == nproc


def _bench_no_launcher(extra, n_lines=1, env_extra=None):
    """`python bench.py --gpus 2 ...` exactly as the driver types it for N > 1, with no torch.distributed.run around it."""
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1", "--backend", "gloo",
           "--single-device", "--no-cpu-baseline", "--batch", "8", "--min-seconds", "0.05", "--full"] + extra
    env = _env()
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    env.update(env_extra or {})
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
    assert res.returncode == 0, (res.stdout[-1500:], res.stderr[-3000:])
    lines = [l for l in res.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == n_lines, res.stdout[-2000:]
    return json.loads(lines[0]) if n_lines == 1 else [json.loads(l) for l in lines]


@pytest.mark.parametrize("mode", ["rccl", "sdma"])
def test_bench_spawns_its_own_ranks(mode):
    d = _bench_no_launcher(["--gather", mode, "--probe-other-gather"])
    assert d["n_gpus"] == 2 and d["config"]["global_batch"] == 8 and d["config"]["per_gpu_batch"] == 4
    mg = d["multi_gpu"]
    assert mg["gather"] == mode and mg["ranks"] == 2 and mg["backend"] == "gloo"
    assert [r["rank"] for r in mg["rank_devices"]] == [0, 1] and len({r["pid"] for r in mg["rank_devices"]}) == 2
    assert mg["forward_only_ms"] > 0 and mg["gather_only_ms"] > 0
    assert mg["other_gather"]["mode"] == ("sdma" if mode == "rccl" else "rccl") and mg["other_gather"]["gather_only_ms"] > 0
    assert d["timing"]["long_run"]["blocks"] >= 5


def test_bench_default_is_the_one_rccl_gather_and_one_line():
    """`python bench.py --gpus N` as the driver types it: the ONE collective the north_star names, exactly one line, nothing of
    the copy-engine transport touched."""
    d = _bench_no_launcher([])
    mg = d["multi_gpu"]
    assert mg["gather_requested"] == "rccl" and mg["gather"] == "rccl" and mg["sdma_self_test"] is None
    assert set(mg["transports_timed_ms_per_step"]) == {"rccl"} and "other_gather" not in mg
    assert "clocks" in d


def test_bench_auto_prints_the_rccl_line_first_then_runs_the_sdma_leg_in_fresh_processes():
    first, second = _bench_no_launcher(["--gather", "auto"], n_lines=2)
    assert first["multi_gpu"]["gather"] == "rccl" and first["value"] > 0
    leg = second["sdma_leg"]
    assert leg["status"] == "ok" and leg["value"] > 0 and leg["multi_gpu"]["gather"] == "sdma"
    assert leg["multi_gpu"]["sdma_self_test"] == "passed" and leg["multi_gpu"]["sdma_flags_fine_grained"] is True


def test_a_fault_inside_the_sdma_leg_costs_neither_the_rccl_line_nor_the_exit_code():
    """TP_BENCH_INJECT_SDMA_FAULT: the last rank of the sdma leg aborts (SIGABRT) right after the transport's self-test — the
    stand-in for a device fault inside never-exercised cross-device code.  The rccl line was printed before the leg started and
    parses; the run's exit code is 0; the leg reports its failure."""
    first, second = _bench_no_launcher(["--gather", "auto", "--sdma-leg-timeout", "120"], n_lines=2,
                                       env_extra={"TP_BENCH_INJECT_SDMA_FAULT": "1"})
    assert first["multi_gpu"]["gather"] == "rccl" and first["value"] > 0 and first["n_gpus"] == 2
    assert second["sdma_leg"]["status"].startswith("failed") or second["sdma_leg"]["status"].startswith("timed out")


def test_bench_sdma_sync_gather_and_ragged():
    d = _bench_no_launcher(["--gather", "sdma", "--sync-gather", "--batch", "7"])
    assert d["config"]["global_batch"] == 7 and d["config"]["per_gpu_batch"] == 4 and d["multi_gpu"]["gather"] == "sdma"
