"""``ShardedMainGradAdamW``: (a) without a process group it IS ``MainGradAdamW``, bit for bit, on the real projector (D = 256,
B = 2, three backward + step rounds; bf16, and fp32 under autocast), with ``p.main_grad`` / ``p.data`` views of its flat buffers;
(b) two ranks over gloo that share the one device and (c) one rank over nccl (RCCL's entry points run once), in fresh child
processes (tests/optim_shard_worker.py): the reduced gradient, the step against tests/optim_ref.py, identical parameters on every
rank, a NaN on one rank, and a resume on another world size through ``consolidated_state_dict()``."""
import os
import socket
import subprocess
import sys

import pytest
import torch

from tokenpacker_amd import MainGradAdamW, ShardedMainGradAdamW, TokenPacker

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV, D, B, S = "cuda", 256, 2, 2


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def make_module(dtype):
    torch.manual_seed(0)
    m = TokenPacker(hidden_size=D, scale_factor=S).to(device=DEV, dtype=torch.bfloat16).to(dtype)     # (values exact in bf16)
    m.use_main_grad = True
    return m


def make_inputs():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, 576, 1024, generator=g).to(device=DEV, dtype=torch.bfloat16)
    xm = torch.randn(B, 576, 4096, generator=g).to(device=DEV, dtype=torch.bfloat16)
    w = torch.randn(B, (24 // S) ** 2, D, generator=g).to(device=DEV)
    return x, xm, w


def groups_of(m):
    named = [(n, p) for n, p in m.named_parameters() if p.requires_grad]
    return [{"params": [p for n, p in named if p.dim() >= 2], "weight_decay": 0.1},
            {"params": [p for n, p in named if p.dim() < 2], "weight_decay": 0.0}]


def backward(m, inputs):
    x, xm, w = inputs
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y = m((x, xm))
    (y.float() * w).sum().backward()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32_autocast"])
def test_without_a_process_group_it_is_main_grad_adamw(dtype):
    inputs = make_inputs()
    a, b = make_module(dtype), make_module(dtype)
    a.init_main_grads()                                      # (b's parameters have no main_grad: the optimizer makes them)
    plain = MainGradAdamW(groups_of(a), lr=1e-3, module=a)
    sharded = ShardedMainGradAdamW(groups_of(b), lr=1e-3, module=b)
    assert sharded.world == 1 and sharded.tensor_names == plain.tensor_names and len(sharded.tensor_names) == 23
    lay = sharded.layout
    for p, off in zip((q for g in sharded.param_groups for q in g["params"]), lay["offsets"]):
        assert p.main_grad.data_ptr() == sharded.flat_grad.data_ptr() + 4 * off
        assert p.data_ptr() == sharded.flat_param.data_ptr() + p.element_size() * off
        assert p.main_grad.shape == p.shape and p.main_grad.dtype == torch.float32 and not bool(p.main_grad.any())
    sched = [torch.optim.lr_scheduler.LambdaLR(o, lambda k: 1.0 / (1 + k)) for o in (plain, sharded)]
    for step in range(3):
        backward(a, inputs)
        backward(b, inputs)
        assert all(p.grad is None for p in b.parameters())
        for (n, pa), (_, pb) in zip(a.named_parameters(), b.named_parameters()):
            assert torch.equal(bits(pa.main_grad), bits(pb.main_grad)) and bool(pb.main_grad.any()), (step, n)
        plain.step()
        sharded.step()
        for s in sched:
            s.step()
        torch.cuda.synchronize()
        assert int(sharded.steps_applied) == step + 1 and float(sharded.clip_coef) < 1.0
        assert torch.equal(plain._block.cpu(), sharded._block.cpu()), f"step {step}: the state words differ"
        for (pa, pb), off in zip(zip((q for g in plain.param_groups for q in g["params"]),
                                     (q for g in sharded.param_groups for q in g["params"])), lay["offsets"]):
            here = slice(off, off + pa.numel())
            assert torch.equal(bits(pa.detach()), bits(pb.detach())), (step, tuple(pa.shape))
            assert torch.equal(bits(plain.state[pa]["exp_avg"].flatten()), bits(sharded.exp_avg[here]))
            assert torch.equal(bits(plain.state[pa]["exp_avg_sq"].flatten()), bits(sharded.exp_avg_sq[here]))
            assert torch.equal(bits(plain.state[pa]["master"].flatten()), bits(sharded.master[here]))
            assert not bool(pb.main_grad.any()), "main_grad is zeroed behind the step"
    if dtype == torch.float32:
        assert sharded.master is sharded.param_shard and "master" not in sharded.state_dict()["shards"]
    # the consolidated form is MainGradAdamW's state dict
    sa, sb = plain.state_dict(), sharded.consolidated_state_dict()
    assert sa["main_grad_adamw"] == sb["main_grad_adamw"] and sorted(sa["state"]) == sorted(sb["state"])
    for i in sa["state"]:
        assert set(sa["state"][i]) == set(sb["state"][i])
        for k in sa["state"][i]:
            assert torch.equal(sa["state"][i][k], sb["state"][i][k]), (i, k)


def test_a_replaced_buffer_is_named():
    m = make_module(torch.bfloat16)
    opt = ShardedMainGradAdamW(m.parameters(), lr=1e-3, module=m)
    p = m.mlp[0].bias
    p.main_grad = torch.zeros_like(p.main_grad)
    with pytest.raises(RuntimeError, match=r"mlp\.0\.bias\.main_grad is no longer the view"):
        opt.step()
    m = make_module(torch.bfloat16)
    opt = ShardedMainGradAdamW(m.parameters(), lr=1e-3, module=m)
    m.mlp[2].weight.data = m.mlp[2].weight.data.clone()
    with pytest.raises(RuntimeError, match=r"parameter mlp\.2\.weight is no longer the view"):
        opt.step()


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def run_ranks(backend, world):
    """The worker as `world` fresh child processes (the suite's process must not own a process group).  A rank that fails or
    runs out of time ends the others; nothing more is started."""
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()), WORLD_SIZE=str(world),
               HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, os.path.join(ROOT, "tests", "optim_shard_worker.py"), backend]
    procs = [subprocess.Popen(cmd, env=dict(env, RANK=str(r), LOCAL_RANK=str(r)), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                              text=True) for r in range(world)]
    outs = []
    try:
        for p in procs:
            outs.append(p.communicate(timeout=240))
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
    for r, (p, (out, err)) in enumerate(zip(procs, outs)):
        assert p.returncode == 0 and f"rank {r}: sharded optimizer OK" in out, (r, p.returncode, out[-2000:], err[-4000:])


def test_two_ranks_over_gloo_on_one_device():
    assert ShardedMainGradAdamW is not None
    run_ranks("gloo", 2)


def test_one_rank_over_nccl():
    run_ranks("nccl", 1)
