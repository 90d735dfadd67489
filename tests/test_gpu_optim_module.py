"""``MainGradAdamW`` on the real projector (D = 256, B = 2, scale_factor 2, bf16, ``use_main_grad``): three training steps under a
``LambdaLR`` with a decay and a no-decay parameter group, each step checked against tests/optim_ref.py from a snapshot of the
gradients and the optimizer state; ``main_grad`` zeroed; the next forward runs on the new weights; a partially frozen module; the
state dict round trip; a ``torch.optim.AdamW`` state dict."""
import copy

import pytest
import torch

from tests import optim_ref as R
from tokenpacker_amd import MainGradAdamW, TokenPacker

pytestmark = pytest.mark.gpu
DEV, D, B, S = "cuda", 256, 2, 2


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def make_module(trainable=("",)):
    torch.manual_seed(0)
    m = TokenPacker(hidden_size=D, scale_factor=S).to(device=DEV, dtype=torch.bfloat16)
    for name, p in m.named_parameters():
        p.requires_grad_(name.startswith(tuple(trainable)))
    m.use_main_grad = True
    m.init_main_grads()
    return m


def make_inputs():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, 576, 1024, generator=g).to(device=DEV, dtype=torch.bfloat16)
    xm = torch.randn(B, 576, 4096, generator=g).to(device=DEV, dtype=torch.bfloat16)
    w = torch.randn(B, (24 // S) ** 2, D, generator=g).to(device=DEV)
    return x, xm, w


def groups_of(m):
    """llava_trainer.create_optimizer's split: weights decay, biases and LayerNorm parameters do not."""
    named = [(n, p) for n, p in m.named_parameters() if p.requires_grad]
    return [{"params": [p for n, p in named if p.dim() >= 2], "weight_decay": 0.1},
            {"params": [p for n, p in named if p.dim() < 2], "weight_decay": 0.0}]


def backward(m, inputs):
    x, xm, w = inputs
    (m((x, xm)).float() * w).sum().backward()


def snapshot(opt):
    out = []
    for group in opt.param_groups:
        for p in group["params"]:
            if p.requires_grad:
                st = opt.state[p]
                out.append({"p": st["master"].flatten().clone(), "m": st["exp_avg"].flatten().clone(), "v": st["exp_avg_sq"].flatten().clone(),
                            "g": p.main_grad.flatten().clone(), "lr": group["lr"], "wd": group["weight_decay"], "param": p})
    return out


def test_three_training_steps_against_the_reference():
    m, inputs = make_module(), make_inputs()
    x, xm, _ = inputs
    opt = MainGradAdamW(groups_of(m), lr=1e-3, module=m)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda k: 1.0 / (1 + k))
    hyper = R.Hyper(0.9, 0.999, 1e-8, 1.0)
    assert sorted(opt.tensor_names) == sorted(n for n, _ in m.named_parameters()) and len(opt.tensor_names) == 23
    with torch.no_grad():
        y_prev = m((x, xm)).clone()                              # (leaves a cached weight image behind: the step must drop it)
    for step in range(3):
        backward(m, inputs)
        assert all(p.grad is None for p in m.parameters())       # use_main_grad: autograd was told nothing
        before = snapshot(opt)
        assert all(bool(t["g"].any()) for t in before if t["g"].numel() > 1)
        lrs = [g["lr"] for g in opt.param_groups]
        assert lrs == [pytest.approx(1e-3 / (1 + step))] * 2
        opt.step()
        sched.step()
        torch.cuda.synchronize()
        ref = R.step_ref(before, hyper, step)
        assert int(opt.found_inf) == 0 and int(opt.steps_applied) == step + 1 and int(opt.steps_skipped) == 0
        norm = float(opt.grad_norm.double())
        assert abs(norm ** 2 - ref["norm"] ** 2) <= R.SUMSQ_REL * ref["norm"] ** 2
        assert float(opt.clip_coef) == pytest.approx(ref["coef"], rel=2 * R.COEF_REL)
        for t, (p2, m2, v2), (ep, em, ev) in zip(before, ref["out"], R.bounds(before, hyper, step, ref)):
            p, st = t["param"], opt.state[t["param"]]
            for name, a, b, e in (("master", st["master"], p2, ep), ("exp_avg", st["exp_avg"], m2, em), ("exp_avg_sq", st["exp_avg_sq"], v2, ev)):
                r = R.worst_ratio(a.flatten(), b, e)
                assert r <= 1.0, f"step {step} {tuple(p.shape)} {name}: |got - ref| / bound = {r:.3f}"
            assert torch.equal(bits(p.detach()), bits(R.cast_ref(st["master"], torch.bfloat16)))
            assert not bool(p.main_grad.any()), "main_grad is zeroed behind the step"
        # the next forward runs on the new weights: not the previous output, and what a fresh module with these weights computes
        with torch.no_grad():
            y = m((x, xm)).clone()
            fresh = TokenPacker(hidden_size=D, scale_factor=S).to(device=DEV, dtype=torch.bfloat16)
            fresh.load_state_dict(m.state_dict())
            y_fresh = fresh((x, xm))
        assert not torch.equal(y, y_prev)
        assert torch.equal(bits(y), bits(y_fresh))
        y_prev = y


def test_a_partially_frozen_module_builds_a_table_of_the_trainable_tensors():
    m, inputs = make_module(trainable=("mlp.",)), make_inputs()
    opt = MainGradAdamW(m.parameters(), lr=1e-3, weight_decay=0.1, module=m)       # every parameter is handed over; 4 are taken
    assert opt.tensor_names == ["mlp.0.weight", "mlp.0.bias", "mlp.2.weight", "mlp.2.bias"]
    assert len(opt.state) == 4 and sorted(opt.state_dict()["state"]) == [19, 20, 21, 22]
    old = {n: p.detach().clone() for n, p in m.named_parameters()}
    backward(m, inputs)
    opt.step()
    torch.cuda.synchronize()
    assert int(opt.steps_applied) == 1
    for n, p in m.named_parameters():
        assert torch.equal(bits(p.detach()), bits(old[n])) != n.startswith("mlp."), n
        assert hasattr(p, "main_grad") == n.startswith("mlp.")


def test_state_dict_round_trip_continues_bit_identically():
    a, inputs = make_module(), make_inputs()
    opt_a = MainGradAdamW(groups_of(a), lr=1e-3, module=a)
    sched = torch.optim.lr_scheduler.LambdaLR(opt_a, lambda k: 1.0 / (1 + k))
    for _ in range(2):
        backward(a, inputs)
        opt_a.step()
        sched.step()
    saved = copy.deepcopy(opt_a.state_dict())
    assert saved["main_grad_adamw"]["steps_applied"] == 2 and set(saved["state"][0]) == {"step", "exp_avg", "exp_avg_sq", "master"}
    b = make_module()
    b.load_state_dict(a.state_dict())
    opt_b = MainGradAdamW(groups_of(b), lr=7.0, module=b)          # (its own lr is replaced by the loaded groups')
    opt_b.load_state_dict(saved)
    assert [g["lr"] for g in opt_b.param_groups] == [g["lr"] for g in opt_a.param_groups] == [pytest.approx(1e-3 / 3)] * 2
    assert int(opt_b.steps_applied) == 2
    for mod, opt in ((a, opt_a), (b, opt_b)):
        backward(mod, inputs)
        opt.step()
    torch.cuda.synchronize()
    assert int(opt_a.steps_applied) == int(opt_b.steps_applied) == 3
    assert torch.equal(bits(opt_a.grad_norm.reshape(1)), bits(opt_b.grad_norm.reshape(1)))
    for (n, pa), (_, pb) in zip(a.named_parameters(), b.named_parameters()):
        assert torch.equal(bits(pa.detach()), bits(pb.detach())), n
        for k in ("master", "exp_avg", "exp_avg_sq"):
            assert torch.equal(bits(opt_a.state[pa][k]), bits(opt_b.state[pb][k])), (n, k)


def test_a_torch_adamw_state_dict_loads():
    """The per-parameter keys and the group keys are torch's: the moments and the step count are taken, the masters come from the
    parameters."""
    g = torch.Generator().manual_seed(5)
    shapes = ((33,), (8, 16))
    ours = [torch.nn.Parameter((0.02 * torch.randn(s, generator=g)).to(device=DEV, dtype=torch.bfloat16)) for s in shapes]
    theirs = [torch.nn.Parameter(p.detach().float()) for p in ours]
    topt = torch.optim.AdamW(theirs, lr=2e-3, weight_decay=0.05)
    for p in theirs:
        p.grad = torch.randn(p.shape, generator=g).to(DEV)
    topt.step()
    for p in ours:
        p.main_grad = torch.zeros(p.shape, dtype=torch.float32, device=DEV)
    opt = MainGradAdamW(ours, lr=1.0)
    opt.load_state_dict(topt.state_dict())
    assert int(opt.steps_applied) == 1 and int(opt.steps_skipped) == 0
    assert opt.param_groups[0]["lr"] == 2e-3 and opt.param_groups[0]["weight_decay"] == 0.05
    for p, q in zip(ours, theirs):
        assert torch.equal(opt.state[p]["exp_avg"], topt.state[q]["exp_avg"])
        assert torch.equal(opt.state[p]["exp_avg_sq"], topt.state[q]["exp_avg_sq"])
        assert torch.equal(opt.state[p]["master"], p.detach().float())
    # ... and the next step carries the bias correction of step 2
    before = [{"p": opt.state[p]["master"].flatten().clone(), "m": opt.state[p]["exp_avg"].flatten().clone(),
               "v": opt.state[p]["exp_avg_sq"].flatten().clone(), "lr": 2e-3, "wd": 0.05} for p in ours]
    for p, t in zip(ours, before):
        p.main_grad.copy_(torch.randn(p.shape, generator=g))
        t["g"] = p.main_grad.flatten().clone()
    opt.step()
    torch.cuda.synchronize()
    hyper = R.Hyper(0.9, 0.999, 1e-8, 1.0)
    ref = R.step_ref(before, hyper, 1)
    assert int(opt.steps_applied) == 2
    for p, (p2, m2, v2), (ep, em, ev) in zip(ours, ref["out"], R.bounds(before, hyper, 1, ref)):
        assert R.worst_ratio(opt.state[p]["master"].flatten(), p2, ep) <= 1.0
        assert R.worst_ratio(opt.state[p]["exp_avg"].flatten(), m2, em) <= 1.0
        assert R.worst_ratio(opt.state[p]["exp_avg_sq"].flatten(), v2, ev) <= 1.0
