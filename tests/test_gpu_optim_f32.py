"""tp_optim_step and ``MainGradAdamW`` on fp32 parameters, which are their own masters (tp_optim_hyper.dtype = TP_F32; `param` NULL):
every step against tests/optim_ref.py from a snapshot, within its bounds — the only tolerances here —; the vector and the scalar
path; a non-finite norm; the zeroing; and the lockstep of an fp32 module under autocast with its bf16 twin, bit for bit."""
import ctypes

import pytest
import torch

from tests import optim_ref as R
from tokenpacker_amd import MainGradAdamW, TokenPacker, _capi

pytestmark = pytest.mark.gpu
DEV, D, B, S = "cuda", 256, 2, 2
NUMELS = (1, 3, R.CHUNK, R.CHUNK + 1, 2 * R.CHUNK + 5)
assert R.CHUNK == 4096
VECTOR = NUMELS.index(R.CHUNK)          # the one tensor whose length lets it take the 16-byte path


def bits(t):
    return t.detach().contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


class Run:
    """fp32 parameters with their gradients and moments, each in its own allocation; tensor `shifted` (or none) sits 4 bytes into
    its allocations: off the 16-byte grid, onto the scalar path.  `param` of every table entry is NULL."""

    def __init__(self, shifted=None, seed=3):
        self.seed = seed
        self.tensors = R.make_tensors(NUMELS, seed, device=DEV, param_dtype=torch.float32)
        for i, t in enumerate(self.tensors):
            off = 1 if i == shifted else 0
            for k in ("p", "m", "v"):
                buf = torch.zeros(t[k].numel() + off, dtype=torch.float32, device=DEV)
                buf[off:].copy_(t[k])
                t[k] = buf[off:]
            t["g"] = torch.zeros(t["p"].numel() + off, dtype=torch.float32, device=DEV)[off:]
            assert all((t[k].data_ptr() % 16 == 0) == (off == 0) for k in ("p", "m", "v", "g"))
        self.table = (_capi.tp_optim_tensor * len(NUMELS))()
        for e, t in zip(self.table, self.tensors):
            e.param = None
            e.master, e.grad, e.exp_avg, e.exp_avg_sq = (t[k].data_ptr() for k in ("p", "g", "m", "v"))
            e.numel, e.lr, e.weight_decay = t["p"].numel(), t["lr"], t["wd"]
        nbytes = _capi.load_library().tp_optim_workspace_bytes(self.table, len(NUMELS))
        assert nbytes > 0, _capi.last_error()
        self.workspace = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
        self.state = torch.zeros(_capi.TP_OPTIM_STATE_BYTES // 4, dtype=torch.int32, device=DEV)

    def set_grads(self, step):
        for t, g in zip(self.tensors, R.make_grads(NUMELS, self.seed, step, "above", device=DEV)):
            t["g"].copy_(g)

    def snapshot(self):
        return [{k: (t[k].clone() if isinstance(t[k], torch.Tensor) else t[k]) for k in ("p", "m", "v", "g", "lr", "wd")}
                for t in self.tensors]

    def step(self, hyper, zero=True):
        h = _capi.tp_optim_hyper(hyper.beta1, hyper.beta2, hyper.eps, hyper.max_grad_norm, _capi.TP_F32,
                                 _capi.TP_OPTIM_ZERO_GRAD if zero else 0)
        rc = _capi.load_library().tp_optim_step(self.table, len(NUMELS), ctypes.byref(h), None, self.state.data_ptr(),
                                                self.workspace.data_ptr(), self.workspace.numel(),
                                                torch.cuda.current_stream().cuda_stream)
        _capi.check(rc, "tp_optim_step")
        torch.cuda.synchronize()
        words = self.state.cpu()
        f = words.view(torch.float32)
        return {"norm": float(f[0].double()), "coef": float(f[1]), "found_inf": int(words[2]), "step": int(words[3]),
                "skipped": int(words[4])}


def check_step(tensors, before, got, hyper, step_before, what):
    """One applied step against the fp64 reference evaluated from the snapshot `before`, within optim_ref's bounds."""
    ref = R.step_ref(before, hyper, step_before)
    assert got["found_inf"] == 0 == ref["found_inf"] and got["step"] == ref["step"] == step_before + 1, (what, got)
    assert abs(got["norm"] ** 2 - ref["norm"] ** 2) <= R.SUMSQ_REL * ref["norm"] ** 2, what
    assert got["coef"] == pytest.approx(ref["coef"], rel=2 * R.COEF_REL), what
    worst = {}
    for i, (t, (p2, m2, v2), (ep, em, ev)) in enumerate(zip(tensors, ref["out"], R.bounds(before, hyper, step_before, ref))):
        for name, a, b, e in (("parameter", t["p"], p2, ep), ("exp_avg", t["m"], m2, em), ("exp_avg_sq", t["v"], v2, ev)):
            r = R.worst_ratio(a.flatten(), b, e)
            worst[name] = max(worst.get(name, 0.0), r)
            assert r <= 1.0, f"{what} tensor {i} ({a.numel()} elements) {name}: |got - ref| / bound = {r:.3f}"
    print(f"{what}: worst |got - ref| / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


@pytest.mark.parametrize("shifted", [None, VECTOR], ids=["aligned", "one_tensor_4_bytes_off"])
def test_three_steps_on_fp32_parameters_match_the_reference(shifted):
    hyper = R.Hyper(0.9, 0.999, 1e-8, 1.0)
    run = Run(shifted)
    for step in range(3):
        run.set_grads(step)
        before = run.snapshot()
        got = run.step(hyper)
        check_step(run.tensors, before, got, hyper, step, f"fp32 parameters, step {step}")
        assert got["coef"] < 1.0 and got["skipped"] == 0
        for t, b in zip(run.tensors, before):
            assert not bool(t["g"].any()), "TP_OPTIM_ZERO_GRAD: the gradients are zeroed behind the update"
            assert not torch.equal(bits(t["p"]), bits(b["p"])), "the parameter itself is updated"


def test_the_scalar_and_the_vector_path_give_the_same_bits():
    hyper = R.Hyper(0.9, 0.999, 1e-8, 1.0)
    a, b = Run(None), Run(VECTOR)
    for step in range(2):
        for r in (a, b):
            r.set_grads(step)
        ga, gb = a.step(hyper), b.step(hyper)
        assert ga == gb
        for ta, tb in zip(a.tensors, b.tensors):
            for k in ("p", "m", "v"):
                assert torch.equal(bits(ta[k]), bits(tb[k])), (step, k, ta["p"].numel())


@pytest.mark.parametrize("zero", [True, False], ids=["zero_grad", "keep_grad"])
@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("shifted", [None, VECTOR], ids=["vector_path", "scalar_path"])
def test_a_non_finite_norm_leaves_every_bit_and_is_counted(shifted, bad, zero):
    hyper = R.Hyper(0.9, 0.999, 1e-8, 1.0)
    run = Run(shifted)
    run.set_grads(0)
    before = run.snapshot()
    got = run.step(hyper, zero)
    check_step(run.tensors, before, got, hyper, 0, "the applied step")
    for t, b in zip(run.tensors, before):                           # zeroing (or not) on an applied step
        assert not bool(t["g"].any()) if zero else torch.equal(bits(t["g"]), bits(b["g"]))
    run.set_grads(1)
    run.tensors[VECTOR]["g"][-1] = bad
    before = run.snapshot()
    got = run.step(hyper, zero)
    assert (got["found_inf"], got["step"], got["skipped"], got["coef"]) == (1, 1, 1, 0.0), got
    for t, b in zip(run.tensors, before):
        for k in ("p", "m", "v"):
            assert torch.equal(bits(t[k]), bits(b[k])), f"{k} of a skipped step changed"
        assert not bool(t["g"].any()) if zero else torch.equal(bits(t["g"]), bits(b["g"]))      # ... and on a skipped one
    run.set_grads(2)                                                # the next clean step carries the bias correction of step 2
    before = run.snapshot()
    got = run.step(hyper, zero)
    assert (got["found_inf"], got["step"], got["skipped"]) == (0, 2, 1), got
    check_step(run.tensors, before, got, hyper, 1, "the step after the skipped one")


# ---- MainGradAdamW on an fp32 module ---------------------------------------------------------------------------------------------
def make_module(dtype):
    """The same initial values in both dtypes: every one representable in bf16."""
    torch.manual_seed(0)
    m = TokenPacker(hidden_size=D, scale_factor=S).to(device=DEV, dtype=torch.bfloat16)
    m = m.to(dtype)
    m.use_main_grad = True
    m.init_main_grads()
    return m


def groups_of(m):
    named = list(m.named_parameters())
    return [{"params": [p for n, p in named if p.dim() >= 2], "weight_decay": 0.1},
            {"params": [p for n, p in named if p.dim() < 2], "weight_decay": 0.0}]


def make_inputs():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, 576, 1024, generator=g).to(device=DEV, dtype=torch.bfloat16)
    xm = torch.randn(B, 576, 4096, generator=g).to(device=DEV, dtype=torch.bfloat16)
    w = torch.randn(B, (24 // S) ** 2, D, generator=g).to(device=DEV)
    return x, xm, w


def backward(m, inputs):
    x, xm, w = inputs
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y = m((x, xm))
    (y.float() * w).sum().backward()
    return y.detach()


def test_the_master_is_the_parameter_and_the_state_dict_keeps_torchs_layout():
    m, inputs = make_module(torch.float32), make_inputs()
    opt = MainGradAdamW(groups_of(m), lr=1e-3, module=m)
    assert len(opt.tensor_names) == 23
    for p in m.parameters():
        assert opt.state[p]["master"].data_ptr() == p.data_ptr() and opt.state[p]["master"].dtype == torch.float32
    hyper = R.Hyper(0.9, 0.999, 1e-8, 1.0)
    for step in range(2):
        backward(m, inputs)
        assert m.last_pack_path == "raw_f32" and all(p.grad is None for p in m.parameters())
        before = [{"p": p.detach().flatten().clone(), "m": opt.state[p]["exp_avg"].flatten().clone(),
                   "v": opt.state[p]["exp_avg_sq"].flatten().clone(), "g": p.main_grad.flatten().clone(), "lr": g["lr"],
                   "wd": g["weight_decay"], "param": p} for g in opt.param_groups for p in g["params"]]
        opt.step()
        torch.cuda.synchronize()
        after = [{"p": t["param"].detach(), "m": opt.state[t["param"]]["exp_avg"], "v": opt.state[t["param"]]["exp_avg_sq"]} for t in before]
        got = {"norm": float(opt.grad_norm.double()), "coef": float(opt.clip_coef), "found_inf": int(opt.found_inf),
               "step": int(opt.steps_applied), "skipped": int(opt.steps_skipped)}
        check_step(after, before, got, hyper, step, f"the fp32 module, step {step}")
        assert all(not bool(p.main_grad.any()) for p in m.parameters())
    saved = opt.state_dict()
    assert set(saved["state"][0]) == {"step", "exp_avg", "exp_avg_sq"} and saved["main_grad_adamw"]["steps_applied"] == 2
    # the round trip: a second optimizer over the same parameters continues from the saved moments and counters
    opt2 = MainGradAdamW(groups_of(m), lr=5.0, module=m)
    opt2.load_state_dict(saved)
    assert int(opt2.steps_applied) == 2 and opt2.param_groups[0]["lr"] == 1e-3
    for p in m.parameters():
        assert torch.equal(opt2.state[p]["exp_avg_sq"], opt.state[p]["exp_avg_sq"]) and opt2.state[p]["master"].data_ptr() == p.data_ptr()


def test_a_torch_adamw_state_dict_loads_onto_fp32_parameters():
    """As for 16-bit parameters: the moments and the step count are taken; the masters are the parameters, as they are."""
    g = torch.Generator().manual_seed(5)
    ours = [torch.nn.Parameter((0.02 * torch.randn(s, generator=g)).to(DEV)) for s in ((33,), (8, 16))]
    theirs = [torch.nn.Parameter(p.detach().clone()) for p in ours]
    topt = torch.optim.AdamW(theirs, lr=2e-3, weight_decay=0.05)
    for p in theirs:
        p.grad = torch.randn(p.shape, generator=g).to(DEV)
    topt.step()
    for p in ours:
        p.main_grad = torch.zeros(p.shape, dtype=torch.float32, device=DEV)
    opt = MainGradAdamW(ours, lr=1.0)
    kept = [p.detach().clone() for p in ours]
    opt.load_state_dict(topt.state_dict())
    assert int(opt.steps_applied) == 1 and opt.param_groups[0]["lr"] == 2e-3 and opt.param_groups[0]["weight_decay"] == 0.05
    for p, q, k in zip(ours, theirs, kept):
        assert torch.equal(opt.state[p]["exp_avg"], topt.state[q]["exp_avg"]) and torch.equal(opt.state[p]["exp_avg_sq"], topt.state[q]["exp_avg_sq"])
        assert opt.state[p]["master"].data_ptr() == p.data_ptr() and torch.equal(bits(p), bits(k))
    before = [{"p": p.detach().flatten().clone(), "m": opt.state[p]["exp_avg"].flatten().clone(),
               "v": opt.state[p]["exp_avg_sq"].flatten().clone(), "lr": 2e-3, "wd": 0.05} for p in ours]
    for p, t in zip(ours, before):
        p.main_grad.copy_(torch.randn(p.shape, generator=g))
        t["g"] = p.main_grad.flatten().clone()
    opt.step()
    torch.cuda.synchronize()
    after = [{"p": p.detach(), "m": opt.state[p]["exp_avg"], "v": opt.state[p]["exp_avg_sq"]} for p in ours]
    got = {"norm": float(opt.grad_norm.double()), "coef": float(opt.clip_coef), "found_inf": int(opt.found_inf),
           "step": int(opt.steps_applied), "skipped": int(opt.steps_skipped)}
    check_step(after, before, got, R.Hyper(0.9, 0.999, 1e-8, 1.0), 1, "the step after loading torch's state")


def test_an_fp32_module_under_autocast_stays_in_lockstep_with_its_bf16_twin():
    inputs = make_inputs()
    full, twin = make_module(torch.float32), make_module(torch.bfloat16)
    for (n, p), (_, q) in zip(full.named_parameters(), twin.named_parameters()):
        assert p.dtype == torch.float32 and q.dtype == torch.bfloat16 and torch.equal(p.detach(), q.detach().float()), n
    opt_full = MainGradAdamW(groups_of(full), lr=1e-3, module=full)
    opt_twin = MainGradAdamW(groups_of(twin), lr=1e-3, module=twin)
    for step in range(3):
        y_full, y_twin = backward(full, inputs), backward(twin, inputs)
        assert full.last_pack_path == "raw_f32" and twin.last_pack_path == "host_cast"
        assert torch.equal(bits(y_full), bits(y_twin)), f"step {step}: both forwards saw the same rounded weights"
        for (n, p), (_, q) in zip(full.named_parameters(), twin.named_parameters()):
            assert torch.equal(bits(p.main_grad), bits(q.main_grad)), (step, n)
        opt_full.step()
        opt_twin.step()
        torch.cuda.synchronize()
        assert int(opt_full.steps_applied) == int(opt_twin.steps_applied) == step + 1
        assert torch.equal(bits(opt_full.grad_norm.reshape(1)), bits(opt_twin.grad_norm.reshape(1)))
        changed = 0
        for (n, p), (_, q) in zip(full.named_parameters(), twin.named_parameters()):
            assert torch.equal(bits(p), bits(opt_twin.state[q]["master"])), f"step {step}: {n} left the twin's master"
            assert torch.equal(bits(q), bits(p.detach().to(torch.bfloat16))), (step, n)
            changed += int(not torch.equal(p.detach(), q.detach().float()))
        assert changed > 0, "after a step the fp32 parameters are no longer bf16 values: the rounding on load is what keeps the lockstep"
