"""tp_optim_step on the GPU, through the C ABI on raw torch buffers, against tests/optim_ref.py (whose bounds and teeth
tests/test_optim_ref_cpu.py proves): every step from a snapshot of the state before it — master / exp_avg / exp_avg_sq within the
derived elementwise bounds, param the bit-exact cast of the stored master, the norm within its bound, the coefficient exact from the
stored norm; loss-scale invariance, the overflow guard, reproducibility.  Shapes: the smallest that can go wrong (one element, below
and at a vector, around a chunk, several chunks and a tail; misaligned views for the scalar path; tables of 1, 23 and 40 tensors)."""
import ctypes

import pytest
import torch

from tests import optim_ref as R
from tokenpacker_amd import _capi

pytestmark = pytest.mark.gpu
DEV = "cuda"
DT = {torch.bfloat16: _capi.TP_BF16, torch.float16: _capi.TP_F16}
CYCLE = (1, 7, 8, R.CHUNK - 1, R.CHUNK + 1, 12, 1024, 260)
CASES = {   # name: (numels, elements every buffer's view is offset by, which gradients)
    "one_tensor": ((3 * R.CHUNK + 5,), 0, "above"),
    "sizes_clipped": (R.NUMELS, 0, "above"),
    "sizes_unclipped": (R.NUMELS, 0, "below"),
    "misaligned_views": (R.NUMELS, 1, "above"),
    "table_of_23": (tuple(CYCLE[i % len(CYCLE)] for i in range(23)), 0, "above"),
    "table_of_40": (tuple(CYCLE[i % len(CYCLE)] for i in range(40)), 0, "above"),
}
assert len(CASES["table_of_23"][0]) < R.TABLE < len(CASES["table_of_40"][0])          # one launch's table | two launches


class Run:
    """The buffers of one optimizer: per tensor param (dtype), master, grad, exp_avg, exp_avg_sq (fp32), every one a view `offset`
    elements into its own allocation; the table, the workspace and the zeroed state block."""

    def __init__(self, numels, dtype, offset=0, seed=3):
        self.numels, self.dtype, self.seed = tuple(numels), dtype, seed
        self.tensors = R.make_tensors(numels, seed, device=DEV, param_dtype=dtype)

        def view(src, dt):
            buf = torch.zeros(src.numel() + offset, dtype=dt, device=DEV)
            buf[offset:].copy_(src)
            return buf[offset:]
        for t in self.tensors:
            t["param"] = view(t["p"], dtype)
            for k in ("p", "m", "v"):
                t[k] = view(t[k], torch.float32)
            t["g"] = view(torch.zeros_like(t["p"]), torch.float32)
            assert offset == 0 or t["g"].data_ptr() % 16 != 0
        n = len(self.tensors)
        self.table = (_capi.tp_optim_tensor * n)()
        for e, t in zip(self.table, self.tensors):
            e.param, e.master, e.grad, e.exp_avg, e.exp_avg_sq = (t[k].data_ptr() for k in ("param", "p", "g", "m", "v"))
            e.numel, e.lr, e.weight_decay = t["p"].numel(), t["lr"], t["wd"]
        lib = _capi.load_library()
        nbytes = lib.tp_optim_workspace_bytes(self.table, n)
        assert nbytes >= sum(-(-k // R.CHUNK) for k in numels) * 4 + _capi.TP_OPTIM_STATE_BYTES
        self.workspace = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
        self.state = torch.zeros(_capi.TP_OPTIM_STATE_BYTES // 4, dtype=torch.int32, device=DEV)

    def set_grads(self, step, kind, scale=1.0):
        for t, g in zip(self.tensors, R.make_grads(self.numels, self.seed, step, kind, device=DEV)):
            t["g"].copy_(g * scale)

    def snapshot(self):
        return [{k: (t[k].clone() if isinstance(t[k], torch.Tensor) else t[k]) for k in ("p", "m", "v", "g", "param", "lr", "wd")}
                for t in self.tensors]

    def step(self, hyper: R.Hyper, zero=True, inv_scale=None):
        h = _capi.tp_optim_hyper(hyper.beta1, hyper.beta2, hyper.eps, hyper.max_grad_norm, DT[self.dtype],
                                 _capi.TP_OPTIM_ZERO_GRAD if zero else 0)
        rc = _capi.load_library().tp_optim_step(self.table, len(self.tensors), ctypes.byref(h),
                                                None if inv_scale is None else inv_scale.data_ptr(), self.state.data_ptr(),
                                                self.workspace.data_ptr(), self.workspace.numel(),
                                                torch.cuda.current_stream().cuda_stream)
        _capi.check(rc, "tp_optim_step")
        torch.cuda.synchronize()
        words = self.state.cpu()
        f = words.view(torch.float32)
        return {"norm": f[0].clone(), "coef": f[1].clone(), "found_inf": int(words[2]), "step": int(words[3]), "skipped": int(words[4])}


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def check_step(run, before, got, hyper, step_before, inv_scale=1.0, what=""):
    """One applied step against the reference evaluated from the snapshot `before`."""
    ref = R.step_ref(before, hyper, step_before, inv_scale)
    assert got["found_inf"] == 0 == ref["found_inf"] and got["step"] == ref["step"], (what, got)
    norm = float(got["norm"].double())
    print(f"{what}: norm {norm:.9g} (ref {ref['norm']:.9g}), |norm^2 - ref| / ref = "
          f"{abs(norm ** 2 - ref['norm'] ** 2) / ref['norm'] ** 2 / R.U32:.2f} u of {R.SUMSQ_REL / R.U32:.0f} u")
    assert abs(norm ** 2 - ref["norm"] ** 2) <= R.SUMSQ_REL * ref["norm"] ** 2, what
    # the coefficient: exactly clip_grad_norm_'s fp32 formula on the STORED norm
    want = torch.ones((), dtype=torch.float32)
    if hyper.clips:
        want = torch.clamp(torch.tensor(hyper.max_grad_norm, dtype=torch.float32) / (got["norm"] + torch.tensor(1e-6, dtype=torch.float32)), max=1.0)
    assert torch.equal(bits(got["coef"].reshape(1)), bits(want.reshape(1))), (what, float(got["coef"]), float(want))
    worst = {}
    for i, (t, (p2, m2, v2), (ep, em, ev)) in enumerate(zip(run.tensors, ref["out"], R.bounds(before, hyper, step_before, ref, inv_scale))):
        for name, a, b, e in (("master", t["p"], p2, ep), ("exp_avg", t["m"], m2, em), ("exp_avg_sq", t["v"], v2, ev)):
            r = R.worst_ratio(a, b, e)
            worst[name] = max(worst.get(name, 0.0), r)
            assert r <= 1.0, f"{what} tensor {i} ({t['p'].numel()} elements) {name}: |got - ref| / bound = {r:.3f}"
        assert torch.equal(bits(t["param"]), bits(R.cast_ref(t["p"], run.dtype))), f"{what} tensor {i}: param is not the cast of master"
    print(f"{what}: worst |got - ref| / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    return ref


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("case", list(CASES))
def test_five_steps_match_the_reference(case, dtype):
    numels, offset, kind = CASES[case]
    hyper = R.Hyper(0.9, 0.999, 1e-8, 1.0)
    run = Run(numels, dtype, offset)
    for step in range(5):
        run.set_grads(step, kind)
        before = run.snapshot()
        got = run.step(hyper)
        ref = check_step(run, before, got, hyper, step, what=f"{case} step {step}")
        assert (ref["coef"] < 1.0) == (kind == "above") and got["skipped"] == 0
        for t in run.tensors:
            assert not bool(t["g"].any()), "TP_OPTIM_ZERO_GRAD: the gradients are zeroed behind the update"


@pytest.mark.parametrize("offset", [0, 1], ids=["vector_path", "scalar_path"])
def test_a_loss_scale_changes_no_bit(offset):
    """inv_scale = 2^-7 on gradients multiplied by 2^7: master, exp_avg, exp_avg_sq, param and the norm are those of the unscaled
    run, bit for bit (the scale is taken out first, exactly)."""
    hyper = R.Hyper(0.9, 0.999, 1e-8, 1.0)
    plain, scaled = Run(R.NUMELS, torch.bfloat16, offset), Run(R.NUMELS, torch.bfloat16, offset)
    inv = torch.tensor([2.0 ** -7], dtype=torch.float32, device=DEV)
    for step in range(3):
        plain.set_grads(step, "above")
        scaled.set_grads(step, "above", scale=2.0 ** 7)
        a, b = plain.step(hyper), scaled.step(hyper, inv_scale=inv)
        assert torch.equal(bits(a["norm"].reshape(1)), bits(b["norm"].reshape(1))) and a["step"] == b["step"] == step + 1
        for ta, tb in zip(plain.tensors, scaled.tensors):
            for k in ("p", "m", "v", "param"):
                assert torch.equal(bits(ta[k]), bits(tb[k])), (step, k, ta["p"].numel())


@pytest.mark.parametrize("zero", [True, False], ids=["zero_grad", "keep_grad"])
@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("offset", [0, 1], ids=["vector_path", "scalar_path"])
def test_a_non_finite_gradient_skips_the_step(offset, bad, zero):
    hyper = R.Hyper(0.9, 0.999, 1e-8, 1.0)
    run = Run(R.NUMELS, torch.float16, offset)
    run.set_grads(0, "above")
    assert run.step(hyper, zero)["step"] == 1
    run.set_grads(1, "above")
    run.tensors[-1]["g"][-1] = bad                                  # the last element of the last tensor
    before = run.snapshot()
    got = run.step(hyper, zero)
    assert (got["found_inf"], got["step"], got["skipped"]) == (1, 1, 1), got
    assert not torch.isfinite(got["norm"])
    for t, b in zip(run.tensors, before):
        for k in ("p", "m", "v", "param"):
            assert torch.equal(bits(t[k]), bits(b[k])), f"{k} of a skipped step changed"
        if zero:
            assert not bool(t["g"].any())                           # zeroed on a skipped step too
        else:
            assert torch.equal(bits(t["g"]), bits(b["g"]))
    # the next clean step applies, with the bias correction of step 2 (the skipped one did not count)
    run.set_grads(2, "above")
    before = run.snapshot()
    got = run.step(hyper, zero)
    assert (got["found_inf"], got["step"], got["skipped"]) == (0, 2, 1), got
    check_step(run, before, got, hyper, 1, what="the step after the skipped one")


def test_two_runs_from_the_same_state_give_the_same_bits():
    hyper = R.Hyper(0.9, 0.999, 1e-8, 1.0)
    numels = CASES["table_of_40"][0]
    a, b = Run(numels, torch.bfloat16), Run(numels, torch.bfloat16)
    for step in range(3):
        for r in (a, b):
            r.set_grads(step, "above")
        ga, gb = a.step(hyper), b.step(hyper)
        assert torch.equal(bits(ga["norm"].reshape(1)), bits(gb["norm"].reshape(1)))
        for ta, tb in zip(a.tensors, b.tensors):
            for k in ("p", "m", "v", "param"):
                assert torch.equal(bits(ta[k]), bits(tb[k])), (step, k)


@pytest.mark.parametrize("max_norm", [0.0, -1.0, float("inf")], ids=["zero", "negative", "inf"])
def test_no_clipping_leaves_the_coefficient_at_one(max_norm):
    hyper = R.Hyper(0.9, 0.999, 1e-8, max_norm)
    run = Run(R.NUMELS, torch.bfloat16)
    run.set_grads(0, "above")                                       # a norm of ~17: max_grad_norm = 1 would clip
    before = run.snapshot()
    got = run.step(hyper)
    assert float(got["coef"]) == 1.0 and float(got["norm"]) > 2.0
    check_step(run, before, got, hyper, 0, what=f"max_grad_norm {max_norm}")
