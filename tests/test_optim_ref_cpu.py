"""tests/optim_ref.py is the yardstick of the GPU optimizer tests; this proves the yardstick without a GPU:
  * its fp64 restatement of one step IS torch.optim.AdamW behind clip_grad_norm_ (5 steps, fp64, per-tensor lr / weight_decay);
  * its error bounds have room: a plain fp32 torch evaluation of the same formulas stays within HALF of them on every element;
  * its error bounds have teeth: each named wrong recipe leaves them on at least one element of the same inputs;
  * its constants are the kernel's."""
import math

import pytest
import torch

from tests import optim_ref as R

STEPS = 5
HYPER = R.Hyper(0.9, 0.999, 1e-8, 1.0)


def _run(kind, dtype, recipe="adamw"):
    """STEPS steps of the reference's inputs; every step starts from the fp64 reference's state rounded to fp32 (what the kernel
    would hold) and is evaluated in `dtype` with `recipe`.  Yields (tensors, step_before, fp64 reference, the evaluation)."""
    tensors = R.make_tensors(R.NUMELS, seed=3)
    for step in range(STEPS):
        for t, g in zip(tensors, R.make_grads(R.NUMELS, 3, step, kind)):
            t["g"] = g
        ref = R.step_ref(tensors, HYPER, step)
        got = ref if (dtype == torch.float64 and recipe == "adamw") else R.step_ref(tensors, HYPER, step, dtype=dtype, recipe=recipe)
        yield tensors, step, ref, got
        for t, (p, m, v) in zip(tensors, ref["out"]):
            t["p"], t["m"], t["v"] = p.float(), m.float(), v.float()


def test_constants_are_the_kernels():
    k = R.kernel_constants()
    assert R.CHUNK == k["kOptimThreads"] * 4 * k["kOptimVecs"] and R.CHAIN == 4 * k["kOptimVecs"]
    assert 2 ** R.TREE_DEPTH == k["kOptimThreads"] and R.TABLE == 32
    assert R.SUMSQ_REL == (R.CHAIN + R.TREE_DEPTH + 2) * 2.0 ** -24
    assert R.SUMSQ_REL <= 64 * 2.0 ** -24                       # (not looser than any fixed-order design needs)
    assert R.NUMELS == (1, 7, 8, R.CHUNK - 1, R.CHUNK, R.CHUNK + 1, 3 * R.CHUNK + 5)


@pytest.mark.parametrize("kind", ["below", "above"])
def test_inputs_cover_what_the_recipes_differ_in(kind):
    tensors = R.make_tensors(R.NUMELS, seed=3)
    assert {t["wd"] for t in tensors} == {0.0, 0.1} and len({t["lr"] for t in tensors}) == 3
    grads = R.make_grads(R.NUMELS, 3, 0, kind)
    norm = math.sqrt(R.sumsq_ref(grads))
    assert (norm < 0.5) if kind == "below" else (norm > 2.0)      # one case is not clipped, the other is
    small = [g for g in grads if 0 < float(g.abs().max()) < 1e-7]
    assert small and any(bool((g == 0).any()) for g in small)   # gradients at ~1e-8 (eps matters) and exact zeros among them


@pytest.mark.parametrize("kind", ["below", "above"])
def test_restatement_is_torch_adamw_behind_clip_grad_norm(kind):
    tensors = R.make_tensors(R.NUMELS, seed=3)
    params = [torch.nn.Parameter(t["p"].double()) for t in tensors]
    opt = torch.optim.AdamW([{"params": [p], "lr": R.f32(t["lr"]), "weight_decay": R.f32(t["wd"])} for p, t in zip(params, tensors)],
                            betas=(HYPER.beta1, HYPER.beta2), eps=HYPER.eps)
    state = [{k: t[k].double() for k in ("p", "m", "v")} | {"lr": t["lr"], "wd": t["wd"]} for t in tensors]
    for step in range(STEPS):
        grads = R.make_grads(R.NUMELS, 3, step, kind)
        for p, t, g in zip(params, state, grads):
            p.grad = g.double()
            t["g"] = g
        total = torch.nn.utils.clip_grad_norm_(params, HYPER.max_grad_norm)
        opt.step()
        ref = R.step_ref(state, HYPER, step)
        assert ref["norm"] == pytest.approx(float(total), rel=1e-13) and ref["found_inf"] == 0 and ref["step"] == step + 1
        assert (ref["coef"] < 1.0) == (kind == "above")
        for p, t, (p2, m2, v2) in zip(params, state, ref["out"]):
            st = opt.state[p]
            # (two fp64 evaluation orders — torch's lerp / addcmul / addcdiv, the restatement's plain formulas — differ by a few
            #  ulps of the largest TERM, which cancellation can leave larger than ulps of the result: 2^-53 = 1.1e-16)
            for a, b in ((p2, p.detach()), (m2, st["exp_avg"]), (v2, st["exp_avg_sq"])):
                torch.testing.assert_close(a, b, rtol=1e-12, atol=1e-14 * float(b.abs().max()))
            t["p"], t["m"], t["v"] = p2, m2, v2                    # (fp64 all the way: no rounding between the steps)


@pytest.mark.parametrize("kind", ["below", "above"])
def test_fp32_evaluation_lies_within_half_the_bound(kind):
    for tensors, step, ref, got in _run(kind, torch.float32):
        assert abs(got["norm"] ** 2 - ref["norm"] ** 2) <= 0.5 * R.SUMSQ_REL * ref["norm"] ** 2
        for i, ((p, m, v), (p2, m2, v2), (ep, em, ev)) in enumerate(zip(got["out"], ref["out"], R.bounds(tensors, HYPER, step, ref))):
            assert p.dtype == torch.float32
            for name, a, b, e in (("master", p, p2, ep), ("exp_avg", m, m2, em), ("exp_avg_sq", v, v2, ev)):
                r = R.worst_ratio(a, b, e)
                assert r <= 0.5, f"step {step} tensor {i} {name}: |fp32 - fp64| / bound = {r:.3f}"


@pytest.mark.parametrize("recipe", R.RECIPES)
def test_wrong_recipes_leave_the_bound(recipe):
    """Over the two cases' five steps, the wrong recipe (evaluated in fp64: nothing but the recipe differs) is outside the bound on
    at least one element of master, exp_avg or exp_avg_sq."""
    worst = 0.0
    for kind in ("below", "above"):
        for tensors, step, ref, got in _run(kind, torch.float64, recipe):
            for (p, m, v), (p2, m2, v2), (ep, em, ev) in zip(got["out"], ref["out"], R.bounds(tensors, HYPER, step, ref)):
                worst = max(worst, R.worst_ratio(p, p2, ep), R.worst_ratio(m, m2, em), R.worst_ratio(v, v2, ev))
    assert worst > 1.0, f"{recipe}: worst |wrong - right| / bound = {worst:.3f}: the bound cannot tell it from AdamW"


def test_non_finite_norm_skips_and_no_clipping_means_coefficient_one():
    tensors = R.make_tensors((7, 8), seed=1)
    for t, g in zip(tensors, R.make_grads((7, 8), 1, 0, "above")):
        t["g"] = g
    for bad in (float("nan"), float("inf")):
        tensors[-1]["g"][-1] = bad
        ref = R.step_ref(tensors, HYPER, 4)
        assert ref["found_inf"] == 1 and ref["step"] == 4
        assert all(torch.equal(p, t["p"].double()) for t, (p, _, _) in zip(tensors, ref["out"]))
    tensors[-1]["g"][-1] = 1.0
    for off in (0.0, -1.0, float("inf")):
        assert R.step_ref(tensors, R.Hyper(max_grad_norm=off), 0)["coef"] == 1.0
    assert R.step_ref(tensors, HYPER, 0)["coef"] < 1.0
    assert torch.equal(R.cast_ref(torch.tensor([1.00390625, 70000.0]), torch.float16), torch.tensor([1.00390625, float("inf")]).half())
