"""Training with an attn_mask (tp_forward_train_masked / tp_backward_masked through the autograd node) on a real MI355X: the masked
training forward is the masked inference forward of the same schedule, an all-zero mask changes no bit, the parameter gradients
and dL/dmask against autograd on the fp64 oracle (same rounded operands) and against the reference module's own bf16 / fp16
autograd error (tests/golden/mask_grad_s*.npz), input gradients with a mask, the four-part x_multi, the exact power-of-two
scaling of the fp16 gradient chain, and determinism."""
import glob
import os

import numpy as np
import pytest
import torch

from oracle import tokenpacker_oracle as orc
from tokenpacker_amd import TokenPacker, synth

pytestmark = pytest.mark.gpu

GATE_L2 = 1e-2                     # the parameter gradients' gate (test_gpu_backward.py)


def _rel_l2(got, want) -> float:
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    return float((got - want).norm() / want.norm())


def _module(params, D, s, dtype, grid=24):
    m = TokenPacker(raw_grid=grid, hidden_size=D, scale_factor=s)
    m.load_state_dict(params)
    return m.to(device="cuda", dtype=dtype).train()


def _masks(s, iseed, B):
    """The masks of tools/make_mask_grad_golden.py (2-D float, 3-D bool, 3-D float) for the case with input seed `iseed`."""
    return synth.make_train_attn_masks(iseed + 1, B, s)


def _leaf(mask, device="cpu", dtype=None):
    """A float mask as a leaf that requires grad (a learnable region bias); a boolean mask as it is."""
    if mask.dtype == torch.bool:
        return mask.to(device)
    return mask.to(device=device, dtype=dtype or mask.dtype).detach().requires_grad_(True)


def _step(m, x, xm, w, mask, inputs=False, scale=1.0):
    """-> (y, {name: grad}, dmask, dx, dx_multi) of sum(y * w * scale); x_multi may be a tuple of four parts."""
    m.zero_grad(set_to_none=True)
    if mask is not None and mask.requires_grad:
        mask.grad = None
    xx = x.cuda().requires_grad_(inputs)
    mm = tuple(t.cuda().requires_grad_(inputs) for t in xm) if isinstance(xm, tuple) else xm.cuda().requires_grad_(inputs)
    y = m((xx, mm), attn_mask=mask)
    (y.float() * (w.cuda().float() * scale)).sum().backward()
    torch.cuda.synchronize()
    grads = {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}
    dxm = tuple(t.grad for t in mm) if isinstance(mm, tuple) else mm.grad
    return y.detach(), grads, (mask.grad if mask is not None and mask.requires_grad else None), xx.grad, dxm


def _oracle(params, x, xm, w, s, dtype, mask, inputs=False, grid=24):
    """fp64 autograd on the same rounded weights and inputs, and the mask the module saw -> (grads, dmask, dx, dx_multi)."""
    pp = {k: v.to(dtype).double().requires_grad_(True) for k, v in params.items()}
    xx, mm = x.double().requires_grad_(inputs), xm.double().requires_grad_(inputs)
    mk = mask.cpu() if mask.dtype == torch.bool else mask.detach().cpu().double().requires_grad_(True)
    y = orc.forward(pp, xx, mm, scale_factor=s, raw_grid=grid, compute_dtype=torch.float64, io_dtype=dtype, attn_mask=mk)
    (y * w.double()).sum().backward()
    return {k: v.grad for k, v in pp.items()}, (None if mask.dtype == torch.bool else mk.grad), xx.grad, mm.grad


def _inputs(seed, B, s, D, dtype, grid=24):
    g = torch.Generator().manual_seed(seed)
    N, M = grid * grid, (grid // s) ** 2
    x = torch.randn(B, N, 1024, generator=g).to(dtype)
    xm = torch.randn(B, N, 4096, generator=g).to(dtype)
    w = torch.randn(B, M, D, generator=g)
    return synth.make_params(seed, D), x, xm, w


@pytest.mark.parametrize("s", [2, 3, 4])
def test_masked_training_forward_is_the_masked_inference_forward(s):
    from tests import gpu_util as gu
    dtype, D, B = torch.bfloat16, 256, 2
    params, x, xm, _ = _inputs(400 + s, B, s, D, dtype)
    m = _module(params, D, s, dtype)
    for kind, mask in _masks(s, 410 + s, B).items():
        if kind == "3d_float":
            continue
        y_tr = m((x.cuda(), xm.cuda()), attn_mask=mask)
        assert y_tr.requires_grad
        with torch.no_grad(), gu.training_schedule_for_inference():
            y_inf = m((x.cuda(), xm.cuda()), attn_mask=mask)
            y_none = m((x.cuda(), xm.cuda()))
        assert torch.equal(y_tr.detach(), y_inf), kind
        assert not torch.equal(y_inf, y_none), kind


def test_all_zero_mask_changes_no_bit():
    """An all-zero float mask (requiring grad): output, the 23 parameter gradients and dx / dx_multi bit-equal to the unmasked
    step, on both dmask layouts."""
    dtype, s, D, B = torch.bfloat16, 2, 256, 2
    params, x, xm, w = _inputs(420, B, s, D, dtype)
    m = _module(params, D, s, dtype)
    m.input_gradients = True
    base = _step(m, x, xm, w, None, inputs=True)
    M = (24 // s) ** 2
    for shape in ((1, s * s), (M * B * 8, 1, s * s)):
        got = _step(m, x, xm, w, torch.zeros(shape, device="cuda", requires_grad=True), inputs=True)
        assert torch.equal(got[0], base[0]), shape
        assert set(got[1]) == set(base[1]) and len(got[1]) == 23
        for k in base[1]:
            assert torch.equal(got[1][k], base[1][k]), (shape, k)
        assert torch.equal(got[3], base[3]) and torch.equal(got[4], base[4]), shape
        assert got[2] is not None and got[2].shape == shape and torch.isfinite(got[2]).all()


GOLD = sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "mask_grad_s*.npz")))


@pytest.mark.parametrize("path", GOLD, ids=[os.path.basename(p)[:-4] for p in GOLD])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("kind", ["2d_float", "3d_bool", "3d_float"])
def test_gradients_with_a_mask_vs_oracle_and_the_reference(path, dtype, kind):
    """Parameter gradients (rel-L2 <= 1e-2 and no worse than 1.5 x the reference's own bf16 / fp16 error, the yard-stick of
    test_gpu_backward.py) and dL/dmask (no worse than the reference's own error) against fp64 autograd with the mask.  The 2-D
    float mask is a CPU fp32 leaf, the 3-D one a device fp32 leaf: the gradient comes back in the leaf's dtype, shape and device."""
    z = np.load(path)
    s, D, B, iseed = int(z["scale_factor"]), int(z["hidden_size"]), int(z["batch"]), int(z["input_seed"])
    names = [str(n) for n in z["names"]]
    params = synth.make_params(int(z["param_seed"]), D)
    x, xm = synth.make_inputs(iseed, B)
    x, xm = x.to(dtype), xm.to(dtype)
    w = torch.randn(B, (24 // s) ** 2, D, generator=torch.Generator().manual_seed(iseed + 1000))
    mask = _leaf(_masks(s, iseed, B)[kind], device="cpu" if kind == "2d_float" else "cuda")
    _, got, dmask, _, _ = _step(_module(params, D, s, dtype), x, xm, w, mask)
    want, want_dmask, _, _ = _oracle(params, x, xm, w, s, dtype, mask)
    errs = synth.grad_errors({k: v.double().cpu() for k, v in got.items()}, want)
    tag = "bf16" if dtype == torch.bfloat16 else "fp16"
    ref_own = dict(zip(names, z[f"ref_{tag}_grad_{kind}"].tolist()))
    line = f"\n[mask-grad] s={s} {tag} {kind}: params worst {max(errs.values()):.3e} (reference's own {max(ref_own.values()):.3e})"
    e = bar = 0.0
    if kind != "3d_bool":
        assert dmask is not None and dmask.dtype == mask.dtype and dmask.shape == mask.shape and dmask.device == mask.device
        e, bar = _rel_l2(dmask, want_dmask), float(z[f"ref_{tag}_dmask_{kind}"])
        line += f"; dmask {e:.3e} (reference's own {bar:.3e})"
    print(line)
    for k in names:
        assert errs[k] <= GATE_L2, (k, errs[k])
        assert errs[k] <= 1.5 * ref_own[k] + 1e-4, (k, errs[k], ref_own[k])
    assert e <= bar, (e, bar)


@pytest.mark.parametrize("s", [3, 4])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("kind", ["2d_float", "3d_bool"])
def test_training_with_inf_at_any_key_position(s, dtype, kind):
    """Masks that do NOT keep key 0 visible (tests/mask_patterns.py: the 2-D float `top_row`, -inf on keys 0 .. s-1 — at s = 4 the
    plain kernel's whole first key group; the 3-D boolean random pattern with its planted rows), on the weights and inputs of
    tests/golden/mask_grad_s*.npz: the training forward is the inference forward of the same schedule bit for bit; parameter
    gradients and dmask at the metrics and gates of test_gradients_with_a_mask_vs_oracle_and_the_reference, input gradients at
    test_input_gradients_with_a_mask's; dmask is exactly 0 where the mask is -inf."""
    from tests import gpu_util as gu, mask_patterns as mp
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", f"mask_grad_s{s}.npz"))
    D, B, iseed = int(z["hidden_size"]), int(z["batch"]), int(z["input_seed"])
    assert (int(z["scale_factor"]), D, B) == (s, 256, 2)
    names = [str(n) for n in z["names"]]
    params = synth.make_params(int(z["param_seed"]), D)
    x, xm = synth.make_inputs(iseed, B)
    x, xm = x.to(dtype), xm.to(dtype)
    w = torch.randn(B, (24 // s) ** 2, D, generator=torch.Generator().manual_seed(iseed + 1000))
    mask = _leaf(mp.top_row_2d(s) if kind == "2d_float" else mp.mode2_bool(24, s, B), device="cuda")
    m = _module(params, D, s, dtype)
    m.input_gradients = True
    y, got, dmask, dx, dxm = _step(m, x, xm, w, mask, inputs=True)
    assert bool(torch.isfinite(y).all()), int((~torch.isfinite(y)).sum())
    with torch.no_grad(), gu.training_schedule_for_inference():
        y_inf = m((x.cuda(), xm.cuda()), attn_mask=mask.detach())
    assert torch.equal(y, y_inf)
    want, want_dmask, want_dx, want_dxm = _oracle(params, x, xm, w, s, dtype, mask, inputs=True)
    errs = synth.grad_errors({k: v.double().cpu() for k, v in got.items()}, want)
    tag = "bf16" if dtype == torch.bfloat16 else "fp16"
    ref_own = dict(zip(names, z[f"ref_{tag}_grad_{kind}"].tolist()))
    e_dx, e_dxm = _rel_l2(dx, want_dx), _rel_l2(dxm, want_dxm)
    line = (f"\n[mask-grad] inf-anywhere s={s} {tag} {kind}: params worst {max(errs.values()):.3e} (reference's own "
            f"{max(ref_own.values()):.3e}); dx {e_dx:.3e}, dx_multi {e_dxm:.3e}")
    e = bar = 0.0
    if kind == "2d_float":
        assert dmask is not None and dmask.dtype == mask.dtype and dmask.shape == mask.shape and dmask.device == mask.device
        assert float(dmask[torch.isinf(mask.detach())].abs().max()) == 0.0              # exactly 0 at the -inf entries
        e, bar = _rel_l2(dmask, want_dmask), float(z[f"ref_{tag}_dmask_{kind}"])
        line += f"; dmask {e:.3e} (reference's own {bar:.3e})"
    print(line)
    for k in names:
        assert errs[k] <= GATE_L2, (k, errs[k])
        assert errs[k] <= 1.5 * ref_own[k] + 1e-4, (k, errs[k], ref_own[k])
    assert e <= bar, (e, bar)
    assert e_dx <= GATE_L2 and e_dxm <= GATE_L2, (e_dx, e_dxm)


def _masked_row_runs(s, dtype, h_star):
    """One head (h_star) of one query fully masked in a 3-D float mask, against the same run with that mask row at zero (every other
    row is zero in both): inference and one training step each -> (geometry, inference pair, training pair)."""
    from tests import gpu_util as gu
    D, B = 256, 2
    G = 24 // s
    M, S2 = G * G, s * s
    b_star, m_star = 1, G + 2                                             # image 1, region (1, 2)
    params, x, xm, w = _inputs(490 + s, B, s, D, dtype)
    m = _module(params, D, s, dtype)
    m.input_gradients = True
    row = (m_star * B + b_star) * 8 + h_star
    runs = []
    for fill in (float("-inf"), 0.0):
        raw = torch.zeros(M * B * 8, 1, S2)
        raw[row] = fill
        with torch.no_grad():
            y_inf = m((x.cuda(), xm.cuda()), attn_mask=raw.cuda())
            sat, rep = m.saturated_stages(clear=True), m.saturation_report()
            with gu.training_schedule_for_inference():
                y_plain = m((x.cuda(), xm.cuda()), attn_mask=raw.cuda())      # (the plain attention kernel at every s)
                sat_plain, rep_plain = m.saturated_stages(clear=True), m.saturation_report()
        step = _step(m, x, xm, w, _leaf(raw, device="cuda"), inputs=True)
        runs.append({"y_inf": y_inf, "sat": sat, "rep": rep, "y_plain": y_plain, "sat_plain": sat_plain, "rep_plain": rep_plain,
                     "step": step, "bwd_sat": m.backward_saturated()})
    return (B, G, M, S2, b_star, m_star, row), runs[0], runs[1]


@pytest.mark.parametrize("s", [2, 3])
def test_fully_masked_row(s):
    """A mode-2 mask that fully masks exactly ONE head of ONE query (every key at -inf), in inference on the plain (s = 2, and the
    training schedule at s = 3) and the absorbed (s = 3) attention kernel and in a training step: every OTHER output row, and every
    gradient slice that depends on other rows only (dx and dx_multi outside that query's region, dmask rows of other queries),
    is bit-identical to the run with that one mask row at zero.  The row itself: what include/tokenpacker.h states, pinned below."""
    dtype, h_star = torch.bfloat16, 5
    (B, G, M, S2, b_star, m_star, row), bad, good = _masked_row_runs(s, dtype, h_star)
    others = torch.ones(B, M, dtype=torch.bool)
    others[b_star, m_star] = False
    for key in ("y_inf", "y_plain"):
        assert torch.equal(bad[key][others.cuda()], good[key][others.cuda()]), key
    yb, _, dmb, dxb, dxmb = bad["step"]
    yg, _, dmg, dxg, dxmg = good["step"]
    assert torch.equal(yb[others.cuda()], yg[others.cuda()])
    assert torch.equal(yb, bad["y_plain"]) and torch.equal(yg, good["y_plain"])       # training forward = inference, that schedule
    tokens = torch.ones(B, 24, 24, dtype=torch.bool)                                   # the tokens of OTHER regions
    i, j = divmod(m_star, G)
    tokens[b_star, i * s:(i + 1) * s, j * s:(j + 1) * s] = False
    tokens = tokens.reshape(B, 576).cuda()
    assert torch.equal(dxb[tokens], dxg[tokens]) and torch.equal(dxmb[tokens], dxmg[tokens])
    rows = torch.ones(M * B * 8, dtype=torch.bool)
    rows[(m_star * B + b_star) * 8:(m_star * B + b_star + 1) * 8] = False
    assert torch.equal(dmb[rows.cuda()], dmg[rows.cuda()])
    assert bool(torch.isfinite(yg).all()) and good["sat"] == () and good["bwd_sat"] == 0
    _pin_fully_masked_row(s, h_star, bad, good, b_star, m_star, row, tokens, rows)


def _pin_fully_masked_row(s, h_star, bad, good, b_star, m_star, row, tokens, rows):
    """What include/tokenpacker.h says comes out for the fully masked row (bf16 model, D = 256) — NOT the reference's NaN row."""
    yb, gb, dmb, dxb, dxmb = bad["step"]
    # the attention's NaN is clamped to -65504 by the fp16 epilogues behind it: the output row is finite in every element ...
    for y in (bad["y_inf"], bad["y_plain"], yb):
        assert bool(torch.isfinite(y[b_star, m_star]).all())
    # ... and the forward's status word names the first stage that then left fp16's range; the scan finds the head's 128 elements of O
    for sat, rep in ((bad["sat"], bad["rep"]), (bad["sat_plain"], bad["rep_plain"])):
        assert sat == ("mlp0_gelu",), sat
        assert rep["O"] == 128 and rep["A2"] > 0 and rep["q0"] == rep["Hkv"] == rep["H2"] == rep["Q1pre"] == rep["Q"] == 0, rep
    assert bad["rep_plain"]["A1"] == 1024 and bad["rep_plain"]["KV"] == 0
    # training: dmask of the row is NaN in every element, the query's other heads are finite; out_proj.weight's gradient is NaN in
    # the head's 128 input columns and nowhere else; every other gradient is finite; the backward's status has bits 0 and 2
    assert bool(torch.isnan(dmb[row]).all()) and int((~torch.isfinite(dmb[~rows])).sum()) == dmb[row].numel()
    assert bool(torch.isfinite(dxb).all()) and bool(torch.isfinite(dxmb).all())
    for k, g in gb.items():
        if k == "clip_attn.out_proj.weight":
            cols = torch.zeros(1024, dtype=torch.bool, device=g.device)
            cols[h_star * 128:(h_star + 1) * 128] = True
            assert bool(torch.isnan(g[:, cols]).all()) and bool(torch.isfinite(g[:, ~cols]).all())
        else:
            assert bool(torch.isfinite(g).all()), k
    assert torch.equal(gb["mlp.2.bias"], good["step"][1]["mlp.2.bias"])                  # (colsum(dy): no activation in it)
    assert bad["bwd_sat"] & 5 == 5, bad["bwd_sat"]
    print(f"\n[masked-row] s={s}: saturated_stages {bad['sat']}, scan {bad['rep']}; plain schedule {bad['rep_plain']}; "
          f"backward status {bad['bwd_sat']:#x}; max |y| of the row {float(yb[b_star, m_star].float().abs().max()):.3g}")


def test_bf16_mask_leaf_gets_a_bf16_gradient():
    """A bf16 2-D leaf on the device: dmask is bf16, its shape, on its device, against the oracle within the reference's own
    bf16 dmask error."""
    z = np.load(GOLD[0])
    s, D, B, iseed = int(z["scale_factor"]), int(z["hidden_size"]), int(z["batch"]), int(z["input_seed"])
    dtype = torch.bfloat16
    params = synth.make_params(int(z["param_seed"]), D)
    x, xm = synth.make_inputs(iseed, B)
    x, xm = x.to(dtype), xm.to(dtype)
    w = torch.randn(B, (24 // s) ** 2, D, generator=torch.Generator().manual_seed(iseed + 1000))
    mask = _leaf(_masks(s, iseed, B)["2d_float"], device="cuda", dtype=dtype)
    _, _, dmask, _, _ = _step(_module(params, D, s, dtype), x, xm, w, mask)
    assert dmask.dtype == dtype and dmask.shape == mask.shape and dmask.device == mask.device
    _, want_dmask, _, _ = _oracle(params, x, xm, w, s, dtype, mask)
    e = _rel_l2(dmask, want_dmask)
    print(f"\n[mask-grad] bf16 leaf s={s}: dmask {e:.3e} (reference's own {float(z['ref_bf16_dmask_2d_float']):.3e})")
    assert e <= float(z["ref_bf16_dmask_2d_float"]), e


def test_bf16_gradient_chain_with_a_mask():
    """A bf16 model with TP_TUNE_BWD_CHAIN = 1 (gradients travel in bf16: the masked kernel's bf16 instantiation) on both dmask
    layouts: parameter gradients within that chain's gate (3e-2, test_gpu_round6.py) and the reference's own bf16 error, dmask
    within the reference's own bf16 error — and not the default fp16 chain's bits."""
    from tokenpacker_amd import _capi
    z = np.load(GOLD[1])
    s, D, B, iseed = int(z["scale_factor"]), int(z["hidden_size"]), int(z["batch"]), int(z["input_seed"])
    dtype, tag = torch.bfloat16, "bf16"
    names = [str(n) for n in z["names"]]
    params = synth.make_params(int(z["param_seed"]), D)
    x, xm = synth.make_inputs(iseed, B)
    x, xm = x.to(dtype), xm.to(dtype)
    w = torch.randn(B, (24 // s) ** 2, D, generator=torch.Generator().manual_seed(iseed + 1000))
    ctx = _capi.TuningContext(bwd_chain=1)
    try:
        for kind in ("2d_float", "3d_float"):
            mask = _leaf(_masks(s, iseed, B)[kind], device="cuda")
            m = _module(params, D, s, dtype)
            _, _, dmask_f16_chain, _, _ = _step(m, x, xm, w, mask)
            m.tuning = ctx
            _, got, dmask, _, _ = _step(m, x, xm, w, mask)
            want, want_dmask, _, _ = _oracle(params, x, xm, w, s, dtype, mask)
            errs = synth.grad_errors({k: v.double().cpu() for k, v in got.items()}, want)
            ref_own = dict(zip(names, z[f"ref_{tag}_grad_{kind}"].tolist()))
            e, bar = _rel_l2(dmask, want_dmask), float(z[f"ref_{tag}_dmask_{kind}"])
            print(f"\n[mask-grad] bf16 chain s={s} {kind}: params worst {max(errs.values()):.3e}, dmask {e:.3e} "
                  f"(reference's own {bar:.3e})")
            assert not torch.equal(dmask, dmask_f16_chain), kind        # (the knob really switched the chain)
            for k in names:
                assert errs[k] <= 3e-2 and errs[k] <= 1.5 * ref_own[k] + 1e-4, (kind, k, errs[k], ref_own[k])
            assert e <= bar, (kind, e, bar)
    finally:
        ctx.close()


def test_learnable_mask_under_no_grad_is_inference():
    """An fp32 device mask that requires grad (a learnable bias, `.to()` hands it through as it is) under no_grad /
    inference_mode: the inference forward, bit-equal to the same mask detached, with `_out` and `output_fp32` accepted."""
    dtype, s, D, B = torch.bfloat16, 2, 256, 2
    params, x, xm, _ = _inputs(480, B, s, D, dtype)
    m = _module(params, D, s, dtype)
    leaf = _leaf(_masks(s, 481, B)["3d_float"], device="cuda")
    assert leaf.dtype == torch.float32 and leaf.is_contiguous()
    for mode in (torch.no_grad, torch.inference_mode):
        with mode():
            want = m((x.cuda(), xm.cuda()), attn_mask=leaf.detach())
            got = m((x.cuda(), xm.cuda()), attn_mask=leaf)
            assert not got.requires_grad and torch.equal(got, want)
            assert m._packed is not None                                 # (the inference path: its weight image is cached)
            out = torch.empty_like(want)
            assert m((x.cuda(), xm.cuda()), attn_mask=leaf, _out=out) is out and torch.equal(out, want)
            m.output_fp32 = True
            want32 = m((x.cuda(), xm.cuda()), attn_mask=leaf.detach())
            got32 = m((x.cuda(), xm.cuda()), attn_mask=leaf)
            m.output_fp32 = False
            assert got32.dtype == torch.float32 and torch.equal(got32, want32)
    assert leaf.grad is None


def test_full_size_hidden_with_a_3d_float_mask():
    """hidden_size 4096 (the reference's LLM width), bf16: parameter gradients and dmask against the fp64 oracle."""
    dtype, s, D, B = torch.bfloat16, 2, 4096, 2
    params, x, xm, w = _inputs(430, B, s, D, dtype)
    mask = _leaf(_masks(s, 431, B)["3d_float"], device="cuda")
    _, got, dmask, _, _ = _step(_module(params, D, s, dtype), x, xm, w, mask)
    want, want_dmask, _, _ = _oracle(params, x, xm, w, s, dtype, mask)
    errs = synth.grad_errors({k: v.double().cpu() for k, v in got.items()}, want)
    e = _rel_l2(dmask, want_dmask)
    print(f"\n[mask-grad] D=4096 bf16 3d_float: params worst {max(errs.values()):.3e}, dmask {e:.3e}")
    assert max(errs.values()) <= GATE_L2 and e <= GATE_L2, (errs, e)


@pytest.mark.parametrize("dtype,s,kind", [(torch.bfloat16, 2, "3d_bool"), (torch.float16, 3, "2d_float")])
def test_input_gradients_with_a_mask(dtype, s, kind):
    D, B = 256, 2
    params, x, xm, w = _inputs(440 + s, B, s, D, dtype)
    mask = _leaf(_masks(s, 441 + s, B)[kind], device="cuda")
    m = _module(params, D, s, dtype)
    m.input_gradients = True
    _, _, _, dx, dxm = _step(m, x, xm, w, mask, inputs=True)
    _, _, want_dx, want_dxm = _oracle(params, x, xm, w, s, dtype, mask, inputs=True)
    e_dx, e_dxm = _rel_l2(dx, want_dx), _rel_l2(dxm, want_dxm)
    print(f"\n[mask-grad] inputs {dtype} s={s} {kind}: dx {e_dx:.3e}, dx_multi {e_dxm:.3e}")
    assert e_dx <= GATE_L2 and e_dxm <= GATE_L2, (e_dx, e_dxm)


def test_parts_with_a_mask_are_the_concatenated_form():
    """x_multi as its four sources + a mask: the inference forward, the training forward, the parameter gradients, dmask and
    the inputs' gradients are those of the concatenated x_multi, bit for bit."""
    dtype, s, D, B = torch.bfloat16, 2, 256, 2
    params, x, xm, w = _inputs(450, B, s, D, dtype)
    parts = tuple(xm[..., 1024 * i:1024 * (i + 1)].contiguous() for i in range(4))
    m = _module(params, D, s, dtype)
    m.input_gradients = True
    for kind, mask in _masks(s, 451, B).items():
        with torch.no_grad():
            y_cat = m((x.cuda(), xm.cuda()), attn_mask=mask)
            y_parts = m((x.cuda(), tuple(t.cuda() for t in parts)), attn_mask=mask)
        assert torch.equal(y_cat, y_parts), kind
        leaf = _leaf(mask, device="cuda")
        a = _step(m, x, xm, w, leaf, inputs=True)
        b = _step(m, x, parts, w, leaf, inputs=True)
        assert torch.equal(a[0], b[0]), kind
        for k in a[1]:
            assert torch.equal(a[1][k], b[1][k]), (kind, k)
        assert (a[2] is None) == (kind == "3d_bool") and (a[2] is None or torch.equal(a[2], b[2])), kind
        assert torch.equal(a[3], b[3]), kind
        for i in range(4):
            assert torch.equal(a[4][..., 1024 * i:1024 * (i + 1)], b[4][i]), (kind, i)


@pytest.mark.parametrize("kind", ["2d_float", "3d_float"])
def test_dmask_scales_exactly_and_is_deterministic(kind):
    """bf16 model, fp16 gradient chain behind its dynamic scale: dy * 2^k gives dmask * 2^k bit for bit; two runs give the same
    bits (mode 1's ordered reduction included); a frozen projector (dmask alone) returns the same dmask."""
    dtype, s, D, B = torch.bfloat16, 2, 256, 3
    params, x, xm, w = _inputs(460, B, s, D, dtype)
    mask = _leaf(_masks(s, 461, B)[kind], device="cuda")
    m = _module(params, D, s, dtype)
    a = _step(m, x, xm, w, mask)
    b = _step(m, x, xm, w, mask)
    assert torch.equal(a[2], b[2]) and all(torch.equal(a[1][k], b[1][k]) for k in a[1])
    for k in (-30, 20):
        sc = _step(m, x, xm, w, mask, scale=2.0 ** k)
        assert torch.equal(sc[2], a[2] * 2.0 ** k), k
    frozen = _module(params, D, s, dtype).requires_grad_(False)
    f = _step(frozen, x, xm, w, mask)
    assert not f[1] and torch.equal(f[2], a[2])


def test_refusals_and_the_empty_batch():
    m = _module(synth.make_params(470, 256), 256, 2, torch.bfloat16)
    x = torch.zeros(1, 576, 1024, device="cuda", dtype=torch.bfloat16)
    xm = torch.zeros(1, 576, 4096, device="cuda", dtype=torch.bfloat16)
    mask = torch.zeros(1, 4, device="cuda", requires_grad=True)
    with pytest.raises(NotImplementedError, match="staged"):
        m((x, xm), attn_mask=mask, _stage_events=[object()] * 11)
    m.output_fp32 = True                                     # inference-only options stay refused in training, mask or not
    with pytest.raises(NotImplementedError, match="inference-only"):
        m((x, xm), attn_mask=mask)
    m.output_fp32 = False
    e = torch.full((1, 4), float("-inf"))
    e[0, 0] = 0.0
    leaf = e.requires_grad_(True)
    m((x[:0], xm[:0]), attn_mask=leaf).float().sum().backward()
    assert leaf.grad is not None and leaf.grad.shape == leaf.shape and float(leaf.grad.abs().max()) == 0.0
