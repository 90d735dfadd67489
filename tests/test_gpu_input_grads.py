"""Opt-in gradients with respect to the CLIP features (``TokenPacker.input_gradients``; tp_backward_inputs*) on a real MI355X:
dx / dx_multi against autograd on the fp64 oracle (same rounded operands) and against the reference module's own bf16 / fp16
autograd error (tests/golden/input_grad_s*.npz), and the bit-level contracts: the switch changes nothing else, a frozen
projector and one-input-at-a-time runs give the same bits, the parts form equals the concatenated form's column slices, a
power-of-two dy scales the result exactly, two runs are identical, and dx has the downsample's tap structure."""
import glob
import os

import numpy as np
import pytest
import torch

from oracle import tokenpacker_oracle as orc
from tokenpacker_amd import TokenPacker, synth
from tokenpacker_amd.tower import select_features

pytestmark = pytest.mark.gpu

GATE_L2 = 1e-2                     # the parameter gradients' gate (test_gpu_backward.py)


def _rel_l2(got, want) -> float:
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    return float((got - want).norm() / want.norm())


def _module(params, D, s, grid, dtype, switch=True):
    m = TokenPacker(raw_grid=grid, hidden_size=D, scale_factor=s)
    m.load_state_dict(params)
    m = m.to(device="cuda", dtype=dtype).train()
    m.input_gradients = switch
    return m


def _case(seed, D, s, grid, B, dtype):
    N, M = grid * grid, (grid // s) ** 2
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, N, 1024, generator=g).to(dtype)
    xm = torch.randn(B, N, 4096, generator=g).to(dtype)
    w = torch.randn(B, M, D, generator=g).to(dtype)
    return synth.make_params(seed, D), x, xm, w


def _run(m, x, xm, w, want_x=True, want_xm=True, scale=1.0):
    """-> (y, dx, dx_multi) of sum(y * w * scale) with the chosen inputs requiring grad."""
    xx = x.cuda().requires_grad_(want_x)
    mm = xm.cuda().requires_grad_(want_xm)
    y = m((xx, mm))
    (y.float() * (w.cuda().float() * scale)).sum().backward()
    torch.cuda.synchronize()
    return y.detach(), xx.grad, mm.grad


def _oracle(params, x, xm, w, s, grid, dtype):
    """fp64 autograd on the same rounded weights and inputs (CPU)."""
    p = {k: v.to(dtype).double() for k, v in params.items()}
    xx = x.double().requires_grad_(True)
    mm = xm.double().requires_grad_(True)
    y = orc.forward(p, xx, mm, scale_factor=s, raw_grid=grid, compute_dtype=torch.float64, io_dtype=dtype)
    (y * w.double()).sum().backward()
    return xx.grad, mm.grad


CASES = [(2, 24, 2, 256), (3, 24, 3, 256), (4, 24, 2, 256), (2, 16, 3, 256), (2, 8, 7, 256)]


# (the full-size case — the reference's pretraining batch per GPU — once, in bf16, the training dtype of the reference)
@pytest.mark.parametrize("dtype,s,grid,B,D", [(dt, *c) for dt in (torch.bfloat16, torch.float16) for c in CASES]
                         + [(torch.bfloat16, 2, 24, 32, 4096)])
def test_input_gradients_vs_oracle_autograd(dtype, s, grid, B, D):
    params, x, xm, w = _case(300 + 7 * s + grid + B, D, s, grid, B, dtype)
    _, dx, dxm = _run(_module(params, D, s, grid, dtype), x, xm, w)
    assert dx.dtype == dtype and dxm.dtype == dtype and dx.shape == x.shape and dxm.shape == xm.shape
    assert torch.isfinite(dx).all() and torch.isfinite(dxm).all()
    want_dx, want_dxm = _oracle(params, x, xm, w, s, grid, dtype)
    e_dx, e_dxm = _rel_l2(dx, want_dx), _rel_l2(dxm, want_dxm)
    print(f"\n[input-grad] {dtype} s={s} grid={grid} B={B} D={D}: dx rel_l2 {e_dx:.3e}, dx_multi rel_l2 {e_dxm:.3e}")
    assert e_dx <= GATE_L2 and e_dxm <= GATE_L2, (e_dx, e_dxm)


GOLD = sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "input_grad_s*.npz")))


@pytest.mark.parametrize("path", GOLD, ids=[os.path.basename(p)[:-4] for p in GOLD])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_input_gradients_against_the_reference_modules_own_error(path, dtype):
    """The reference module's own bf16 / fp16 autograd dx / dx_multi against fp64 autograd on the same rounded operands
    (tools/make_input_grad_golden.py): ours must be no worse than 1.5 x that, like the parameter gradients' yard-stick."""
    z = np.load(path)
    s, D, B = int(z["scale_factor"]), int(z["hidden_size"]), int(z["batch"])
    params = synth.make_params(int(z["param_seed"]), D)
    x, xm = synth.make_inputs(int(z["input_seed"]), B)
    w = torch.randn(B, (24 // s) ** 2, D, generator=torch.Generator().manual_seed(int(z["input_seed"]) + 1000))
    x, xm = x.to(dtype), xm.to(dtype)
    _, dx, dxm = _run(_module(params, D, s, 24, dtype), x, xm, w)
    want_dx, want_dxm = _oracle(params, x, xm, w, s, 24, dtype)
    ours = np.array([_rel_l2(dx, want_dx), _rel_l2(dxm, want_dxm)])
    tag = "bf16" if dtype == torch.bfloat16 else "fp16"
    ref_own = z[f"ref_{tag}_rel_l2"]
    print(f"\n[input-grad-yardstick] s={s} {tag}: ours dx {ours[0]:.3e} dx_multi {ours[1]:.3e}; "
          f"reference's own dx {ref_own[0]:.3e} dx_multi {ref_own[1]:.3e}")
    assert (ours <= 1.5 * ref_own + 1e-4).all(), (ours, ref_own)


def test_switch_changes_nothing_else():
    """With the switch on and the inputs requiring grad, the forward output and every parameter gradient are bit-identical to
    the default module with detached inputs."""
    dtype, s, grid, B, D = torch.bfloat16, 2, 24, 2, 256
    params, x, xm, w = _case(11, D, s, grid, B, dtype)
    runs = []
    for switch in (False, True):
        m = _module(params, D, s, grid, dtype, switch=switch)
        y, dx, dxm = _run(m, x, xm, w, want_x=switch, want_xm=switch)
        assert (dx is not None) == switch and (dxm is not None) == switch
        runs.append((y, {n: p.grad.clone() for n, p in m.named_parameters()}))
    assert torch.equal(runs[0][0], runs[1][0])
    for n in runs[0][1]:
        assert torch.equal(runs[0][1][n], runs[1][1][n]), n


def test_switch_off_still_refuses():
    m = TokenPacker(hidden_size=256).to(device="cuda", dtype=torch.bfloat16)
    x = torch.zeros(1, 576, 1024, device="cuda", dtype=torch.bfloat16, requires_grad=True)
    xm = torch.zeros(1, 576, 4096, device="cuda", dtype=torch.bfloat16)
    with pytest.raises(NotImplementedError, match="input_gradients"):
        m((x, xm))
    m.input_gradients = True
    m.output_fp32 = True                                       # inference-only options stay refused in training
    with pytest.raises(NotImplementedError, match="inference-only"):
        m((x, xm))


def test_frozen_projector_and_one_input_at_a_time():
    """A frozen projector (no parameter gradients: tp_backward_inputs with grads = NULL) and runs that want only dx or only
    dx_multi return the same bits as the full run; frozen parameters get no .grad, an input not requiring grad none."""
    dtype, s, grid, B, D = torch.bfloat16, 3, 24, 3, 256
    params, x, xm, w = _case(12, D, s, grid, B, dtype)
    _, dx, dxm = _run(_module(params, D, s, grid, dtype), x, xm, w)
    frozen = _module(params, D, s, grid, dtype).requires_grad_(False)
    _, fdx, fdxm = _run(frozen, x, xm, w)
    assert all(p.grad is None for p in frozen.parameters())
    assert torch.equal(fdx, dx) and torch.equal(fdxm, dxm)
    _, odx, odxm = _run(_module(params, D, s, grid, dtype), x, xm, w, want_xm=False)
    assert odxm is None and torch.equal(odx, dx)
    _, odx, odxm = _run(frozen, x, xm, w, want_x=False)
    assert odx is None and torch.equal(odxm, dxm)


def test_parts_form_and_select_features_aliasing():
    """The four sources' gradients are bit-equal to the concatenated form's column slices; with tower.select_features' views
    (x is the last part's hidden state) autograd sums the two contributions into the hidden state, as the oracle does."""
    dtype, s, grid, B, D = torch.bfloat16, 2, 24, 2, 256
    params, x, xm, w = _case(13, D, s, grid, B, dtype)
    m = _module(params, D, s, grid, dtype)
    _, _, dxm = _run(m, x, xm, w, want_x=False)
    parts = [xm[..., 1024 * i:1024 * (i + 1)].contiguous().cuda().requires_grad_(True) for i in range(4)]
    xx = x.cuda().requires_grad_(True)
    (m((xx, tuple(parts))).float() * w.cuda().float()).sum().backward()
    for i in range(4):
        assert torch.equal(parts[i].grad, dxm[..., 1024 * i:1024 * (i + 1)]), i

    g = torch.Generator().manual_seed(14)
    hidden = torch.randn(25, B, 577, 1024, generator=g).to(dtype)
    h = hidden.cuda().requires_grad_(True)
    xs, ps = select_features(list(h.unbind(0)))
    (m((xs, ps)).float() * w.cuda().float()).sum().backward()
    h64 = hidden.double().requires_grad_(True)
    layers = h64.unbind(0)
    p = {k: v.to(dtype).double() for k, v in params.items()}
    y = orc.forward(p, layers[-2][:, 1:], torch.cat([layers[l] for l in (12, 16, 22, 23)], dim=2)[:, 1:],
                    scale_factor=s, compute_dtype=torch.float64, io_dtype=dtype)
    (y * w.double()).sum().backward()
    for l in (12, 16, 22, 23):
        e = _rel_l2(h.grad[l], h64.grad[l])
        print(f"[input-grad] select_features hidden state {l}: rel_l2 {e:.3e}")
        assert e <= GATE_L2, (l, e)
    assert float(h.grad[:, :, 0].abs().max()) == 0.0 and float(h.grad[0].abs().max()) == 0.0   # CLS row / unused layers


@pytest.mark.parametrize("k", [-30, 20])
def test_power_of_two_dy_scales_exactly(k):
    """bf16 model, fp16 gradient chain behind its dynamic scale: dy * 2^k gives dx * 2^k and dx_multi * 2^k bit for bit."""
    dtype, s, grid, B, D = torch.bfloat16, 2, 24, 2, 256
    params, x, xm, w = _case(15, D, s, grid, B, dtype)
    m = _module(params, D, s, grid, dtype)
    _, dx, dxm = _run(m, x, xm, w)
    _, sdx, sdxm = _run(m, x, xm, w, scale=2.0 ** k)
    assert torch.equal(sdx, dx * 2.0 ** k) and torch.equal(sdxm, dxm * 2.0 ** k)


def test_deterministic():
    dtype, s, grid, B, D = torch.float16, 2, 16, 3, 256
    params, x, xm, w = _case(16, D, s, grid, B, dtype)
    m = _module(params, D, s, grid, dtype)
    a, b = _run(m, x, xm, w), _run(m, x, xm, w)
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])


def test_tap_structure():
    """s = 3: dx is exactly 0 off the centre pixel of every 3 x 3 block; s = 2: the four pixels of a block receive the same value."""
    dtype, grid, B, D = torch.bfloat16, 24, 2, 256
    for s in (3, 2):
        params, x, xm, w = _case(17 + s, D, s, grid, B, dtype)
        _, dx, _ = _run(_module(params, D, s, grid, dtype), x, xm, w, want_xm=False)
        blk = dx.reshape(B, grid // s, s, grid // s, s, 1024)
        if s == 3:
            centre = torch.zeros(3, 3, dtype=torch.bool, device=dx.device)
            centre[1, 1] = True
            off = blk.permute(0, 1, 3, 2, 4, 5)[:, :, :, ~centre]
            assert float(off.abs().max()) == 0.0
            assert float(blk[:, :, 1, :, 1].abs().max()) > 0.0
        else:
            ref = blk[:, :, :1, :, :1]
            assert torch.equal(blk, ref.expand_as(blk))
            assert float(ref.abs().max()) > 0.0


def test_empty_batch_connects_the_inputs():
    m = _module(synth.make_params(18, 256), 256, 2, 24, torch.bfloat16)
    x = torch.zeros(0, 576, 1024, device="cuda", dtype=torch.bfloat16, requires_grad=True)
    xm = torch.zeros(0, 576, 4096, device="cuda", dtype=torch.bfloat16, requires_grad=True)
    m((x, xm)).float().sum().backward()
    assert x.grad is not None and x.grad.shape == x.shape and xm.grad is not None and xm.grad.shape == xm.shape
