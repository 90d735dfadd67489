"""Mint tests/golden/input_grad_s{2,3,4}.npz: the yard-stick for the opt-in input gradients (dx, dx_multi).

For each case the REAL reference module (builder.py, imported by file path through oracle.reference_loader, unmodified) is
differentiated with respect to its inputs and compared with autograd on the fp64 oracle:
  * oracle_vs_ref_fp32      rel-L2 of the oracle's fp64 dx / dx_multi against the reference's fp32 autograd (the oracle's input
                            gradients ARE the reference's, up to fp32 round-off);
  * ref_{bf16,fp16}_rel_l2  the reference's own bf16 / fp16 autograd dx / dx_multi against fp64 autograd on the same rounded
                            operands — the "no worse than the reference" bar of tests/test_gpu_input_grads.py;
  * dx_sub / dxm_sub        the oracle's fp64 dx / dx_multi (fp32 operands), subsampled (token rows tok_dx / tok_dxm, every
                            4th channel of dx_multi) and stored as fp32 — pinned by tests/test_input_grads_cpu.py.
Needs the reference sources (build container only):  python tools/make_input_grad_golden.py
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import reference_loader  # noqa: E402
from oracle import tokenpacker_oracle as orc  # noqa: E402
from tokenpacker_amd import synth  # noqa: E402

OUT_DIR = os.path.join(ROOT, "tests", "golden")
CASES = [("input_grad_s2", 2, 61, 161), ("input_grad_s3", 3, 62, 162), ("input_grad_s4", 4, 63, 163)]
D, B = 256, 1
TOK_DX = np.arange(0, 576, 5)          # every 5th token (5 is prime to 24: every column and row residue — tap and off-tap pixels of s = 2, 3, 4)
TOK_DXM = np.arange(0, 576, 11)


def rel_l2(got: torch.Tensor, want: torch.Tensor) -> float:
    return float((got.double() - want.double()).norm() / want.double().norm())


def weights_for(s: int, iseed: int) -> torch.Tensor:
    return torch.randn(B, (24 // s) ** 2, D, generator=torch.Generator().manual_seed(iseed + 1000))


def oracle_input_grads(params, x, xm, s, w, io_dtype=None):
    """fp64 autograd of sum(y * w) with respect to (x, x_multi) on the given (possibly rounded) operands."""
    xx = x.double().detach().requires_grad_(True)
    mm = xm.double().detach().requires_grad_(True)
    y = orc.forward(params, xx, mm, scale_factor=s, compute_dtype=torch.float64, io_dtype=io_dtype)
    (y * w.double()).sum().backward()
    return xx.grad, mm.grad


def reference_input_grads(ref, params, x, xm, s, w, dtype):
    cfg = type("Cfg", (), {"hidden_size": D, "scale_factor": s})()
    m = ref.build_vision_projector(cfg)
    m.load_state_dict(params, strict=True)
    m = m.to(dtype).train()
    xx = x.to(dtype).detach().requires_grad_(True)
    mm = xm.to(dtype).detach().requires_grad_(True)
    (m((xx, mm)).float() * w).sum().backward()
    return xx.grad.double(), mm.grad.double()


def run_case(ref, name, s, pseed, iseed):
    params = synth.make_params(pseed, D)
    x, xm = synth.make_inputs(iseed, B)
    w = weights_for(s, iseed)
    out = {"scale_factor": np.int64(s), "hidden_size": np.int64(D), "batch": np.int64(B),
           "param_seed": np.int64(pseed), "input_seed": np.int64(iseed), "tok_dx": TOK_DX, "tok_dxm": TOK_DXM}
    dx64, dxm64 = oracle_input_grads(params, x, xm, s, w)
    dx32, dxm32 = reference_input_grads(ref, params, x, xm, s, w, torch.float32)
    out["oracle_vs_ref_fp32"] = np.array([rel_l2(dx64, dx32), rel_l2(dxm64, dxm32)])
    out["dx_sub"] = dx64[:, TOK_DX].float().numpy()
    out["dxm_sub"] = dxm64[:, TOK_DXM, ::4].float().numpy()
    print(f"  {name}: oracle fp64 vs reference fp32 autograd: dx {out['oracle_vs_ref_fp32'][0]:.2e}, "
          f"dx_multi {out['oracle_vs_ref_fp32'][1]:.2e}")
    for tag, dt in (("bf16", torch.bfloat16), ("fp16", torch.float16)):
        p_lp = {k: v.to(dt) for k, v in params.items()}
        g_lp = reference_input_grads(ref, p_lp, x, xm, s, w, dt)
        g64 = oracle_input_grads(p_lp, x.to(dt), xm.to(dt), s, w, io_dtype=dt)
        out[f"ref_{tag}_rel_l2"] = np.array([rel_l2(g_lp[0], g64[0]), rel_l2(g_lp[1], g64[1])])
        print(f"  {name}: reference {tag} autograd vs fp64: dx {out[f'ref_{tag}_rel_l2'][0]:.3e}, "
              f"dx_multi {out[f'ref_{tag}_rel_l2'][1]:.3e}")
    path = os.path.join(OUT_DIR, f"{name}.npz")
    np.savez_compressed(path, **out)
    print(f"{name}: -> {path} ({os.path.getsize(path) / 1e6:.2f} MB)")


def main():
    if not reference_loader.reference_available():
        sys.exit("the reference sources are not available here")
    torch.manual_seed(0)
    ref = reference_loader.load_builder()
    for name, s, pseed, iseed in CASES:
        run_case(ref, name, s, pseed, iseed)


if __name__ == "__main__":
    main()
