"""Mint tests/golden/mask_grad_s{2,3,4}.npz: the yard-stick for training with an attn_mask (parameter gradients through the masked
attention, and dL/dmask of a float mask that requires grad).

For each case the REAL reference module (builder.py, imported by file path through oracle.reference_loader, unmodified) is called
with a mask and differentiated, for the three masks of synth.make_train_attn_masks — "2d_float" ([1, s*s] additive, requires
grad), "3d_bool" ([(M*B)*8, 1, s*s], no gradient of its own) and "3d_float" ([(M*B)*8, 1, s*s] additive, requires grad) — and
compared with autograd on the fp64 oracle (which differentiates through mask_to_regions):
  * oracle_vs_ref_fp32_<mask>     the 23 parameter gradients' error (synth.grad_errors) of the oracle's fp64 autograd against the
                                  reference's fp32 autograd, then dmask's rel-L2 (0 for the boolean mask) — the oracle's
                                  gradients ARE the reference's, up to fp32 round-off;
  * ref_{bf16,fp16}_grad_<mask>   the reference's own bf16 / fp16 autograd parameter gradients against fp64 autograd on the same
                                  rounded operands (the mask rounded to the module's dtype, as the reference needs it) — the
                                  "no worse than the reference" bar of tests/test_gpu_mask_train.py;
  * ref_{bf16,fp16}_dmask_<mask>  the same for dmask (rel-L2; float masks only);
  * dmask_<mask>                  the oracle's fp64 dmask (fp32 operands) as fp32: all s*s entries of the 2-D mask, every 7th row
                                  of the 3-D one — pinned by tests/test_mask_train_cpu.py.
D = 256, B = 2.  Needs the reference sources (build container only):  python tools/make_mask_grad_golden.py
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
CASES = [("mask_grad_s2", 2, 81, 181), ("mask_grad_s3", 3, 82, 182), ("mask_grad_s4", 4, 83, 183)]
D, B = 256, 2
ROW_STEP = 7                          # rows of the 3-D dmask kept in the golden


def weights_for(s: int, iseed: int) -> torch.Tensor:
    return torch.randn(B, (24 // s) ** 2, D, generator=torch.Generator().manual_seed(iseed + 1000))


def rel_l2(got: torch.Tensor, want: torch.Tensor) -> float:
    return float((got.double() - want.double()).norm() / want.double().norm())


def oracle_grads(params, x, xm, s, w, mask, io_dtype=None):
    """fp64 autograd of sum(y * w) -> ({name: dW}, dmask or None) on the given (possibly rounded) operands."""
    pp = {k: v.double().requires_grad_(True) for k, v in params.items()}
    mm = mask if mask.dtype == torch.bool else mask.double().requires_grad_(True)
    y = orc.forward(pp, x, xm, scale_factor=s, compute_dtype=torch.float64, io_dtype=io_dtype, attn_mask=mm)
    (y * w.double()).sum().backward()
    return {k: v.grad for k, v in pp.items()}, (None if mask.dtype == torch.bool else mm.grad)


def reference_grads(ref, params, x, xm, s, w, mask, dtype):
    cfg = type("Cfg", (), {"hidden_size": D, "scale_factor": s})()
    m = ref.build_vision_projector(cfg)
    m.load_state_dict(params, strict=True)
    m = m.to(dtype).train()
    mm = mask if mask.dtype == torch.bool else mask.to(dtype).detach().requires_grad_(True)
    (m((x.to(dtype), xm.to(dtype)), attn_mask=mm).float() * w).sum().backward()
    return ({k: p.grad.detach().double() for k, p in m.named_parameters()},
            None if mask.dtype == torch.bool else mm.grad.double())


def run_case(ref, name, s, pseed, iseed):
    params = synth.make_params(pseed, D)
    names = list(params.keys())
    x, xm = synth.make_inputs(iseed, B)
    w = weights_for(s, iseed)
    out = {"scale_factor": np.int64(s), "hidden_size": np.int64(D), "batch": np.int64(B), "param_seed": np.int64(pseed),
           "input_seed": np.int64(iseed), "names": np.array(names), "row_step": np.int64(ROW_STEP)}

    def errs(got, want):
        e = synth.grad_errors(got, want)
        return np.array([e[n] for n in names])

    for kind, mask in synth.make_train_attn_masks(iseed + 1, B, s).items():
        g64, dm64 = oracle_grads(params, x, xm, s, w, mask)
        g32, dm32 = reference_grads(ref, params, x, xm, s, w, mask, torch.float32)
        out[f"oracle_vs_ref_fp32_{kind}"] = np.append(errs(g64, g32), 0.0 if dm64 is None else rel_l2(dm64, dm32))
        if dm64 is not None:
            out[f"dmask_{kind}"] = (dm64.reshape(1, -1) if kind.startswith("2d") else dm64.reshape(-1, s * s)[::ROW_STEP]).float().numpy()
        line = f"  {name} {kind}: oracle fp64 vs reference fp32 autograd, worst {out[f'oracle_vs_ref_fp32_{kind}'].max():.2e}"
        for tag, dt in (("bf16", torch.bfloat16), ("fp16", torch.float16)):
            p_lp = {k: v.to(dt) for k, v in params.items()}
            m_lp = mask if mask.dtype == torch.bool else mask.to(dt)
            g_lp, dm_lp = reference_grads(ref, p_lp, x, xm, s, w, m_lp, dt)
            g64_lp, dm64_lp = oracle_grads(p_lp, x.to(dt), xm.to(dt), s, w, m_lp, io_dtype=dt)
            out[f"ref_{tag}_grad_{kind}"] = errs(g_lp, g64_lp)
            line += f"; {tag} params {out[f'ref_{tag}_grad_{kind}'].max():.3e}"
            if dm64_lp is not None:
                out[f"ref_{tag}_dmask_{kind}"] = np.float64(rel_l2(dm_lp, dm64_lp))
                line += f" dmask {float(out[f'ref_{tag}_dmask_{kind}']):.3e}"
        print(line)
    path = os.path.join(OUT_DIR, f"{name}.npz")
    np.savez_compressed(path, **out)
    print(f"{name}: -> {path} ({os.path.getsize(path) / 1e3:.1f} kB)")


def main():
    if not reference_loader.reference_available():
        sys.exit("the reference sources are not available here")
    torch.manual_seed(0)
    ref = reference_loader.load_builder()
    for name, s, pseed, iseed in CASES:
        run_case(ref, name, s, pseed, iseed)


if __name__ == "__main__":
    main()
