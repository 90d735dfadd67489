#!/usr/bin/env python3
"""Training-step timing of the projector on one MI355X: HIP forward+backward (tp_forward_train / tp_backward
through the autograd node) next to the reference's op sequence under PyTorch-ROCm eager autograd
(oracle/reference_ops.py).  Batch 32 is the reference's per-GPU pretraining batch (scripts/v1_5/pretrain.sh:19).
A step is forward + backward + OPTIMIZER STEP (plain SGD on the 23 parameters; `--optimizer none` leaves it out;
`--optimizer main_grad_adamw` is the reference's recipe instead — the backward into fp32 main_grad, then clipping + AdamW on fp32
masters in one call, tokenpacker_amd.optim.MainGradAdamW; the eager side then runs clip_grad_norm_ + torch.optim.AdamW):
the weight update is what makes the next forward re-pack the kernel-side weight image (casts, LayerNorm folds) and
the backward re-transpose the weights, so it belongs inside the timed step.  FLOPs are priced on the work the
backward actually has to do: no input gradient for k/v_proj_1[0] (the CLIP features come from a frozen tower).

    python tools/train_bench.py [--batches 32 256] [--scale-factor 2] [--out gpurun_out/train_bench.json]

--input-grads also times the step with the opt-in gradients with respect to x and x_multi (module.input_gradients, both
inputs requiring grad) and prices the two extra dgrads: dx_multi = dZ1 · [Wk0; Wv0] and dq0 = dQ1pre · Wq1.
--mask also times the step with an attn_mask that is a learnable region bias (a float mask requiring grad: the masked attention
backward and dL/dmask): the 2-D [1, s*s] form (dmask summed over every image, query and head) and the 3-D [(M*B)*8, 1, s*s]
form (every entry written once).
--amp times the step of an fp32 module under torch.autocast(bf16) — fp32 master weights, what the reference's train.py runs outside
DeepSpeed's bf16 engine: the library reads the fp32 parameters in place (module.last_pack_path == "raw_f32"); --host-cast forces the
host-side casts instead (the A/B).  With --optimizer main_grad_adamw the fp32 parameters are their own masters.  HIP only.
--reps R repeats the timing of the step R times in one process and reports every repetition and their median.
--trainable not_kv / mlp times the step of a partially frozen projector (the K/V branches frozen; only mlp.* trainable): the backward
computes the gradients of the parameters that require one and nothing else (tp_backward_sink).  HIP only: no eager baseline.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.reference_ops import eager_forward  # noqa: E402  (baseline only)
from tokenpacker_amd import TokenPacker  # noqa: E402


def flops_fwd(B, s, D):
    N, M, E = 576, (24 // s) ** 2, 1024
    return 2.0 * B * (N * 4096 * E * 2 + N * E * E * 4 + M * E * E * 3 + M * E * D + M * D * D)


def flops_train(B, s, D):
    """forward + weight gradients of every linear + input gradients of every linear EXCEPT the two first K/V layers
    (their input is x_multi, which gets no gradient: 2 x 4.83 GF / image of dgrad that nobody has to compute)."""
    N, E = 576, 1024
    return 3.0 * flops_fwd(B, s, D) - 2.0 * B * (N * 4096 * E * 2)


def flops_input_grads(B, s):
    """the two dgrads the input gradients add: dx_multi [B*N, 4096] over K = 2048 and dq0 [B*M, 1024] over K = 1024"""
    N, M, E = 576, (24 // s) ** 2, 1024
    return 2.0 * B * (N * 2 * E * 4096 + M * E * E)


def timed(fn, iters, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[32, 256])
    ap.add_argument("--scale-factor", type=int, default=2)
    ap.add_argument("--hidden-size", type=int, default=4096)
    ap.add_argument("--out", default="gpurun_out/train_bench.json")
    ap.add_argument("--hip-only", action="store_true", help="skip the eager baseline (profiling runs)")
    ap.add_argument("--optimizer", default="sgd", choices=["sgd", "none", "main_grad_adamw"])
    ap.add_argument("--input-grads", action="store_true", help="also time the step with gradients with respect to x / x_multi")
    ap.add_argument("--mask", action="store_true", help="also time the step with a learnable attn_mask (2-D and 3-D float)")
    ap.add_argument("--trainable", default="all", choices=["all", "not_kv", "mlp"],
                    help="freeze the K/V branches (k_proj_1, v_proj_1, ln_k_1, ln_v_1), or everything but mlp.* (implies --hip-only)")
    ap.add_argument("--amp", action="store_true", help="fp32 parameters under torch.autocast(bf16) (implies --hip-only)")
    ap.add_argument("--host-cast", action="store_true", help="with --amp: force the host-side casts (module.host_cast_weights)")
    ap.add_argument("--reps", type=int, default=1, help="repetitions of the step's timing; the median is reported")
    ap.add_argument("--tune", action="append", default=[], metavar="KEY=VALUE", help="library tuning knob, e.g. BWD_CHAIN=1")
    args = ap.parse_args()
    from tokenpacker_amd import _capi
    for kv in args.tune:
        key, val = kv.split("=")
        _capi.set_tuning(getattr(_capi, "TP_TUNE_" + key.upper()), int(val))
    s, D, dtype = args.scale_factor, args.hidden_size, torch.bfloat16
    args.hip_only = args.hip_only or args.trainable != "all" or args.amp
    import contextlib
    autocast = (lambda: torch.autocast("cuda", dtype=dtype)) if args.amp else contextlib.nullcontext
    frozen = {"all": (), "not_kv": ("k_proj_1.", "v_proj_1.", "ln_k_1.", "ln_v_1."), "mlp": ("",)}[args.trainable]
    results = []
    for B in args.batches:
        torch.manual_seed(0)
        m = TokenPacker(hidden_size=D, scale_factor=s).to(device="cuda", dtype=torch.float32 if args.amp else dtype)
        m.host_cast_weights = args.host_cast
        for name, p in m.named_parameters():
            if name.startswith(frozen) and not (args.trainable == "mlp" and name.startswith("mlp.")):
                p.requires_grad_(False)
        g = torch.Generator(device="cuda").manual_seed(1)
        x = torch.randn(B, 576, 1024, generator=g, device="cuda").to(dtype)
        xm = torch.randn(B, 576, 4096, generator=g, device="cuda").to(dtype)
        w = torch.randn(B, (24 // s) ** 2, D, generator=g, device="cuda").to(dtype)

        import copy
        m_eager = copy.deepcopy(m)                       # each pipeline trains its own copy of the weights
        # (the objective sum(y * w) is linear in y and has no minimum: bf16 parameters round a 1e-7 update away, fp32 parameters
        # take it, and mlp.* then grows without bound — non-finite after a few hundred steps.  --amp steps 1000 x shorter: same work.)
        lr_sgd = 1e-10 if args.amp else 1e-7
        opt = torch.optim.SGD([p for p in m.parameters() if p.requires_grad], lr=lr_sgd) if args.optimizer == "sgd" else None
        opt_e = torch.optim.SGD(m_eager.parameters(), lr=lr_sgd) if args.optimizer == "sgd" else None
        clip_e = None
        if args.optimizer == "main_grad_adamw":
            from tokenpacker_amd import MainGradAdamW
            m.use_main_grad = True
            m.init_main_grads()
            opt = MainGradAdamW(m.parameters(), lr=1e-7, weight_decay=0.0, max_grad_norm=1.0, module=m)
            opt_e = torch.optim.AdamW(m_eager.parameters(), lr=1e-7, weight_decay=0.0)
            clip_e = 1.0

        def step_hip():
            m.zero_grad(set_to_none=True)
            with autocast():
                y = m((x, xm))
            (y * w).sum().backward()
            if opt is not None:
                opt.step()

        def step_eager():
            m_eager.zero_grad(set_to_none=True)
            (eager_forward(m_eager, x, xm) * w).sum().backward()
            if clip_e is not None:
                torch.nn.utils.clip_grad_norm_(m_eager.parameters(), clip_e)
            if opt_e is not None:
                opt_e.step()

        def fwd_hip():
            with torch.no_grad(), autocast():
                m((x, xm))

        x_in, xm_in = x.clone().requires_grad_(True), xm.clone().requires_grad_(True)

        def step_hip_inputs():
            m.zero_grad(set_to_none=True)
            x_in.grad = xm_in.grad = None
            m.input_gradients = True
            (m((x_in, xm_in)) * w).sum().backward()
            m.input_gradients = False
            if opt is not None:
                opt.step()

        S2, M = s * s, (24 // s) ** 2
        masks = {}                                        # (built only when asked for: they draw from the same generator)
        if args.mask:
            masks = {"2d": (0.5 * torch.randn(1, S2, generator=g, device="cuda")).requires_grad_(True),
                     "3d": (0.5 * torch.randn(M * B * 8, 1, S2, generator=g, device="cuda")).requires_grad_(True)}

        def step_hip_mask(mask):
            m.zero_grad(set_to_none=True)
            mask.grad = None
            (m((x, xm), attn_mask=mask) * w).sum().backward()
            if opt is not None:
                opt.step()

        iters = 20 if B <= 64 else 8
        reps = sorted(timed(step_hip, iters) for _ in range(max(args.reps, 1)))
        ms_hip = reps[len(reps) // 2] if len(reps) % 2 else 0.5 * (reps[len(reps) // 2 - 1] + reps[len(reps) // 2])
        ig = {}
        if args.reps > 1:
            ig["hip_fwd_bwd_ms_reps"] = [round(r, 3) for r in reps]
        if args.amp:
            ig.update({"amp": True, "optimizer_in_step": args.optimizer, "pack_path": getattr(m, "last_pack_path", None)})
        if args.mask:
            for kind, mask in masks.items():
                ms_mask = timed(lambda: step_hip_mask(mask), iters)
                ig.update({f"hip_fwd_bwd_mask_{kind}_ms": round(ms_mask, 3), f"mask_{kind}_extra_ms": round(ms_mask - ms_hip, 3)})
                mask.grad = None
        if args.input_grads:
            ms_in = timed(step_hip_inputs, iters)
            ig.update({"hip_fwd_bwd_input_grads_ms": round(ms_in, 3), "input_grads_extra_ms": round(ms_in - ms_hip, 3),
                       "input_grads_extra_gflop": round(flops_input_grads(B, s) / 1e9, 1),
                       "input_grads_extra_tflops": round(flops_input_grads(B, s) / max(ms_in - ms_hip, 1e-6) / 1e9, 1)})
            x_in.grad = xm_in.grad = None
        ms_eager = timed(step_eager, iters) if not args.hip_only else float("nan")
        ms_fwd = timed(fwd_hip, iters)
        # gradient agreement of the two bf16 pipelines (sanity, loose)
        # (ln_k_1.bias and the k third of in_proj_bias have a mathematically zero gradient: round-off in both)
        E = 1024
        if args.hip_only:
            if args.amp:
                ig["weights_finite_after_training"] = all(bool(torch.isfinite(p).all()) for p in m.parameters())
            rec ={"B": B, "trainable": args.trainable, "hip_fwd_bwd_ms": round(ms_hip, 3), "hip_fwd_only_ms": round(ms_fwd, 3), **ig}
            print(json.dumps(rec), flush=True)
            results.append(rec)
            del m, x, xm, w, x_in, xm_in, masks
            torch.cuda.empty_cache()
            continue
        finite = {"hip": all(bool(torch.isfinite(p.float()).all()) for p in m.parameters()),
                  "eager": all(bool(torch.isfinite(p.float()).all()) for p in m_eager.parameters())}
        m.use_main_grad = False                          # (the agreement check reads .grad)
        m_eager.load_state_dict(m.state_dict())          # gradient agreement on identical weights
        step_eager(); ge = {k: p.grad.float().clone() for k, p in m_eager.named_parameters()}
        m.load_state_dict(m_eager.state_dict()) if False else None
        m.zero_grad(set_to_none=True); (m((x, xm)) * w).sum().backward()
        gh = {k: p.grad.float().clone() for k, p in m.named_parameters()}
        for d in (ge, gh):
            d.pop("ln_k_1.bias")
            d["clip_attn.in_proj_bias"] = torch.cat([d["clip_attn.in_proj_bias"][:E], d["clip_attn.in_proj_bias"][2 * E:]])
        agree = max(float((gh[k] - ge[k]).norm() / (ge[k].norm() + 1e-20)) for k in ge)
        rec = {"B": B, "scale_factor": s, "D": D, "dtype": "bf16", "hip_fwd_bwd_ms": round(ms_hip, 3),
               "hip_fwd_only_ms": round(ms_fwd, 3), "eager_rocm_fwd_bwd_ms": round(ms_eager, 3),
               "speedup": round(ms_eager / ms_hip, 3), "images_per_s_train": round(B / ms_hip * 1e3, 1),
               "optimizer_in_step": args.optimizer,
               "train_tflops_algorithmic": round(flops_train(B, s, D) / ms_hip / 1e9, 1),
               "train_gflop_per_image": round(flops_train(1, s, D) / 1e9, 2),
               "weights_finite_after_training": finite, "max_param_grad_rel_l2_vs_eager": agree, "tune": args.tune, **ig}
        print(json.dumps(rec), flush=True)
        results.append(rec)
        del m, m_eager, x, xm, w, x_in, xm_in, masks
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    json.dump(results, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
