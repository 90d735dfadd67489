#!/usr/bin/env python3
"""The optimizer step of stage-1 training (clip to max_grad_norm 1.0 + AdamW on fp32 masters + bf16 write-back + zeroing of the
fp32 main_grad buffers) on one MI355X, two ways:

  fused     tokenpacker_amd.optim.MainGradAdamW: one tp_optim_step call, three launches;
  composed  what a user of use_main_grad would write from torch: clip_grad_norm_ over the main_grads,
            torch.optim.AdamW(fused=True) on fp32 masters whose .grad IS the main_grad, torch._foreach_copy_ into the bf16
            parameters, torch._foreach_zero_ over the main_grads.

Shapes: the projector at D = 4096, bf16 — `all` 23 tensors (36.7 M parameters) and `mlp` (mlp.* only, 21.0 M).  Both paths run
in one process, alternating, after warm-up, on the same refilled gradients; device-synchronised medians over --reps repetitions
(wall time around the call and a device-event pair inside it).  Bytes from the shapes: the fused step moves 34 B per parameter
in the update (grad, master, exp_avg, exp_avg_sq read; master, exp_avg, exp_avg_sq, param, zeroed grad written) and 4 B in the
norm; achieved bytes/s = that over the fused step's device time.

    python tools/optim_bench.py [--reps 30] [--out profiles/optim_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tokenpacker_amd import MainGradAdamW, TokenPacker  # noqa: E402

D = 4096
SHAPES = {"all": ("",), "mlp": ("mlp.",)}
BYTES_PER_PARAM = 34 + 4
LR, WD, MAX_NORM = 1e-4, 0.1, 1.0


def make(shape):
    torch.manual_seed(0)
    m = TokenPacker(hidden_size=D, scale_factor=2).to(device="cuda", dtype=torch.bfloat16)
    for name, p in m.named_parameters():
        p.requires_grad_(name.startswith(SHAPES[shape]))
    m.init_main_grads()
    params = [p for p in m.parameters() if p.requires_grad]
    g = torch.Generator(device="cuda").manual_seed(1)
    grads = [torch.randn(p.shape, generator=g, device="cuda") * 1e-3 for p in params]
    return m, params, grads


def timed_once(fn, refill):
    refill()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    start.record()
    fn()
    stop.record()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, start.elapsed_time(stop)


def bench(shape, reps, warmup):
    m, params, grads = make(shape)
    main_grads = [p.main_grad for p in params]
    fused_opt = MainGradAdamW(params, lr=LR, weight_decay=WD, max_grad_norm=MAX_NORM, module=m)
    # the composed path trains its own copy of the weights: fp32 masters whose .grad is the main_grad buffer itself
    shadow = [p.detach().clone() for p in params]
    masters = [torch.nn.Parameter(p.detach().float()) for p in params]
    for q, mg in zip(masters, main_grads):
        q.grad = mg
    torch_opt = torch.optim.AdamW(masters, lr=LR, weight_decay=WD, fused=True)

    def refill():
        torch._foreach_copy_(main_grads, grads)

    def fused():
        fused_opt.step()

    def composed():
        torch.nn.utils.clip_grad_norm_(masters, MAX_NORM)
        torch_opt.step()
        with torch.no_grad():                                        # (the masters require grad: no autograd record of the cast)
            torch._foreach_copy_(shadow, masters)
            torch._foreach_zero_(main_grads)

    paths = {"fused": fused, "composed": composed}
    for _ in range(warmup):
        for fn in paths.values():
            timed_once(fn, refill)
    t = {k: ([], []) for k in paths}
    for _ in range(reps):                                            # alternating
        for k, fn in paths.items():
            wall, dev = timed_once(fn, refill)
            t[k][0].append(wall)
            t[k][1].append(dev)
    numel = sum(p.numel() for p in params)
    entry = dict(tensors=len(params), parameters=numel, reps=reps, fused_bytes=numel * BYTES_PER_PARAM)
    for k in paths:
        entry[f"{k}_ms_median"] = round(statistics.median(t[k][0]), 4)
        entry[f"{k}_ms_minmax"] = [round(min(t[k][0]), 4), round(max(t[k][0]), 4)]
        entry[f"{k}_device_ms_median"] = round(statistics.median(t[k][1]), 4)
    entry["fused_achieved_TBps"] = round(entry["fused_bytes"] / (entry["fused_device_ms_median"] * 1e-3) / 1e12, 3)
    entry["composed_over_fused"] = round(entry["composed_ms_median"] / entry["fused_ms_median"], 3)
    # the two paths took the same steps from the same start: their bf16 weights agree to a rounding of the last update
    worst = max(float((p.detach().float() - s.float()).abs().max()) for p, s in zip(params, shadow))
    entry["max_abs_weight_difference_fused_vs_composed"] = worst
    entry["fused_steps_applied"], entry["fused_steps_skipped"] = int(fused_opt.steps_applied), int(fused_opt.steps_skipped)
    print(f"{shape}: fused {entry['fused_ms_median']:.3f} ms ({entry['fused_achieved_TBps']:.2f} TB/s on the device), "
          f"composed {entry['composed_ms_median']:.3f} ms", flush=True)
    return entry


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES), choices=list(SHAPES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("optim_bench needs a GPU")
    res = dict(device=torch.cuda.get_device_name(0), D=D, dtype="bf16", lr=LR, weight_decay=WD, max_grad_norm=MAX_NORM)
    for shape in a.shapes:
        res[shape] = bench(shape, a.reps, a.warmup)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    print("wrote", a.out)


if __name__ == "__main__":
    main()
