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

`--shards W [W ...]`: the per-rank kernel time of the SHARDED step (optim.ShardedMainGradAdamW's two calls, tp_optim_sumsq +
tp_optim_apply with W sums) on rank 0's shard of the 23-tensor table, for every W, on ONE GPU — beside tp_optim_step on the full
table from this build and, with `--baseline-lib path/to/libtokenpacker_hip.so`, from another build (the parent commit's) loaded
into the same process; all arms alternate.  No collective runs: what a reduce-scatter and the two all-gathers cost is NOT in
these numbers.

    python tools/optim_bench.py --shards 1 2 4 8 [--baseline-lib ...] [--out profiles/optim_shard_bench.json]
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


def bench_shards(worlds, reps, warmup, baseline_lib):
    import ctypes
    from tokenpacker_amd import _capi, shard_layout, shard_slices
    lib = _capi.load_library()
    if not _capi.sharded_optim_supported():
        sys.exit("--shards: the library has no tp_optim_sumsq / tp_optim_apply")
    _m, params, grads = make("all")
    numels = [p.numel() for p in params]
    del _m, params
    flat_g = torch.cat([g.flatten() for g in grads])
    del grads
    hyper = _capi.tp_optim_hyper(0.9, 0.999, 1e-8, MAX_NORM, _capi.TP_BF16, 0)
    stream = torch.cuda.current_stream().cuda_stream

    def arrays(n):
        g = torch.Generator(device="cuda").manual_seed(2)
        a = {k: torch.zeros(n, dtype=torch.float32, device="cuda") for k in ("grad", "exp_avg", "exp_avg_sq")}
        a["master"] = torch.randn(n, generator=g, device="cuda") * 0.02
        a["param"] = a["master"].to(torch.bfloat16)
        return a

    def table_of(a, pieces):                       # pieces: [(offset in the arrays, length)]
        tab = (_capi.tp_optim_tensor * len(pieces))()
        for e, (off, n) in zip(tab, pieces):
            e.param = a["param"].data_ptr() + 2 * off
            e.master, e.grad, e.exp_avg, e.exp_avg_sq = (a[k].data_ptr() + 4 * off for k in ("master", "grad", "exp_avg", "exp_avg_sq"))
            e.numel, e.lr, e.weight_decay = n, LR, WD
        return tab

    arms, info = {}, {}
    # the full table: tp_optim_step of this build, and of the baseline build
    lay1 = shard_layout(numels, 1)
    full = arrays(lay1["total"])
    full_tab = table_of(full, list(zip(lay1["offsets"], numels)))
    ws = torch.empty(lib.tp_optim_workspace_bytes(full_tab, len(numels)), dtype=torch.uint8, device="cuda")
    libs = {"step_full": lib}
    if baseline_lib:
        base = ctypes.CDLL(baseline_lib)
        base.tp_optim_step.restype = ctypes.c_int
        base.tp_optim_step.argtypes = lib.tp_optim_step.argtypes
        libs["step_full_baseline"] = base
    for name, which in libs.items():
        state = torch.zeros(16, dtype=torch.int32, device="cuda")

        def step(which=which, state=state):
            rc = which.tp_optim_step(full_tab, len(numels), ctypes.byref(hyper), None, state.data_ptr(), ws.data_ptr(), ws.numel(), stream)
            assert rc == 0, rc

        def refill_full():
            for (off, n), src in zip(zip(lay1["offsets"], numels), flat_g.split(numels)):
                full["grad"][off:off + n].copy_(src)
        arms[name] = (step, refill_full)
        info[name] = dict(elements=sum(numels), entries=len(numels))
    # rank 0's shard for every W (rank 0 of the layout: full chunks of real data for every W here)
    keep = [full, ws]
    for w in worlds:
        lay = shard_layout(numels, w)
        sl = shard_slices(lay, 0)
        a = arrays(lay["shard"])
        tab = table_of(a, [(off, n) for _i, _start, n, off in sl])
        wsw = torch.empty(lib.tp_optim_workspace_bytes(tab, len(sl)), dtype=torch.uint8, device="cuda")
        state = torch.zeros(16, dtype=torch.int32, device="cuda")
        mine, sums = torch.zeros(1, dtype=torch.float64, device="cuda"), torch.zeros(w, dtype=torch.float64, device="cuda")
        src = torch.zeros(lay["shard"], dtype=torch.float32, device="cuda")
        for i, start, n, off in sl:
            src[off:off + n].copy_(flat_g.split(numels)[i][start:start + n])
        src *= w                                   # (a summed gradient; grad_scale = 1 / w takes the average)
        keep += [a, wsw, src]

        def sharded(tab=tab, n=len(sl), wsw=wsw, state=state, mine=mine, sums=sums, w=w):
            rc = lib.tp_optim_sumsq(tab, n, None, 1.0 / w, mine.data_ptr(), wsw.data_ptr(), wsw.numel(), stream)
            assert rc == 0, rc
            sums[:1].copy_(mine)                   # (stands where the all-gather of the W doubles would: the other sums stay 0)
            rc = lib.tp_optim_apply(tab, n, ctypes.byref(hyper), None, 1.0 / w, sums.data_ptr(), w, state.data_ptr(), stream)
            assert rc == 0, rc

        def refill(a=a, src=src):
            a["grad"].copy_(src)
        arms[f"sharded_W{w}"] = (sharded, refill)
        info[f"sharded_W{w}"] = dict(world=w, elements=sum(n for _i, _s, n, _o in sl), shard_elements=lay["shard"], entries=len(sl))
    for _ in range(warmup):
        for fn, refill in arms.values():
            timed_once(fn, refill)
    t = {k: ([], []) for k in arms}
    for _ in range(reps):                          # alternating
        for k, (fn, refill) in arms.items():
            wall, dev = timed_once(fn, refill)
            t[k][0].append(wall)
            t[k][1].append(dev)
    out = {}
    for k in arms:
        e = dict(info[k], reps=reps, device_ms_median=round(statistics.median(t[k][1]), 4),
                 device_ms_minmax=[round(min(t[k][1]), 4), round(max(t[k][1]), 4)], wall_ms_median=round(statistics.median(t[k][0]), 4))
        e["achieved_TBps"] = round(e["elements"] * (BYTES_PER_PARAM - 4) / (e["device_ms_median"] * 1e-3) / 1e12, 3)
        out[k] = e
        print(f"{k}: {e['device_ms_median']:.4f} ms on the device [{e['device_ms_minmax'][0]:.4f} - {e['device_ms_minmax'][1]:.4f}], "
              f"{e['elements']} elements, {e['achieved_TBps']:.2f} TB/s", flush=True)
    out["note"] = ("one GPU, no collective: the per-rank kernel time of tp_optim_sumsq + tp_optim_apply on rank 0's shard (flags 0: no "
                   "zeroing of the gradient, 30 B + 4 B per element) beside tp_optim_step on the full table; the reduce-scatter, the "
                   "all-gathers and any end-to-end multi-GPU gain are not measured")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES), choices=list(SHAPES))
    ap.add_argument("--shards", nargs="+", type=int, default=None, metavar="W",
                    help="time the sharded step's two calls on rank 0's shard for these world sizes instead (see the module docstring)")
    ap.add_argument("--baseline-lib", default=None, help="with --shards: another build of the library whose tp_optim_step is timed too")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "optim_shard_bench.json" if a.shards else "optim_bench.json")
    if not torch.cuda.is_available():
        sys.exit("optim_bench needs a GPU")
    res = dict(device=torch.cuda.get_device_name(0), D=D, dtype="bf16", lr=LR, weight_decay=WD, max_grad_norm=MAX_NORM)
    if a.shards:
        res["shards"] = bench_shards(a.shards, a.reps, a.warmup, a.baseline_lib)
    for shape in ([] if a.shards else a.shapes):
        res[shape] = bench(shape, a.reps, a.warmup)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    print("wrote", a.out)


if __name__ == "__main__":
    main()
