#!/usr/bin/env python3
"""The LLM's shifted cross-entropy on given logits on one MI355X, forward + backward, three legs:

  ours          loss.shifted_cross_entropy (tp_shift_ce_forward / tp_shift_ce_backward), the gradient in a fresh buffer;
  ours_inplace  the same with inplace_grad=True (the logits are restored from a copy before every repetition, untimed);
  eager         the reference's op sequence (llava_llama.py:98-106) with PyTorch-ROCm eager ops on the same device:
                logits[..., :-1, :].contiguous(), labels[..., 1:].contiguous(), view, CrossEntropyLoss, autograd.

Shapes (V = 32 000, bf16):
  finetune_all      16 x 2 033 rows (the batch splice_bench.py calls `finetune`), every row labelled
  finetune_quarter  the same, a quarter of the rows labelled (the answers of a conversation)
  captions          32 x 200 rows, every row labelled (stage-1 captions)
The legs alternate in one process after warm-up.  Per leg: device-event times of the forward and of the backward, the
device-synchronised wall time of both together (medians over --reps), and the rise of torch.cuda.max_memory_allocated over
the repetition.  Bytes from the shapes: the forward reads the labelled rows once; the backward reads them once more and writes
every row of the gradient; the floors are those bytes at the 8 TB/s the project's documents use as the HBM peak (for
finetune_all: 0.26 ms forward, 0.52 ms backward).

    python tools/loss_bench.py [--reps 20] [--out profiles/loss_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tokenpacker_amd import loss  # noqa: E402

VOCAB = 32000
HBM_PEAK = 8.0e12                # MI355X HBM3E peak (MI355X_MICROARCH.md)
SHAPES = {"finetune_all": dict(B=16, L=2033, labelled=1.0, seed=921),
          "finetune_quarter": dict(B=16, L=2033, labelled=0.25, seed=922),
          "captions": dict(B=32, L=200, labelled=1.0, seed=923)}
LEGS = ("ours", "ours_inplace", "eager")


def make_batch(name, dev, dtype=torch.bfloat16):
    cfg = SHAPES[name]
    g = torch.Generator(device=dev).manual_seed(cfg["seed"])
    B, L = cfg["B"], cfg["L"]
    master = torch.empty(B, L, VOCAB, dtype=dtype, device=dev)
    for b in range(B):                                                   # (sample by sample: no fp32 copy of the whole batch)
        master[b] = (torch.randn(L, VOCAB, generator=g, device=dev) * 4).to(dtype)
    labels = torch.randint(0, VOCAB, (B, L), generator=g, device=dev)
    if cfg["labelled"] < 1.0:                                            # the labelled rows are the tail of every sample: the answer
        labels[:, :L - int(L * cfg["labelled"])] = -100
    return master, labels


def eager_loss(logits, labels):
    shifted = logits[..., :-1, :].contiguous().view(-1, logits.shape[-1])
    targets = labels[..., 1:].contiguous().view(-1)
    return F.cross_entropy(shifted, targets)


def run_leg(leg, logits, labels):
    """One forward + backward; -> (loss, gradient, forward ms, backward ms) from device events."""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    ev[0].record()
    if leg == "eager":
        out = eager_loss(logits, labels)
    else:
        out = loss.shifted_cross_entropy(logits, labels, inplace_grad=leg == "ours_inplace")
    ev[1].record()
    grad, = torch.autograd.grad(out, logits)
    ev[2].record()
    torch.cuda.synchronize()
    return out.detach(), grad, ev[0].elapsed_time(ev[1]), ev[1].elapsed_time(ev[2])


def timed_once(leg, master, work, labels):
    if leg == "ours_inplace":
        with torch.no_grad():
            work.copy_(master)                                          # the previous repetition left its gradient there
    logits = work if leg == "ours_inplace" else master
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    t0 = time.perf_counter()
    out, grad, fwd_ms, bwd_ms = run_leg(leg, logits, labels)
    wall = (time.perf_counter() - t0) * 1e3
    peak = torch.cuda.max_memory_allocated() - before
    del grad
    return dict(fwd=fwd_ms, bwd=bwd_ms, wall=wall, peak=peak, loss=float(out))


def bench(shapes, legs, reps, warmup):
    dev = torch.device("cuda")
    res = {}
    for name in shapes:
        master, labels = make_batch(name, dev)
        master.requires_grad_(True)
        work = torch.empty_like(master).requires_grad_(True) if "ours_inplace" in legs else None
        B, L, V = master.shape
        n_labelled = int((labels[:, 1:] != -100).sum())
        row_bytes = V * master.element_size()
        fwd_bytes, bwd_bytes = n_labelled * row_bytes, (n_labelled + B * L) * row_bytes
        entry = dict(B=B, L=L, V=V, rows=B * (L - 1), labelled_rows=n_labelled, logits_bytes=B * L * row_bytes, reps=reps,
                     fwd_bytes=fwd_bytes, bwd_bytes=bwd_bytes, fwd_floor_ms=round(fwd_bytes / HBM_PEAK * 1e3, 4),
                     bwd_floor_ms=round(bwd_bytes / HBM_PEAK * 1e3, 4))
        for _ in range(warmup):
            for leg in legs:
                timed_once(leg, master, work, labels)
        t = {leg: [] for leg in legs}
        for _ in range(reps):                                            # alternating
            for leg in legs:
                t[leg].append(timed_once(leg, master, work, labels))
        for leg in legs:
            for key in ("fwd", "bwd", "wall"):
                v = [r[key] for r in t[leg]]
                entry[f"{leg}_{key}_ms_median"] = round(statistics.median(v), 4)
                entry[f"{leg}_{key}_ms_minmax"] = [round(min(v), 4), round(max(v), 4)]
            entry[f"{leg}_peak_memory_rise_bytes"] = max(r["peak"] for r in t[leg])
            entry[f"{leg}_loss"] = t[leg][-1]["loss"]
        for leg in legs:
            if leg != "eager":                                          # bound by bytes: about ten fp32 operations per element
                entry[f"{leg}_fwd_fraction_of_floor"] = round(entry["fwd_floor_ms"] / entry[f"{leg}_fwd_ms_median"], 3)
                entry[f"{leg}_bwd_fraction_of_floor"] = round(entry["bwd_floor_ms"] / entry[f"{leg}_bwd_ms_median"], 3)
        print(f"{name}: floors fwd {entry['fwd_floor_ms']:.3f} / bwd {entry['bwd_floor_ms']:.3f} ms; " + "; ".join(
            f"{leg} fwd {entry[f'{leg}_fwd_ms_median']:.3f} bwd {entry[f'{leg}_bwd_ms_median']:.3f} wall {entry[f'{leg}_wall_ms_median']:.3f} ms, "
            f"peak +{entry[f'{leg}_peak_memory_rise_bytes'] / 1e9:.3f} GB, loss {entry[f'{leg}_loss']:.5f}" for leg in legs), flush=True)
        res[name] = entry
        del master, work, labels
        torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loss_bench.json"))
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES), choices=list(SHAPES))
    ap.add_argument("--legs", nargs="+", default=list(LEGS), choices=list(LEGS))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("loss_bench needs a GPU")
    res = dict(device=torch.cuda.get_device_name(0), vocab=VOCAB, dtype="bf16", hbm_peak_bytes_per_s=HBM_PEAK,
               **bench(a.shapes, a.legs, a.reps, a.warmup))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
