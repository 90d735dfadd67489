#!/usr/bin/env python3
"""Forward + backward of the HD token splice in a TokenPacker-HD training step (mode 'slice', patch_num 9) on one MI355X:
hd.build_multimodal_inputs (one embedding call for the text, one for ',' / '\\n', one tp_hd_assemble launch; backward through
tp_hd_assemble_backward) next to the reference-style loop, oracle/hd_oracle.splice_inputs_embeds with autograd on the same device
and inputs (one embedding call per text piece, torch.cat per image and per sample).  The loop embeds ',' and '\\n' once per
batch where the reference embeds them once per separator, so the comparison favours the loop.

Shapes (M = 144, D = 4096, grids from hd.select_grid on seeded image sizes, vocab 32000 in bf16):
  finetune_hd  16 samples, each <= 2048 rows (model_max_length), the embedding table requires grad (scripts/v1_5/finetune_hd.sh)
  pretrain_hd  32 samples, 32-64 text tokens each (the 'plain' template), the table frozen (scripts/v1_5/pretrain_hd.sh)
Both paths run in one process, alternating, after warm-up; device-synchronised medians over --reps repetitions.

    python tools/hd_train_bench.py [--reps 30] [--out profiles/hd_train_bench.json]
    python tools/hd_train_bench.py --stats SHAPE <kernel_stats.csv> [--out ...]   # add the kernels' time + bytes/s of a
                                                      # rocprofv3 --kernel-trace --stats run of `--shapes SHAPE` alone

The bytes of the backward kernels come from the shapes: the token kernel writes every dtokens row and reads the dout row of every
crop row (2 x n_crops x M x D x 2 B); the plan kernel reads the separator rows and writes fp32 partials.
"""
import argparse
import csv
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import hd_oracle  # noqa: E402  (the loop it is compared with)
from tokenpacker_amd import hd  # noqa: E402

M, D, VOCAB, SEP_ID, RET_ID = 144, 4096, 32000, 29892, 13
HBM_PEAK = 8.0e12                # MI355X HBM3E peak (MI355X_MICROARCH.md)
KERNELS = ("hd_assemble_kernel", "hd_assemble_bwd_plan_kernel", "hd_assemble_bwd_tokens_kernel", "hd_assemble_bwd_sum_kernel")
SHAPES = {"finetune_hd": dict(B=16, train_table=True, seed=901), "pretrain_hd": dict(B=32, train_table=False, seed=902)}


def make_batch(name, dev, dtype=torch.bfloat16):
    cfg = SHAPES[name]
    g = torch.Generator().manual_seed(cfg["seed"])
    ids, hb, wb, n_crops = [], [], [], 0
    for _ in range(cfg["B"]):
        h, w = (int(v) for v in torch.randint(200, 2400, (2,), generator=g))
        gh, gw = hd.select_grid(h, w, patch_num=9)
        hb.append(gh)
        wb.append(gw)
        n_crops += hd.hd_crop_count(gh, gw)
    # finetune: input_ids padded to L_in, and every sample's spliced length L_in - 1 + rows <= 2048
    L_in = 2049 - max(hd.hd_token_rows(a, b, M) for a, b in zip(hb, wb))
    for _ in range(cfg["B"]):
        n_text = (int(torch.randint(32, 65, (1,), generator=g)) if name == "pretrain_hd"
                  else int(torch.randint(max(L_in - 400, 32), L_in, (1,), generator=g)))
        text = torch.randint(100, VOCAB, (n_text,), generator=g)
        pos = int(torch.randint(0, min(n_text, 40) + 1, (1,), generator=g))
        ids.append(torch.cat([text[:pos], torch.tensor([-200]), text[pos:]]))
    L = max(len(t) for t in ids)
    labels = torch.full((len(ids), L), -100, dtype=torch.long)
    mask = torch.zeros(len(ids), L, dtype=torch.bool)
    padded = torch.zeros(len(ids), L, dtype=torch.long)                 # right padding with id 0, masked out
    for b, t in enumerate(ids):
        padded[b, :len(t)] = t
        labels[b, :len(t)] = torch.where(t == -200, torch.tensor(-100), t)
        mask[b, :len(t)] = True
    feats = (torch.randn(n_crops, M, D, generator=g) * 0.5).to(dtype).to(dev).requires_grad_(True)
    emb = torch.nn.Embedding(VOCAB, D).to(device=dev, dtype=dtype).requires_grad_(cfg["train_table"])
    return dict(ids=padded.to(dev), labels=labels.to(dev), mask=mask.to(dev), hb=hb, wb=wb, feats=feats, emb=emb, n_crops=n_crops)


def run_ours(bt, dout):
    _, embeds, _ = hd.build_multimodal_inputs(bt["ids"], bt["emb"], bt["feats"], bt["hb"], bt["wb"], SEP_ID, RET_ID,
                                              labels=bt["labels"], attention_mask=bt["mask"])
    embeds.backward(dout)


def run_loop(bt, dout):
    dev = bt["feats"].device
    embeds = hd_oracle.splice_inputs_embeds(bt["ids"], lambda t: bt["emb"](t.to(dev)), bt["feats"], bt["hb"], bt["wb"],
                                            SEP_ID, RET_ID)
    embeds.backward(dout)


def timed_once(fn, bt, dout):
    bt["feats"].grad = None
    bt["emb"].weight.grad = None
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn(bt, dout)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def bench(shapes, reps, warmup):
    dev = torch.device("cuda")
    res = {}
    for name in shapes:
        bt = make_batch(name, dev)
        with torch.no_grad():
            shape = hd.build_inputs_embeds(bt["ids"], bt["emb"], bt["feats"], bt["hb"], bt["wb"], SEP_ID, RET_ID).shape
        dout = torch.randn(shape, generator=torch.Generator().manual_seed(7)).to(torch.bfloat16).to(dev)
        # the two paths compute the same values and gradients (the loop's table gradient sums in another order)
        run_ours(bt, dout)
        g_ours = bt["feats"].grad.clone()
        bt["feats"].grad = None
        run_loop(bt, dout)
        assert torch.equal(g_ours, bt["feats"].grad), "dL/dfeatures differs between the two paths"
        for _ in range(warmup):
            timed_once(run_ours, bt, dout)
            timed_once(run_loop, bt, dout)
        t_ours, t_loop = [], []
        for _ in range(reps):                                            # alternating
            t_ours.append(timed_once(run_ours, bt, dout))
            t_loop.append(timed_once(run_loop, bt, dout))
        mo, ml = statistics.median(t_ours), statistics.median(t_loop)
        res[name] = dict(samples=len(bt["hb"]), max_len=int(shape[1]), n_crops=bt["n_crops"], grids=[f"{a}x{b}" for a, b in zip(bt["hb"], bt["wb"])],
                         table_requires_grad=SHAPES[name]["train_table"], reps=reps,
                         ours_ms_median=round(mo, 4), loop_ms_median=round(ml, 4), speedup=round(ml / mo, 3),
                         ours_ms_minmax=[round(min(t_ours), 4), round(max(t_ours), 4)],
                         loop_ms_minmax=[round(min(t_loop), 4), round(max(t_loop), 4)],
                         bwd_tokens_kernel_bytes=2 * bt["n_crops"] * M * D * 2)
        print(f"{name}: new path {mo:.3f} ms, loop {ml:.3f} ms (x{ml / mo:.2f}), {bt['n_crops']} crops, max_len {shape[1]}", flush=True)
        del bt, dout
        torch.cuda.empty_cache()
    return res


def add_stats(res, path, shape):
    """Merge the hd_assemble* kernels of a rocprofv3 --stats CSV, taken over a run of `shape` alone (--shapes), into res[shape]."""
    out = {}
    for r in csv.DictReader(open(path)):
        for k in KERNELS:                                   # (templated kernels are listed by their mangled names)
            if k in r["Name"]:
                out[k] = dict(calls=int(r["Calls"]), avg_us=round(float(r["AverageNs"]) / 1e3, 3))
    res[shape]["kernel_stats"] = out
    tok = out.get("hd_assemble_bwd_tokens_kernel")
    if tok:
        bps = res[shape]["bwd_tokens_kernel_bytes"] / (tok["avg_us"] * 1e-6)
        res[shape]["bwd_tokens_achieved_TBps"] = round(bps / 1e12, 3)
        res[shape]["bwd_tokens_share_of_hbm_peak"] = round(bps / HBM_PEAK, 3)     # bound by bytes: no arithmetic
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hd_train_bench.json"))
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES), choices=list(SHAPES))
    ap.add_argument("--stats", nargs=2, metavar=("SHAPE", "CSV"),
                    help="merge a rocprofv3 kernel_stats.csv of a run of SHAPE alone into --out (no timing run)")
    a = ap.parse_args()
    if a.reps < 20 and not a.stats:
        print("note: fewer than 20 repetitions", file=sys.stderr)
    if a.stats:
        res = add_stats(json.load(open(a.out)), a.stats[1], a.stats[0])
    else:
        if not torch.cuda.is_available():
            sys.exit("hd_train_bench needs a GPU")
        res = dict(device=torch.cuda.get_device_name(0), M=M, D=D, vocab=VOCAB, dtype="bf16", **bench(a.shapes, a.reps, a.warmup))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
