#!/usr/bin/env python3
"""The token splice of the DEFAULT mode (prepare_inputs_labels_for_multimodal with mode != 'slice') on one MI355X, three ways:

  new       splice.build_multimodal_inputs: one tp_splice launch (embeds + labels + mask), backward tp_splice_backward;
  composed  the torch composition the slice path uses (hd._embeds_from_layout + hd.splice_labels_and_mask, restated here for
            the default mode): torch.zeros over the buffer, ONE embedding call for all text + index_copy_, one index_copy_
            for the visual tokens, about ten small torch ops for labels and mask; backward through autograd;
  loop      the reference-style walk per sample, tests/splice_ref.py with autograd, on the device.

Shapes (M = 144, D = 4096, vocab 32000, bf16, one image per sample):
  pretrain  32 samples, 32-64 text tokens, the table frozen          (scripts/v1_5/pretrain.sh)
  finetune  16 samples, <= 2048 rows each, the table trainable       (scripts/v1_5/finetune.sh)
  eval1     1 sample, about 60 text tokens, nothing trainable        (llava/eval/*, serve/cli.py): forward only
  finetune_padrow   finetune padded with id 1, which is not the table's padding_idx 0: thousands of readers of one table row
All paths run in one process, alternating, after warm-up; device-synchronised medians over --reps repetitions of the
forward alone and of forward + backward.

    python tools/splice_bench.py [--reps 30] [--out profiles/splice_bench.json]
    python tools/splice_bench.py --stats SHAPE <kernel_stats.csv> [--out ...]   # add the kernels' time + bytes/s of a
                                   # rocprofv3 --kernel-trace --stats run of `--shapes SHAPE --paths new` alone

Bytes from the shapes: the forward kernel writes every row of inputs_embeds and reads every row that is not padding; the
feature-gradient kernel writes every dfeats row and reads one dout row per visual token; the table-gradient kernel writes the
dense [V, D] table and reads one dout row per text token.
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
from tests import splice_ref  # noqa: E402  (the reference-style loop)
from tokenpacker_amd import splice  # noqa: E402

M, D, VOCAB = 144, 4096, 32000
HBM_PEAK = 8.0e12                # MI355X HBM3E peak (MI355X_MICROARCH.md)
KERNELS = ("splice_kernel", "splice_bwd_map_kernel", "splice_bwd_feats_kernel", "splice_bwd_table_kernel")
SHAPES = {"pretrain": dict(B=32, text=(32, 64), train_table=False, train_feats=True, seed=911),
          "finetune": dict(B=16, text=(1200, 1904), train_table=True, train_feats=True, seed=912),
          "eval1": dict(B=1, text=(60, 60), train_table=False, train_feats=False, seed=913),
          # finetune with a pad id that is NOT the table's padding_idx: every padding position reads one table row, whose
          # gradient the table kernel sums in one workgroup (the worst case of its one-workgroup-per-row design)
          "finetune_padrow": dict(B=16, text=(1200, 1904), train_table=True, train_feats=True, seed=912, pad_id=1)}
PATHS = ("new", "composed", "loop")


def make_batch(name, dev, dtype=torch.bfloat16):
    cfg = SHAPES[name]
    g = torch.Generator().manual_seed(cfg["seed"])
    ids = []
    for _ in range(cfg["B"]):
        n_text = int(torch.randint(cfg["text"][0], cfg["text"][1] + 1, (1,), generator=g))
        text = torch.randint(100, VOCAB, (n_text,), generator=g)
        pos = int(torch.randint(0, min(n_text, 40) + 1, (1,), generator=g))
        ids.append(torch.cat([text[:pos], torch.tensor([-200]), text[pos:]]))
    L = max(len(t) for t in ids)
    labels = torch.full((len(ids), L), -100, dtype=torch.long)
    mask = torch.zeros(len(ids), L, dtype=torch.bool)
    padded = torch.full((len(ids), L), cfg.get("pad_id", 0), dtype=torch.long)   # right padding (id 0 = padding_idx), masked out
    for b, t in enumerate(ids):
        padded[b, :len(t)] = t
        labels[b, :len(t)] = torch.where(t == -200, torch.tensor(-100), t)
        mask[b, :len(t)] = True
    feats = (torch.randn(cfg["B"], M, D, generator=g) * 0.5).to(dtype).to(dev).requires_grad_(cfg["train_feats"])
    emb = torch.nn.Embedding(VOCAB, D, padding_idx=0).to(device=dev, dtype=dtype).requires_grad_(cfg["train_table"])
    return dict(ids=padded.to(dev), labels=labels.to(dev), mask=mask.to(dev), feats=feats, emb=emb,
                trains=cfg["train_feats"] or cfg["train_table"])


def run_new(bt):
    return splice.build_multimodal_inputs(bt["ids"], bt["emb"], bt["feats"], bt["labels"], bt["mask"])


def run_composed(bt):
    """The default mode written the way the slice path is composed (hd._embeds_from_layout + hd.splice_labels_and_mask)."""
    ids, emb, feats, labels, mask = bt["ids"], bt["emb"], bt["feats"], bt["labels"], bt["mask"]
    dev = feats.device
    lay = splice.splice_layout(ids.cpu(), M)                            # the same tiny device -> host copy
    B, L_in, L = lay.batch, lay.in_len, lay.max_len
    kind, pay = torch.from_numpy(lay.kinds()), torch.from_numpy(lay.payloads())
    rows = torch.arange(B * L)
    text_dst, text_src = rows[kind == 0].to(dev), pay[kind == 0].to(dev)
    feat_dst, feat_src = rows[kind == 2].to(dev), pay[kind == 2].to(dev)
    out = torch.zeros(B * L, D, dtype=feats.dtype, device=dev)
    out.index_copy_(0, text_dst, emb(ids.reshape(-1).index_select(0, text_src)))
    out.index_copy_(0, feat_dst, feats.reshape(-1, D).index_select(0, feat_src))
    new_labels = torch.full((B * L,), -100, dtype=labels.dtype, device=dev)
    new_labels[text_dst] = labels.reshape(-1).index_select(0, text_src)
    left = torch.from_numpy(lay.lengths).to(dev).long() - L_in
    src = torch.arange(L, device=dev).unsqueeze(0) - left.unsqueeze(1)
    inside = (src >= 0) & (src < L_in)
    given = mask.gather(1, src.clamp(0, L_in - 1))
    new_mask = torch.where(inside, given, (src < 0).to(mask.dtype))
    return new_mask, out.view(B, L, D), new_labels.view(B, L)


def run_loop(bt):
    return splice_ref.build_multimodal_inputs(bt["ids"], bt["emb"], bt["feats"], bt["labels"], bt["mask"])


RUN = dict(new=run_new, composed=run_composed, loop=run_loop)


def timed_once(fn, bt, dout):
    bt["feats"].grad = None
    bt["emb"].weight.grad = None
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    _, embeds, _ = fn(bt)
    if dout is not None:
        embeds.backward(dout)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def bench(shapes, paths, reps, warmup):
    dev = torch.device("cuda")
    res = {}
    for name in shapes:
        bt = make_batch(name, dev)
        outs = {p: RUN[p](bt) for p in paths}
        shape = outs[paths[0]][1].shape
        for p in paths[1:]:                                              # the paths compute the same three tensors
            assert all(torch.equal(a.detach(), b.detach()) for a, b in zip(outs[paths[0]], outs[p])), p
        del outs
        dout = torch.randn(shape, generator=torch.Generator().manual_seed(7)).to(torch.bfloat16).to(dev) if bt["trains"] else None
        lay = splice.splice_layout(bt["ids"].cpu(), M)
        n_text, n_feat, n_rows = int((lay.kinds() == 0).sum()), int((lay.kinds() == 2).sum()), lay.batch * lay.max_len
        entry = dict(samples=lay.batch, in_len=lay.in_len, max_len=lay.max_len, rows=n_rows, text_rows=n_text, feature_rows=n_feat,
                     table_requires_grad=SHAPES[name]["train_table"], features_require_grad=SHAPES[name]["train_feats"], reps=reps,
                     fwd_kernel_bytes=(n_rows + n_text + n_feat) * D * 2, bwd_feats_kernel_bytes=2 * n_feat * D * 2,
                     bwd_table_kernel_bytes=(VOCAB + n_text) * D * 2)
        for what, d in (("fwd", None), ("fwd_bwd", dout)):
            if what == "fwd_bwd" and dout is None:
                continue
            for _ in range(warmup):
                for p in paths:
                    timed_once(RUN[p], bt, d)
            t = {p: [] for p in paths}
            for _ in range(reps):                                        # alternating
                for p in paths:
                    t[p].append(timed_once(RUN[p], bt, d))
            for p in paths:
                entry[f"{what}_{p}_ms_median"] = round(statistics.median(t[p]), 4)
                entry[f"{what}_{p}_ms_minmax"] = [round(min(t[p]), 4), round(max(t[p]), 4)]
            print(f"{name} {what}: " + ", ".join(f"{p} {entry[f'{what}_{p}_ms_median']:.3f} ms" for p in paths), flush=True)
        res[name] = entry
        del bt, dout
        torch.cuda.empty_cache()
    return res


def add_stats(res, path, shape):
    """Merge the splice kernels of a rocprofv3 --stats CSV, taken over a run of `shape` alone, into res[shape]."""
    out = {}
    for r in csv.DictReader(open(path)):
        for k in KERNELS:                                   # (templated kernels are listed by their mangled names)
            if k in r["Name"]:
                out[k] = dict(calls=int(r["Calls"]), avg_us=round(float(r["AverageNs"]) / 1e3, 3))
    res[shape]["kernel_stats"] = out
    for k, key in (("splice_kernel", "fwd_kernel"), ("splice_bwd_feats_kernel", "bwd_feats_kernel"), ("splice_bwd_table_kernel", "bwd_table_kernel")):
        if k in out:
            bps = res[shape][key + "_bytes"] / (out[k]["avg_us"] * 1e-6)
            res[shape][key + "_achieved_TBps"] = round(bps / 1e12, 3)
            res[shape][key + "_share_of_hbm_peak"] = round(bps / HBM_PEAK, 3)     # bound by bytes: no arithmetic
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "splice_bench.json"))
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES), choices=list(SHAPES))
    ap.add_argument("--paths", nargs="+", default=list(PATHS), choices=list(PATHS))
    ap.add_argument("--stats", nargs=2, metavar=("SHAPE", "CSV"),
                    help="merge a rocprofv3 kernel_stats.csv of a run of SHAPE alone into --out (no timing run)")
    a = ap.parse_args()
    if a.reps < 20 and not a.stats:
        print("note: fewer than 20 repetitions", file=sys.stderr)
    if a.stats:
        res = add_stats(json.load(open(a.out)), a.stats[1], a.stats[0])
    else:
        if not torch.cuda.is_available():
            sys.exit("splice_bench needs a GPU")
        res = dict(device=torch.cuda.get_device_name(0), M=M, D=D, vocab=VOCAB, dtype="bf16", **bench(a.shapes, a.paths, a.reps, a.warmup))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
