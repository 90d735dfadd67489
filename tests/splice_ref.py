"""Plain-torch twin of tokenpacker_amd.splice.build_multimodal_inputs.  TEST INFRASTRUCTURE ONLY.

Restates what the reference's ``prepare_inputs_labels_for_multimodal`` (``llava/model/llava_arch.py:100-233``, default flags)
does, sample by sample, in any floating dtype and on any device: text pieces go through ``embed`` one by one, every image
token is replaced by its block of visual tokens, samples are padded on the right, labels get ``IGNORE_INDEX`` under the
visual tokens and the padding, the attention mask gets ``True`` on the left for the rows the images added and ``False`` on the
padding.  Gradients come from torch autograd.  ``tests/test_splice_cpu.py`` pins it to ``tests/golden/splice_plain.npz``
(minted from the unmodified reference by ``tools/make_splice_golden.py``) and, in slice mode, to the HD oracle.
``tools/splice_bench.py`` times it on the device as the reference-style loop.

Also what the two splice test modules share: the golden loader and the project's bound for a fixed-order fp32 sum rounded
once (stated in ``tests/test_gpu_hd_train.py``; ``check_sum`` restates the one there, so no test module imports another)."""
from __future__ import annotations

import hashlib
import os
from typing import Optional, Sequence

import numpy as np
import torch

IGNORE_INDEX = -100
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "splice_plain.npz")
HD_GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "hd_splice_train.npz")
BATCHES = ("ragged", "equal", "one")
INPUTS = ("ids", "feats", "table", "labels", "attention_mask", "dout")
OUTPUTS = ("new_input_embeds", "new_labels", "attention_mask_out", "d_feats", "d_table")


def load_batch(name, path=GOLDEN):
    """One batch of a golden file as torch tensors (its inputs checked against the recorded hash)."""
    z = np.load(path)
    b = {k[len(name) + 1:]: z[k] for k in z.files if k.startswith(name + "_")}
    t = {k: torch.from_numpy(b[k]) for k in INPUTS + OUTPUTS}
    h = hashlib.sha256()
    for k in INPUTS:
        h.update(t[k].contiguous().numpy().tobytes())
    assert h.hexdigest() == str(b["inputs_sha256"])
    if "padding_idx" in b:
        t["padding_idx"] = int(b["padding_idx"])
    else:
        t.update(hb=[int(v) for v in b["h_block"]], wb=[int(v) for v in b["w_block"]], sep_id=int(b["sep_id"]),
                 ret_id=int(b["ret_id"]))
    return t


def half_ulp(x: torch.Tensor, dtype) -> torch.Tensor:
    """1/2 ulp of |x| (float64) in `dtype` (p = 8 significant bits for bf16, 11 for fp16; subnormal floor)."""
    p, tiny = {torch.bfloat16: (8, 2.0 ** -133), torch.float16: (11, 2.0 ** -24)}[dtype]
    _, e = torch.frexp(x.abs())
    return torch.clamp(torch.ldexp(torch.ones_like(x), e - p), min=tiny) / 2


def check_sum(got, S, n, abs_sum, dtype, what):
    """|got - S| <= 1/2 ulp_dtype(max(|S|, |got|)) + (n - 1) 2^-24 sum|t_i|, element by element (float64 CPU tensors)."""
    got = got.detach().double().cpu()
    mag = torch.maximum(S.abs(), got.abs())
    bound = half_ulp(mag, dtype) + (n - 1).clamp(min=0) * 2.0 ** -24 * abs_sum
    err = (got - S).abs()
    print(f"{what}: max|got - S| {float(err.max()):.3e}, worst err/bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all()), f"{what}: {int((err > bound).sum())} elements out of bound"


def image_block(image_features, first: int, mode, hb: int, wb: int, sep_e, ret_e):
    """-> (rows of one image token [n, D], the next feature block).  Default mode: one block as it is.  'slice': the crops
    row-major, ',' between the crops of a grid row, '\\n' after every grid row, then the global view and '\\n'."""
    if mode != "slice":
        return image_features[first], first + 1
    pieces, k = [], first
    for _ in range(hb):
        for w in range(wb):
            pieces.append(image_features[k])
            k += 1
            if w < wb - 1:
                pieces.append(sep_e)
        pieces.append(ret_e)
    if hb * wb > 1:
        pieces += [image_features[k], ret_e]
        k += 1
    return torch.cat(pieces, dim=0), k


def build_multimodal_inputs(input_ids: torch.Tensor, embed, image_features: torch.Tensor, labels: Optional[torch.Tensor] = None,
                            attention_mask: Optional[torch.Tensor] = None, *, mode: Optional[str] = None,
                            h_block: Optional[Sequence[int]] = None, w_block: Optional[Sequence[int]] = None,
                            sep_id: Optional[int] = None, ret_id: Optional[int] = None, image_token_index: int = -200):
    """``(attention_mask, inputs_embeds, labels)`` like the product function.  ``embed``: ids -> embeddings (an nn.Embedding,
    or ``lambda t: table[t]``).  One device round trip per sample (``torch.where``), as in the reference."""
    dev = image_features.device
    sep_e = ret_e = None
    if mode == "slice":
        sep_e = embed(torch.tensor([sep_id], device=input_ids.device))
        ret_e = embed(torch.tensor([ret_id], device=input_ids.device))
    embeds, new_labels, k = [], [], 0
    for b, ids in enumerate(input_ids):
        where = torch.where(ids == image_token_index)[0].tolist()
        if not where:
            embeds.append(embed(ids))
            if labels is not None:
                new_labels.append(labels[b])
            k += 1                                              # an image-less sample consumes one feature block
            continue
        hb, wb = (int(h_block[b]), int(w_block[b])) if mode == "slice" else (1, 1)
        pieces, lab, start = [], [], 0
        for pos in where:
            blk, k = image_block(image_features, k, mode, hb, wb, sep_e, ret_e)
            pieces += [embed(ids[start:pos]), blk]
            if labels is not None:
                lab += [labels[b, start:pos], torch.full((blk.shape[0],), IGNORE_INDEX, dtype=labels.dtype, device=labels.device)]
            start = pos + 1
        if start < ids.shape[0]:
            pieces.append(embed(ids[start:]))
            if labels is not None:
                lab.append(labels[b, start:])
        embeds.append(torch.cat([p.to(dev) for p in pieces], dim=0))
        if labels is not None:
            new_labels.append(torch.cat(lab, dim=0))
    lengths = [e.shape[0] for e in embeds]
    L, L_in = max(lengths), input_ids.shape[1]
    out = torch.stack([torch.cat([e, e.new_zeros(L - e.shape[0], e.shape[1])], dim=0) for e in embeds], dim=0)
    out_labels = out_mask = None
    if labels is not None:
        out_labels = torch.stack([torch.cat([t, t.new_full((L - t.shape[0],), IGNORE_INDEX)], dim=0) for t in new_labels], dim=0)
    if attention_mask is not None:
        if labels is None and any(n != lengths[0] for n in lengths):
            raise ValueError("ragged lengths with an attention_mask need labels")
        out_mask = torch.stack([torch.cat([m.new_ones(n - L_in), m, m.new_zeros(L - n)], dim=0)
                                for m, n in zip(attention_mask, lengths)], dim=0)
    return out_mask, out, out_labels
