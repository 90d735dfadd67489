"""Mint tests/golden/splice_plain.npz: the yard-stick for splice.build_multimodal_inputs in the DEFAULT mode.

The reference's UNMODIFIED prepare_inputs_labels_for_multimodal (llava/model/llava_arch.py:100-233, imported through
oracle.reference_loader.import_llava_arch()) is called with mode=None in float64 on the CPU, with labels, an attention_mask and
autograd live on the projector output and on the embedding table (an nn.Embedding WITH a padding_idx, as LlamaModel builds it);
a seeded upstream gradient is then backpropagated through new_input_embeds.  Its collaborators are stand-ins as in
tools/make_hd_train_golden.py: encode_images returns the seeded features, the LM is an nn.Embedding.

Three batches, every value representable in bf16 and fp16 (the GPU tests compare copies bit for bit in either dtype):
  * "ragged": a sample with one image token, an image-less sample (it consumes feature block 1, which nothing reads), a sample
    with two image tokens; text ids repeat inside and across samples, one id equals the table's padding_idx, the given mask
    has a False; lengths differ -> the padding branch of :197-222;
  * "equal":  three samples with one image each -> equal lengths, the :223-231 branch;
  * "one":    B = 1.
Per batch <name>_*: ids, feats, table, padding_idx, labels, attention_mask, dout (the upstream gradient), inputs_sha256, and
the reference's new_input_embeds, new_labels, attention_mask_out, d_feats, d_table.  Arrays only.
Needs the reference sources (build container only):  python tools/make_splice_golden.py
"""
from __future__ import annotations

import hashlib
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import reference_loader  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "splice_plain.npz")
M, D, VOCAB, PADDING_IDX, IMG = 16, 48, 24, 0, -200
BATCHES = {
    "ragged": dict(seed=4101, ids=[[1, IMG, 5, 5, 7, 0, 9, 5],
                                   [10, 11, 12, 13, 14, 15, 11, 2],
                                   [3, IMG, 4, IMG, 7, 6, 2, 9]]),
    "equal": dict(seed=4102, ids=[[1, IMG, 2, 3, 4, 2], [5, 6, IMG, 8, 9, 0], [IMG, 12, 13, 1, 14, 14]]),
    "one": dict(seed=4103, ids=[[21, 22, IMG, 23, 22, 20, 19]]),
}


def exact(t: torch.Tensor) -> torch.Tensor:
    """Round to a value that bf16 and fp16 both hold exactly."""
    return t.to(torch.bfloat16).half().double()


def batch_inputs(name: str):
    spec = BATCHES[name]
    g = torch.Generator().manual_seed(spec["seed"])
    ids = torch.tensor(spec["ids"])
    n_blocks = sum(max(1, row.count(IMG)) for row in spec["ids"])          # an image-less sample consumes one (:124-131)
    feats = exact(torch.randn(n_blocks, M, D, generator=g))
    table = exact(torch.randn(VOCAB, D, generator=g))
    labels = torch.randint(0, VOCAB, ids.shape, generator=g)
    labels[ids == IMG] = -100                                              # what a data loader puts under the image token
    labels[:, 0] = -100
    mask = torch.ones(ids.shape, dtype=torch.bool)
    mask[0, -1] = False                                                    # a padded position the mask must carry through
    return ids, feats, table, labels, mask


def run_reference(arch, ids, feats, table, labels, mask):
    feats = feats.clone().requires_grad_(True)

    class LM(arch.LlavaMetaForCausalLM, torch.nn.Module):
        def __init__(self):
            torch.nn.Module.__init__(self)
            self.model = torch.nn.Module()
            self.model.embed_tokens = torch.nn.Embedding.from_pretrained(table.clone(), freeze=False, padding_idx=PADDING_IDX)
            self.config = types.SimpleNamespace()
            self.device = torch.device("cpu")

        def get_model(self):
            return self.model

        def get_vision_tower(self):
            return object()

        def encode_images(self, images):
            return feats

    lm = LM()
    _, mask_out, _, embeds, new_labels = lm.prepare_inputs_labels_for_multimodal(ids, mask.clone(), None, labels.clone(),
                                                                                  torch.zeros(1), None, None, None)
    return lm, feats, mask_out, embeds, new_labels


def digest(*ts) -> str:
    h = hashlib.sha256()
    for t in ts:
        h.update(t.contiguous().numpy().tobytes())
    return h.hexdigest()


def main():
    if not reference_loader.reference_available():
        sys.exit("the reference sources are not available here")
    for name in ("torchvision", "torchvision.ops", "torchvision.ops.boxes"):
        if name in sys.modules and getattr(sys.modules[name], "__spec__", None) is None:
            del sys.modules[name]
    arch = reference_loader.import_llava_arch()
    out = {}
    for name, spec in BATCHES.items():
        ids, feats, table, labels, mask = batch_inputs(name)
        lm, f, mask_out, embeds, new_labels = run_reference(arch, ids, feats, table, labels, mask)
        dout = exact(torch.randn(embeds.shape, generator=torch.Generator().manual_seed(spec["seed"] + 1000)))
        (embeds * dout).sum().backward()
        out.update({f"{name}_ids": ids.numpy(), f"{name}_feats": feats.numpy(), f"{name}_table": table.numpy(),
                    f"{name}_padding_idx": np.int64(PADDING_IDX), f"{name}_labels": labels.numpy(),
                    f"{name}_attention_mask": mask.numpy(), f"{name}_dout": dout.numpy(),
                    f"{name}_inputs_sha256": np.array(digest(ids, feats, table, labels, mask, dout)),
                    f"{name}_new_input_embeds": embeds.detach().numpy(), f"{name}_new_labels": new_labels.numpy(),
                    f"{name}_attention_mask_out": mask_out.numpy(), f"{name}_d_feats": f.grad.numpy(),
                    f"{name}_d_table": lm.model.embed_tokens.weight.grad.numpy()})
        print(f"{name}: embeds {tuple(embeds.shape)}, labels {tuple(new_labels.shape)}, mask {tuple(mask_out.shape)}")
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT} ({os.path.getsize(OUT) / 1e3:.1f} kB)")


if __name__ == "__main__":
    main()
