"""Mint tests/golden/hd_splice_train.npz: the yard-stick for TRAINING through the HD token splice (hd.build_multimodal_inputs).

The reference's UNMODIFIED prepare_inputs_labels_for_multimodal (llava/model/llava_arch.py:100-233, mode 'slice', imported through
oracle.reference_loader.import_llava_arch()) is called in float64 on the CPU with labels, an attention_mask and autograd live on the
projector output and on the embedding table; a seeded upstream gradient is then backpropagated through new_input_embeds.  Its
collaborators are the stand-ins of oracle/make_hd_golden.py:mint_splice (restated here): encode_images returns the seeded features, the
tokenizer maps ',' / '\\n' to two ids, the LM is an nn.Embedding.

Two batches, every value representable in bf16 and fp16 (so that the GPU tests compare copies bit for bit in either dtype):
  * "ragged": the SPLICE batch of make_hd_golden (an image-less sample, a sample with two image tokens, grids 1x1, 2x3, 3x1),
    lengths differ -> the padding branch of :197-222 (left pad of True in the mask);
  * "equal":  three samples with one image each and the same grid -> equal assembled lengths, the :223-231 branch.
Per batch <name>_*: ids, h_block, w_block, sep_id, ret_id, feats, table, labels, attention_mask, dout (the upstream gradient),
inputs_sha256, and the reference's new_input_embeds, new_labels, attention_mask_out, d_feats, d_table.
Needs the reference sources (build container only):  python tools/make_hd_train_golden.py
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
sys.path.insert(0, os.path.join(ROOT, "oracle"))

from oracle import reference_loader  # noqa: E402
import make_hd_golden as mk  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "hd_splice_train.npz")
EQUAL = dict(seed=777, samples=[([1, -200, 2, 3, 4], 2, 2), ([5, 6, -200, 8, 9], 2, 2), ([10, 12, 13, -200, 14], 2, 2)])


def exact(t: torch.Tensor) -> torch.Tensor:
    """Round to a value that bf16 and fp16 both hold exactly (make_hd_golden.splice_inputs)."""
    return t.to(torch.bfloat16).half().double()


def batch_inputs(name: str):
    if name == "ragged":
        ids, hb, wb, feats, table = mk.splice_inputs()
        seed = mk.SPLICE["seed"] + 1
    else:
        g = torch.Generator().manual_seed(EQUAL["seed"])
        ids = torch.tensor([s[0] for s in EQUAL["samples"]])
        hb, wb = [s[1] for s in EQUAL["samples"]], [s[2] for s in EQUAL["samples"]]
        n_crops = sum(h * w + (1 if h * w > 1 else 0) for _, h, w in EQUAL["samples"])
        feats = torch.randn(n_crops, mk.SPLICE["M"], mk.SPLICE["D"], generator=g).to(torch.bfloat16).half().float()
        table = torch.randn(mk.SPLICE["vocab"], mk.SPLICE["D"], generator=g).to(torch.bfloat16).half().float()
        seed = EQUAL["seed"] + 1
    g = torch.Generator().manual_seed(seed)
    labels = torch.randint(0, mk.SPLICE["vocab"], ids.shape, generator=g)
    labels[ids == -200] = -100                                 # what a data loader puts under the image token
    labels[:, 0] = -100
    mask = torch.ones(ids.shape, dtype=torch.bool)
    mask[0, -1] = False                                        # a padded position the mask must carry through
    return ids, hb, wb, feats.double(), table.double(), labels, mask, seed


def run_reference(arch, ids, hb, wb, feats, table, labels, mask):
    feats = feats.clone().requires_grad_(True)

    class LM(arch.LlavaMetaForCausalLM, torch.nn.Module):
        def __init__(self):
            torch.nn.Module.__init__(self)
            self.model = torch.nn.Module()
            self.model.embed_tokens = torch.nn.Embedding.from_pretrained(table.clone(), freeze=False)
            self.config = types.SimpleNamespace()
            self.tokenizer = types.SimpleNamespace(
                convert_tokens_to_ids=lambda toks: [{",": mk.SPLICE["sep_id"], "\n": mk.SPLICE["ret_id"]}[t] for t in toks])
            self.device = torch.device("cpu")

        def get_model(self):
            return self.model

        def get_vision_tower(self):
            return object()

        def encode_images(self, images):
            return feats

    lm = LM()
    _, mask_out, _, embeds, new_labels = lm.prepare_inputs_labels_for_multimodal(ids, mask.clone(), None, labels.clone(),
                                                                                  torch.zeros(1), "slice", hb, wb)
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
    for name in ("ragged", "equal"):
        ids, hb, wb, feats, table, labels, mask, seed = batch_inputs(name)
        lm, f, mask_out, embeds, new_labels = run_reference(arch, ids, hb, wb, feats, table, labels, mask)
        dout = exact(torch.randn(embeds.shape, generator=torch.Generator().manual_seed(seed + 1)))
        (embeds * dout).sum().backward()
        out.update({f"{name}_ids": ids.numpy(), f"{name}_h_block": np.array(hb), f"{name}_w_block": np.array(wb),
                    f"{name}_sep_id": np.int64(mk.SPLICE["sep_id"]), f"{name}_ret_id": np.int64(mk.SPLICE["ret_id"]),
                    f"{name}_feats": feats.numpy(), f"{name}_table": table.numpy(), f"{name}_labels": labels.numpy(),
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
