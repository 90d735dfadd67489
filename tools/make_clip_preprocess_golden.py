#!/usr/bin/env python3
"""Mint tests/golden/clip_preprocess.npz from the reference's own ``process_images`` / ``expand2square`` (llava/mm_utils.py, loaded
unmodified from the reference checkout with ``sys.modules['llava']`` pre-seeded) and the installed
``transformers.CLIPImageProcessor`` (336-pixel shortest edge and crop, bicubic, CLIP mean / std — the openai/clip-vit-large-patch14-336
settings every reference script names).  Needs the reference checkout, Pillow and transformers; the tests need none of them.

The reference pins transformers 4.31; the fixture is minted with what is installed and records the versions it was minted with.

Stored (data only):
  cases   int64 [n, 4]      (h, w, mode, seed); mode 0 = square (the dataclass default), 1 = pad; the input is
                            tests/clip_preprocess_ref.test_image(h, w, seed)
  input_sha256, output_sha256   hex digests of the input bytes and of the fp32 pixel_values [3, 336, 336] of every case
  full_index, full_bytes    for two small cases the whole result as uint8 [3, 336, 336], recovered through the table (the script
                            asserts that the table maps them back onto pixel_values exactly)
  table   float32 [3, 256]  what the reference's processor makes of byte u in channel c
  versions                  "pillow x.y transformers a.b <processor class>"

    python tools/make_clip_preprocess_golden.py
"""
import importlib
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.reference_loader import REFERENCE_ROOT  # noqa: E402
from tests import clip_preprocess_ref as ref  # noqa: E402

SIZES = [(336, 336), (336, 500), (337, 500), (335, 336), (40, 39), (5, 5), (50, 71), (71, 50), (1, 37), (37, 1), (3, 900), (1000, 41),
         (1201, 1600), (2500, 700)]
FULL = [(40, 39, 1), (50, 71, 0)]          # (h, w, mode) stored whole
SEED = 7


def load_mm_utils():
    """llava.mm_utils of the reference, unmodified: `import llava` itself fails under the installed transformers, so an empty package
    whose __path__ points at the reference directory stands in for it."""
    if "llava" not in sys.modules:
        pkg = types.ModuleType("llava")
        pkg.__path__ = [os.path.join(REFERENCE_ROOT, "llava")]
        pkg.__package__ = "llava"
        sys.modules["llava"] = pkg
    return importlib.import_module("llava.mm_utils")


def main():
    import PIL
    import transformers
    from PIL import Image
    from transformers import CLIPImageProcessor

    mm = load_mm_utils()
    proc = CLIPImageProcessor(size={"shortest_edge": 336}, crop_size={"height": 336, "width": 336}, resample=3)
    # (without torchvision the installed transformers hands out its PIL backend, the arithmetic transformers 4.31 ran; the class
    # name is recorded with the versions)

    def run(u8, mode):
        cfg = types.SimpleNamespace(image_aspect_ratio="pad" if mode else None)
        out = mm.process_images([Image.fromarray(u8)], proc, cfg)
        return np.ascontiguousarray(out[0].numpy())

    # the table: a 336 x 336 picture needs no resize, so byte u in all channels of pixel (0, u) comes back as table[:, u]
    probe = np.zeros((336, 336, 3), dtype=np.uint8)
    probe[0, :256] = np.arange(256, dtype=np.uint8)[:, None]
    table = run(probe, 0)[:, 0, :256].copy()
    assert table.dtype == np.float32 and all(len(np.unique(table[c])) == 256 for c in range(3))

    cases, din, dout, full_index, full_bytes = [], [], [], [], []
    for h, w in SIZES:
        for mode in (0, 1):
            u8 = ref.test_image(h, w, SEED)
            pv = run(u8, mode)
            assert pv.shape == (3, 336, 336) and pv.dtype == np.float32
            cases.append((h, w, mode, SEED))
            din.append(ref.digest(u8))
            dout.append(ref.digest(pv))
            if (h, w, mode) in FULL:
                b = np.stack([np.searchsorted(table[c], pv[c]) for c in range(3)]).astype(np.uint8)      # the table is increasing
                back = np.stack([table[c][b[c]] for c in range(3)])
                assert np.array_equal(back.view(np.int32), pv.view(np.int32)), "the table does not recover pixel_values"
                full_index.append(len(cases) - 1)
                full_bytes.append(b)
    out = os.path.join(ROOT, "tests", "golden", "clip_preprocess.npz")
    np.savez_compressed(out, cases=np.asarray(cases, dtype=np.int64), input_sha256=np.asarray(din), output_sha256=np.asarray(dout),
                        full_index=np.asarray(full_index, dtype=np.int64), full_bytes=np.stack(full_bytes), table=table,
                        versions=np.asarray(f"pillow {PIL.__version__} transformers {transformers.__version__} "
                                            f"{type(proc).__name__}"))
    print(f"wrote {out}: {len(cases)} cases, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
