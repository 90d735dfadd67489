#!/usr/bin/env python3
"""From decoded RGB pictures to the tower's input (image modes 'pad' and 'square', 336 pixels, bf16) on one MI355X: the reference-style
CPU path and preprocess.preprocess_images, in one process, alternating, after warm-up.

  pil    what the reference's loader and drivers do (mm_utils.py:14-37, CLIPImageProcessor.preprocess, `.to(dtype)`), restated with
         Pillow itself: expand2square for 'pad', Image.resize(BICUBIC) of the shortest edge, centre crop, then / 255, - mean, / std in
         torch on the CPU; the fp32 batch uploaded (12 bytes per output pixel) and cast on the device.  Only where PIL imports: where
         it does not, the record says so and holds the `ours` leg alone.
  ours   preprocess.preprocess_images from the uint8 arrays: one pinned staging buffer (3 bytes per source pixel + plan + tables), one
         copy, two launches.

Shapes: eval1 — one 1344 x 1008 picture; batch32 — the 32 seeded image sizes of tools/hd_slice_bench.py's `pretrain_hd`.
Per leg, mode and shape: the median over --reps repetitions of the host wall time (ends in a device synchronise) and of the HIP-event
time between the first enqueue and the last completion, separately.  The two launches alone (`kernels`): HIP events around
--kernel-reps back-to-back tp_clip_preprocess calls on device-resident pixels, plan and tables.  Where both legs ran, their bf16
results are compared bit for bit before anything is timed.

    python tools/preprocess_bench.py [--reps 30] [--out profiles/clip_preprocess_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tokenpacker_amd import _capi, hd  # noqa: E402
from tokenpacker_amd import preprocess as pp  # noqa: E402

try:
    import PIL
    from PIL import Image
    PIL_NOTE = None
except ImportError as exc:                                      # the record says so
    Image = None
    PIL_NOTE = f"PIL does not import on this box ({exc}): no CPU leg was measured"

SIZE, DTYPE = 336, torch.bfloat16
MODES = ("square", "pad")


def make_images(name):
    """Seeded uint8 [H, W, 3] numpy arrays (what np.asarray(pil.convert('RGB')) gives)."""
    if name == "eval1":
        sizes = [(1344, 1008)]
    else:                                                       # tools/hd_slice_bench.py: `pretrain_hd` (32 samples, seed 902)
        g = torch.Generator().manual_seed(902)
        sizes = [tuple(int(v) for v in torch.randint(200, 2400, (2,), generator=g)) for _ in range(32)]
    g = torch.Generator().manual_seed(len(sizes))
    return [torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, generator=g).numpy() for h, w in sizes]


def leg_pil(imgs, mode, dev):
    m, s = torch.tensor(hd.CLIP_MEAN), torch.tensor(hd.CLIP_STD)
    out = []
    for u8 in imgs:
        im = Image.fromarray(u8)
        if mode == "pad" and im.width != im.height:
            side = max(im.size)
            sq = Image.new(im.mode, (side, side), tuple(int(v * 255) for v in hd.CLIP_MEAN))
            sq.paste(im, (0, (im.width - im.height) // 2) if im.width > im.height else ((im.height - im.width) // 2, 0))
            im = sq
        w, h = im.size
        oh, ow = (SIZE, int(SIZE * w / h)) if h <= w else (int(SIZE * h / w), SIZE)
        im = im.resize((ow, oh), Image.BICUBIC)
        top, left = (oh - SIZE) // 2, (ow - SIZE) // 2
        t = torch.from_numpy(np.array(im.crop((left, top, left + SIZE, top + SIZE)))).permute(2, 0, 1).to(torch.float32).div(255)
        out.append(t.sub_(m[:, None, None]).div_(s[:, None, None]))
    return torch.stack(out).to(dev).to(DTYPE)


def leg_ours(imgs, mode, dev):
    return pp.preprocess_images(imgs, mode, SIZE, DTYPE, device=dev)


def timed_once(fn, imgs, mode, dev):
    """-> (host wall ms, HIP-event ms) of one call, from an idle device to an idle device."""
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    start.record()
    fn(imgs, mode, dev)
    end.record()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, start.elapsed_time(end)


def kernels_alone(imgs, mode, dev, reps):
    """HIP-event time of one tp_clip_preprocess call (two launches) on device-resident data: median of 5 batches of `reps` calls."""
    plan = pp.clip_batch_plan([u8.shape[:2] for u8 in imgs], mode, SIZE, tuple(int(v * 255) for v in hd.CLIP_MEAN))
    pix = np.zeros(plan.pixel_bytes, dtype=np.uint8)
    for u8, rec in zip(imgs, plan.images):
        at = int(rec["src_offset"])
        pix[at:at + u8.size] = u8.reshape(-1)
    records = plan.images.view(np.uint8)
    plan_dev, coeffs_dev, pix_dev = torch.from_numpy(records).to(dev), torch.from_numpy(plan.coeffs).to(dev), torch.from_numpy(pix).to(dev)
    lut = hd.normalisation_table().to(dev)
    workspace = torch.empty(plan.workspace_bytes, dtype=torch.uint8, device=dev)
    out = torch.empty(len(imgs), 3, SIZE, SIZE, dtype=DTYPE, device=dev)
    lib, stream = _capi.load_library(), torch.cuda.current_stream(dev).cuda_stream

    def launch():
        _capi.check(lib.tp_clip_preprocess(records.ctypes.data, plan_dev.data_ptr(), len(imgs), pix_dev.data_ptr(), plan.pixel_bytes,
                                           lut.data_ptr(), plan.coeffs.ctypes.data, coeffs_dev.data_ptr(), plan.coeffs.size,
                                           workspace.data_ptr(), plan.workspace_bytes, out.data_ptr(), SIZE, _capi.TP_BF16, stream),
                    "tp_clip_preprocess")
    for _ in range(3):
        launch()
    times = []
    for _ in range(5):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        for _ in range(reps):
            launch()
        end.record()
        torch.cuda.synchronize()
        times.append(start.elapsed_time(end) / reps)
    return dict(kernels_ms=round(statistics.median(times), 5), pixel_bytes=int(sum(u8.size for u8 in imgs)),
                workspace_bytes=int(plan.workspace_bytes), coeff_bytes=int(plan.coeffs.size * 4),
                output_bytes=out.numel() * out.element_size())


def bench(shapes, reps, warmup, kernel_reps):
    dev = torch.device("cuda", torch.cuda.current_device())
    fns = dict(ours=leg_ours)
    if Image is not None:
        fns["pil"] = leg_pil
    legs = tuple(fns)
    res = {}
    for name in shapes:
        imgs = make_images(name)
        for mode in MODES:
            outs = {leg: fns[leg](imgs, mode, dev).cpu() for leg in legs}
            r = dict(images=len(imgs), sizes=[list(u8.shape[:2]) for u8 in imgs], mode=mode, reps=reps)
            if "pil" in outs:
                r["bit_equal_to_pil_bf16"] = bool(torch.equal(outs["pil"].view(torch.int16), outs["ours"].view(torch.int16)))
                assert r["bit_equal_to_pil_bf16"], (name, mode)
            for _ in range(warmup):
                for leg in legs:
                    timed_once(fns[leg], imgs, mode, dev)
            host, device = {leg: [] for leg in legs}, {leg: [] for leg in legs}
            for _ in range(reps):                                        # alternating
                for leg in legs:
                    h, d = timed_once(fns[leg], imgs, mode, dev)
                    host[leg].append(h)
                    device[leg].append(d)
            for leg in legs:
                r[leg] = dict(host_ms_median=round(statistics.median(host[leg]), 4), device_ms_median=round(statistics.median(device[leg]), 4),
                              host_ms_minmax=[round(min(host[leg]), 4), round(max(host[leg]), 4)],
                              device_ms_minmax=[round(min(device[leg]), 4), round(max(device[leg]), 4)])
            if "pil" in legs:
                r["pil_over_ours_host"] = round(r["pil"]["host_ms_median"] / r["ours"]["host_ms_median"], 2)
            r["kernels"] = kernels_alone(imgs, mode, dev, kernel_reps)
            res[f"{name}_{mode}"] = r
            print(f"{name} {mode}: host ms " + " ".join(f"{leg} {r[leg]['host_ms_median']:.3f}" for leg in legs) +
                  f"; two launches alone {r['kernels']['kernels_ms']:.4f} ms", flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--kernel-reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clip_preprocess_bench.json"))
    ap.add_argument("--shapes", nargs="+", default=["eval1", "batch32"], choices=["eval1", "batch32"])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("preprocess_bench.py needs an AMD GPU: nothing is measured without one")
    res = bench(a.shapes, a.reps, a.warmup, a.kernel_reps)
    res["device"] = torch.cuda.get_device_name(0)
    res["pil"] = PIL_NOTE or f"Pillow {PIL.__version__} on the host CPU"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
