#!/usr/bin/env python3
"""From decoded RGB pictures to the tower's input crops (mode 'slice', patch_num 9, bf16) on one MI355X: three ways to do what the
reference's loader and drivers do (train.py:696-731, then `.to(dtype)`), in one process, alternating, after warm-up.

  parent     what this repository offered before hd.slice_images: ToTensor + Normalize restated on the CPU, the fp32 image uploaded
             (12 bytes per pixel), hd.slice_image per image (two launches each), torch.cat, .to(bfloat16)
  reference  the reference-style CPU path: the same normalisation, oracle/hd_oracle.slice_image (F.interpolate on the CPU), the fp32
             crops uploaded, .to(bfloat16) on the device
  ours       hd.slice_images from the uint8 arrays: one pinned staging buffer (3 bytes per pixel + the plan), one copy, ONE launch

Shapes: eval1 — one 1344 x 1008 picture; pretrain_hd — the 32 seeded image sizes of tools/hd_train_bench.py's `pretrain_hd`.
Per leg and shape: the median over --reps repetitions of the host wall time (ends in a device synchronise) and of the HIP-event time
between the first enqueue and the last completion, separately.  The kernel alone (`kernel`): HIP events around --kernel-reps
back-to-back tp_hd_slice_u8 launches on device-resident pixels, and the output bytes it writes per second.

    python tools/hd_slice_bench.py [--reps 30] [--out profiles/hd_slice_bench.json]
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
from oracle import hd_oracle  # noqa: E402  (the reference-style leg)
from tokenpacker_amd import _capi, hd  # noqa: E402

BLOCK, DTYPE = 336, torch.bfloat16
LEGS = ("parent", "reference", "ours")


def make_images(name):
    """Seeded uint8 [H, W, 3] numpy arrays (what np.asarray(pil.convert('RGB')) gives)."""
    if name == "eval1":
        sizes = [(1344, 1008)]
    else:                                                   # tools/hd_train_bench.py: SHAPES['pretrain_hd'] (32 samples, seed 902)
        g = torch.Generator().manual_seed(902)
        sizes = [tuple(int(v) for v in torch.randint(200, 2400, (2,), generator=g)) for _ in range(32)]
    g = torch.Generator().manual_seed(len(sizes))
    return [torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, generator=g).numpy() for h, w in sizes]


def normalise(u8):
    """Compose([ToTensor(), Normalize(CLIP mean, CLIP std)]) in torch on the CPU: [H, W, 3] uint8 -> [3, H, W] fp32."""
    t = torch.from_numpy(u8).permute(2, 0, 1).contiguous().to(torch.float32).div(255)
    m, s = torch.tensor(hd.CLIP_MEAN), torch.tensor(hd.CLIP_STD)
    return t.sub_(m[:, None, None]).div_(s[:, None, None])


def leg_parent(imgs, dev):
    return torch.cat([hd.slice_image(normalise(u8).to(dev), 9, BLOCK)[0] for u8 in imgs]).to(DTYPE)


def leg_reference(imgs, dev):
    crops = []
    for u8 in imgs:
        hb, wb = hd.select_grid(u8.shape[0], u8.shape[1], 9, BLOCK)
        crops.append(hd_oracle.slice_image(normalise(u8).unsqueeze(0), hb, wb, BLOCK))
    return torch.cat(crops).to(dev).to(DTYPE)


def leg_ours(imgs, dev):
    return hd.slice_images(imgs, 9, BLOCK, DTYPE, device=dev)[0]


def timed_once(fn, imgs, dev):
    """-> (host wall ms, HIP-event ms) of one call, from an idle device to an idle device."""
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    start.record()
    fn(imgs, dev)
    end.record()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, start.elapsed_time(end)


def kernel_alone(imgs, dev, reps):
    """HIP-event time of one tp_hd_slice_u8 launch on device-resident pixels (median of 5 batches of `reps` launches)."""
    plan = hd.slice_batch_plan([u8.shape[:2] for u8 in imgs], 9, BLOCK)
    words = plan.words()
    pix = np.zeros(plan.pixel_bytes, dtype=np.uint8)
    for u8, rec in zip(imgs, plan.images):
        at = int(rec["src_offset"])
        pix[at:at + u8.size] = u8.reshape(-1)
    plan_dev, pix_dev = torch.from_numpy(words).to(dev), torch.from_numpy(pix).to(dev)
    lut = hd.normalisation_table().to(dev)
    crops = torch.empty(plan.n_crops, 3, BLOCK, BLOCK, dtype=DTYPE, device=dev)
    lib, stream = _capi.load_library(), torch.cuda.current_stream(dev).cuda_stream

    def launch():
        _capi.check(lib.tp_hd_slice_u8(words.ctypes.data, plan_dev.data_ptr(), len(imgs), pix_dev.data_ptr(), plan.pixel_bytes,
                                       lut.data_ptr(), crops.data_ptr(), plan.n_crops, BLOCK, _capi.TP_BF16, stream), "tp_hd_slice_u8")
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
    ms = statistics.median(times)
    out_bytes = crops.numel() * crops.element_size()
    return dict(kernel_ms=round(ms, 5), output_bytes=out_bytes, pixel_bytes=int(sum(u8.size for u8 in imgs)),
                output_TB_per_s=round(out_bytes / (ms * 1e-3) / 1e12, 4))


def bench(shapes, reps, warmup, kernel_reps):
    dev = torch.device("cuda", torch.cuda.current_device())
    fns = dict(parent=leg_parent, reference=leg_reference, ours=leg_ours)
    res = {}
    for name in shapes:
        imgs = make_images(name)
        outs = {leg: fns[leg](imgs, dev).float().cpu() for leg in LEGS}
        # the three legs compute the same crops: fp32 results a few ulps apart, rounded once to bf16 (one bf16 ulp where a tie flips)
        top = outs["parent"].abs().max().item()
        diffs = {leg: (outs[leg] - outs["parent"]).abs().max().item() for leg in ("reference", "ours")}
        assert all(d <= 2.0 ** -7 * top for d in diffs.values()), diffs
        for _ in range(warmup):
            for leg in LEGS:
                timed_once(fns[leg], imgs, dev)
        host, device = {leg: [] for leg in LEGS}, {leg: [] for leg in LEGS}
        for _ in range(reps):                                            # alternating
            for leg in LEGS:
                h, d = timed_once(fns[leg], imgs, dev)
                host[leg].append(h)
                device[leg].append(d)
        med_h = {leg: statistics.median(host[leg]) for leg in LEGS}
        med_d = {leg: statistics.median(device[leg]) for leg in LEGS}
        r = dict(images=len(imgs), sizes=[list(u8.shape[:2]) for u8 in imgs], n_crops=int(outs["ours"].shape[0]), reps=reps,
                 max_abs_diff_vs_parent_bf16=diffs)
        for leg in LEGS:
            r[leg] = dict(host_ms_median=round(med_h[leg], 4), device_ms_median=round(med_d[leg], 4),
                          host_ms_minmax=[round(min(host[leg]), 4), round(max(host[leg]), 4)],
                          device_ms_minmax=[round(min(device[leg]), 4), round(max(device[leg]), 4)])
        r["parent_over_ours"] = dict(host=round(med_h["parent"] / med_h["ours"], 2), device=round(med_d["parent"] / med_d["ours"], 2))
        r["reference_over_ours"] = dict(host=round(med_h["reference"] / med_h["ours"], 2), device=round(med_d["reference"] / med_d["ours"], 2))
        r["kernel"] = kernel_alone(imgs, dev, kernel_reps)
        res[name] = r
        print(f"{name}: {r['n_crops']} crops; host ms parent {med_h['parent']:.3f} reference {med_h['reference']:.3f} ours "
              f"{med_h['ours']:.3f}; device ms parent {med_d['parent']:.3f} reference {med_d['reference']:.3f} ours {med_d['ours']:.3f}; "
              f"kernel {r['kernel']['kernel_ms']:.4f} ms = {r['kernel']['output_TB_per_s']:.2f} TB/s of output", flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--kernel-reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hd_slice_bench.json"))
    ap.add_argument("--shapes", nargs="+", default=["eval1", "pretrain_hd"], choices=["eval1", "pretrain_hd"])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("hd_slice_bench.py needs an AMD GPU: nothing is measured without one")
    res = bench(a.shapes, a.reps, a.warmup, a.kernel_reps)
    res["device"] = torch.cuda.get_device_name(0)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
