"""CLIP preprocessing on the device for the reference's ``'pad'`` and default (``'square'``) image modes.

What ``llava/mm_utils.py:14-37`` and the loader (``train.py:679-694, 732-734``) do to a decoded picture when
``image_aspect_ratio`` is not ``'slice'``: optionally ``expand2square`` with the colour ``tuple(int(m * 255) for m in image_mean)``,
then ``CLIPImageProcessor.preprocess`` — PIL's 8-bit bicubic resize, centre crop, rescale by 1/255, normalise — and the driver's
``.to(dtype)``.  Pillow's 8-bit resize is integer arithmetic, so the result equals the reference's ``pixel_values`` bit for bit.

* :func:`preprocess_plan` — the per-image geometry (pure host logic).
* :func:`preprocess_images` — a batch of raw RGB uint8 images of any sizes -> ``[n, 3, size, size]`` in the tower's dtype from two
  launches (``tp_clip_preprocess``): 3 bytes per pixel travel to the device, not 12.  ``'slice'`` is :func:`hd.slice_images`.
"""
from __future__ import annotations

import ctypes
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _capi
from .hd import CLIP_MEAN, CLIP_STD, _PIXEL_ALIGN, _as_hwc_uint8, _device_table, _table_key

MAX_SIDE = 16384                     # pixels per side the library accepts (197 taps at size 336)


class ClipGeometry(NamedTuple):
    """One image's geometry.  The resize reads an ``in_h x in_w`` picture — the image itself, or in pad mode the square of side
    ``max(H, W)`` in which the image sits at ``(pad_top, pad_left)`` — makes it ``out_h x out_w`` and keeps the ``size x size``
    window at ``(crop_top, crop_left)``."""
    mode: str                        # "pad" or "square"
    H: int
    W: int
    in_h: int
    in_w: int
    pad_top: int
    pad_left: int
    out_h: int
    out_w: int
    crop_top: int
    crop_left: int


def _mode(image_aspect_ratio) -> str:
    if image_aspect_ratio == "slice":
        raise ValueError("image_aspect_ratio 'slice' is TokenPacker-HD slicing: use tokenpacker_amd.hd.slice_images")
    return "pad" if image_aspect_ratio == "pad" else "square"       # mm_utils.py:31-37: anything but 'pad' is the processor alone


def preprocess_plan(sizes: Sequence[Tuple[int, int]], image_aspect_ratio: str = "square", size: int = 336) -> List[ClipGeometry]:
    """Geometry for images of ``sizes [(H, W), ...]``.  ``'pad'``: ``expand2square`` (mm_utils.py:14-25: the content at row
    ``(W - H) // 2`` when ``W > H``, else at column ``(H - W) // 2``), then the square resized to ``size x size``.  Otherwise the
    processor's rule: the shortest edge to ``size``, the long one to ``int(size * long / short)``, then the centre crop with
    ``top = (out_h - size) // 2``, ``left = (out_w - size) // 2``.  Pure host logic."""
    mode = _mode(image_aspect_ratio)
    if size < 8 or size % 8 != 0:
        raise ValueError(f"size = {size} must be a positive multiple of 8 (a lane stores 8 consecutive pixels)")
    plan = []
    for i, (H, W) in enumerate(sizes):
        H, W = int(H), int(W)
        if H < 1 or W < 1:
            raise ValueError(f"image {i}: size {H} x {W}")
        if H > MAX_SIDE or W > MAX_SIDE:
            raise ValueError(f"image {i}: {H} x {W} exceeds the supported maximum of {MAX_SIDE} pixels per side")
        if mode == "pad":
            S = max(H, W)
            top, left = ((W - H) // 2, 0) if W > H else (0, (H - W) // 2)
            plan.append(ClipGeometry(mode, H, W, S, S, top, left, size, size, 0, 0))
        else:
            if H <= W:
                oh, ow = size, int(size * W / H)
            else:
                oh, ow = int(size * H / W), size
            plan.append(ClipGeometry(mode, H, W, H, W, 0, 0, oh, ow, (oh - size) // 2, (ow - size) // 2))
    return plan


def resize_coeffs(in_size: int, out_size: int, first_out: int, n_out: int) -> Tuple[np.ndarray, np.ndarray]:
    """Pillow's 8-bit bicubic coefficients from the library (``tp_resize_coeffs``, the single source; no GPU needed):
    ``(kk int32 [n_out, ksize], bounds int32 [n_out, 2] = (xmin, xcount))`` for output positions ``[first_out, first_out + n_out)``."""
    if not _capi.clip_preprocess_supported():
        raise RuntimeError("the loaded libtokenpacker_hip.so lacks tp_resize_coeffs; rebuild it")
    lib = _capi.load_library()
    ksize = ctypes.c_int(0)
    _capi.check(lib.tp_resize_coeffs(in_size, out_size, first_out, n_out, None, None, ctypes.byref(ksize)), "tp_resize_coeffs")
    kk = np.empty((n_out, ksize.value), dtype=np.int32)
    bounds = np.empty((n_out, 2), dtype=np.int32)
    _capi.check(lib.tp_resize_coeffs(in_size, out_size, first_out, n_out, kk.ctypes.data, bounds.ctypes.data, ctypes.byref(ksize)),
                "tp_resize_coeffs")
    return kk, bounds


_PLAN_IMAGE = np.dtype([("src_offset", "<i8"), ("ws_offset", "<i8"), ("H", "<i4"), ("W", "<i4"), ("row_stride", "<i4"), ("mode", "<i4"),
                        ("in_h", "<i4"), ("in_w", "<i4"), ("pad_top", "<i4"), ("pad_left", "<i4"),
                        ("out_h", "<i4"), ("out_w", "<i4"), ("crop_top", "<i4"), ("crop_left", "<i4"),
                        ("ksize_h", "<i4"), ("ksize_v", "<i4"), ("row0", "<i4"), ("rows", "<i4"),
                        ("kk_h", "<i4"), ("bounds_h", "<i4"), ("kk_v", "<i4"), ("bounds_v", "<i4"),
                        ("background", "u1", (4,)), ("reserved", "<i4")])
assert _PLAN_IMAGE.itemsize == ctypes.sizeof(_capi.tp_clip_image)


class ClipBatchPlan(NamedTuple):
    """Host plan of one :func:`preprocess_images` call.  ``images``: one ``tp_clip_image`` record per image (a numpy structured
    array with the C struct's layout); ``coeffs`` (int32): all coefficient tables, addressed by the records' word offsets;
    ``pixel_bytes``: the size of the pixel buffer the offsets address; ``workspace_bytes``: what the two passes need between them."""
    images: np.ndarray
    coeffs: np.ndarray
    geometry: List[ClipGeometry]
    pixel_bytes: int
    workspace_bytes: int


def clip_batch_plan(sizes: Sequence[Tuple[int, int]], image_aspect_ratio: str = "square", size: int = 336,
                    background: Sequence[int] = (0, 0, 0), row_strides: Optional[Sequence[int]] = None,
                    offsets: Optional[Sequence[int]] = None) -> ClipBatchPlan:
    """The plan for images of ``sizes``: :func:`preprocess_plan`'s geometry, the coefficient tables of the crop window's ``size``
    positions per axis (the horizontal one tap-major), the source rows the horizontal pass covers, packed workspace slices, and where
    each image's bytes lie (``row_strides`` / ``offsets`` as in :func:`hd.slice_batch_plan`).  Host logic; no GPU needed."""
    n = len(sizes)
    if n == 0:
        raise ValueError("clip_batch_plan: no images")
    geometry = preprocess_plan(sizes, image_aspect_ratio, size)
    bg = tuple(int(v) for v in background)
    if len(bg) != 3 or min(bg) < 0 or max(bg) > 255:
        raise ValueError("background must be three bytes (R, G, B)")
    images = np.zeros(n, dtype=_PLAN_IMAGE)
    tables, word, ws, at = [], 0, 0, 0
    for i, g in enumerate(geometry):
        stride = 3 * g.W if row_strides is None else int(row_strides[i])
        if stride < 3 * g.W or stride > 0x7FFFFFFF:
            raise ValueError(f"image {i}: row stride {stride} (3 * W = {3 * g.W} .. 2^31 - 1)")
        kk_h, bounds_h = resize_coeffs(g.in_w, g.out_w, g.crop_left, size)
        kk_v, bounds_v = resize_coeffs(g.in_h, g.out_h, g.crop_top, size)
        row0, row1 = int(bounds_v[0, 0]), int(bounds_v[-1, 0] + bounds_v[-1, 1])
        off = at if offsets is None else int(offsets[i])
        where = []
        for t in (np.ascontiguousarray(kk_h.T), bounds_h, kk_v, bounds_v):
            where.append(word)
            tables.append(t.reshape(-1))
            word += t.size
        images[i] = (off, ws, g.H, g.W, stride, _capi.TP_CLIP_PAD if g.mode == "pad" else _capi.TP_CLIP_SQUARE,
                     g.in_h, g.in_w, g.pad_top, g.pad_left, g.out_h, g.out_w, g.crop_top, g.crop_left,
                     kk_h.shape[1], kk_v.shape[1], row0, row1 - row0, *where, bg + (0,), 0)
        ws += -(-(row1 - row0) * size * 3 // 16) * 16
        end = off + (g.H - 1) * stride + 3 * g.W
        at = max(at, -(-end // _PIXEL_ALIGN) * _PIXEL_ALIGN)
    if word > 0x7FFFFFFF:
        raise ValueError("the batch's coefficient tables exceed 2^31 words")
    need = _capi.load_library().tp_clip_preprocess_workspace_bytes(images.ctypes.data, n, size)
    if need == 0:
        raise ValueError(f"tp_clip_preprocess_workspace_bytes: {_capi.last_error()}")
    assert need == ws, (need, ws)
    return ClipBatchPlan(images, np.concatenate(tables), geometry, at, need)


def preprocess_images(images, image_aspect_ratio: str = "square", size: int = 336, dtype: torch.dtype = torch.bfloat16,
                      mean: Sequence[float] = CLIP_MEAN, std: Sequence[float] = CLIP_STD, background: Optional[Sequence[int]] = None,
                      device=None) -> torch.Tensor:
    """A batch of raw RGB images -> ``[n, 3, size, size]`` in ``dtype`` on the device: the ``images`` tensor of the reference's
    loader and ``process_images`` for ``image_aspect_ratio == 'pad'`` (pad to a square with ``background``, resize to
    ``size x size``) or anything else but ``'slice'`` (shortest edge to ``size``, centre crop), after the driver's ``.to(dtype)``.

    ``images``: as for :func:`hd.slice_images` — a sequence of ``[H, W, 3]`` uint8 torch tensors or numpy arrays of any sizes, all
    on the CPU or all on one device, rows may be strided.  The plan, the coefficient tables and (for CPU images) the pixels travel
    in one pinned staging buffer and one asynchronous copy.  ``background`` (pad mode only) defaults to the reference's
    ``tuple(int(m * 255) for m in mean)``.  ``dtype``: float32 — bit-equal to the reference's ``pixel_values`` — or bfloat16 /
    float16, that value rounded once.  No host synchronisation; two launches per batch."""
    if isinstance(images, (torch.Tensor, np.ndarray)) or not isinstance(images, Sequence):
        raise TypeError("images must be a sequence (list / tuple) of [H, W, 3] uint8 images")
    if len(images) == 0:
        raise ValueError("images is empty")
    _mode(image_aspect_ratio)
    imgs = [_as_hwc_uint8(img, i) for i, img in enumerate(images)]
    out_dt = {torch.float32: _capi.TP_F32, torch.bfloat16: _capi.TP_BF16, torch.float16: _capi.TP_F16}.get(dtype)
    if out_dt is None:
        raise TypeError("dtype must be float32, bfloat16 or float16")
    on_dev = [isinstance(img, torch.Tensor) and img.is_cuda for img in imgs]
    if any(on_dev) and not all(on_dev):
        raise ValueError("images must all be on the CPU or all on one device")
    sizes = [(int(img.shape[0]), int(img.shape[1])) for img in imgs]
    preprocess_plan(sizes, image_aspect_ratio, size)                    # (refuses a bad size or an over-size side by name)
    table_key = _table_key(mean, std)
    if background is None:
        background = tuple(int(m * 255) for m in table_key[0])          # mm_utils.py:33
    if not torch.cuda.is_available():
        raise RuntimeError("preprocess_images runs only on an AMD GPU (HIP kernels); there is no CPU fallback")
    if not _capi.clip_preprocess_supported():
        raise RuntimeError("the loaded libtokenpacker_hip.so lacks tp_clip_preprocess; rebuild it")
    if on_dev[0]:
        devices = {img.device for img in imgs}
        if len(devices) != 1 or (device is not None and torch.device(device) != next(iter(devices))):
            raise ValueError("device images must all live on one device (and `device`, when given, must be that one)")
        dev = next(iter(devices))
        pieces, strides, offsets, at = [], [], [], 0
        for img, (H, W) in zip(imgs, sizes):
            # rows of adjacent RGB bytes are read in place through their stride; anything else is made dense first
            if img.stride(2) == 1 and img.stride(1) == 3 and (H == 1 or 3 * W <= img.stride(0) <= 0x7FFFFFFF):
                stride = img.stride(0) if H > 1 else 3 * W
            else:
                img, stride = img.contiguous(), 3 * W
            pieces.append(img.as_strided(((H - 1) * stride + 3 * W,), (1,)))
            strides.append(stride)
            offsets.append(at)
            at += pieces[-1].numel()
        if at < 8:
            pieces.append(torch.zeros(8, dtype=torch.uint8, device=dev))
            at += 8
        plan = clip_batch_plan(sizes, image_aspect_ratio, size, background, strides, offsets)._replace(pixel_bytes=at)
    else:
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        plan = clip_batch_plan(sizes, image_aspect_ratio, size, background)
    records, coeffs = plan.images.view(np.uint8), plan.coeffs.view(np.uint8)
    coeff_base = -(-records.size // _PIXEL_ALIGN) * _PIXEL_ALIGN
    pix_base = -(-(coeff_base + coeffs.size) // _PIXEL_ALIGN) * _PIXEL_ALIGN
    staging = torch.empty(pix_base + (0 if on_dev[0] else plan.pixel_bytes), dtype=torch.uint8, pin_memory=True)
    stage_np = staging.numpy()
    stage_np[:records.size] = records
    stage_np[coeff_base:coeff_base + coeffs.size] = coeffs
    if not on_dev[0]:
        for img, rec, (H, W) in zip(imgs, plan.images, sizes):
            at = pix_base + int(rec["src_offset"])
            np.copyto(stage_np[at:at + H * W * 3].reshape(H, W, 3), img.numpy() if isinstance(img, torch.Tensor) else img)
    out = torch.empty(len(imgs), 3, size, size, dtype=dtype, device=dev)
    workspace = torch.empty(plan.workspace_bytes, dtype=torch.uint8, device=dev)
    lib = _capi.load_library()
    with torch.cuda.device(dev):
        lut = _device_table(table_key, dev)
        staged_dev = staging.to(dev, non_blocking=True)                 # the one host -> device copy: plan, tables (+ pixels)
        pixels = torch.cat(pieces) if on_dev[0] else staged_dev[pix_base:]
        _capi.check(lib.tp_clip_preprocess(stage_np.ctypes.data, staged_dev.data_ptr(), len(imgs), pixels.data_ptr(), plan.pixel_bytes,
                                           lut.data_ptr(), stage_np.ctypes.data + coeff_base, staged_dev.data_ptr() + coeff_base,
                                           plan.coeffs.size, workspace.data_ptr(), plan.workspace_bytes, out.data_ptr(), size, out_dt,
                                           torch.cuda.current_stream(dev).cuda_stream), "tp_clip_preprocess")
    return out


__all__ = ["MAX_SIDE", "ClipGeometry", "ClipBatchPlan", "preprocess_plan", "clip_batch_plan", "resize_coeffs", "preprocess_images"]
