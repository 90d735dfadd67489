"""TokenPacker-HD helpers on either side of the projector.

* :func:`select_grid` — the crop-grid choice for one image (host-side scalar math; reference
  ``llava/patch_divide.py:71-104`` ``Image_Patch.calculate``).  Pure CPU, like the reference.
* :func:`slice_image` — resize / zero-pad / tile / global view of ONE normalised fp32 image on the device (``tp_hd_slice``);
  :func:`slice_images` — the same for a BATCH of raw RGB uint8 images, ``ToTensor`` + ``Normalize`` and the cast to the tower's
  dtype included, from one launch (``tp_hd_slice_u8``; reference ``llava/train/train.py:696-731``).
* :func:`hd_token_rows`, :func:`assemble_hd_tokens` — what ``prepare_inputs_labels_for_multimodal`` does
  with the projected crops in ``mode == 'slice'`` (reference ``llava/model/llava_arch.py:140-154``): the crops
  of one image row are joined with the ``','`` token embedding, every row and the trailing global view end
  with the ``'\\n'`` embedding.  The reference builds this with a Python loop and one ``torch.cat`` per image;
  here ONE kernel launch (``tp_hd_assemble``) writes all images of the batch straight into one
  ``[rows, D]`` buffer, of which per-image views are returned.  Device tensors only, no CPU fallback.
* :func:`build_inputs_embeds`, :func:`build_multimodal_inputs` — the whole slice branch (embeddings, labels, attention
  mask); differentiable with respect to the projector output and the embedding table (``tp_hd_assemble_backward``), so
  a TokenPacker-HD training step runs through them too.
"""
from __future__ import annotations

import ctypes
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _capi

# Candidate grids (h_block, w_block) in the reference's order — the order decides argmax ties, e.g. between
# (a, b) and (b, a) on square images (patch_divide.py:4-54).  Rule behind the data: every factor pair with
# product <= 9, and for larger products only pairs with both factors >= 2.
_GRIDS_9 = ("1x1 1x2 2x1 1x3 3x1 2x2 1x4 4x1 1x5 5x1 1x6 6x1 2x3 3x2 1x7 7x1 4x2 2x4 1x8 8x1 3x3 1x9 9x1")
_GRIDS_16 = _GRIDS_9 + " 2x5 5x2 2x6 6x2 3x4 4x3 2x7 7x2 3x5 5x3 2x8 8x2 4x4"
_GRIDS_25 = _GRIDS_16 + (" 3x6 6x3 2x9 9x2 4x5 5x4 2x10 10x2 3x7 7x3 11x2 2x11 4x6 6x4 12x2 2x12 3x8 8x3 4x6 6x4 5x5")
_GRID_TABLES = {n: tuple(tuple(int(v) for v in g.split("x")) for g in s.split())
                for n, s in ((9, _GRIDS_9), (16, _GRIDS_16), (25, _GRIDS_25))}


def select_grid(h: int, w: int, patch_num: int = 9, image_size: int = 336) -> Tuple[int, int]:
    """(h_block, w_block) for an ``h x w`` image: the candidate grid maximising
    ``round(h r) round(w r) / area + 0.1 IoU(grid box, 1.4 x image box)`` with ``r`` the largest scale that fits
    the image into the grid box — evaluated in float32 tensor arithmetic exactly as the reference does
    (int64 / int64 true division -> float32, ``torch.round`` half-to-even, first maximum wins)."""
    if patch_num not in _GRID_TABLES:
        raise NotImplementedError(f"patch_num {patch_num} (the reference defines 9, 16, 25)")
    grids = _GRID_TABLES[patch_num]
    size = (image_size, image_size) if isinstance(image_size, int) else tuple(image_size)
    box = torch.tensor([[g[0] * size[0], g[1] * size[1]] for g in grids])           # int64 [n, 2] (far corner)
    area = box[:, 0] * box[:, 1]                                                      # int64
    img = torch.tensor([h, w])
    r = (box / img).min(dim=-1)[0]                                                    # float32
    score = torch.round(h * r) * torch.round(w * r) / area
    img14 = img * 1.4                                                                 # float32
    inter = torch.min(box, img14).clamp(min=0).prod(dim=-1)
    union = area + img14.prod() - inter
    score = score + inter / (union + 1e-5) * 0.1
    return grids[int(torch.argmax(score))]


def slice_plan(h: int, w: int, patch_num: int = 9, block: int = 336):
    """Sizes of the reference's HD slicing for an ``h x w`` image (train.py:699-708, 720-727):
    ``(h_block, w_block, h_res, w_res, hg, wg)`` — the grid, the size the image is resized to inside the
    ``h_block x w_block`` canvas (aspect preserved, Python ``round`` = half-to-even), and the size of the global
    view inside its single block (``0, 0`` when there is only one crop)."""
    hb, wb = select_grid(h, w, patch_num, block)

    def fit(bh, bw):
        h_ratio, w_ratio = bh / h, bw / w
        if h_ratio <= w_ratio:
            return bh, min(bw, round(w * h_ratio))
        return min(bh, round(h * w_ratio)), bw
    h_res, w_res = fit(block * hb, block * wb)
    hg, wg = fit(block, block) if hb * wb > 1 else (0, 0)
    return hb, wb, h_res, w_res, hg, wg


def slice_image(image: torch.Tensor, patch_num: int = 9, block: int = 336):
    """``image [3, H, W]`` fp32 on the GPU (normalised pixels) -> ``(crops [n, 3, block, block] fp32, h_block,
    w_block)`` exactly as the reference's data loader builds ``image_tensor`` in ``'slice'`` mode
    (train.py:695-731): resize + zero-pad + tile, plus the global view when there is more than one crop."""
    if not image.is_cuda:
        raise RuntimeError("slice_image runs only on an AMD GPU (HIP kernel); there is no CPU fallback")
    if image.dim() == 4 and image.shape[0] == 1:
        image = image[0]
    if image.dim() != 3 or image.shape[0] != 3 or image.dtype != torch.float32:
        raise ValueError("image must be a float32 [3, H, W] tensor")
    image = image.contiguous()
    H, W = int(image.shape[1]), int(image.shape[2])
    hb, wb, h_res, w_res, hg, wg = slice_plan(H, W, patch_num, block)
    n = hd_crop_count(hb, wb)
    crops = torch.empty(n, 3, block, block, dtype=torch.float32, device=image.device)
    lib = _capi.load_library()
    with torch.cuda.device(image.device):
        _capi.check(lib.tp_hd_slice(image.data_ptr(), H, W, hb, wb, h_res, w_res, hg, wg, crops.data_ptr(), block,
                                    torch.cuda.current_stream(image.device).cuda_stream), "tp_hd_slice")
    return crops, hb, wb


CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)        # the reference's Normalize (train.py:645, every eval driver)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


def normalisation_table(mean: Sequence[float] = CLIP_MEAN, std: Sequence[float] = CLIP_STD) -> torch.Tensor:
    """``[3, 256]`` fp32 on the CPU: entry ``[c, u]`` is what ``Compose([ToTensor(), Normalize(mean, std)])`` makes of byte
    ``u`` in channel ``c`` — ``fl(fl(fl(u / 255) - mean_c) / std_c)``, computed with the CPU ops torchvision itself runs, in its
    order (true divisions, not multiplications by a reciprocal).  The value depends on ``(c, u)`` only, so a lookup in this
    table IS the reference's normalisation, bit for bit."""
    mean, std = _table_key(mean, std)
    m, s = torch.tensor(mean, dtype=torch.float32), torch.tensor(std, dtype=torch.float32)
    return torch.arange(256).to(torch.float32).div(255).sub(m[:, None]).div(s[:, None])


def _table_key(mean, std):
    mean, std = tuple(float(v) for v in mean), tuple(float(v) for v in std)
    if len(mean) != 3 or len(std) != 3:
        raise ValueError("mean and std must have three entries (RGB)")
    if 0.0 in std:
        raise ValueError("std must be non-zero")
    return mean, std


_table_cache = {}


def _device_table(key, device: torch.device) -> torch.Tensor:
    """The table on ``device``: uploaded once per (mean, std, device)."""
    t = _table_cache.get((key, device))
    if t is None:
        t = _table_cache[(key, device)] = normalisation_table(*key).to(device)
    return t


_PLAN_IMAGE = np.dtype([("src_offset", "<i8"), ("H", "<i4"), ("W", "<i4"), ("row_stride", "<i4"), ("h_block", "<i4"),
                        ("w_block", "<i4"), ("h_res", "<i4"), ("w_res", "<i4"), ("hg", "<i4"), ("wg", "<i4"), ("first_crop", "<i4")])
_PIXEL_ALIGN = 16


class SliceBatchPlan(NamedTuple):
    """Host plan of one :func:`slice_images` call.  ``images``: one ``tp_hd_slice_image`` record per image (a numpy structured
    array with the C struct's layout); ``crop_image`` (int32 ``[n_crops]``): the image of every crop; ``pixel_bytes``: the size
    of the pixel buffer the offsets address."""
    images: np.ndarray
    crop_image: np.ndarray
    h_block: List[int]
    w_block: List[int]
    n_crops: int
    pixel_bytes: int

    def words(self) -> np.ndarray:
        """The plan as the bytes ``tp_hd_slice_u8`` reads: the image records, then the crop-to-image index."""
        return np.concatenate([self.images.view(np.uint8), self.crop_image.view(np.uint8)])


def slice_batch_plan(sizes: Sequence[Tuple[int, int]], patch_num: int = 9, block: int = 336,
                     row_strides: Optional[Sequence[int]] = None, offsets: Optional[Sequence[int]] = None) -> SliceBatchPlan:
    """The plan for images of ``sizes [(H, W), ...]``: grids and sizes from :func:`slice_plan`, consecutive crop ranges, and
    where each image's bytes lie.  ``row_strides`` (bytes, default ``3 W``: dense rows); ``offsets`` (byte offset of every
    image's first pixel; default: the images packed one behind the other, each on a 16-byte boundary, which is how
    :func:`slice_images` stages CPU images).  Pure host logic."""
    n = len(sizes)
    if n == 0:
        raise ValueError("slice_batch_plan: no images")
    images = np.zeros(n, dtype=_PLAN_IMAGE)
    hbs, wbs, owner, first, at = [], [], [], 0, 0
    for i, (H, W) in enumerate(sizes):
        H, W = int(H), int(W)
        if H < 1 or W < 1:
            raise ValueError(f"image {i}: size {H} x {W}")
        stride = 3 * W if row_strides is None else int(row_strides[i])
        if stride < 3 * W or stride > 0x7FFFFFFF:
            raise ValueError(f"image {i}: row stride {stride} (3 * W = {3 * W} .. 2^31 - 1)")
        hb, wb, h_res, w_res, hg, wg = slice_plan(H, W, patch_num, block)
        if min(h_res, w_res) < 1 or (hb * wb > 1 and min(hg, wg) < 1):
            raise ValueError(f"image {i}: {H} x {W} is too elongated, a resized side rounds to 0 pixels (resize {h_res} x {w_res}, "
                             f"global view {hg} x {wg}); the reference's F.interpolate refuses such an image too")
        off = at if offsets is None else int(offsets[i])
        images[i] = (off, H, W, stride, hb, wb, h_res, w_res, hg, wg, first)
        count = hd_crop_count(hb, wb)
        owner.append(np.full(count, i, dtype=np.int32))
        hbs.append(hb)
        wbs.append(wb)
        first += count
        end = off + (H - 1) * stride + 3 * W
        at = max(at, -(-end // _PIXEL_ALIGN) * _PIXEL_ALIGN)
    if first > 0x7FFFFFFF:
        raise ValueError("the batch exceeds 2^31 crops")
    return SliceBatchPlan(images, np.concatenate(owner), hbs, wbs, first, at)


def _as_hwc_uint8(img, i: int):
    """One entry of ``slice_images``' input, checked: a ``[H, W, 3]`` uint8 torch tensor or numpy array."""
    if not isinstance(img, (torch.Tensor, np.ndarray)):
        raise TypeError(f"images[{i}] must be a torch.Tensor or a numpy array, not {type(img).__name__}")
    if img.dtype != (torch.uint8 if isinstance(img, torch.Tensor) else np.uint8):
        raise TypeError(f"images[{i}] must be uint8 (raw RGB bytes), not {img.dtype}")
    if img.ndim != 3 or img.shape[2] != 3:
        raise ValueError(f"images[{i}] must be [H, W, 3] (RGB, channels last), got {tuple(img.shape)}")
    if img.shape[0] < 1 or img.shape[1] < 1:
        raise ValueError(f"images[{i}] is empty: {tuple(img.shape)}")
    return img


def slice_images(images, patch_num: int = 9, block: int = 336, dtype: torch.dtype = torch.bfloat16,
                 mean: Sequence[float] = CLIP_MEAN, std: Sequence[float] = CLIP_STD, device=None):
    """A batch of raw RGB images -> ``(crops [n_total, 3, block, block] in dtype, h_block list, w_block list)``: the
    ``images`` / ``h_block`` / ``w_block`` of a collated batch of the reference's loader in ``'slice'`` mode
    (train.py:696-731, then the driver's ``.to(dtype)``) — ToTensor + Normalize, resize, zero-pad, tile and global view of
    every image from ONE launch (``tp_hd_slice_u8``).

    ``images``: a sequence of ``[H, W, 3]`` uint8 torch tensors or numpy arrays (``np.asarray(pil.convert("RGB"))``) of any
    sizes; rows need not be contiguous.  CPU images and the plan are packed into one pinned staging buffer and travel in one
    asynchronous copy — 3 bytes per pixel; device images (all on one device) are packed with one ``torch.cat`` of their bytes.
    ``dtype``: float32, bfloat16 or float16 — one rounding at the store.  ``block`` must be a multiple of 8."""
    if isinstance(images, (torch.Tensor, np.ndarray)) or not isinstance(images, Sequence):
        raise TypeError("images must be a sequence (list / tuple) of [H, W, 3] uint8 images")
    if len(images) == 0:
        raise ValueError("images is empty")
    imgs = [_as_hwc_uint8(img, i) for i, img in enumerate(images)]
    out_dt = {torch.float32: _capi.TP_F32, torch.bfloat16: _capi.TP_BF16, torch.float16: _capi.TP_F16}.get(dtype)
    if out_dt is None:
        raise TypeError("dtype must be float32, bfloat16 or float16")
    if block < 8 or block % 8 != 0:
        raise ValueError(f"block = {block} must be a positive multiple of 8 (a lane stores 8 consecutive pixels)")
    on_dev = [isinstance(img, torch.Tensor) and img.is_cuda for img in imgs]
    if any(on_dev) and not all(on_dev):
        raise ValueError("images must all be on the CPU or all on one device")
    sizes = [(int(img.shape[0]), int(img.shape[1])) for img in imgs]
    table_key = _table_key(mean, std)
    if not torch.cuda.is_available():
        raise RuntimeError("slice_images runs only on an AMD GPU (HIP kernel); there is no CPU fallback")
    if not _capi.hd_slice_u8_supported():
        raise RuntimeError("the loaded libtokenpacker_hip.so lacks tp_hd_slice_u8; rebuild it")
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
        plan = slice_batch_plan(sizes, patch_num, block, strides, offsets)._replace(pixel_bytes=at)
    else:
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        plan = slice_batch_plan(sizes, patch_num, block)
    words = plan.words()
    pix_base = -(-words.size // _PIXEL_ALIGN) * _PIXEL_ALIGN
    staging = torch.empty(pix_base + (0 if on_dev[0] else plan.pixel_bytes), dtype=torch.uint8, pin_memory=True)
    stage_np = staging.numpy()
    stage_np[:words.size] = words
    if not on_dev[0]:
        for img, rec, (H, W) in zip(imgs, plan.images, sizes):
            at = pix_base + int(rec["src_offset"])
            np.copyto(stage_np[at:at + H * W * 3].reshape(H, W, 3), img.numpy() if isinstance(img, torch.Tensor) else img)
    crops = torch.empty(plan.n_crops, 3, block, block, dtype=dtype, device=dev)
    lib = _capi.load_library()
    with torch.cuda.device(dev):
        lut = _device_table(table_key, dev)
        staged_dev = staging.to(dev, non_blocking=True)                 # the one host -> device copy: plan (+ pixels)
        pixels = torch.cat(pieces) if on_dev[0] else staged_dev[pix_base:]
        _capi.check(lib.tp_hd_slice_u8(stage_np.ctypes.data, staged_dev.data_ptr(), len(imgs), pixels.data_ptr(), plan.pixel_bytes,
                                       lut.data_ptr(), crops.data_ptr(), plan.n_crops, block, out_dt,
                                       torch.cuda.current_stream(dev).cuda_stream), "tp_hd_slice_u8")
    return crops, list(plan.h_block), list(plan.w_block)


def hd_token_rows(h_block: int, w_block: int, num_queries: int) -> int:
    """Rows of one image's visual-token block: ``h*w`` crops of ``M`` tokens, a separator after every crop
    (',' inside a row, '\\n' at its end), and — when there is more than one crop — the global view + '\\n'."""
    n = h_block * w_block
    return n * (num_queries + 1) + ((num_queries + 1) if n > 1 else 0)


def hd_crop_count(h_block: int, w_block: int) -> int:
    n = h_block * w_block
    return n + (1 if n > 1 else 0)


def assemble_hd_tokens(image_features: torch.Tensor, h_block: Sequence[int], w_block: Sequence[int],
                       sep_embed: torch.Tensor, ret_embed: torch.Tensor, out: Optional[torch.Tensor] = None,
                       out_rows: Optional[Sequence[int]] = None, crop_map: Optional[torch.Tensor] = None) -> List[torch.Tensor]:
    """``image_features [n_crops, M, D]`` (projector output for all crops of the batch, crops of image 0 first,
    row-major inside an image, global view last) -> list of per-image ``[rows_i, D]`` views of one buffer, equal
    to the reference's ``cur_image_features`` for each image.

    With ``out [rows, D]`` and ``out_rows`` (first row of each image's block, increasing) the blocks are written
    INTO a caller-owned buffer — e.g. the flattened ``inputs_embeds`` with the text embeddings already in place
    (llava_arch.py:172-191) — and everything between the blocks is left untouched: the visual tokens land where
    the LLM reads them, with no per-image ``torch.cat``.

    ``crop_map`` (int32 device tensor, one entry per crop): crop c is row block ``crop_map[c]`` of ``image_features``
    — the b_max-strided buffer of a ragged all-gather (``shard.GatheredTokens.buf`` / ``.crop_map()``) is read in
    place instead of being compacted first.

    Differentiable with respect to ``image_features``, ``sep_embed`` and ``ret_embed``: with a gradient live on any of
    them (or on ``out``) the launch is an autograd node whose backward is ``tp_hd_assemble_backward`` — dL/dfeatures is a
    copy of the incoming rows (zero for crops no block reads), dL/dsep and dL/dret are fp32 sums in a fixed order.  With
    ``out`` it behaves like the in-place ``out[block rows] = block``: ``out``'s earlier content gets the incoming gradient
    with the block rows zeroed.  A ``crop_map`` is then copied to the host once and must be injective (``ValueError``).
    Nothing live (``torch.no_grad()`` or no input requiring grad): one launch, no synchronisation."""
    if not image_features.is_cuda:
        raise RuntimeError("assemble_hd_tokens runs only on an AMD GPU (HIP kernel); there is no CPU fallback")
    live = torch.is_grad_enabled() and (image_features.requires_grad or sep_embed.requires_grad or ret_embed.requires_grad
                                        or (out is not None and out.requires_grad))
    if image_features.dim() != 3:
        raise ValueError("image_features must be [n_crops, M, D]")
    if len(h_block) != len(w_block):
        raise ValueError("h_block and w_block must have one entry per image")
    n_crops, M, D = image_features.shape
    if crop_map is not None:
        if crop_map.dtype != torch.int32 or crop_map.dim() != 1 or crop_map.device != image_features.device \
                or not crop_map.is_contiguous():
            raise ValueError("crop_map must be a contiguous int32 vector on the features' device")
        n_crops = crop_map.numel()
    dt = {torch.bfloat16: _capi.TP_BF16, torch.float16: _capi.TP_F16}.get(image_features.dtype)
    if dt is None:
        raise TypeError("image_features must be bfloat16 or float16")
    feats = image_features.contiguous()
    sep = sep_embed.reshape(-1).to(device=feats.device, dtype=feats.dtype).contiguous()
    ret = ret_embed.reshape(-1).to(device=feats.device, dtype=feats.dtype).contiguous()
    if sep.numel() != D or ret.numel() != D:
        raise ValueError(f"separator embeddings must have {D} elements")
    if (out is None) != (out_rows is None):
        raise ValueError("pass `out` and `out_rows` together")
    if out_rows is not None and len(out_rows) != len(h_block):
        raise ValueError("out_rows must have one entry per image")
    plan = (_capi.tp_hd_image * len(h_block))()
    first, row, spans = 0, 0, []
    for i, (hb, wb) in enumerate(zip(h_block, w_block)):
        hb, wb = int(hb), int(wb)
        if hb < 1 or wb < 1:
            raise ValueError("h_block / w_block must be >= 1")
        if out_rows is not None:
            if int(out_rows[i]) < row:
                raise ValueError(f"out_rows[{i}] = {int(out_rows[i])} overlaps the previous image's block (ends at {row})")
            row = int(out_rows[i])
        plan[i] = _capi.tp_hd_image(first, hb, wb, 0, row)
        rows = hd_token_rows(hb, wb, M)
        spans.append((row, rows))
        first += hd_crop_count(hb, wb)
        row += rows
    if first != n_crops:
        raise ValueError(f"h_block/w_block describe {first} crops, image_features holds {n_crops}")
    if out is None:
        out = torch.empty(row, D, dtype=feats.dtype, device=feats.device)
    else:
        if out.dim() != 2 or out.shape[1] != D or out.dtype != feats.dtype or out.device != feats.device \
                or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous [rows, {D}] {feats.dtype} tensor on {feats.device}")
        if row > out.shape[0]:
            raise ValueError(f"the last image's block ends at row {row}, out has {out.shape[0]} rows")
    spec = _AssembleSpec(plan, len(h_block), n_crops, crop_map, spans, M, D, dt)
    if not live:
        _assemble_launch(spec, feats, sep, ret, out)
        return [out[a:a + n] for a, n in spans]
    if out is not None and out.is_leaf and out.requires_grad:
        raise RuntimeError("a leaf Variable that requires grad is being used in an in-place operation (out=)")
    if crop_map is not None:
        cm = crop_map.cpu()
        if int(cm.min()) < 0 or int(cm.max()) >= feats.shape[0]:
            raise ValueError(f"crop_map values must lie in [0, {feats.shape[0]})")
        if torch.unique(cm).numel() != cm.numel():
            raise ValueError("crop_map must be injective when a gradient is live (two crops would share one gradient row)")
    out = _AssembleFn.apply(feats, sep, ret, out, spec)
    return [out[a:a + n] for a, n in spans]


class _AssembleSpec:
    """What one tp_hd_assemble call and its backward share: the host plan and the shapes."""

    def __init__(self, plan, n_images, n_crops, crop_map, spans, M, D, dt):
        self.plan, self.n_images, self.n_crops, self.crop_map = plan, n_images, n_crops, crop_map
        self.spans, self.M, self.D, self.dt = spans, M, D, dt


def _assemble_launch(spec: _AssembleSpec, feats, sep, ret, out) -> None:
    lib = _capi.load_library()
    with torch.cuda.device(feats.device):
        _capi.check(lib.tp_hd_assemble(spec.plan, spec.n_images, feats.data_ptr(), spec.n_crops,
                                       spec.crop_map.data_ptr() if spec.crop_map is not None else None, sep.data_ptr(),
                                       ret.data_ptr(), out.data_ptr(), out.shape[0], spec.M, spec.D, spec.dt,
                                       torch.cuda.current_stream(feats.device).cuda_stream),
                    "tp_hd_assemble")


def _assemble_backward(spec: _AssembleSpec, dout: torch.Tensor, n_token_crops: int):
    """-> (dtokens [n_token_crops, M, D], dsep [D], dret [D]) from one tp_hd_assemble_backward call."""
    lib = _capi.load_library()
    dev, M, D = dout.device, spec.M, spec.D
    dtok = torch.empty(n_token_crops, M, D, dtype=dout.dtype, device=dev)
    dsep = torch.empty(D, dtype=dout.dtype, device=dev)
    dret = torch.empty(D, dtype=dout.dtype, device=dev)
    ws = torch.empty(lib.tp_hd_assemble_backward_workspace_bytes(spec.n_images, n_token_crops, D), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _capi.check(lib.tp_hd_assemble_backward(spec.plan, spec.n_images, dout.data_ptr(), dout.shape[0], spec.n_crops,
                                                spec.crop_map.data_ptr() if spec.crop_map is not None else None,
                                                dtok.data_ptr(), n_token_crops, dsep.data_ptr(), dret.data_ptr(), M, D, spec.dt,
                                                ws.data_ptr(), ws.numel(), torch.cuda.current_stream(dev).cuda_stream),
                    "tp_hd_assemble_backward")
    return dtok, dsep, dret


class _AssembleFn(torch.autograd.Function):
    """``out[block rows] = assembled blocks`` as one autograd node (``out`` is modified in place and returned)."""

    @staticmethod
    def forward(ctx, feats, sep, ret, out, spec):
        _assemble_launch(spec, feats, sep, ret, out)
        ctx.spec, ctx.n_token_crops = spec, feats.shape[0]
        ctx.mark_dirty(out)
        return out

    @staticmethod
    def backward(ctx, g):
        spec = ctx.spec
        g = g.contiguous()
        dfeats = dsep = dret = dprev = None
        need_f, need_s, need_r, need_o = ctx.needs_input_grad[:4]
        if need_f or need_s or need_r:
            dtok, ds, dr = _assemble_backward(spec, g, ctx.n_token_crops)
            dfeats, dsep, dret = (dtok if need_f else None), (ds if need_s else None), (dr if need_r else None)
        if need_o:
            rows = torch.cat([torch.arange(a, a + n) for a, n in spec.spans]).to(g.device)
            dprev = g.index_fill(0, rows, 0)
        return dfeats, dsep, dret, dprev, None


def splice_layout(input_ids: torch.Tensor, h_block: Sequence[int], w_block: Sequence[int], num_queries: int,
                  image_token_index: int = -200):
    """Host-side layout of ``new_input_embeds`` in ``mode == 'slice'`` (llava_arch.py:115-207): for ``input_ids [B, L]``
    returns ``(max_len, text_src, text_dst, img_plan, n_crops)`` — flat source positions (``b * L + pos``) of the text
    tokens, their flat destination rows (``b * max_len + row``), one ``(dest_row, first_crop, h_block, w_block)`` per image
    token in (sample, position) order, and the number of crop indices consumed (a sample without an image token still
    consumes one, :124-134).  Pure integer logic, no device work."""
    return _splice_layout(input_ids, h_block, w_block, num_queries, image_token_index)[:5]


def _splice_layout(input_ids, h_block, w_block, num_queries, image_token_index):
    """:func:`splice_layout` plus the per-sample lengths of ``new_input_embeds`` before padding."""
    ids = input_ids.detach().cpu().tolist()
    per_sample, lengths, crop = [], [], 0
    for b, row_ids in enumerate(ids):
        hb, wb = int(h_block[b]), int(w_block[b])
        segs, row, has_img = [], 0, False
        for pos, tok in enumerate(row_ids):
            if tok == image_token_index:
                has_img = True
                segs.append(("img", row, crop, hb, wb))
                row += hd_token_rows(hb, wb, num_queries)
                crop += hd_crop_count(hb, wb)
            else:
                segs.append(("txt", row, pos))
                row += 1
        if not has_img:
            crop += 1                                     # llava_arch.py:124-134: cur_image_idx += 1
        per_sample.append(segs)
        lengths.append(row)
    L_in, L = (len(ids[0]) if ids else 0), (max(lengths) if lengths else 0)
    text_src, text_dst, img_plan = [], [], []
    for b, segs in enumerate(per_sample):
        for seg in segs:
            if seg[0] == "txt":
                text_src.append(b * L_in + seg[2])
                text_dst.append(b * L + seg[1])
            else:
                img_plan.append((b * L + seg[1], seg[2], seg[3], seg[4]))
    return L, text_src, text_dst, img_plan, crop, lengths


def build_inputs_embeds(input_ids: torch.Tensor, embed_tokens, image_features: torch.Tensor, h_block: Sequence[int],
                        w_block: Sequence[int], sep_id: int, ret_id: int, image_token_index: int = -200,
                        crop_map: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``new_input_embeds [B, max_len, D]`` of the reference's ``prepare_inputs_labels_for_multimodal`` in
    ``mode == 'slice'`` (``llava_arch.py:115-207``, default flags), with the visual tokens LANDING IN PLACE.

    The reference walks every sample in Python, embeds text pieces one by one, builds each image's block with a
    loop + ``torch.cat`` (:140-154), concatenates per sample (:190-191) and pads (:193-200).  Here the layout is
    computed once on the host from ``input_ids`` (a tiny D2H copy — the reference synchronises per sample too),
    ALL text tokens of the batch are embedded by one ``embed_tokens`` call and scattered into a zero-initialised
    ``[B * max_len, D]`` buffer, and ONE ``tp_hd_assemble`` launch writes every image block into its rows of that
    same buffer (gaps — the text rows — are left untouched).  ``image_features [n_crops, M, D]`` may be the
    b_max-strided buffer of a ragged all-gather, read through ``crop_map`` (``shard.GatheredTokens``).
    Every image token of sample b uses the grid ``h_block[b] x w_block[b]``; a sample without an image token still
    consumes one crop index, as in the reference (:124-134).  Labels and the attention mask: :func:`build_multimodal_inputs`.

    Differentiable with respect to ``image_features`` and ``embed_tokens`` (see :func:`assemble_hd_tokens`): the text
    rows and the ',' / '\\n' embeddings (one more ``embed_tokens`` call for ``[sep_id, ret_id]``) reach the table through
    autograd of those two calls.  The values are the same with and without a live gradient."""
    if not image_features.is_cuda:
        raise RuntimeError("build_inputs_embeds runs only on an AMD GPU (HIP kernel); there is no CPU fallback")
    ids_cpu = input_ids.detach().cpu()
    if ids_cpu.dim() != 2 or len(h_block) != ids_cpu.shape[0] or len(w_block) != ids_cpu.shape[0]:
        raise ValueError("input_ids must be [B, L] with one h_block / w_block entry per sample")
    layout = _splice_layout(ids_cpu, h_block, w_block, image_features.shape[1], image_token_index)
    return _embeds_from_layout(input_ids, ids_cpu, layout, embed_tokens, image_features, sep_id, ret_id, crop_map)


def _embeds_from_layout(input_ids, ids_cpu, layout, embed_tokens, image_features, sep_id, ret_id, crop_map):
    M, D = image_features.shape[1], image_features.shape[2]
    device, dtype = image_features.device, image_features.dtype
    L, text_src, text_dst, img_plan, crop = layout[:5]
    n_logical = crop_map.numel() if crop_map is not None else image_features.shape[0]
    if crop != n_logical:
        raise ValueError(f"input_ids / h_block / w_block describe {crop} crops, image_features holds {n_logical}")
    out = torch.zeros(ids_cpu.shape[0] * L, D, dtype=dtype, device=device)
    ids_dev = input_ids.to(device).reshape(-1)
    if text_src:
        src = torch.tensor(text_src, dtype=torch.long, device=device)
        dst = torch.tensor(text_dst, dtype=torch.long, device=device)
        out.index_copy_(0, dst, embed_tokens(ids_dev.index_select(0, src)).to(dtype))
    if img_plan:
        seps = embed_tokens(torch.tensor([sep_id, ret_id], dtype=ids_dev.dtype, device=device)).to(dtype)
        # the plan entries are in (sample, position) order = increasing rows and crops: what tp_hd_assemble requires
        hbs, wbs, rows = [p[2] for p in img_plan], [p[3] for p in img_plan], [p[0] for p in img_plan]
        if crop_map is None and all(p[1] == sum(hd_crop_count(a, c) for a, c in zip(hbs[:i], wbs[:i])) for i, p in enumerate(img_plan)):
            assemble_hd_tokens(image_features, hbs, wbs, seps[0], seps[1], out=out, out_rows=rows)
        else:
            # crops skipped by image-less samples (or a ragged gather buffer): address every crop through a map
            first = torch.tensor([p[1] for p in img_plan])
            logical = torch.cat([torch.arange(int(f), int(f) + hd_crop_count(a, c)) for f, a, c in zip(first, hbs, wbs)])
            cmap = logical.to(device=device, dtype=torch.int32)
            if crop_map is not None:
                cmap = crop_map.index_select(0, cmap.long()).contiguous()
            assemble_hd_tokens(image_features, hbs, wbs, seps[0], seps[1], out=out, out_rows=rows, crop_map=cmap)
    return out.view(ids_cpu.shape[0], L, D)


IGNORE_INDEX = -100           # llava/constants.py


def splice_labels_and_mask(input_ids: torch.Tensor, h_block: Sequence[int], w_block: Sequence[int], num_queries: int,
                           labels: Optional[torch.Tensor] = None, attention_mask: Optional[torch.Tensor] = None,
                           image_token_index: int = -200, _layout=None):
    """``(attention_mask, new_labels)`` of ``prepare_inputs_labels_for_multimodal`` in ``mode == 'slice'``
    (``llava_arch.py:119-231``, default flags) — plain torch on the device of ``labels`` / ``attention_mask`` (CPU too).

    ``new_labels [B, max_len]``: every text token keeps its label, every row of an image block is ``IGNORE_INDEX``
    (:176), a sample without an image token keeps its labels (:129-130), and shorter samples are padded on the right with
    ``IGNORE_INDEX`` (:206-212).  ``attention_mask [B, max_len]``: ``True`` for the ``len_b - L`` rows the images added,
    then the given mask, then ``False`` up to ``max_len`` (:214-221 ragged, :228-230 equal lengths — the same rule).
    Either output is ``None`` when its input is.  Ragged lengths with an ``attention_mask`` but no ``labels`` raise
    ``ValueError``: the reference reads an unbound ``_new_labels`` there (:216)."""
    ids_cpu = input_ids.detach().cpu()
    B, L_in = ids_cpu.shape
    layout = _layout if _layout is not None else _splice_layout(ids_cpu, h_block, w_block, num_queries, image_token_index)
    L, text_src, text_dst, lengths = layout[0], layout[1], layout[2], layout[5]
    ragged = any(n != lengths[0] for n in lengths)
    if ragged and attention_mask is not None and labels is None:
        raise ValueError("ragged lengths with an attention_mask need labels (the reference reads an unbound _new_labels, "
                         "llava_arch.py:216)")
    new_labels = new_mask = None
    if labels is not None:
        if tuple(labels.shape) != (B, L_in):
            raise ValueError(f"labels must be [{B}, {L_in}] like input_ids")
        dev = labels.device
        new_labels = torch.full((B * L,), IGNORE_INDEX, dtype=labels.dtype, device=dev)
        if text_src:
            new_labels[torch.tensor(text_dst, dtype=torch.long, device=dev)] = \
                labels.reshape(-1).index_select(0, torch.tensor(text_src, dtype=torch.long, device=dev))
        new_labels = new_labels.view(B, L)
    if attention_mask is not None:
        if tuple(attention_mask.shape) != (B, L_in):
            raise ValueError(f"attention_mask must be [{B}, {L_in}] like input_ids")
        dev = attention_mask.device
        left = torch.tensor([n - L_in for n in lengths], dtype=torch.long, device=dev)
        src = torch.arange(L, device=dev).unsqueeze(0) - left.unsqueeze(1)                 # [B, L] position in the given mask
        inside = (src >= 0) & (src < L_in)
        given = attention_mask.gather(1, src.clamp(0, max(L_in - 1, 0))) if L_in > 0 else attention_mask.new_zeros(B, L)
        new_mask = torch.where(inside, given, (src < 0).to(attention_mask.dtype))
    return new_mask, new_labels


def build_multimodal_inputs(input_ids: torch.Tensor, embed_tokens, image_features: torch.Tensor, h_block: Sequence[int],
                            w_block: Sequence[int], sep_id: int, ret_id: int, labels: Optional[torch.Tensor] = None,
                            attention_mask: Optional[torch.Tensor] = None, image_token_index: int = -200,
                            crop_map: Optional[torch.Tensor] = None):
    """``(attention_mask, inputs_embeds, labels)``: elements 1, 3 and 4 of what the reference's
    ``prepare_inputs_labels_for_multimodal`` returns in ``mode == 'slice'`` (``llava_arch.py:100-233``) — the slice
    branch of a TokenPacker-HD training step (``scripts/v1_5/{pretrain,finetune}_hd.sh``) between the projector and the LLM.

    ``inputs_embeds`` is :func:`build_inputs_embeds` (differentiable with respect to ``image_features`` and
    ``embed_tokens``); labels and mask come from :func:`splice_labels_and_mask`.  The layout is computed once.

    Out of scope: the ``tune_mm_mlp_adapter and mm_use_im_start_end`` branch that detaches the text embeddings
    (:161-165, :178-185; both HD scripts set ``mm_use_im_start_end False``), and the decode-step early return (:104-107)
    — call this only for a prompt with images."""
    if not image_features.is_cuda:
        raise RuntimeError("build_multimodal_inputs runs only on an AMD GPU (HIP kernel); there is no CPU fallback")
    ids_cpu = input_ids.detach().cpu()
    if ids_cpu.dim() != 2 or len(h_block) != ids_cpu.shape[0] or len(w_block) != ids_cpu.shape[0]:
        raise ValueError("input_ids must be [B, L] with one h_block / w_block entry per sample")
    layout = _splice_layout(ids_cpu, h_block, w_block, image_features.shape[1], image_token_index)
    mask, new_labels = splice_labels_and_mask(ids_cpu, h_block, w_block, image_features.shape[1], labels, attention_mask,
                                              image_token_index, _layout=layout)
    embeds = _embeds_from_layout(input_ids, ids_cpu, layout, embed_tokens, image_features, sep_id, ret_id, crop_map)
    return mask, embeds, new_labels
