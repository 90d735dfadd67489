"""The splice of text and visual tokens between the projector and the LLM — ``prepare_inputs_labels_for_multimodal`` of the
reference (``llava/model/llava_arch.py:100-233``) — as ONE launch, for the default mode and for ``mode == 'slice'``.

The reference walks every sample in Python: two or more ``embed_tokens`` calls, several ``torch.cat`` and a pad per sample,
per-sample label and mask tensors, and one device round trip per sample (``torch.where(...)[0]``).  Here the layout is computed
once on the host from ``input_ids`` (:func:`splice_layout`, numpy integer logic) as one int32 code per output row, and one
gather kernel (``tp_splice``) writes every row of ``inputs_embeds`` exactly once — from the embedding table (the id is read on
the device), from the projector output, or zeros — together with ``labels`` and ``attention_mask``.  No zero-fill pass, no
temporary for the text embeddings.

:func:`build_multimodal_inputs` is differentiable with respect to the projector output and the embedding table
(``tp_splice_backward``): the feature gradient is a copy of the incoming rows, the table gradient is dense ``[V, D]`` like
``nn.Embedding``'s, summed in fp32 in a fixed order without atomics.  A frozen table (stage-1 pre-training) costs nothing.

The row plan belongs to one batch and is rebuilt on the host for every call, so a call CANNOT be captured in a HIP graph
and replayed for other ``input_ids``.  ``input_ids`` on the CPU: no device-to-host copy at all; on the device: one copy.
Host to device, per call: one asynchronous copy of a pinned staging buffer (the plan, for a trainable table the sorted order,
and the ids when they live on the CPU); ``labels`` or an ``attention_mask`` on the CPU cost one more copy each.  Host work per
call is the layout, for a trainable table a radix sort of the ids, and the C validation of the plan (forward and backward):
about 0.1 ms at B = 1 and 1 ms at 30 000 rows, more than the kernels take (``profiles/README.md``).
``hd.build_multimodal_inputs`` (the composed slice path) is unchanged; this module does not route through it.
"""
from __future__ import annotations

import ctypes
from functools import lru_cache
from typing import NamedTuple, Optional, Sequence

import numpy as np
import torch

from . import _capi
from .hd import IGNORE_INDEX, hd_crop_count, hd_token_rows  # noqa: F401  (IGNORE_INDEX: what the kernel writes)

_TEXT, _LITERAL, _FEATURE, _PAD = (np.uint32(k << 30) for k in range(4))
_PAYLOAD = np.uint32(0x3FFFFFFF)
SEP, RET = 0, 1                      # symbolic payloads of the ',' and '\n' rows in SpliceLayout.codes


class SpliceLayout(NamedTuple):
    """Host-side layout of one batch.  ``codes`` (uint32 ``[batch * max_len]``): ``kind << 30 | payload`` per output row —
    kind 0 text (payload: flat position ``b * in_len + pos``), 1 separator (payload :data:`SEP` or :data:`RET`, slice mode
    only), 2 feature (payload ``block * M + token``), 3 padding.  ``lengths`` (int32 ``[batch]``): rows of every sample
    before padding.  ``n_blocks``: feature blocks consumed (an image-less sample consumes one, llava_arch.py:124-131)."""
    batch: int
    in_len: int
    max_len: int
    num_queries: int
    lengths: np.ndarray
    codes: np.ndarray
    n_blocks: int

    def kinds(self) -> np.ndarray:
        return (self.codes >> np.uint32(30)).astype(np.int64)

    def payloads(self) -> np.ndarray:
        return (self.codes & _PAYLOAD).astype(np.int64)


@lru_cache(maxsize=64)
def _image_block(mode, hb: int, wb: int, M: int):
    """(codes of one image's rows relative to its first feature block, feature blocks it reads)."""
    if mode != "slice":
        return _FEATURE | np.arange(M, dtype=np.uint32), 1
    n, seg = hb * wb, M + 1
    rel = np.empty(hd_token_rows(hb, wb, M), dtype=np.uint32)
    tok = np.arange(M, dtype=np.uint32)
    for s in range(n):
        rel[s * seg:s * seg + M] = _FEATURE | (np.uint32(s * M) + tok)
        rel[s * seg + M] = _LITERAL | np.uint32(RET if s % wb == wb - 1 else SEP)
    if n > 1:
        rel[n * seg:n * seg + M] = _FEATURE | (np.uint32(n * M) + tok)
        rel[n * seg + M] = _LITERAL | np.uint32(RET)
    return rel, hd_crop_count(hb, wb)


def splice_layout(input_ids, num_queries: int, mode: Optional[str] = None, h_block: Optional[Sequence[int]] = None,
                  w_block: Optional[Sequence[int]] = None, image_token_index: int = -200) -> SpliceLayout:
    """Layout of ``new_input_embeds`` for ``input_ids [B, L]`` (llava_arch.py:119-207, default flags).  In the default mode an
    image token becomes the ``num_queries`` rows of the next feature block; with ``mode == 'slice'`` it becomes the
    ``hd.hd_token_rows(h_block[b], w_block[b], num_queries)`` rows of the HD block (crops, ',' and '\\n' rows, global view).
    A sample without an image token keeps its rows and still consumes one feature block.  Pure host integer logic."""
    ids = input_ids.detach().cpu().numpy() if isinstance(input_ids, torch.Tensor) else np.asarray(input_ids)
    if ids.ndim != 2:
        raise ValueError("input_ids must be [B, L]")
    B, L_in = ids.shape
    M = int(num_queries)
    if M < 1:
        raise ValueError("num_queries must be >= 1")
    if mode == "slice":
        if h_block is None or w_block is None or len(h_block) != B or len(w_block) != B:
            raise ValueError("mode 'slice' needs one h_block / w_block entry per sample")
        grids = [(int(h), int(w)) for h, w in zip(h_block, w_block)]
        if any(h < 1 or w < 1 for h, w in grids):
            raise ValueError("h_block / w_block must be >= 1")
    else:
        grids = [(1, 1)] * B
    blocks = [_image_block(mode, h, w, M) for h, w in grids]
    is_img = ids == image_token_index
    n_img = is_img.sum(axis=1)
    rows_per = np.array([len(rel) for rel, _ in blocks], dtype=np.int64)
    lengths = L_in - n_img + n_img * rows_per
    L = int(lengths.max()) if B else 0
    # row of every input position inside its sample: the images before it each add rows_per - 1 rows
    before = np.cumsum(is_img, axis=1) - is_img
    dst = np.arange(L_in)[None, :] + before * (rows_per[:, None] - 1) + (np.arange(B) * L)[:, None]
    codes = np.full(B * L, _PAD, dtype=np.uint32)
    text = ~is_img
    codes[dst[text]] = _TEXT | np.nonzero(text.reshape(-1))[0].astype(np.uint32)
    block = 0
    img_b, img_pos = np.nonzero(is_img)
    at = 0
    for b in range(B):
        rel, cc = blocks[b]
        if n_img[b] == 0:
            block += 1
            continue
        feat = (rel >> np.uint32(30)) == 2
        for _ in range(int(n_img[b])):
            start = dst[img_b[at], img_pos[at]]
            codes[start:start + len(rel)] = rel + feat * np.uint32(block * M)
            block += cc
            at += 1
    if B * max(L, L_in) > int(_PAYLOAD) or block * M > int(_PAYLOAD):
        raise ValueError("the batch exceeds 2^30 rows")
    return SpliceLayout(B, L_in, L, M, lengths.astype(np.int32), codes, block)


def _resolve_table(embed_tokens, feats):
    """-> (weight [V, D], padding_idx or -1), or the refusals of the module contract."""
    padding_idx = -1
    if isinstance(embed_tokens, torch.nn.Embedding):
        if embed_tokens.max_norm is not None:
            raise TypeError("embed_tokens.max_norm is set: the lookup would renormalise the table in place; not supported")
        if embed_tokens.sparse:
            raise TypeError("embed_tokens.sparse = True: the table gradient here is dense [V, D]")
        if embed_tokens.scale_grad_by_freq:
            raise TypeError("embed_tokens.scale_grad_by_freq = True is not supported")
        w = embed_tokens.weight
        if embed_tokens.padding_idx is not None:
            padding_idx = int(embed_tokens.padding_idx)
        expected = (embed_tokens.num_embeddings, embed_tokens.embedding_dim)
    elif isinstance(embed_tokens, torch.Tensor):
        w, expected = embed_tokens, None
    else:
        raise TypeError(f"embed_tokens must be an nn.Embedding or its weight tensor, not {type(embed_tokens).__name__}")
    if w.numel() == 0 or w.dim() != 2 or (expected is not None and tuple(w.shape) != expected):
        raise RuntimeError(
            f"the embedding weight has shape {tuple(w.shape)}" + (f" (expected {expected})" if expected else "") + ": the parameter "
            "looks partitioned (DeepSpeed ZeRO-3?).  The splice reads the table directly and does not trigger per-submodule gather "
            "hooks; use ZeRO-2, or wrap the call in deepspeed.zero.GatheredParameters([embed_tokens.weight]).")
    if w.dtype != feats.dtype:
        raise TypeError(f"the embedding table is {w.dtype}, image_features are {feats.dtype}: they must share one dtype")
    if not w.is_contiguous():
        raise TypeError("the embedding table must be contiguous")
    return w, padding_idx


class _Spec:
    """What one tp_splice call and its backward share: the plan (host and device copies) and the argument struct."""


def _launch(spec: "_Spec", feats, table) -> torch.Tensor:
    """Allocate inputs_embeds [B * L, D] and enqueue the one launch that fills it (and spec's labels / mask buffers)."""
    lib = _capi.load_library()
    a = spec.args
    out = torch.empty(a.batch * a.out_len, a.D, dtype=feats.dtype, device=feats.device)
    a.out = out.data_ptr()
    with torch.cuda.device(feats.device):
        _capi.check(lib.tp_splice(ctypes.byref(a), torch.cuda.current_stream(feats.device).cuda_stream), "tp_splice")
    return out


class _SpliceFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feats, table, spec):
        ctx.spec = spec                               # (holds no tensor with a grad_fn: no reference cycle through the graph)
        return _launch(spec, feats, table)

    @staticmethod
    def backward(ctx, g):
        spec = ctx.spec
        need_f, need_t = ctx.needs_input_grad[:2]
        if not (need_f or need_t):
            return None, None, None
        lib = _capi.load_library()
        g = g.contiguous()
        dev = g.device
        a = _capi.tp_splice_args.from_buffer_copy(spec.args)
        a.dout = g.data_ptr()
        dfeats = dtable = ws = None
        if need_f:
            dfeats = torch.empty(spec.feats_shape, dtype=g.dtype, device=dev)
            ws = torch.empty(lib.tp_splice_backward_workspace_bytes(spec.feats_shape[0], spec.feats_shape[1]), dtype=torch.uint8, device=dev)
            a.dfeats, a.workspace, a.workspace_bytes = dfeats.data_ptr(), ws.data_ptr(), ws.numel()
        if need_t:                                    # (a frozen table: nothing is allocated or launched for it)
            dtable = torch.empty(spec.table_shape, dtype=g.dtype, device=dev)
            a.dtable = dtable.data_ptr()
        with torch.cuda.device(dev):
            _capi.check(lib.tp_splice_backward(ctypes.byref(a), torch.cuda.current_stream(dev).cuda_stream), "tp_splice_backward")
        return dfeats, dtable, None


def build_multimodal_inputs(input_ids: torch.Tensor, embed_tokens, image_features: torch.Tensor,
                            labels: Optional[torch.Tensor] = None, attention_mask: Optional[torch.Tensor] = None, *,
                            mode: Optional[str] = None, h_block: Optional[Sequence[int]] = None,
                            w_block: Optional[Sequence[int]] = None, sep_id: Optional[int] = None, ret_id: Optional[int] = None,
                            image_token_index: int = -200, crop_map: Optional[torch.Tensor] = None):
    """``(attention_mask, inputs_embeds, labels)``: elements 1, 3 and 4 of what the reference's
    ``prepare_inputs_labels_for_multimodal`` returns (``llava_arch.py:100-233``), in the default mode (``mode`` anything but
    ``'slice'``: what ``scripts/v1_5/pretrain.sh`` / ``finetune.sh``, the eval loaders and ``serve/cli.py`` run) or in
    ``mode == 'slice'`` (then ``h_block``, ``w_block``, ``sep_id``, ``ret_id`` are required) — one ``tp_splice`` launch.

    ``embed_tokens``: the LLM's ``nn.Embedding`` or its weight ``[V, D]`` (same dtype as ``image_features``, contiguous).
    ``image_features [n, M, D]``: the projector output, bf16 / fp16 on the GPU; ``crop_map`` as in ``hd.assemble_hd_tokens``.
    ``labels`` (int64) and ``attention_mask`` (bool or int64) are ``[B, L]`` like ``input_ids``; either output is ``None`` when
    its input is.  ``input_ids`` may live on the CPU (then nothing is copied from the device) or on the device (one copy).

    With a gradient live on ``image_features`` or the table the call is one autograd node (``tp_splice_backward``): the
    feature gradient is a copy of the incoming rows (zero for a block no sample reads), the table gradient is dense, an
    fp32 sum in increasing row order rounded once, zero in the ``padding_idx`` row; the values are the same with and without
    a live gradient.  A ``crop_map`` must then be injective (``ValueError``).  Not capturable in a graph (module docstring).

    Out of scope, as in ``hd.build_multimodal_inputs``: the ``tune_mm_mlp_adapter and mm_use_im_start_end`` branch
    (:161-165, :178-185) and the decode-step early return (:104-107)."""
    if not isinstance(image_features, torch.Tensor) or image_features.dim() != 3:
        raise ValueError("image_features must be [n, M, D]")
    table, padding_idx = _resolve_table(embed_tokens, image_features)
    dt = {torch.bfloat16: _capi.TP_BF16, torch.float16: _capi.TP_F16}.get(image_features.dtype)
    if dt is None:
        raise TypeError("image_features must be bfloat16 or float16")
    n_blocks, M, D = image_features.shape
    V = table.shape[0]
    if table.shape[1] != D:
        raise ValueError(f"the embedding table has {table.shape[1]} columns, image_features have {D}")
    if input_ids.dim() != 2 or input_ids.numel() == 0:
        raise ValueError("input_ids must be a non-empty [B, L]")
    if mode == "slice" and (sep_id is None or ret_id is None):
        raise ValueError("mode 'slice' needs sep_id and ret_id (the ids of ',' and '\\n')")
    ids_cpu = input_ids.detach()
    if ids_cpu.is_cuda:
        ids_cpu = ids_cpu.cpu()                                   # the one device -> host copy
    ids_cpu = ids_cpu.to(torch.int64).contiguous()
    ids_np = ids_cpu.numpy()
    lay = splice_layout(ids_np, M, mode, h_block, w_block, image_token_index)
    B, L_in, L = lay.batch, lay.in_len, lay.max_len
    text_ids = ids_np[ids_np != image_token_index]
    if text_ids.size and (int(text_ids.min()) < 0 or int(text_ids.max()) >= V):
        bad = text_ids[(text_ids < 0) | (text_ids >= V)][0]
        raise ValueError(f"input id {int(bad)} is outside the embedding table [0, {V})")
    codes = lay.codes
    if mode == "slice":
        for name, v in (("sep_id", sep_id), ("ret_id", ret_id)):
            if not 0 <= int(v) < V:
                raise ValueError(f"{name} = {v} is outside the embedding table [0, {V})")
        lit = (codes >> np.uint32(30)) == 1
        codes = np.where(lit, _LITERAL | np.where((codes & _PAYLOAD) == RET, np.uint32(int(ret_id)), np.uint32(int(sep_id))), codes)
    if crop_map is not None:
        if crop_map.dtype != torch.int32 or crop_map.dim() != 1 or crop_map.device != image_features.device \
                or not crop_map.is_contiguous():
            raise ValueError("crop_map must be a contiguous int32 vector on the features' device")
    n_logical = crop_map.numel() if crop_map is not None else n_blocks
    if lay.n_blocks != n_logical:
        raise ValueError(f"input_ids describe {lay.n_blocks} feature blocks (one per image token{' crop' if mode == 'slice' else ''}, "
                         f"one per image-less sample), image_features hold {n_logical}")
    for name, t, ok in (("labels", labels, (torch.int64,)), ("attention_mask", attention_mask, (torch.bool, torch.int64))):
        if t is not None:
            if tuple(t.shape) != (B, L_in):
                raise ValueError(f"{name} must be [{B}, {L_in}] like input_ids")
            if t.dtype not in ok:
                raise TypeError(f"{name} must be {' or '.join(str(d) for d in ok)}, not {t.dtype}")
    if attention_mask is not None and labels is None and bool((lay.lengths != lay.lengths[0]).any()):
        raise ValueError("ragged lengths with an attention_mask need labels (the reference reads an unbound _new_labels, "
                         "llava_arch.py:216)")
    if not image_features.is_cuda:
        raise RuntimeError("build_multimodal_inputs runs only on an AMD GPU (HIP kernel); there is no CPU fallback")
    device = image_features.device
    if table.device != device:
        raise ValueError(f"the embedding table is on {table.device}, image_features on {device}")
    need_f = torch.is_grad_enabled() and image_features.requires_grad
    need_t = torch.is_grad_enabled() and table.requires_grad
    if need_f and crop_map is not None:
        cm = crop_map.cpu()
        if int(cm.min()) < 0 or int(cm.max()) >= n_blocks:
            raise ValueError(f"crop_map values must lie in [0, {n_blocks})")
        if torch.unique(cm).numel() != cm.numel():
            raise ValueError("crop_map must be injective when a gradient is live (two blocks would share one gradient row)")

    # the plan: codes | lengths, and for a trainable table order | offsets; ids that live on the CPU ride in front of it.
    # One pinned staging buffer, one asynchronous host -> device copy (a pageable copy would block the host on the stream).
    rows = B * L
    parts = [codes.view(np.int32), lay.lengths]
    n_table = 0
    if need_t:
        kind = codes >> np.uint32(30)
        table_rows = np.nonzero(kind <= 1)[0]
        payload = (codes[table_rows] & _PAYLOAD).astype(np.int64)
        row_ids = np.where(kind[table_rows] == 0, ids_np.reshape(-1)[np.minimum(payload, ids_np.size - 1)], payload)
        # (16-bit keys take numpy's radix sort, several times faster than the merge sort of int64 at 30 000 rows)
        by_id = np.argsort(row_ids.astype(np.uint16) if V <= 65536 else row_ids, kind="stable")
        n_table = int(table_rows.size)
        offsets = np.zeros(V + 1, dtype=np.int32)
        np.cumsum(np.bincount(row_ids, minlength=V), out=offsets[1:])
        parts += [table_rows[by_id].astype(np.int32), offsets]
    ids_words = 0 if input_ids.is_cuda else 2 * B * L_in          # int64 ids as int32 pairs, first: 8-byte aligned
    staging = torch.empty(ids_words + sum(p.size for p in parts), dtype=torch.int32, pin_memory=True)
    stage_np = staging.numpy()
    if ids_words:
        stage_np[:ids_words] = ids_np.reshape(-1).view(np.int32)
    np.concatenate(parts, out=stage_np[ids_words:])
    plan_host = stage_np[ids_words:]
    staged_dev = staging.to(device, non_blocking=True)
    plan_dev = staged_dev[ids_words:]
    if ids_words:
        ids_dev = staged_dev[:ids_words].view(torch.int64)
    else:
        ids_dev = input_ids.detach().to(device=device, dtype=torch.int64).contiguous()
    feats = image_features.contiguous()
    spec = _Spec()
    spec.keep = (staging, staged_dev, ids_cpu, ids_dev, crop_map)
    out_labels = out_mask = None
    spec.feats_shape, spec.table_shape = tuple(feats.shape), tuple(table.shape)
    a = _capi.tp_splice_args()
    a.batch, a.in_len, a.out_len, a.M, a.D, a.dtype = B, L_in, L, M, D, dt
    a.V, a.n_feat_blocks, a.n_logical = V, n_blocks, n_logical
    a.plan_host, a.plan_dev = plan_host.ctypes.data, plan_dev.data_ptr()
    a.ids_host, a.ids_dev = ids_cpu.data_ptr(), ids_dev.data_ptr()
    a.table, a.feats = table.data_ptr(), feats.data_ptr()
    a.crop_map = crop_map.data_ptr() if crop_map is not None else None
    a.mask_bytes = 1
    if labels is not None:                                           # (on the CPU: a copy of its own, as for the mask)
        lab = labels.to(device).contiguous()
        out_labels = torch.empty(B, L, dtype=torch.int64, device=device)
        spec.keep += (lab,)
        a.labels, a.out_labels = lab.data_ptr(), out_labels.data_ptr()
    if attention_mask is not None:
        msk = attention_mask.to(device).contiguous()
        out_mask = torch.empty(B, L, dtype=msk.dtype, device=device)
        spec.keep += (msk,)
        a.mask, a.out_mask, a.mask_bytes = msk.data_ptr(), out_mask.data_ptr(), msk.element_size()
    a.padding_idx, a.n_table_rows = padding_idx, n_table
    if need_t:
        a.order_host = plan_host.ctypes.data + 4 * (rows + B)
        a.order_dev = plan_dev.data_ptr() + 4 * (rows + B)
    spec.args = a
    if need_f or need_t:
        out = _SpliceFn.apply(feats, table, spec)
    else:
        out = _launch(spec, feats, table)
    return out_mask, out.view(B, L, D), out_labels
