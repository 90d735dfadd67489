"""The LLM's loss on given logits — ``llava/model/language_model/llava_llama.py:95-106`` of the reference — as one forward
and one backward HIP launch over the LABELLED rows only (``tp_shift_ce_forward`` / ``tp_shift_ce_backward``).

The reference shifts (``logits[..., :-1, :].contiguous()``, ``labels[..., 1:].contiguous()``), flattens and calls
``CrossEntropyLoss()`` on the bf16 logits: a shifted copy, a log-softmax and a gradient, each as large as the logits, for
every row — although the splice (:mod:`tokenpacker_amd.splice`) has just written ``-100`` into the label of every image,
separator, prompt and padding row.  Here a row whose target is ``ignore_index`` is not read at all, a labelled row is read once
in the forward and read and written once in the backward, nothing of the logits' size is allocated in the forward, and with
``inplace_grad=True`` nothing in the backward either.  Nothing synchronises with the host: the count of labelled rows, the
mean and the incoming gradient stay on the device.
"""
from __future__ import annotations

import ctypes

import torch

from . import _capi

_DTYPES = {torch.bfloat16: _capi.TP_BF16, torch.float16: _capi.TP_F16, torch.float32: _capi.TP_F32}
_REDUCTIONS = {"mean": _capi.TP_CE_MEAN, "sum": _capi.TP_CE_SUM}


def _args(logits: torch.Tensor, labels: torch.Tensor, ws: torch.Tensor, ignore_index: int, reduction: int) -> "_capi.tp_shift_ce_args":
    B, L, V = logits.shape
    a = _capi.tp_shift_ce_args()
    a.batch, a.len, a.V, a.dtype, a.reduction = B, L, V, _DTYPES[logits.dtype], reduction
    # (the stride of a dimension of size 1 is never used to form an address: any value torch reports there is replaced)
    a.row_stride = logits.stride(1) if L > 1 else V
    a.batch_stride = logits.stride(0) if B > 1 else 0
    a.ignore_index = ignore_index
    a.logits, a.labels = logits.data_ptr(), labels.data_ptr()
    a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
    return a


def _forward(logits, labels, ignore_index, reduction):
    """-> (loss, n_valid, workspace): two 0-dim views of the workspace's head and the workspace itself (uint8)."""
    lib = _capi.load_library()
    B, L, _ = logits.shape
    ws = torch.empty(lib.tp_shift_ce_workspace_bytes(B, L), dtype=torch.uint8, device=logits.device)
    a = _args(logits, labels, ws, ignore_index, reduction)
    with torch.cuda.device(logits.device):
        _capi.check(lib.tp_shift_ce_forward(ctypes.byref(a), torch.cuda.current_stream(logits.device).cuda_stream),
                    "tp_shift_ce_forward")
    loss = ws[_capi.TP_SHIFT_CE_LOSS_OFFSET:_capi.TP_SHIFT_CE_LOSS_OFFSET + 4].view(torch.float32).view(())
    n_valid = ws[_capi.TP_SHIFT_CE_N_VALID_OFFSET:_capi.TP_SHIFT_CE_N_VALID_OFFSET + 8].view(torch.int64).view(())
    return loss, n_valid, ws


def _grad_buffer(logits: torch.Tensor) -> torch.Tensor:
    """A fresh [B, L, V] gradient, compact up to 15 bytes a row, whose every row sits at the same offset from a 16-byte boundary
    as the logits row it belongs to (the kernel splits both rows into head / 16-byte vectors / tail with one computation)."""
    B, L, V = logits.shape
    es = logits.element_size()
    per16 = 16 // es
    row = V + ((logits.stride(1) if L > 1 else V) - V) % per16
    batch = L * row + ((logits.stride(0) if B > 1 else 0) - L * row) % per16
    lead = (logits.data_ptr() % 16) // es
    flat = torch.empty(lead + B * batch, dtype=logits.dtype, device=logits.device)     # (allocations are 16-byte aligned)
    return flat.as_strided((B, L, V), (batch, row, 1), lead)


class _ShiftedCrossEntropyFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels, ignore_index, reduction, inplace_grad):
        loss, n_valid, ws = _forward(logits, labels, ignore_index, reduction)
        ctx.save_for_backward(logits, labels, ws)          # references: nothing is copied
        ctx.ignore_index, ctx.reduction, ctx.inplace_grad = ignore_index, reduction, inplace_grad
        ctx.consumed = False
        ctx.mark_non_differentiable(n_valid)
        return loss, n_valid

    @staticmethod
    def backward(ctx, g, _g_n_valid):
        if ctx.consumed:
            raise RuntimeError("shifted_cross_entropy(inplace_grad=True): the first backward overwrote the logits with their "
                               "gradient; a second backward through the same node has nothing to read")
        logits, labels, ws = ctx.saved_tensors
        lib = _capi.load_library()
        a = _args(logits, labels, ws, ctx.ignore_index, ctx.reduction)
        g = g.to(torch.float32).contiguous()
        dlogits = logits.detach() if ctx.inplace_grad else _grad_buffer(logits)
        a.grad_loss, a.dlogits = g.data_ptr(), dlogits.data_ptr()
        a.d_row_stride = a.row_stride if ctx.inplace_grad else dlogits.stride(1)
        a.d_batch_stride = a.batch_stride if ctx.inplace_grad else dlogits.stride(0)
        with torch.cuda.device(logits.device):
            _capi.check(lib.tp_shift_ce_backward(ctypes.byref(a), torch.cuda.current_stream(logits.device).cuda_stream),
                        "tp_shift_ce_backward")
        ctx.consumed = ctx.inplace_grad
        return dlogits, None, None, None, None


def shifted_cross_entropy(logits: torch.Tensor, labels: torch.Tensor, *, ignore_index: int = -100, reduction: str = "mean",
                          inplace_grad: bool = False, return_n_valid: bool = False):
    """``CrossEntropyLoss(ignore_index, reduction)(logits[..., :-1, :].reshape(-1, V), labels[..., 1:].reshape(-1))`` —
    what the reference's ``LlavaLlamaForCausalLM.forward`` computes from its ``logits`` and ``labels``
    (``llava_llama.py:95-106``) — as a 0-dim **fp32** tensor on the logits' device.  The reference's loss has the logits' dtype;
    ``.to(logits.dtype)`` reproduces that rounding, and the fp32 value is the closer one to exact arithmetic.

    ``logits [B, L, V]``: bf16, fp16 or fp32 on the GPU, last-dimension stride 1, any row and batch stride (a padded-vocabulary
    view ``buf[..., :V]`` is read in place) and no alignment beyond one element.  ``labels [B, L]``: int64 on the same device
    (made contiguous if it is not).  ``reduction``: ``"mean"`` over the labelled rows (the reference's) or ``"sum"``.
    With ``return_n_valid`` the result is ``(loss, n_valid)``, ``n_valid`` a 0-dim int64 device tensor: the rows whose target is
    not ``ignore_index``.  Both are views of one small workspace; nothing is copied to the host.

    Differentiable with respect to ``logits`` only.  The logits are saved by reference, never copied.  The gradient has the
    logits' dtype and shape; every unlabelled row and row ``L - 1`` of every sample are zeros — also when no row is labelled
    at all (the loss is then NaN, as the reference's).  With ``inplace_grad=True`` the gradient is written over the logits and
    shares their storage: the logits are gone after the backward, and a second backward through the same node raises.

    Non-finite logits behave as ``F.cross_entropy`` on the logits upcast to fp32.  A target outside ``[0, V)`` that is not
    ``ignore_index`` makes the loss NaN and its gradient row zero; it is not an error on the device.

    Raises on CPU tensors (there is no CPU fallback), an unsupported dtype, a last-dimension stride other than 1, or a
    ``labels`` shape that does not match."""
    if not isinstance(logits, torch.Tensor) or not isinstance(labels, torch.Tensor):
        raise TypeError("logits and labels must be tensors")
    if logits.dim() != 3 or logits.numel() == 0:
        raise ValueError("logits must be a non-empty [B, L, V]")
    if logits.dtype not in _DTYPES:
        raise TypeError(f"logits must be bfloat16, float16 or float32, not {logits.dtype}")
    if tuple(labels.shape) != tuple(logits.shape[:2]):
        raise ValueError(f"labels must be {list(logits.shape[:2])} like the logits' leading dimensions, not {list(labels.shape)}")
    if labels.dtype != torch.int64:
        raise TypeError(f"labels must be int64, not {labels.dtype}")
    if reduction not in _REDUCTIONS:
        raise ValueError(f"reduction must be 'mean' or 'sum', not {reduction!r}")
    if logits.shape[2] > 1 and logits.stride(2) != 1:
        raise ValueError(f"the last dimension of logits must have stride 1, not {logits.stride(2)}")
    if not logits.is_cuda or not labels.is_cuda:
        raise RuntimeError("shifted_cross_entropy runs only on an AMD GPU (HIP kernels); there is no CPU fallback")
    if labels.device != logits.device:
        raise ValueError(f"labels are on {labels.device}, logits on {logits.device}")
    labels = labels.detach().contiguous()
    if torch.is_grad_enabled() and logits.requires_grad:
        loss, n_valid = _ShiftedCrossEntropyFn.apply(logits, labels, int(ignore_index), _REDUCTIONS[reduction], bool(inplace_grad))
    else:
        loss, n_valid, _ = _forward(logits.detach(), labels, int(ignore_index), _REDUCTIONS[reduction])
    return (loss, n_valid) if return_n_valid else loss
