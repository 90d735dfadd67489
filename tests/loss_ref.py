"""The reference's loss (llava/model/language_model/llava_llama.py:98-106) with torch on the CPU, for the tests of
tokenpacker_amd.loss: drop the last position of the logits and the first of the labels, flatten both, CrossEntropyLoss —
in float64 (the yardstick), in float32, and in the logits' own dtype (what the reference itself computes), each with its
autograd gradient."""
from __future__ import annotations

from typing import NamedTuple, Optional

import torch
import torch.nn.functional as F

IGNORE_INDEX = -100


class LossRef(NamedTuple):
    loss: torch.Tensor          # 0-dim, the compute dtype
    grad: torch.Tensor          # [B, L, V], the compute dtype: d(loss * grad_out) / d logits (row L - 1 is zero)
    n_valid: int                # rows whose target is not ignore_index


def shifted_cross_entropy(logits: torch.Tensor, labels: torch.Tensor, compute_dtype: Optional[torch.dtype] = torch.float64, *,
                          ignore_index: int = IGNORE_INDEX, reduction: str = "mean", grad_out: float = 1.0) -> LossRef:
    """The reference's op sequence on CPU copies of `logits` [B, L, V] (any dtype; its values are taken as they are) and `labels`
    [B, L], computed in `compute_dtype` (None: the logits' own dtype, as the reference does)."""
    x = logits.detach().cpu().to(logits.dtype if compute_dtype is None else compute_dtype).clone().requires_grad_(True)
    y = labels.detach().cpu()
    V = x.shape[-1]
    shifted = x[..., :-1, :].contiguous().view(-1, V)
    targets = y[..., 1:].contiguous().view(-1)
    loss = F.cross_entropy(shifted, targets, ignore_index=ignore_index, reduction=reduction)
    if x.shape[-2] > 1:
        grad, = torch.autograd.grad(loss, x, torch.tensor(grad_out, dtype=loss.dtype))
    else:
        grad = torch.zeros_like(x)                    # (no row: nothing of x reaches the loss)
    return LossRef(loss.detach(), grad, int((targets != ignore_index).sum()))


def ordered_bits(t: torch.Tensor) -> torch.Tensor:
    """A 16-bit float tensor as int32 whose order is the order of the values (+0 and -0 both 0): the distance between two
    finite values in units in the last place is the difference of these."""
    bits = t.contiguous().view(torch.int16).to(torch.int32)
    return torch.where(bits >= 0, bits, -(bits & 0x7FFF))
