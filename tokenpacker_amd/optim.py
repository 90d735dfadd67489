"""``MainGradAdamW`` — gradient clipping + AdamW on the fp32 ``main_grad`` buffers, as one enqueued call (``tp_optim_step``).

The consumer of ``module.use_main_grad``: with it every backward ADDS unrounded fp32 gradients to ``p.main_grad`` and hands
autograd ``None``, so ``p.grad`` stays ``None`` and no stock optimizer sees a gradient.  This optimizer reads those buffers:
the global L2 norm (``clip_grad_norm_``'s formula, HF's ``max_grad_norm``), ``torch.optim.AdamW``'s update (the reference's
``optim = "adamw_torch"``, train.py:81) on fp32 master weights, the write-back into the bf16 / fp16 parameters and the zeroing of
``main_grad`` — three launches on the current stream, no host synchronisation, bit-reproducible.  fp32 parameters (an fp32 module
that runs under ``torch.autocast``) are their own masters: the update is applied to them in place, with no copy and no write-back.  A non-finite gradient norm skips
the step on the device and is counted (``found_inf``, ``steps_skipped``).

It is a ``torch.optim.Optimizer``: parameter groups with their own ``lr`` / ``weight_decay`` (what
``llava_trainer.create_optimizer`` builds, llava_trainer.py:164-222) and ``LambdaLR`` and friends work as usual.  ``betas`` and
``eps`` are one per optimizer.  Device tensors only: there is no CPU path."""
from __future__ import annotations

import ctypes
import math
from typing import Optional

import torch

from . import _capi
from .projector import checked_main_grad

_DTYPES = {torch.bfloat16: _capi.TP_BF16, torch.float16: _capi.TP_F16, torch.float32: _capi.TP_F32}
# words of the device state block (tp_optim_state, include/tokenpacker.h)
_W_NORM, _W_COEF, _W_FOUND_INF, _W_STEP, _W_SKIPPED = 0, 1, 2, 3, 4
_STATE_WORDS = _capi.TP_OPTIM_STATE_BYTES // 4


class MainGradAdamW(torch.optim.Optimizer):
    """AdamW (no amsgrad, no maximize) with global-norm clipping over the parameters' fp32 ``main_grad``.

    ``params``: parameters or parameter groups; every parameter that requires grad must carry a well-formed ``main_grad``
    (``TokenPacker.check_main_grads``'s contract, same named errors); parameters that do not require grad are left alone.
    ``max_grad_norm``: ``<= 0`` / ``inf`` / ``None`` = no clipping (the norm and ``found_inf`` are computed all the same).
    ``zero_main_grads``: zero ``main_grad`` behind the update, on a skipped step too.
    ``module``: a ``TokenPacker`` whose weight image is dropped after every step (``invalidate_packed()``: the step writes
    ``p.data`` through raw pointers, without a version bump); also names the parameters in error messages.

    Master weights start as ``p.detach().float()``; for fp32 parameters ``state[p]["master"]`` is ``p.data`` itself (12 bytes of
    state per element less, and ``state_dict()`` carries no ``master``: the module's own state dict has it).  ``grad_norm``, ``clip_coef``, ``found_inf``, ``steps_applied`` and
    ``steps_skipped`` are views of the device state block: reading them (``.item()``) is the caller's synchronisation."""

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0,
                 max_grad_norm: Optional[float] = 1.0, zero_main_grads: bool = True, module=None):
        if not (lr >= 0.0 and math.isfinite(lr)):
            raise ValueError(f"Invalid learning rate: {lr}")
        if not (eps >= 0.0 and math.isfinite(eps)):
            raise ValueError(f"Invalid epsilon value: {eps}")
        for i, b in enumerate(betas):
            if not 0.0 <= b < 1.0:
                raise ValueError(f"Invalid beta parameter at index {i}: {b}")
        if not (weight_decay >= 0.0 and math.isfinite(weight_decay)):
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        self._built = False
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False))
        self.max_grad_norm = 0.0 if max_grad_norm is None else float(max_grad_norm)
        self.zero_main_grads = bool(zero_main_grads)
        self.module = module
        names = {id(p): n for n, p in module.named_parameters()} if module is not None else {}
        self._entries = []                          # (group, parameter, name) of the table, in parameter order
        index = 0
        for group in self.param_groups:
            for p in group["params"]:
                name = names.get(id(p), f"#{index}")
                index += 1
                if not p.requires_grad:
                    continue
                checked_main_grad(name, p)           # (the named TypeError / ValueError comes first, as in the module)
                self._entries.append((group, p, name))
        first = self._entries[0][1] if self._entries else None
        for _, p, name in self._entries:                    # (what the parameters ARE before where they are: named on any device)
            if p.dtype not in _DTYPES:
                raise TypeError(f"MainGradAdamW: parameter {name} is {p.dtype}; the parameters are torch.bfloat16 or torch.float16 "
                                f"(their fp32 masters live in the optimizer), or torch.float32 (their own masters)")
            if p.dtype != first.dtype or p.device != first.device:
                raise ValueError(f"MainGradAdamW: parameter {name} is {p.dtype} on {p.device}, the first one {first.dtype} on "
                                 f"{first.device}: one dtype and one device per optimizer")
            if not p.is_contiguous():
                raise ValueError(f"MainGradAdamW: parameter {name} must be contiguous")
        for _, p, name in self._entries:
            if not p.is_cuda:
                raise RuntimeError("tokenpacker_amd.optim.MainGradAdamW runs only on an AMD GPU (HIP kernels); there is no CPU fallback")
        self._device = first.device if first is not None else None
        self._dtype = first.dtype if first is not None else None
        self._own_master = self._dtype == torch.float32      # fp32 parameters: updated in place, tp_optim_tensor.param stays NULL
        if self._own_master and not _capi.raw_f32_supported():
            raise RuntimeError("MainGradAdamW: fp32 parameters need a library with the TP_F32 optimizer mode (tp_desc_known_flags); "
                               "rebuild libtokenpacker_hip.so")
        n = len(self._entries)
        self._table = (_capi.tp_optim_tensor * max(n, 1))()
        for i, (_, p, _name) in enumerate(self._entries):
            st = self.state[p]
            st["step"] = torch.tensor(0.0)
            st["master"] = p.data if self._own_master else p.detach().float().contiguous()
            st["exp_avg"] = torch.zeros(p.shape, dtype=torch.float32, device=p.device)
            st["exp_avg_sq"] = torch.zeros(p.shape, dtype=torch.float32, device=p.device)
            e = self._table[i]
            e.master, e.exp_avg, e.exp_avg_sq = st["master"].data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr()
            e.numel = p.numel()
        self._block = self._workspace = None
        if n:
            lib = _capi.load_library()
            nbytes = lib.tp_optim_workspace_bytes(self._table, n)
            if nbytes == 0:
                raise RuntimeError(f"tp_optim_workspace_bytes: {_capi.last_error()}")
            self._workspace = torch.empty(nbytes, dtype=torch.uint8, device=self._device)
            self._block = torch.zeros(_STATE_WORDS, dtype=torch.int32, device=self._device)
        self._built = True

    def add_param_group(self, param_group):
        if self._built:
            raise RuntimeError("MainGradAdamW: parameter groups are fixed at construction (the kernel table is built from them)")
        super().add_param_group(param_group)

    @property
    def tensor_names(self):
        """Names of the tensors of the kernel table, in its order: the parameters that require grad."""
        return [name for _, _, name in self._entries]

    # ---- views of the device state block ------------------------------------------------------------------------------------
    def _word(self, i: int, as_float: bool = False) -> torch.Tensor:
        if self._block is None:
            raise RuntimeError("MainGradAdamW: no parameter requires grad; there is no state")
        return (self._block.view(torch.float32) if as_float else self._block)[i]

    @property
    def grad_norm(self) -> torch.Tensor:
        """Norm of ``main_grad * inv_scale`` of the last step, before clipping (0-dim fp32 device view)."""
        return self._word(_W_NORM, True)

    @property
    def clip_coef(self) -> torch.Tensor:
        return self._word(_W_COEF, True)

    @property
    def found_inf(self) -> torch.Tensor:
        """1 when the last step met a non-finite gradient norm and was skipped (0-dim int32 device view)."""
        return self._word(_W_FOUND_INF)

    @property
    def steps_applied(self) -> torch.Tensor:
        return self._word(_W_STEP)

    @property
    def steps_skipped(self) -> torch.Tensor:
        return self._word(_W_SKIPPED)

    # ---- the step -----------------------------------------------------------------------------------------------------------
    def step(self, closure=None, inv_scale: Optional[torch.Tensor] = None):
        """Clip + AdamW + write-back (none for fp32 parameters) (+ zeroing) on the current stream; returns without synchronising.  ``inv_scale``: a one-element
        fp32 device tensor the gradients are multiplied by (the reciprocal of a loss scale), or None."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        n = len(self._entries)
        if n == 0:
            return loss
        betas, eps = self.param_groups[0]["betas"], self.param_groups[0]["eps"]
        for i, (group, p, name) in enumerate(self._entries):
            if group["betas"] != betas or group["eps"] != eps:
                raise ValueError("MainGradAdamW: betas and eps are one per optimizer, not per parameter group")
            e = self._table[i]
            mg = getattr(p, "main_grad", None)
            ptr = mg.data_ptr() if isinstance(mg, torch.Tensor) else None
            if ptr is None or ptr != e.grad:
                e.grad = checked_main_grad(name, p).data_ptr()     # (a new buffer: held to the contract before its address is used)
            if p.data_ptr() != (e.master if self._own_master else e.param):
                if p.dtype != self._dtype or p.device != self._device or not p.is_contiguous() or p.numel() != e.numel:
                    raise RuntimeError(f"MainGradAdamW: parameter {name} changed its dtype, device, size or layout after the "
                                       f"optimizer was built")
                if self._own_master:             # (p.data was replaced: the master follows the parameter)
                    self.state[p]["master"] = p.data
                    e.master = p.data_ptr()
                else:
                    e.param = p.data_ptr()
            e.lr, e.weight_decay = group["lr"], group["weight_decay"]
        inv_ptr = None
        if inv_scale is not None:
            if not (isinstance(inv_scale, torch.Tensor) and inv_scale.dtype == torch.float32 and inv_scale.numel() == 1
                    and inv_scale.device == self._device):
                raise TypeError("MainGradAdamW.step: inv_scale must be a one-element torch.float32 tensor on the parameters' device")
            inv_ptr = inv_scale.data_ptr()
        hyper = _capi.tp_optim_hyper(betas[0], betas[1], eps, self.max_grad_norm, _DTYPES[self._dtype],
                                     _capi.TP_OPTIM_ZERO_GRAD if self.zero_main_grads else 0)
        with torch.cuda.device(self._device):
            stream = torch.cuda.current_stream(self._device).cuda_stream
            rc = _capi.load_library().tp_optim_step(self._table, n, ctypes.byref(hyper), inv_ptr, self._block.data_ptr(),
                                                    self._workspace.data_ptr(), self._workspace.numel(), stream)
        _capi.check(rc, "tp_optim_step")
        if self.module is not None:
            self.module.invalidate_packed()
        return loss

    # ---- state dict ---------------------------------------------------------------------------------------------------------
    def _indexed_params(self):
        return [p for group in self.param_groups for p in group["params"]]

    def state_dict(self):
        """torch's layout (``state`` by parameter index with ``step`` / ``exp_avg`` / ``exp_avg_sq``, ``param_groups`` with torch's
        keys) plus ``master`` per bf16 / fp16 parameter and the device counters under ``main_grad_adamw``.  Reads the counters: synchronises."""
        applied, skipped = (0, 0) if self._block is None else (int(v) for v in self._block[_W_STEP:_W_SKIPPED + 1].tolist())
        index = {id(p): i for i, p in enumerate(self._indexed_params())}
        state = {}
        for _, p, _name in self._entries:
            st = self.state[p]
            state[index[id(p)]] = {"step": torch.tensor(float(applied)), "exp_avg": st["exp_avg"], "exp_avg_sq": st["exp_avg_sq"]}
            if not self._own_master:
                state[index[id(p)]]["master"] = st["master"]
        groups, start = [], 0
        for group in self.param_groups:
            packed = {k: v for k, v in group.items() if k != "params"}
            packed["params"] = list(range(start, start + len(group["params"])))
            start += len(group["params"])
            groups.append(packed)
        return {"state": state, "param_groups": groups,
                "main_grad_adamw": {"steps_applied": applied, "steps_skipped": skipped, "max_grad_norm": self.max_grad_norm}}

    def load_state_dict(self, state_dict):
        """Loads what ``state_dict()`` returned — or a ``torch.optim.AdamW`` state dict over the same parameters: its moments and
        step count are taken, the masters then come from the parameters as they are now."""
        saved_groups = state_dict["param_groups"]
        if len(saved_groups) != len(self.param_groups):
            raise ValueError("loaded state dict has a different number of parameter groups")
        for group, saved in zip(self.param_groups, saved_groups):
            if len(group["params"]) != len(saved["params"]):
                raise ValueError("loaded state dict contains a parameter group that doesn't match the size of optimizer's group")
        for group, saved in zip(self.param_groups, saved_groups):
            group.update({k: (tuple(v) if k == "betas" else v) for k, v in saved.items() if k != "params"})
        index = {id(p): i for i, p in enumerate(self._indexed_params())}
        saved_state = {int(k): v for k, v in state_dict["state"].items()}
        step_seen = 0
        with torch.no_grad():
            for _, p, _name in self._entries:
                st, saved = self.state[p], saved_state.get(index[id(p)])
                if saved is None:                          # (an optimizer saved before its first step: fresh moments)
                    st["exp_avg"].zero_()
                    st["exp_avg_sq"].zero_()
                    st["master"].copy_(p.detach())
                    continue
                st["exp_avg"].copy_(saved["exp_avg"])
                st["exp_avg_sq"].copy_(saved["exp_avg_sq"])
                st["master"].copy_(saved["master"] if "master" in saved else p.detach())
                step_seen = max(step_seen, int(float(saved.get("step", 0))))
        own = state_dict.get("main_grad_adamw")
        applied, skipped = (own["steps_applied"], own["steps_skipped"]) if own is not None else (step_seen, 0)
        if own is not None:
            self.max_grad_norm = float(own.get("max_grad_norm", self.max_grad_norm))
        if self._block is not None:
            words = torch.zeros(_STATE_WORDS, dtype=torch.int32)
            words[_W_STEP], words[_W_SKIPPED] = int(applied), int(skipped)
            self._block.copy_(words)
        for _, p, _name in self._entries:
            self.state[p]["step"] = torch.tensor(float(applied))
