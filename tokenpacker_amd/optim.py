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


# ---- the sharded step ----------------------------------------------------------------------------------------------------------
CHUNK = 4096            # elements of one workgroup of the optimizer kernels (kOptimChunk, tp_optim.hip; tests hold the two equal)


def shard_layout(numels, world: int, align: int = 64, chunk: int = CHUNK) -> dict:
    """Where tensors of ``numels`` elements lie in ONE flat index space cut into ``world`` equal shards: every tensor starts at a
    multiple of ``align`` elements, and the total is padded to a multiple of ``world * chunk`` (so every shard starts 16-byte
    aligned in every element type and covers whole chunks).  Pure host arithmetic, no device:
    -> ``{"world", "align", "chunk", "numels", "offsets", "total", "shard"}`` (``shard = total // world`` elements per rank)."""
    numels = [int(n) for n in numels]
    if world < 1 or align < 1 or chunk < 1:
        raise ValueError(f"shard_layout: world = {world}, align = {align} and chunk = {chunk} must be positive")
    if any(n <= 0 for n in numels):
        raise ValueError(f"shard_layout: every tensor has at least one element, got {numels}")
    offsets, end = [], 0
    for n in numels:
        start = -(-end // align) * align
        offsets.append(start)
        end = start + n
    unit = world * chunk
    total = max(-(-end // unit), 1) * unit
    return {"world": int(world), "align": int(align), "chunk": int(chunk), "numels": numels, "offsets": offsets, "total": total,
            "shard": total // world}


def shard_slices(layout: dict, rank: int):
    """What shard ``rank`` of ``layout`` holds: ``[(tensor index, start in tensor, length, offset in shard)]``, one per tensor it
    intersects, in tensor order.  Padding (between tensors and behind the last one) is in nobody's slices."""
    if not 0 <= rank < layout["world"]:
        raise ValueError(f"shard_slices: rank {rank} outside a world of {layout['world']}")
    lo, hi = rank * layout["shard"], (rank + 1) * layout["shard"]
    out = []
    for i, (off, n) in enumerate(zip(layout["offsets"], layout["numels"])):
        a, b = max(off, lo), min(off + n, hi)
        if a < b:
            out.append((i, a - off, b - a, a - lo))
    return out


_LAYOUT_KEYS = ("world", "align", "chunk", "numels", "offsets", "total")


class ShardedMainGradAdamW(torch.optim.Optimizer):
    """``MainGradAdamW`` over several ranks, ZeRO-1 style: the gradients are reduced across the process group, and every rank keeps
    the moments and fp32 masters of — and applies clip + AdamW to — ONE shard of a flat parameter space (``shard_layout``); the
    updated parameters are gathered back.  Same arguments as ``MainGradAdamW`` plus ``process_group`` (None: the default group;
    no initialised group: world size 1, no collective call) and ``average`` (divide the summed gradients by the world size).

    Construction RE-POINTS the parameters: it allocates ``flat_grad`` (fp32) and ``flat_param`` (the parameters' dtype), copies
    every ``p.main_grad`` (a parameter without one gets a zeroed one) and ``p.data`` into them and makes ``p.main_grad`` and
    ``p.data`` views of these buffers — so one reduce-scatter and one all-gather serve all tensors.  Build it after the module is
    on its device and in its dtype, and before anything keeps the old storages; ``step()`` raises a ``RuntimeError`` naming the
    parameter whose ``main_grad`` or ``data`` no longer is that view.  Every rank must hold the same parameters in the same order.

    ``step()``: ``reduce_scatter_tensor(grad_shard, flat_grad, SUM)``; ``tp_optim_sumsq`` (this shard's sum of squares, one
    double); ``all_gather_into_tensor`` of the doubles in rank order; ``tp_optim_apply`` with ``grad_scale = 1 / world`` (the
    norm, the clipping and the update are those of the AVERAGED gradient); ``all_gather_into_tensor(flat_param, param_shard)``;
    ``flat_grad.zero_()``.  All on the current stream, no host synchronisation (RCCL; a ``gloo`` group, which has no device
    collectives, is served through host copies: for tests on one device).  Every rank sees the same W doubles and writes the
    same state block: ``grad_norm``, ``clip_coef``, ``found_inf``, ``steps_applied`` and ``steps_skipped`` are device views as in
    ``MainGradAdamW``, and a non-finite gradient on one rank skips the step on all.  ``grad_shard`` keeps the reduced (summed,
    not yet averaged) gradient after the step.  fp32 parameters are their own masters: ``param_shard`` is the master shard."""

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0,
                 max_grad_norm: Optional[float] = 1.0, zero_main_grads: bool = True, module=None, process_group=None,
                 average: bool = True):
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
        self.average = bool(average)
        self.module = module
        import torch.distributed as dist
        self._dist = dist if dist.is_available() and dist.is_initialized() else None
        self._group = process_group if self._dist is not None else None
        self.world = self._dist.get_world_size(self._group) if self._dist is not None else 1
        self.rank = self._dist.get_rank(self._group) if self._dist is not None else 0
        # (gloo moves host memory only: device tensors travel through host copies, which synchronise — a test backend)
        self._host_staged = self._dist is not None and self._dist.get_backend(self._group) == "gloo"
        names = {id(p): n for n, p in module.named_parameters()} if module is not None else {}
        self._entries = []                          # (group, parameter, name), in parameter order: the tensors of the layout
        index = 0
        for group in self.param_groups:
            for p in group["params"]:
                name = names.get(id(p), f"#{index}")
                index += 1
                if not p.requires_grad:
                    continue
                if getattr(p, "main_grad", None) is None:
                    p.main_grad = torch.zeros(p.shape, dtype=torch.float32, device=p.device)
                checked_main_grad(name, p)
                self._entries.append((group, p, name))
        first = self._entries[0][1] if self._entries else None
        for _, p, name in self._entries:
            if p.dtype not in _DTYPES:
                raise TypeError(f"ShardedMainGradAdamW: parameter {name} is {p.dtype}; the parameters are torch.bfloat16 or "
                                f"torch.float16 (their fp32 masters live in the optimizer), or torch.float32 (their own masters)")
            if p.dtype != first.dtype or p.device != first.device:
                raise ValueError(f"ShardedMainGradAdamW: parameter {name} is {p.dtype} on {p.device}, the first one {first.dtype} on "
                                 f"{first.device}: one dtype and one device per optimizer")
            if not p.is_contiguous():
                raise ValueError(f"ShardedMainGradAdamW: parameter {name} must be contiguous")
        for _, p, name in self._entries:
            if not p.is_cuda:
                raise RuntimeError("tokenpacker_amd.optim.ShardedMainGradAdamW runs only on an AMD GPU (HIP kernels); there is no "
                                   "CPU fallback")
        self._device = first.device if first is not None else None
        self._dtype = first.dtype if first is not None else None
        self._own_master = self._dtype == torch.float32
        self._block = self._workspace = None
        self._n = 0
        if self._entries:
            if not _capi.sharded_optim_supported():
                raise RuntimeError("ShardedMainGradAdamW needs a library with tp_optim_sumsq / tp_optim_apply; rebuild "
                                   "libtokenpacker_hip.so")
            self._build()
        self._built = True

    def _build(self):
        dev, dt = self._device, self._dtype
        self.layout = shard_layout([p.numel() for _, p, _ in self._entries], self.world)
        total, shard = self.layout["total"], self.layout["shard"]
        self.flat_grad = torch.zeros(total, dtype=torch.float32, device=dev)
        self.flat_param = torch.zeros(total, dtype=dt, device=dev)
        with torch.no_grad():
            for (_, p, _), off in zip(self._entries, self.layout["offsets"]):
                n = p.numel()
                self.flat_grad[off:off + n].copy_(p.main_grad.reshape(-1))
                self.flat_param[off:off + n].copy_(p.detach().reshape(-1))
                p.main_grad = self.flat_grad[off:off + n].view(p.shape)
                p.data = self.flat_param[off:off + n].view(p.shape)
        lo = self.rank * shard
        self.grad_shard = torch.zeros(shard, dtype=torch.float32, device=dev)
        self.param_shard = self.flat_param[lo:lo + shard].clone()
        self.exp_avg = torch.zeros(shard, dtype=torch.float32, device=dev)
        self.exp_avg_sq = torch.zeros(shard, dtype=torch.float32, device=dev)
        self.master = self.param_shard if self._own_master else self.param_shard.float()
        self._slices = shard_slices(self.layout, self.rank)
        self._n = n = len(self._slices)
        self._table = (_capi.tp_optim_tensor * max(n, 1))()
        for e, (_i, _start, length, off) in zip(self._table, self._slices):
            e.param = None if self._own_master else self.param_shard.data_ptr() + off * self.param_shard.element_size()
            e.master, e.grad = self.master.data_ptr() + 4 * off, self.grad_shard.data_ptr() + 4 * off
            e.exp_avg, e.exp_avg_sq = self.exp_avg.data_ptr() + 4 * off, self.exp_avg_sq.data_ptr() + 4 * off
            e.numel = length
        if n:
            nbytes = _capi.load_library().tp_optim_workspace_bytes(self._table, n)
            if nbytes == 0:
                raise RuntimeError(f"tp_optim_workspace_bytes: {_capi.last_error()}")
            self._workspace = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        self._block = torch.zeros(_STATE_WORDS, dtype=torch.int32, device=dev)
        self._sumsq = torch.zeros(1, dtype=torch.float64, device=dev)
        self._sums = torch.zeros(self.world, dtype=torch.float64, device=dev)
        if self.module is not None:
            self.module.invalidate_packed()             # (the parameters moved: a cached weight image names the old storages)

    def add_param_group(self, param_group):
        if self._built:
            raise RuntimeError("ShardedMainGradAdamW: parameter groups are fixed at construction (the flat buffers are laid out "
                               "from them)")
        super().add_param_group(param_group)

    @property
    def tensor_names(self):
        """Names of the tensors of the layout, in its order: the parameters that require grad."""
        return [name for _, _, name in self._entries]

    _word = MainGradAdamW._word
    grad_norm = MainGradAdamW.grad_norm
    clip_coef = MainGradAdamW.clip_coef
    found_inf = MainGradAdamW.found_inf
    steps_applied = MainGradAdamW.steps_applied
    steps_skipped = MainGradAdamW.steps_skipped

    # ---- collectives (a world of one without a process group: plain copies) ----------------------------------------------------
    def _reduce_scatter(self, out, src):
        if self._dist is None:
            out.copy_(src)
        elif self._host_staged:
            host = torch.empty(out.shape, dtype=out.dtype)
            self._dist.reduce_scatter_tensor(host, src.cpu(), op=self._dist.ReduceOp.SUM, group=self._group)
            out.copy_(host)
        else:
            self._dist.reduce_scatter_tensor(out, src, op=self._dist.ReduceOp.SUM, group=self._group)

    def _all_gather(self, out, src):
        if self._dist is None:
            out.copy_(src)
        elif self._host_staged:
            host = torch.empty(out.shape, dtype=out.dtype)
            self._dist.all_gather_into_tensor(host, src.cpu(), group=self._group)
            out.copy_(host)
        else:
            self._dist.all_gather_into_tensor(out, src, group=self._group)

    # ---- the step -----------------------------------------------------------------------------------------------------------
    def step(self, closure=None, inv_scale: Optional[torch.Tensor] = None):
        """Reduce-scatter + clip + AdamW on this rank's shard + all-gather of the parameters (+ zeroing) on the current stream.
        ``inv_scale``: as in ``MainGradAdamW.step`` (the same tensor value on every rank)."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if not self._entries:
            return loss
        betas, eps = self.param_groups[0]["betas"], self.param_groups[0]["eps"]
        gbase, pbase, psize = self.flat_grad.data_ptr(), self.flat_param.data_ptr(), self.flat_param.element_size()
        for (group, p, name), off in zip(self._entries, self.layout["offsets"]):
            if group["betas"] != betas or group["eps"] != eps:
                raise ValueError("ShardedMainGradAdamW: betas and eps are one per optimizer, not per parameter group")
            mg = getattr(p, "main_grad", None)
            if not isinstance(mg, torch.Tensor) or mg.data_ptr() != gbase + 4 * off or mg.dtype != torch.float32 \
                    or mg.shape != p.shape or not mg.is_contiguous():
                raise RuntimeError(f"ShardedMainGradAdamW: {name}.main_grad is no longer the view of flat_grad the optimizer made "
                                   f"(something replaced it after construction)")
            if p.data_ptr() != pbase + psize * off or p.dtype != self._dtype or not p.is_contiguous():
                raise RuntimeError(f"ShardedMainGradAdamW: the data of parameter {name} is no longer the view of flat_param the "
                                   f"optimizer made (something replaced it after construction, a .to() for instance)")
        for e, (i, _start, _length, _off) in zip(self._table, self._slices):
            group = self._entries[i][0]
            e.lr, e.weight_decay = group["lr"], group["weight_decay"]
        inv_ptr = None
        if inv_scale is not None:
            if not (isinstance(inv_scale, torch.Tensor) and inv_scale.dtype == torch.float32 and inv_scale.numel() == 1
                    and inv_scale.device == self._device):
                raise TypeError("ShardedMainGradAdamW.step: inv_scale must be a one-element torch.float32 tensor on the parameters' "
                                "device")
            inv_ptr = inv_scale.data_ptr()
        hyper = _capi.tp_optim_hyper(betas[0], betas[1], eps, self.max_grad_norm, _DTYPES[self._dtype], 0)
        grad_scale = 1.0 / self.world if self.average else 1.0
        lib, n = _capi.load_library(), self._n
        ws_ptr, ws_bytes = (self._workspace.data_ptr(), self._workspace.numel()) if n else (None, 0)
        with torch.cuda.device(self._device), torch.no_grad():
            stream = torch.cuda.current_stream(self._device).cuda_stream
            self._reduce_scatter(self.grad_shard, self.flat_grad)
            _capi.check(lib.tp_optim_sumsq(self._table, n, inv_ptr, grad_scale, self._sumsq.data_ptr(), ws_ptr, ws_bytes, stream),
                        "tp_optim_sumsq")
            self._all_gather(self._sums, self._sumsq)
            _capi.check(lib.tp_optim_apply(self._table, n, ctypes.byref(hyper), inv_ptr, grad_scale, self._sums.data_ptr(), self.world,
                                           self._block.data_ptr(), stream), "tp_optim_apply")
            self._all_gather(self.flat_param, self.param_shard)
            if self.zero_main_grads:
                self.flat_grad.zero_()
        if self.module is not None:
            self.module.invalidate_packed()
        return loss

    # ---- state dicts --------------------------------------------------------------------------------------------------------
    def _indexed_params(self):
        return [p for group in self.param_groups for p in group["params"]]

    def _packed_groups(self):
        groups, start = [], 0
        for group in self.param_groups:
            packed = {k: v for k, v in group.items() if k != "params"}
            packed["params"] = list(range(start, start + len(group["params"])))
            start += len(group["params"])
            groups.append(packed)
        return groups

    def _counters(self):
        applied, skipped = (0, 0) if self._block is None else (int(v) for v in self._block[_W_STEP:_W_SKIPPED + 1].tolist())
        return {"steps_applied": applied, "steps_skipped": skipped, "max_grad_norm": self.max_grad_norm}

    def state_dict(self):
        """THIS rank's shards (``exp_avg``, ``exp_avg_sq``, and ``master`` for bf16 / fp16 parameters) with the layout they belong
        to, the parameter groups and the counters.  Loads only into the same layout (same world size, same tensors); to resume on
        another number of ranks use ``consolidated_state_dict()``.  Reads the counters: synchronises."""
        shards = {}
        if self._entries:
            shards = {"exp_avg": self.exp_avg, "exp_avg_sq": self.exp_avg_sq}
            if not self._own_master:
                shards["master"] = self.master
        layout = dict({k: self.layout[k] for k in _LAYOUT_KEYS}, rank=self.rank) if self._entries else None
        return {"sharded": layout, "shards": shards, "param_groups": self._packed_groups(), "main_grad_adamw": self._counters()}

    def consolidated_state_dict(self):
        """``MainGradAdamW``'s per-parameter state dict, on EVERY rank (a collective: call it on all ranks): the shards gathered
        and cut back into tensors.  ``load_state_dict`` takes it at any world size."""
        counters = self._counters()
        index = {id(p): i for i, p in enumerate(self._indexed_params())}
        state = {}
        if self._entries:
            total = self.layout["total"]
            full = {}
            for key, shard in (("exp_avg", self.exp_avg), ("exp_avg_sq", self.exp_avg_sq)) + \
                    (() if self._own_master else (("master", self.master),)):
                full[key] = torch.empty(total, dtype=torch.float32, device=self._device)
                self._all_gather(full[key], shard)
            for (_, p, _name), off in zip(self._entries, self.layout["offsets"]):
                state[index[id(p)]] = dict({"step": torch.tensor(float(counters["steps_applied"]))},
                                           **{k: v[off:off + p.numel()].view(p.shape).clone() for k, v in full.items()})
        return {"state": state, "param_groups": self._packed_groups(), "main_grad_adamw": counters}

    def load_state_dict(self, state_dict):
        """Loads ``state_dict()``'s sharded form (identical layout only: a ``ValueError`` says what differs), or the per-parameter
        form of ``consolidated_state_dict()`` / ``MainGradAdamW.state_dict()`` / ``torch.optim.AdamW.state_dict()`` at any world
        size: every rank takes its slices; masters a state dict does not carry come from the parameters as they are now."""
        saved_groups = state_dict["param_groups"]
        if len(saved_groups) != len(self.param_groups):
            raise ValueError("loaded state dict has a different number of parameter groups")
        for group, saved in zip(self.param_groups, saved_groups):
            if len(group["params"]) != len(saved["params"]):
                raise ValueError("loaded state dict contains a parameter group that doesn't match the size of optimizer's group")
        sharded = "sharded" in state_dict
        if sharded and self._entries:
            theirs = state_dict["sharded"]
            if theirs is None:
                raise ValueError("loaded sharded state dict has no tensors, this optimizer has")
            mine = dict({k: self.layout[k] for k in _LAYOUT_KEYS}, rank=self.rank)
            differs = [f"{k}: saved {theirs.get(k)} != {mine[k]}" for k in ("world", "rank", "total", "align", "chunk")
                       if theirs.get(k) != mine[k]]
            for k in ("numels", "offsets"):
                if list(theirs.get(k, ())) != mine[k]:
                    differs.append(f"{k} differ")
            if differs:
                raise ValueError("ShardedMainGradAdamW.load_state_dict: the sharded state dict belongs to another layout ("
                                 + "; ".join(differs) + "); load a consolidated_state_dict() to change the world size")
        for group, saved in zip(self.param_groups, saved_groups):
            group.update({k: (tuple(v) if k == "betas" else v) for k, v in saved.items() if k != "params"})
        step_seen = 0
        with torch.no_grad():
            if sharded and self._entries:
                shards = state_dict["shards"]
                self.exp_avg.copy_(shards["exp_avg"])
                self.exp_avg_sq.copy_(shards["exp_avg_sq"])
                if not self._own_master:
                    self.master.copy_(shards["master"])
            elif self._entries:
                index = {id(p): i for i, p in enumerate(self._indexed_params())}
                saved_state = {int(k): v for k, v in state_dict["state"].items()}
                for i, start, length, off in self._slices:
                    p = self._entries[i][1]
                    saved = saved_state.get(index[id(p)])
                    here = slice(off, off + length)
                    now = p.detach().reshape(-1)[start:start + length]
                    if saved is None:                      # (an optimizer saved before its first step: fresh moments)
                        self.exp_avg[here].zero_()
                        self.exp_avg_sq[here].zero_()
                        self.master[here].copy_(now)
                        continue
                    for key, dst in (("exp_avg", self.exp_avg), ("exp_avg_sq", self.exp_avg_sq)):
                        dst[here].copy_(saved[key].reshape(-1)[start:start + length])
                    self.master[here].copy_(saved["master"].reshape(-1)[start:start + length] if "master" in saved else now)
                    step_seen = max(step_seen, int(float(saved.get("step", 0))))
                if self.world > 1 and "main_grad_adamw" not in state_dict:       # (a rank sees the steps of ITS tensors only)
                    seen = torch.tensor([float(step_seen)], dtype=torch.float64, device=self._device)
                    every = torch.empty(self.world, dtype=torch.float64, device=self._device)
                    self._all_gather(every, seen)
                    step_seen = int(every.max().item())
        own = state_dict.get("main_grad_adamw")
        applied, skipped = (own["steps_applied"], own["steps_skipped"]) if own is not None else (step_seen, 0)
        if own is not None:
            self.max_grad_norm = float(own.get("max_grad_norm", self.max_grad_norm))
        if self._block is not None:
            words = torch.zeros(_STATE_WORDS, dtype=torch.int32)
            words[_W_STEP], words[_W_SKIPPED] = int(applied), int(skipped)
            self._block.copy_(words)
