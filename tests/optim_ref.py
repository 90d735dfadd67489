"""fp64 restatement of one tp_optim_step (tokenpacker_amd/csrc/tp_optim.hip): gradient norm, clipping coefficient, found_inf, the
AdamW update and the cast — with the ELEMENTWISE error bound each comparison uses, the named wrong recipes the bound must exclude,
and the input generator the CPU proof (tests/test_optim_ref_cpu.py) and the GPU tests share.

``dtype`` is the arithmetic a formula is evaluated in: float64 for the reference, float32 for the "the bound has room" proof.
The hyper-parameters are the fp32 values the C ABI carries (``f32``): the kernel never sees a double.

Bounds are derived from the roundings of the kernel as written, not tuned.  u = 2^-24 (half an ulp of fp32, relative).

Norm.  Every lane adds CHAIN squares to its accumulator with one fma each (one rounding per term), a fixed tree of TREE_DEPTH
additions joins the workgroup, the chunks' partials are summed in fp64 (nothing at this scale), and the fp32 rounding of the stored
norm moves its square by 2u: a term passes through at most CHAIN + TREE_DEPTH roundings, all terms are positive, so
    |norm^2 - sum g^2| <= (CHAIN + TREE_DEPTH + 2) u * sum g^2            (SUMSQ_REL; must not exceed 64 u)
(exact for inv_scale = NULL or a power of two; another scale would add 2u for its product).  The coefficient
min(1, max_norm / (norm + 1e-6)) is 1-Lipschitz in max_norm / (norm + 1e-6), whose relative error is half the norm's square's plus
the addition and the division: COEF_REL = SUMSQ_REL / 2 + 3u.

Update, per element, in the kernel's order (adamw_update; no contraction except the two written fmas):
    g  = (grad * inv_scale) * coef                  2 roundings, + the coefficient's error:        rg = 2u + COEF_REL
    m' = fma(beta1, m, omb1 * g)                    omb1 = 1 - beta1 (u), the product (u), the fma (u of m'; counted u|beta1 m| on top
                                                    so that an unfused evaluation is covered too)
         E_m = u (|m'| + |beta1 m|) + (rg + 2u) |(1 - beta1) g|
    v' = fma(beta2, v, (omb2 * g) * g)              omb2 (u), two products (2u), g twice (2 rg)
         E_v = u (|v'| + |beta2 v|) + (2 rg + 3u) (1 - beta2) g^2
    d  = sqrt(v') / sqrt_bc2 + eps                  sqrt of a value off by E_v: E_v / (2 v') relative; sqrt, the stored fp32 sqrt_bc2
                                                    and the division (3u); the addition (u d)
         E_d = s (E_v / (2 v') + 3u) + u d,  s = sqrt(v') / sqrt(bc2)
    p1 = p * decay, decay = 1 - lr * wd             lr * wd (u, absolute <= u), the subtraction (u), the product (u): 3u |p1|
    w  = (step_size * m') / d, step_size = lr / bc1 bc1 stored in fp32 (u), three operations (3u), the errors of m' and d
         E_w = |w| (4u + E_d / d) + step_size E_m / d
    p' = p1 - w                                     E_p = 3u |p1| + E_w + u |p'|
Each bound is then DOUBLED: first-order terms only were counted, and tests/test_optim_ref_cpu.py demands that a plain fp32 torch
evaluation of the same formulas stays within HALF of what is asserted.  ``param`` has no bound: it is the round-to-nearest-even
cast of the stored master, compared bit for bit."""
from __future__ import annotations

import math
import os
import re

import torch

U32 = 2.0 ** -24
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def kernel_constants():
    """kOptimThreads, kOptimVecs, kOptimTreeDepth, kOptimTable as tp_optim.hip states them."""
    src = open(os.path.join(ROOT, "tokenpacker_amd", "csrc", "tp_optim.hip")).read()
    return {k: int(re.search(rf"constexpr int {k} = (\d+);", src).group(1))
            for k in ("kOptimThreads", "kOptimVecs", "kOptimTreeDepth", "kOptimTable")}


_K = kernel_constants()
CHAIN = 4 * _K["kOptimVecs"]                       # terms of a lane's serial chain
CHUNK = _K["kOptimThreads"] * CHAIN                # elements per workgroup
TREE_DEPTH = _K["kOptimTreeDepth"]
TABLE = _K["kOptimTable"]                          # tensors of one launch
SUMSQ_REL = (CHAIN + TREE_DEPTH + 2) * U32
COEF_REL = 0.5 * SUMSQ_REL + 3 * U32
RECIPES = ("l2_coupled_decay", "no_bias_correction", "eps_inside_sqrt", "coef_not_clamped", "step_off_by_one")


def f32(x: float) -> float:
    """The fp32 value the C ABI carries for a Python float."""
    return float(torch.tensor(float(x), dtype=torch.float32))


class Hyper:
    def __init__(self, beta1=0.9, beta2=0.999, eps=1e-8, max_grad_norm=1.0):
        self.beta1, self.beta2, self.eps, self.max_grad_norm = f32(beta1), f32(beta2), f32(eps), f32(max_grad_norm)

    @property
    def clips(self) -> bool:
        return self.max_grad_norm > 0 and math.isfinite(self.max_grad_norm)


def sumsq_ref(grads, inv_scale: float = 1.0, dtype=torch.float64) -> float:
    """sum over every tensor of (grad * inv_scale)^2, evaluated in `dtype` (fp32: per-tensor norms, then their norm — what
    clip_grad_norm_ does)."""
    if dtype == torch.float64:
        return float(sum(((g.double() * inv_scale) ** 2).sum() for g in grads))
    norms = torch.stack([torch.linalg.vector_norm(g.to(dtype) * inv_scale) for g in grads])
    return float(torch.linalg.vector_norm(norms).double() ** 2)


def coef_ref(norm: float, hyper: Hyper, dtype=torch.float64, clamp: bool = True) -> float:
    if not hyper.clips:
        return 1.0
    q = torch.tensor(hyper.max_grad_norm, dtype=dtype) / (torch.tensor(norm, dtype=dtype) + torch.tensor(1e-6, dtype=dtype))
    return float(torch.clamp(q, max=1.0) if clamp else q)


def step_ref(tensors, hyper: Hyper, step_before: int, inv_scale: float = 1.0, dtype=torch.float64, recipe: str = "adamw"):
    """One step from the state `tensors` = [{"p", "g", "m", "v" (fp32 tensors), "lr", "wd"}] with `step_before` steps applied.
    -> {"norm", "coef", "found_inf", "step", "out": [(p', m', v')] in `dtype`}.  A non-finite norm leaves everything as it is.
    `recipe`: "adamw" (the kernel's), or one of RECIPES — a named WRONG recipe the bounds have to exclude."""
    assert recipe == "adamw" or recipe in RECIPES, recipe
    sumsq = sumsq_ref([t["g"] for t in tensors], inv_scale, dtype)
    norm = math.sqrt(sumsq) if sumsq >= 0 else float("nan")
    if not math.isfinite(norm):
        return {"norm": norm, "coef": 0.0, "found_inf": 1, "step": step_before,
                "out": [(t["p"].to(dtype), t["m"].to(dtype), t["v"].to(dtype)) for t in tensors]}
    coef = coef_ref(norm, hyper, dtype, clamp=recipe != "coef_not_clamped")
    step = step_before + (2 if recipe == "step_off_by_one" else 1)
    b1, b2 = hyper.beta1, hyper.beta2
    bc1, bc2 = (1.0, 1.0) if recipe == "no_bias_correction" else (1.0 - b1 ** step, 1.0 - b2 ** step)
    out = []
    for t in tensors:
        lr, wd = f32(t["lr"]), f32(t["wd"])
        p, m, v = t["p"].to(dtype), t["m"].to(dtype), t["v"].to(dtype)
        g = (t["g"].to(dtype) * inv_scale) * coef
        if recipe == "l2_coupled_decay":
            g = g + wd * p
        else:
            p = p * (1.0 - lr * wd)
        m = b1 * m + (1.0 - b1) * g
        v = b2 * v + ((1.0 - b2) * g) * g
        if recipe == "eps_inside_sqrt":
            denom = torch.sqrt(v / bc2 + hyper.eps)
        else:
            denom = torch.sqrt(v) / math.sqrt(bc2) + hyper.eps
        p = p - ((lr / bc1) * m) / denom
        out.append((p, m, v))
    return {"norm": norm, "coef": coef, "found_inf": 0, "step": step_before + 1, "out": out}


def bounds(tensors, hyper: Hyper, step_before: int, ref, inv_scale: float = 1.0):
    """Elementwise bounds [(E_p, E_m, E_v)] for the fp64 result `ref` = step_ref(tensors, ...) (the derivation: module docstring)."""
    u, b1, b2 = U32, hyper.beta1, hyper.beta2
    rg = 2 * u + (COEF_REL if hyper.clips else 0.0)
    step = step_before + 1
    bc1, sbc2 = 1.0 - b1 ** step, math.sqrt(1.0 - b2 ** step)
    tiny = 2.0 ** -126                                  # below this fp32 is on its subnormal grid: absolute, not relative, roundings
    out = []
    for t, (p2, m2, v2) in zip(tensors, ref["out"]):
        lr, wd = f32(t["lr"]), f32(t["wd"])
        p, m, v = t["p"].double(), t["m"].double(), t["v"].double()
        g = (t["g"].double() * inv_scale) * ref["coef"]
        e_m = u * (m2.abs() + (b1 * m).abs()) + (rg + 2 * u) * ((1.0 - b1) * g).abs()
        e_v = u * (v2.abs() + (b2 * v).abs()) + (2 * rg + 3 * u) * (1.0 - b2) * g * g
        s = torch.sqrt(v2) / sbc2
        d = s + hyper.eps
        rel_sqrt = torch.where(v2 > 0, e_v / (2 * v2.clamp(min=1e-300)), torch.zeros_like(v2))
        e_d = s * (rel_sqrt + 3 * u) + u * d
        step_size = lr / bc1
        w = (step_size * m2) / d
        e_w = w.abs() * (4 * u + e_d / d) + step_size * e_m / d
        p1 = p * (1.0 - lr * wd)
        e_p = 3 * u * p1.abs() + e_w + u * p2.abs()
        out.append((2 * e_p + tiny, 2 * e_m + tiny, 2 * e_v + tiny))
    return out


def worst_ratio(got: torch.Tensor, ref: torch.Tensor, bound: torch.Tensor) -> float:
    """max over the elements of |got - ref| / bound (0 / 0 = 0, a NaN = inf): <= 1 passes."""
    err = (got.double() - ref.double()).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    r = torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)
    return float(r.max()) if r.numel() else 0.0


def cast_ref(master: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """The parameter the step stores: the stored fp32 master rounded to nearest even, no clamp."""
    return master.to(torch.float32).to(dtype)


# ---- inputs ------------------------------------------------------------------------------------------------------------------
# numel of the tensors of a case: one element, below / at a vector, around a chunk, several chunks and a tail
NUMELS = (1, 7, 8, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 5)
LRS = (1e-3, 5e-4, 2e-3)
GRAD_SCALE = {"below": 1e-3, "above": 1e-1}           # norm ~ 0.17 (< max_grad_norm = 1: no clipping) | ~ 17 (clipped)


def make_tensors(numels, seed: int, device="cpu", param_dtype=torch.bfloat16):
    """The state before a first step: masters that are exact in `param_dtype` (they start as p.float()), zero moments;
    weight_decay 0.1 on every other tensor, 0 on the rest; a different lr per tensor."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for i, n in enumerate(numels):
        p = (0.02 * torch.randn(n, generator=g)).to(param_dtype).float().to(device)
        out.append({"p": p, "m": torch.zeros(n, device=device), "v": torch.zeros(n, device=device), "g": None,
                    "lr": LRS[i % len(LRS)], "wd": 0.1 if i % 2 == 0 else 0.0})
    return out


def make_grads(numels, seed: int, step: int, kind: str, device="cpu"):
    """Gradients of step `step`: normal at GRAD_SCALE[kind]; every third tensor at magnitude ~1e-8, where eps = 1e-8 decides the
    update (and exact zeros in it: v = 0, the update's 0 / eps)."""
    g = torch.Generator().manual_seed(1000 * seed + step)
    out = []
    for i, n in enumerate(numels):
        x = torch.randn(n, generator=g) * (1e-8 if i % 3 == 2 else GRAD_SCALE[kind])
        if i % 3 == 2 and n > 2:
            x[::5] = 0.0
        out.append(x.to(device))
    return out
