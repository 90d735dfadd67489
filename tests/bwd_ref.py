"""fp64 references of the backward's kernels (tokenpacker_amd/csrc/tp_bwd.hip, point_queries_bwd_kernel, the TP_LINEAR_GELU_BWD /
out_scale epilogue), one plain torch function per kernel, with the ELEMENTWISE error bound each comparison uses.

Every function takes the same rounded operands the kernel gets and works on whatever device they live on (the two full-size row
counts are referenced on the GPU in float64; everything else on the CPU).  ``dtype`` is the arithmetic the formula is evaluated
in: float64 for the reference, float32 for the "the bound has room" proof of tests/test_bwd_ref_cpu.py.

Bounds are derived, not tuned:
  * U[T] is the half-ulp of the output type T relative to the value (2^-11 fp16, 2^-8 bf16, 2^-24 fp32); an fp16 result below
    2^-14 lands on the subnormal grid, half a quantum = 2^-25 absolute;
  * a sum whose terms pass through at most d additions errs by at most d * 2^-24 * sum|terms|;
  * moves and casts are exact: compared bit for bit with torch's rounding of the exact fp32 value (``cast_exact``).
The input generators and the case lists of tests/test_gpu_bwd_kernels.py live here too, so that the CPU proof runs over the very
cases the GPU tests run."""
from __future__ import annotations

import math

import torch

from oracle import tokenpacker_oracle as orc

E, HEADS, HEAD_DIM = 1024, 8, 128
EPS32 = 2.0 ** -24
U = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8, torch.float32: 2.0 ** -24}
F16_MAX = 65504.0
SAT_THRESHOLD = 65520.0          # what IEEE rounding would turn into an fp16 inf
INV_SQRT_D = 1.0 / math.sqrt(HEAD_DIM)


# ---- rounding ------------------------------------------------------------------------------------------------------------------
def cast_exact(v: torch.Tensor, dtype: torch.dtype, clamp: bool = True) -> torch.Tensor:
    """torch's own rounding to `dtype` of a value that is exact in fp32 (asserted), with the kernels' +-65504 clamp for fp16
    (`clamp` False: plain IEEE rounding, an overflow is an inf)."""
    f = v.to(torch.float32)
    assert torch.equal(f.to(v.dtype), v) or bool(torch.isnan(v).any()), "cast_exact: the value is not exact in fp32"
    if dtype == torch.float16 and clamp:
        f = f.clamp(-F16_MAX, F16_MAX)
    return f.to(dtype)


def round_bound(ref: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """One rounding of `ref` to `dtype`: half an ulp."""
    b = U[dtype] * ref.abs()
    return b.clamp(min=2.0 ** -25) if dtype == torch.float16 else b


def worst_ratio(got: torch.Tensor, ref: torch.Tensor, bound: torch.Tensor) -> float:
    """max over the elements of |got - ref| / bound (0 / 0 = 0, x / 0 = inf): <= 1 passes."""
    err = (got.to(ref.dtype) - ref).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    r = torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)
    return float(r.max()) if r.numel() else 0.0


# ---- sums ----------------------------------------------------------------------------------------------------------------------
def sum_depth(rows: int, groups: int) -> int:
    """Upper estimate of the longest addition chain of a two-stage sum of `rows` terms over `groups` slices / workgroups whose
    threads each own every 4th row: ceil(rows / (4 groups)) in the thread, then the lane / slice / stage-2 trees (<= 64)."""
    return -(-int(rows) // (4 * max(1, int(groups)))) + 64


def colsum_ref(v: torch.Tensor, depth: int, out_dtype: torch.dtype = torch.float32, out_scale: float = 1.0, dtype=torch.float64,
               chunk: int = 16384):
    """Column sums of v [R, C] times out_scale (a power of two) -> (ref [C], bound [C]); row chunks keep the widened copy small."""
    ref = torch.zeros(v.shape[1], dtype=dtype, device=v.device)
    tot = torch.zeros(v.shape[1], dtype=torch.float64, device=v.device)
    for r0 in range(0, v.shape[0], chunk):
        w = v[r0:r0 + chunk].to(dtype)
        ref += w.sum(0)
        tot += w.abs().sum(0).double()
    ref = ref * out_scale
    return ref, round_bound(ref.double(), out_dtype) + depth * EPS32 * tot * abs(out_scale)


# ---- transposes ----------------------------------------------------------------------------------------------------------------
def transpose_ref(a: torch.Tensor, rpad: int, out_dtype: torch.dtype, mean_rstd=None, gamma=None, beta=None, dtype=torch.float64):
    """dst [C, rpad] of the [R, C] matrix `a`: -> (ref, bound); bound None = a move (compare bits with cast_exact(ref))."""
    R, C = a.shape
    w = a.to(dtype)
    ref = torch.zeros(C, rpad, dtype=dtype, device=a.device)
    if mean_rstd is None:
        ref[:, :R] = w.t()
        return ref, None
    mu, rstd = mean_rstd[:, 0:1].to(dtype), mean_rstd[:, 1:2].to(dtype)
    gm, bt = gamma.to(dtype)[None, :], beta.to(dtype)[None, :]
    t = (w - mu) * rstd * gm
    ref[:, :R] = (t + bt).t()
    extra = torch.zeros(C, rpad, dtype=torch.float64, device=a.device)
    extra[:, :R] = (8 * EPS32 * (t.abs() + bt.abs())).double().t()
    return ref, round_bound(ref.double(), out_dtype) + extra


# ---- dynamic scale -------------------------------------------------------------------------------------------------------------
def dynamic_scale_ref(amax: float):
    """(S, 1 / S): S = 2^k with amax * S in [16, 32), |k| <= 60; 1 for 0 / inf / NaN."""
    if not (amax > 0.0 and amax < math.inf):
        return 1.0, 1.0
    _, e = math.frexp(amax)
    k = max(-60, min(60, 5 - e))
    return 2.0 ** k, 2.0 ** -k


# ---- LayerNorm backward --------------------------------------------------------------------------------------------------------
def ln_backward_ref(dy, x, mean_rstd, gamma, beta=None, gdtype=torch.float16, dtype=torch.float64):
    """dy [rows, E] (gdtype), x [rows, E] fp16, mean_rstd fp32 [rows, 2] (used as given), gamma / beta fp32 [E] ->
    dict(dx, dx_bound, xn, xn_bound, dgamma_terms, dbeta_terms): the *_terms are the per-row summands of dgamma / dbeta."""
    dyw, xw = dy.to(dtype), x.to(dtype)
    mu, rstd = mean_rstd[:, 0:1].to(dtype), mean_rstd[:, 1:2].to(dtype)
    gm = gamma.to(dtype)[None, :]
    xh = (xw - mu) * rstd
    g = dyw * gm
    m1, m2 = g.mean(1, keepdim=True), (g * xh).mean(1, keepdim=True)
    dx = rstd * (g - m1 - xh * m2)
    out = {"dx": dx, "dgamma_terms": dyw * xh, "dbeta_terms": dyw}
    out["dx_bound"] = round_bound(dx.double(), gdtype) + (32 * EPS32 * rstd * (
        g.abs() + g.abs().mean(1, keepdim=True) + xh.abs() * (g * xh).abs().mean(1, keepdim=True))).double()
    if beta is not None:
        bt = beta.to(dtype)[None, :]
        out["xn"] = xh * gm + bt
        out["xn_bound"] = round_bound(out["xn"].double(), gdtype) + (8 * EPS32 * ((xh * gm).abs() + bt.abs())).double()
    return out


# ---- region attention backward -------------------------------------------------------------------------------------------------
def region_scatter(t: torch.Tensor, g: int, s: int) -> torch.Tensor:
    """Inverse of oracle.region_gather: [B, G, G, s*s, c] -> [B, g*g, c]."""
    B, G, _, S2, c = t.shape
    return t.reshape(B, G, G, s, s, c).permute(0, 1, 3, 2, 4, 5).reshape(B, g * g, c)


def mask_regions(mask: torch.Tensor, mode: int, B: int, G: int, s: int, dtype) -> torch.Tensor:
    """The library's two mask layouts ([s*s] | [(M B) 8, s*s], batch index region * B + image) as [B, G, G, 8, s*s]."""
    S2 = s * s
    m = mask.to(dtype)
    if mode == 1:
        return m.reshape(1, 1, 1, 1, S2).expand(B, G, G, HEADS, S2)
    return m.reshape(G * G, B, HEADS, S2).permute(1, 0, 2, 3).reshape(B, G, G, HEADS, S2)


def regions_to_mask2(t: torch.Tensor) -> torch.Tensor:
    """[B, G, G, 8, s*s] -> the mode-2 layout [(M B) 8, s*s]."""
    B, G, _, H, S2 = t.shape
    return t.reshape(B, G * G, H, S2).permute(1, 0, 2, 3).reshape(G * G * B * H, S2)


def attention_forward(q, k, v, g, s, mask=None, mode=0, dtype=torch.float64):
    """softmax(Q K^T / sqrt(128) + mask) V over oracle.region_gather (autograd-friendly): [B, M, E]."""
    B = q.shape[0]
    G, S2 = g // s, s * s
    Q = q.to(dtype).reshape(B, G, G, HEADS, HEAD_DIM)
    K = orc.region_gather(k.to(dtype), g, s).reshape(B, G, G, S2, HEADS, HEAD_DIM)
    V = orc.region_gather(v.to(dtype), g, s).reshape(B, G, G, S2, HEADS, HEAD_DIM)
    logits = torch.einsum("bijhd,bijkhd->bijhk", Q, K) * INV_SQRT_D
    if mode:
        logits = logits + mask_regions(mask, mode, B, G, s, dtype)
    P = torch.softmax(logits, dim=-1)
    return torch.einsum("bijhk,bijkhd->bijhd", P, V).reshape(B, G * G, E)


def attention_bwd_ref(q, k, v, dout, g, s, mask=None, mode=0, gdtype=torch.float16, inv_scale=1.0, dtype=torch.float64):
    """q [B, M, E], k / v [B, g*g, E] fp16, dout [B, M, E] (gdtype), mask fp32 in the layout of `mode` ->
    dict(dq, dk, dv, dmask, *_bound, p): dmask in the mask's layout times inv_scale (mode 1: summed over queries and heads;
    its bound's sum term is added by the caller, who knows the geometry: `dmask_abs` = sum|terms| * inv_scale)."""
    B = q.shape[0]
    G, S2 = g // s, s * s
    M = G * G
    Q = q.to(dtype).reshape(B, G, G, HEADS, HEAD_DIM)
    K = orc.region_gather(k.to(dtype), g, s).reshape(B, G, G, S2, HEADS, HEAD_DIM)
    V = orc.region_gather(v.to(dtype), g, s).reshape(B, G, G, S2, HEADS, HEAD_DIM)
    dO = dout.to(dtype).reshape(B, G, G, HEADS, HEAD_DIM)
    logits = torch.einsum("bijhd,bijkhd->bijhk", Q, K) * INV_SQRT_D
    lam_terms = torch.einsum("bijhd,bijkhd->bijhk", Q.abs(), K.abs()) * INV_SQRT_D
    if mode:
        mr = mask_regions(mask, mode, B, G, s, dtype)
        logits = logits + mr
        lam_terms = lam_terms + torch.where(torch.isinf(mr), torch.zeros_like(mr), mr.abs())
    P = torch.softmax(logits, dim=-1)                                   # [B, G, G, H, S2]
    dP = torch.einsum("bijhd,bijkhd->bijhk", dO, V)
    D = (P * dP).sum(-1, keepdim=True)
    dS = P * (dP - D)
    dV = torch.einsum("bijhk,bijhd->bijkhd", P, dO)
    dK = torch.einsum("bijhk,bijhd->bijkhd", dS, Q) * INV_SQRT_D
    dQ = torch.einsum("bijhk,bijkhd->bijhd", dS, K) * INV_SQRT_D
    # bounds (float64 whatever `dtype`)
    Pd, dPd = P.double(), dP.double()
    un = Pd * (dPd.abs() + (Pd * dPd.abs()).sum(-1, keepdim=True))     # the un-cancelled size of dS_j
    lam = torch.where(Pd > 0, lam_terms.double(), torch.zeros_like(Pd)).amax(-1, keepdim=True)
    c = 1e-5 + 2.0 ** -20 * lam                                         # [B, G, G, H, 1]
    back = lambda t: region_scatter(t.reshape(B, G, G, S2, E), g, s)    # noqa: E731  ([.., S2, H, d] -> [B, N, E])
    out = {"p": P, "dq": dQ.reshape(B, M, E), "dk": back(dK), "dv": back(dV)}
    if s == 1:                                                          # p = 1: dQ = dK = 0 and dV = cast(dO), exactly
        for n in ("dq", "dk"):
            out[n] = torch.zeros_like(out[n])
            out[n + "_bound"] = torch.zeros_like(out[n], dtype=torch.float64)
        out["dv_bound"] = torch.zeros_like(out["dv"], dtype=torch.float64)
    else:
        bdV = torch.einsum("bijhk,bijhd->bijkhd", c * Pd, dO.double().abs())
        bdK = torch.einsum("bijhk,bijhd->bijkhd", c * un, Q.double().abs()) * INV_SQRT_D
        bdQ = torch.einsum("bijhk,bijkhd->bijhd", c * un, K.double().abs()) * INV_SQRT_D
        out["dv_bound"] = round_bound(out["dv"].double(), gdtype) + back(bdV)
        out["dk_bound"] = round_bound(out["dk"].double(), gdtype) + back(bdK)
        out["dq_bound"] = round_bound(out["dq"].double(), gdtype) + bdQ.reshape(B, M, E)
    if mode == 2:
        out["dmask"] = regions_to_mask2(dS) * inv_scale
        out["dmask_bound"] = regions_to_mask2(c * un) * inv_scale
    elif mode == 1:
        out["dmask"] = dS.sum(dim=(0, 1, 2, 3)) * inv_scale
        out["dmask_bound"] = (c * un).sum(dim=(0, 1, 2, 3)) * inv_scale
        out["dmask_abs"] = dS.double().abs().sum(dim=(0, 1, 2, 3)) * inv_scale
    return out


# ---- point-query transpose -----------------------------------------------------------------------------------------------------
def point_queries_bwd_ref(dq0: torch.Tensor, B: int, g: int, s: int, inv_scale: float = 1.0, dtype=torch.float64) -> torch.Tensor:
    """dx [B, g*g, C]: the transpose of the bilinear downsample's integer-ratio form applied to dq0 [B*M, C], times inv_scale —
    even s: weight 1/4 on the inner 2 x 2 of every s x s block, odd s: weight 1 on its centre; exact in fp32."""
    G, C = g // s, dq0.shape[-1]
    d = dq0.to(dtype).reshape(B, G, G, C) * inv_scale
    dx = torch.zeros(B, G, s, G, s, C, dtype=dtype, device=dq0.device)
    if s & 1:
        o = (s - 1) // 2
        dx[:, :, o, :, o] = d
    else:
        h = s // 2
        for a in (h - 1, h):
            for e in (h - 1, h):
                dx[:, :, a, :, e] = 0.25 * d
    return dx.reshape(B, g * g, C)


# ---- gelu' and the data-gradient epilogue --------------------------------------------------------------------------------------
GELU_GRAD_ABS = 6e-7             # A&S 7.1.26's 1.5e-7 on erf, halved in the cdf, + 8 * 2^-24 for the fp32 evaluation


def gelu_grad_ref(z: torch.Tensor, dtype=torch.float64) -> torch.Tensor:
    """d/dz of the exact erf GELU: Phi(z) + z phi(z)."""
    w = z.to(dtype)
    return 0.5 * (1.0 + torch.erf(w * (1.0 / math.sqrt(2.0)))) + w * torch.exp(-0.5 * w * w) * (1.0 / math.sqrt(2.0 * math.pi))


def linear_bwd_ref(dy, w, z=None, out_scale: float = 1.0, out_dtype=torch.float16, dtype=torch.float64):
    """dX = out_scale * (dY [M, K] · W [N, K]^T) * gelu'(Z [M, N]) -> (ref, bound):
    u_T |ref| + 2e-5 max_row|ref| (fp32 accumulation order, the suite's TOL_F32OUT) + 6e-7 |dY · W| (gelu')."""
    acc = dy.to(dtype) @ w.to(dtype).t()
    ref = acc * out_scale
    extra = torch.zeros_like(acc, dtype=torch.float64)
    if z is not None:
        ref = ref * gelu_grad_ref(z, dtype)
        extra = GELU_GRAD_ABS * acc.double().abs() * abs(out_scale)
    rd = ref.double()
    return ref, round_bound(rd, out_dtype) + 2e-5 * rd.abs().amax(1, keepdim=True) + extra


# ================================================================================================================================
# Input generators and case lists shared by tests/test_gpu_bwd_kernels.py and the CPU proof (tests/test_bwd_ref_cpu.py)
# ================================================================================================================================
GDTYPES = (torch.bfloat16, torch.float16)
FULL_ROWS = (18432, 147456)                      # referenced in float64 on the GPU, one gradient dtype
LN_ROWS = (1, 3, 4, 5, 36, 1023) + FULL_ROWS
LN_NBLOCKS = (1, 7, 256)
LN_FAMILIES = ("plain", "mean40", "tinyvar", "mixed")
LN_FULL_CASES = ((18432, "mixed"), (18432, "mean40"), (147456, "plain"), (147456, "tinyvar"))    # (rows, family): bf16, every LN_NBLOCKS
ATTN_CASES = ((24, 1, 2), (24, 2, 3), (24, 3, 1), (24, 4, 3), (24, 6, 2), (24, 8, 1), (24, 8, 3), (24, 12, 3), (16, 4, 1),
              (8, 2, 5))                        # (grid, s, B): s = 8 has 9 queries per image — B M % 4 != 0 twice
ATTN_VARIANTS = ("plain", "peaked", "mask1", "mask2", "mask1_neg", "mask2_inf", "mask1_lead", "mask2_lead")
PQ_CASES = tuple((24, s) for s in (1, 2, 3, 4, 6)) + ((16, 4), (8, 2))
COLSUM_CASES = tuple((R, C, C) for R in (1, 63, 64, 65, 100, 4097) for C in (8, 520, 1024)) + (
    (100, 2048, 4096), (4097, 4096, 4096), (18432, 2048, 4096), (18432, 4096, 4096), (147456, 1024, 2048), (147456, 8, 8))   # (R, C, ld)
REDUCE_CASES = tuple((n, p) for n in (4, 12, 16, 384, 1024) for p in (1, 7, 8, 255, 256, 2304))                                  # (n, nparts)
GELU_Z_SPECIALS = (0.0, -0.0, 0.5, -0.5, 6.0, -6.0, 12.0, -12.0, 100.0, -100.0, 65504.0, -65504.0, 2.0 ** -24, -3 * 2.0 ** -24)
DGRAD_CASES = ((77, 128, 64), (300, 256, 256), (4608, 4096, 256), (18432, 1024, 128))                                         # (M, N, K)


def _gen(seed: int, device):
    return torch.Generator(device=device).manual_seed(seed)


def ln_inputs(family: str, rows: int, gdtype, seed: int, device="cpu", ln_eps: float = 1e-6):
    """(dy, x, mean_rstd, gamma, beta) of one LayerNorm-backward case.  (mean, rstd) are the fp32 rounding of the fp64 statistics
    of the fp16 rows, as the forward's statistics kernels deliver them to within fp32 round-off."""
    g = _gen(seed, device)
    rn = lambda *shape: torch.randn(*shape, generator=g, device=device)     # noqa: E731
    z = rn(rows, E)
    dy = rn(rows, E)
    if family == "plain":
        x = 1.5 * z + 0.3 * rn(rows, 1)
    elif family == "mean40":                       # row mean = 40 sigma
        x = z + 40.0
    elif family == "tinyvar":                      # variance 1e-4
        x = 0.01 * z + 0.5
    elif family == "mixed":                        # rows of mixed scale, 1e-2 .. 1e2, in the values and in the gradient
        sc = 10.0 ** (4.0 * torch.rand(rows, 1, generator=g, device=device) - 2.0)
        x = sc * (z + rn(rows, 1))
        dy = dy * 10.0 ** (2.0 * torch.rand(rows, 1, generator=g, device=device) - 1.0)
    else:
        raise ValueError(family)
    x = x.half()
    xd = x.double()
    mu = xd.mean(1)
    rstd = 1.0 / torch.sqrt(((xd - mu[:, None]) ** 2).mean(1) + ln_eps)
    mean_rstd = torch.stack([mu, rstd], dim=1).float().contiguous()
    gamma = 1.0 + 0.3 * rn(E)
    gamma[::97] = 0.0
    gamma[5::131] = -gamma[5::131].abs() - 0.1
    beta = 0.2 * rn(E)
    return dy.to(gdtype), x, mean_rstd, gamma, beta


def attn_inputs(grid: int, s: int, B: int, gdtype, variant: str, seed: int, device="cpu"):
    """(q, k, v, dout, mask, mode) of one attention-backward case.  Masks never mask a whole row; the `_neg` / `_inf` variants keep
    key 0 visible, the `_lead` variants mask the leading keys and keep the later ones."""
    g = _gen(seed, device)
    M, N, S2 = (grid // s) ** 2, grid * grid, s * s
    q = torch.randn(B, M, E, generator=g, device=device) * (6.0 if variant == "peaked" else 1.0)
    k = torch.randn(B, N, E, generator=g, device=device)
    v = torch.randn(B, N, E, generator=g, device=device)
    dout = torch.randn(B, M, E, generator=g, device=device)
    mask, mode = None, 0
    if variant.startswith("mask"):
        mode = 1 if variant.startswith("mask1") else 2
        rows = 1 if mode == 1 else M * B * HEADS
        mask = 3.0 * torch.randn(rows, S2, generator=g, device=device)
        if S2 > 1 and variant.endswith(("_neg", "_inf")):
            hit = torch.rand(rows, S2, generator=g, device=device) < 0.3
            hit[:, 0] = False                                           # (key 0 always stays: no fully masked row)
            mask[hit] = -1e4 if variant.endswith("_neg") else float("-inf")
            if mode == 1:
                mask[0, S2 - 1] = -1e4 if variant.endswith("_neg") else float("-inf")
        if S2 > 1 and variant.endswith("_lead"):                            # -inf on the LEADING keys 0..3 (mode 2: 0..3 | 0..4 by row)
            lead = torch.full((rows,), 4, device=device)
            lead[1::2] = 5
            lead = lead.clamp(max=S2 - 1)                                   # (at least the last key stays: no fully masked row)
            mask[torch.arange(S2, device=device)[None, :] < lead[:, None]] = float("-inf")
        mask = mask.reshape(S2) if mode == 1 else mask
    return q.half(), k.half(), v.half(), dout.to(gdtype), mask, mode


def gelu_z(M: int, N: int, seed: int, device="cpu"):
    """fp16 pre-activations [M, N]: random in +-4 with the special values of GELU_Z_SPECIALS strewn over every row."""
    g = _gen(seed, device)
    z = (2.0 * torch.randn(M, N, generator=g, device=device)).half()
    sp = torch.tensor(GELU_Z_SPECIALS, dtype=torch.float32, device=device).half()
    for i in range(len(GELU_Z_SPECIALS)):
        z[:, (7 * i + 3) % N] = sp[i]
    return z


# ---- the weight-gradient contraction dW = dY^T · X (tests/test_gpu_wgrad_edges.py) ---------------------------------------------------
WGRAD_FAMILIES = ("ints", "gauss")
WGRAD_TOL = {torch.float32: 1e-5, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}      # max-norm error / max|ref|, by OUTPUT dtype
WGRAD_DIGITS = 7                                 # at most this many base-5 digits of the row number are stamped into x: 78125 rows


def wgrad_ref(dy: torch.Tensor, x: torch.Tensor, rows: int, chunk: int = 4608) -> torch.Tensor:
    """dW [n_out, k_in] = dy[:rows]^T · x[:rows] in float64 on the rounded operands (row chunks keep the widened copies small).
    Rows at and beyond `rows` are never touched: they may hold anything."""
    ref = torch.zeros(dy.shape[1], x.shape[1], dtype=torch.float64, device=dy.device)
    for r0 in range(0, rows, chunk):
        r1 = min(rows, r0 + chunk)
        ref += dy[r0:r1].double().t() @ x[r0:r1].double()
    return ref


def wgrad_operands(family: str, rows: int, n_out: int, k_in: int, dtype, seed: int, device="cpu"):
    """(dy [rows, n_out], x [rows, k_in]) of one weight-gradient case, rounded to `dtype`.
      gauss: N(0, 1).
      ints:  seeded integers in [-2, 2] (exact in bf16 and fp16), made row-dependent: dy[:, 0] = x[:, 0] = 1 and x[r, 1..] = the
             base-5 digits of r, minus 2 (as many digits as `rows` needs — a digit that never left 0 would be a constant column,
             whose sums grow like 2 * rows towards fp16's range).  dy_r (x) x_r = dy_s (x) x_s then forces dy_r = dy_s (column 0 of x), x_r = x_s (column 0 of
             dy) and r = s (the digits): no two token rows contribute the same outer product, so a row that is dropped, counted
             twice or paired with another row's partner changes the exact result.  Every product is an integer of magnitude <= 4 and
             every partial sum one below 4 * rows < 2^24 (rows < 2^22): fp32 accumulation is EXACT in any order, the fp32 result
             equals the float64 reference bit for bit, a 16-bit result equals its one rounding."""
    g = _gen(seed, device)
    if family == "gauss":
        dy = torch.randn(rows, n_out, generator=g, device=device)
        x = torch.randn(rows, k_in, generator=g, device=device)
    elif family == "ints":
        assert rows < 5 ** WGRAD_DIGITS and k_in > WGRAD_DIGITS
        dy = torch.randint(-2, 3, (rows, n_out), generator=g, device=device).float()
        x = torch.randint(-2, 3, (rows, k_in), generator=g, device=device).float()
        r = torch.arange(rows, device=device)
        dy[:, 0] = 1.0
        x[:, 0] = 1.0
        d = 0
        while d == 0 or 5 ** d < rows:
            x[:, 1 + d] = ((r // 5 ** d) % 5 - 2).float()
            d += 1
    else:
        raise ValueError(family)
    return dy.to(dtype), x.to(dtype)
