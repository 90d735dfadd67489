"""Proof of tests/bwd_ref.py before any GPU run (no GPU, no library): for every reference of a backward kernel
  (a) the float64 formula equals torch autograd in float64 (1e-12 relative);
  (b) the bound has room: a plain float32 torch evaluation of the same formula stays within 0.5 x the bound's fp32-class part (the
      output rounding excluded: the fp32 evaluation is not rounded to the output type) at every case tests/test_gpu_bwd_kernels.py
      runs — 2 x left for the GPU's different but same-class rounding (v_exp_f32, v_rcp_f32, another summation tree);
  (c) the bound bites: a deliberately wrong evaluation fails it."""
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import tokenpacker_oracle as orc
from tests import bwd_ref as br

F32, F64 = torch.float32, torch.float64
ROOM = 0.5


def _close(a, b, what):
    scale = float(b.abs().max()) + 1e-300
    assert float((a - b).abs().max()) <= 1e-12 * scale, what


# ---- LayerNorm backward --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", br.LN_FAMILIES)
def test_ln_backward_equals_autograd(family):
    dy, x, _, gamma, beta = br.ln_inputs(family, 37, torch.float16, 1)
    xd = x.double().requires_grad_(True)
    gd, bd = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    y = F.layer_norm(xd, (br.E,), gd, bd, eps=1e-6)
    y.backward(dy.double())
    mu = x.double().mean(1)
    rstd = 1.0 / torch.sqrt(((x.double() - mu[:, None]) ** 2).mean(1) + 1e-6)
    r = br.ln_backward_ref(dy, x, torch.stack([mu, rstd], 1), gamma.double(), beta.double())
    _close(r["dx"], xd.grad, "dx")
    _close(r["dgamma_terms"].sum(0), gd.grad, "dgamma")
    _close(r["dbeta_terms"].sum(0), bd.grad, "dbeta")
    _close(r["xn"], y.detach(), "xn")
    t, _ = br.transpose_ref(x, 40, torch.float16, torch.stack([mu, rstd], 1), gamma.double(), beta.double())
    _close(t[:, :37], y.detach().t(), "transpose with LayerNorm")
    assert float(t[:, 37:].abs().max()) == 0.0


def _ln_room(rows, family, gdtype, seed, chunk=8192):
    dy, x, mr, gamma, beta = br.ln_inputs(family, rows, gdtype, seed)
    worst = {"dx": 0.0, "xn": 0.0, "transpose": 0.0}
    sums = {k: [torch.zeros(br.E, dtype=F32), torch.zeros(br.E, dtype=F64), torch.zeros(br.E, dtype=F64)] for k in ("dgamma", "dbeta")}
    for r0 in range(0, rows, chunk):
        sl = slice(r0, r0 + chunk)
        ref = br.ln_backward_ref(dy[sl], x[sl], mr[sl], gamma, beta, gdtype=F32)
        lo = br.ln_backward_ref(dy[sl], x[sl], mr[sl], gamma, beta, gdtype=F32, dtype=F32)
        worst["dx"] = max(worst["dx"], br.worst_ratio(lo["dx"], ref["dx"], ref["dx_bound"]))
        worst["xn"] = max(worst["xn"], br.worst_ratio(lo["xn"], ref["xn"], ref["xn_bound"]))
        if rows <= 1023:
            tref, tb = br.transpose_ref(x[sl], x[sl].shape[0] + 3, F32, mr[sl], gamma, beta)
            tlo, _ = br.transpose_ref(x[sl], x[sl].shape[0] + 3, F32, mr[sl], gamma, beta, dtype=F32)
            worst["transpose"] = max(worst["transpose"], br.worst_ratio(tlo, tref, tb))
        for k in ("dgamma", "dbeta"):
            sums[k][0] += lo[k + "_terms"].sum(0)
            sums[k][1] += ref[k + "_terms"].sum(0)
            sums[k][2] += ref[k + "_terms"].abs().sum(0)
    for nblocks in br.LN_NBLOCKS:
        d = br.sum_depth(rows, nblocks)
        for k in ("dgamma", "dbeta"):
            worst[f"{k}/{nblocks}"] = br.worst_ratio(sums[k][0], sums[k][1], d * br.EPS32 * sums[k][2])
    return worst


@pytest.mark.parametrize("family", br.LN_FAMILIES)
@pytest.mark.parametrize("rows", [r for r in br.LN_ROWS if r not in br.FULL_ROWS])
def test_ln_backward_bound_has_room(family, rows):
    for gdtype in br.GDTYPES:
        worst = _ln_room(rows, family, gdtype, 100 + rows)
        assert max(worst.values()) <= ROOM, (family, rows, gdtype, worst)


@pytest.mark.parametrize("rows,family", br.LN_FULL_CASES)
def test_ln_backward_bound_has_room_full_size(rows, family):
    worst = _ln_room(rows, family, torch.bfloat16, 100 + rows)
    assert max(worst.values()) <= ROOM, (family, rows, worst)


def test_ln_backward_bound_bites():
    dy, x, mr, gamma, beta = br.ln_inputs("plain", 36, torch.float16, 7)
    ref = br.ln_backward_ref(dy, x, mr, gamma, beta, gdtype=torch.float16)
    good = ref["dx"].to(torch.float16)
    assert br.worst_ratio(good, ref["dx"], ref["dx_bound"]) <= 1.0
    # the xhat * mean(g xhat) term dropped for one row
    xh = (x.double() - mr[:, 0:1].double()) * mr[:, 1:2].double()
    g = dy.double() * gamma.double()
    wrong = ref["dx"].clone()
    wrong[17] = (mr[17, 1].double() * (g[17] - g[17].mean())).to(torch.float16).double()
    assert br.worst_ratio(wrong, ref["dx"], ref["dx_bound"]) > 1.0
    assert float((xh[17] * (g[17] * xh[17]).mean()).abs().max()) > 0
    # one output element moved by 2 ulp of the output type
    bits = good.clone().view(torch.int16)
    bits[5, 100] += 2
    assert br.worst_ratio(bits.view(torch.float16), ref["dx"], ref["dx_bound"]) > 1.0
    xn = ref["xn"].to(torch.float16).view(torch.int16)
    xn[3, 9] += 2
    assert br.worst_ratio(xn.view(torch.float16), ref["xn"], ref["xn_bound"]) > 1.0


# ---- sums ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,C,ld", br.COLSUM_CASES)
def test_colsum_bound_has_room_and_integer_sums_are_exact(R, C, ld):
    g = torch.Generator().manual_seed(R + C)
    for dtype in br.GDTYPES:
        if R in br.FULL_ROWS and dtype != torch.bfloat16:
            continue
        v = torch.randn(R, C, generator=g).to(dtype)
        depth = br.sum_depth(R, 1)                                    # (one slice: the smallest depth any launch can have is larger)
        ref, bound = br.colsum_ref(v, depth)
        lo, _ = br.colsum_ref(v, depth, dtype=F32)
        bound = bound - br.round_bound(ref, F32)
        assert br.worst_ratio(lo, ref, bound) <= ROOM, (R, C, dtype)
        iv = torch.randint(-8, 9, (R, C), generator=g).to(dtype)
        assert torch.equal(br.colsum_ref(iv, depth, dtype=F32)[0].double(), iv.double().sum(0))   # every partial sum exact in fp32


def test_colsum_bound_bites():
    g = torch.Generator().manual_seed(3)
    v = torch.randn(4097, 520, generator=g).to(torch.bfloat16)
    ref, bound = br.colsum_ref(v, br.sum_depth(4097, 64))
    assert br.worst_ratio(v[:-1].double().sum(0), ref, bound) > 1.0           # the last row left out
    assert br.worst_ratio(v.double().sum(0), ref, bound) == 0.0
    iv = torch.randint(-8, 9, (65, 8), generator=g).to(torch.bfloat16)
    iv[64] = 1.0
    assert not torch.equal(iv[:-1].double().sum(0), iv.double().sum(0))          # the integer case: zero tolerance


# ---- dynamic scale -------------------------------------------------------------------------------------------------------------
def test_dynamic_scale_ref():
    for e in range(-70, 71):
        for m in (1.0, 1.5, 1.9999999):
            a = m * 2.0 ** e
            S, inv = br.dynamic_scale_ref(a)
            assert S * inv == 1.0 and math.frexp(S)[0] == 0.5
            k = round(math.log2(S))
            assert abs(k) <= 60
            if abs(k) < 60:
                assert 16.0 <= a * S < 32.0, (a, S)
    assert br.dynamic_scale_ref(16.0) == (1.0, 1.0) and br.dynamic_scale_ref(32.0) == (0.5, 2.0)
    assert br.dynamic_scale_ref(math.nextafter(32.0, 0.0)) == (1.0, 1.0)
    for a in (0.0, math.inf, math.nan):
        assert br.dynamic_scale_ref(a) == (1.0, 1.0)
    assert br.dynamic_scale_ref(2.0 ** -133)[0] == 2.0 ** 60                   # a bf16 subnormal
    assert br.dynamic_scale_ref(17.0) != br.dynamic_scale_ref(34.0)            # (bites: k off by one is another S)


# ---- attention backward --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", br.ATTN_VARIANTS)
@pytest.mark.parametrize("grid,s,B", [(24, 4, 2), (8, 2, 3), (24, 12, 1), (24, 1, 1)])
def test_attention_backward_equals_autograd(variant, grid, s, B):
    q, k, v, dout, mask, mode = br.attn_inputs(grid, s, B, torch.float16, variant, 5)
    qd, kd, vd = (t.double().requires_grad_(True) for t in (q, k, v))
    md = mask.double().requires_grad_(True) if mode else None
    o = br.attention_forward(qd, kd, vd, grid, s, md, mode)
    o.backward(dout.double())
    r = br.attention_bwd_ref(q, k, v, dout, grid, s, mask, mode)
    _close(r["dq"], qd.grad, "dq")
    _close(r["dk"], kd.grad, "dk")
    _close(r["dv"], vd.grad, "dv")
    if mode:
        _close(r["dmask"], md.grad.reshape(r["dmask"].shape), "dmask")
    # ... and the forward this differentiates is the oracle's attention (identity in-projection)
    eye, zero = torch.eye(br.E, dtype=F64).repeat(3, 1), torch.zeros(3 * br.E, dtype=F64)
    am = None
    if mode:
        am = mask.double().reshape(1, s * s) if mode == 1 else mask.double().reshape(-1, 1, s * s)
    _close(o.detach(), orc.region_attention(q.double(), k.double(), v.double(), eye, zero, grid, s, attn_mask=am), "forward")


@pytest.mark.parametrize("variant", br.ATTN_VARIANTS)
@pytest.mark.parametrize("grid,s,B", br.ATTN_CASES)
def test_attention_backward_bound_has_room(variant, grid, s, B):
    q, k, v, dout, mask, mode = br.attn_inputs(grid, s, B, torch.bfloat16, variant, 11 + s)
    ref = br.attention_bwd_ref(q, k, v, dout, grid, s, mask, mode, gdtype=F32)
    lo = br.attention_bwd_ref(q, k, v, dout, grid, s, mask, mode, gdtype=F32, dtype=F32)
    if variant == "peaked" and s > 1:
        assert float(ref["p"].max()) > 0.99
    worst = {n: br.worst_ratio(lo[n], ref[n], ref[n + "_bound"]) for n in ("dq", "dk", "dv")}
    if mode == 2:
        worst["dmask"] = br.worst_ratio(lo["dmask"], ref["dmask"], ref["dmask_bound"])
    if mode == 1:
        nq = B * (grid // s) ** 2
        bound = ref["dmask_bound"] + (br.sum_depth(nq, 1) + 8) * br.EPS32 * ref["dmask_abs"]
        worst["dmask"] = br.worst_ratio(lo["dmask"], ref["dmask"], bound)
    if s == 1:                                                   # exact: dQ = dK = 0, dV = dO
        assert worst["dq"] == worst["dk"] == worst["dv"] == 0.0
    assert max(worst.values()) <= ROOM, worst


def test_attention_backward_bound_bites():
    grid, s, B = 24, 4, 1
    q, k, v, dout, mask, mode = br.attn_inputs(grid, s, B, torch.float16, "mask2", 9)
    ref = br.attention_bwd_ref(q, k, v, dout, grid, s, mask, mode, gdtype=torch.float16)
    good = ref["dk"].to(torch.float16)
    assert br.worst_ratio(good, ref["dk"], ref["dk_bound"]) <= 1.0
    # one key's dK (region 3, head 2, key 5) computed with the previous key's p
    G, S2 = grid // s, s * s
    Q = q.double().reshape(B, G, G, br.HEADS, br.HEAD_DIM)
    V = orc.region_gather(v.double(), grid, s).reshape(B, G, G, S2, br.HEADS, br.HEAD_DIM)
    P = ref["p"]
    dP = torch.einsum("bijhd,bijkhd->bijhk", dout.double().reshape(B, G, G, br.HEADS, br.HEAD_DIM), V)
    D = (P * dP).sum(-1, keepdim=True)
    i, j, h, kk = 0, 3, 2, 5
    ds_wrong = P[0, i, j, h, kk - 1] * (dP[0, i, j, h, kk] - D[0, i, j, h, 0])
    wrong = orc.region_gather(ref["dk"].clone(), grid, s).reshape(B, G, G, S2, br.HEADS, br.HEAD_DIM)
    wrong[0, i, j, kk, h] = ds_wrong * Q[0, i, j, h] * br.INV_SQRT_D
    wrong = br.region_scatter(wrong.reshape(B, G, G, S2, br.E), grid, s)
    assert br.worst_ratio(wrong.to(torch.float16), ref["dk"], ref["dk_bound"]) > 1.0
    dm = ref["dmask"].clone()
    dm[100, 3] *= 1.001
    assert br.worst_ratio(dm, ref["dmask"], ref["dmask_bound"]) > 1.0


# ---- point-query transpose -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid,s", br.PQ_CASES)
def test_point_queries_bwd_equals_autograd_of_the_oracle_downsample(grid, s):
    B, C = 2, 16
    g = torch.Generator().manual_seed(s)
    x = torch.randn(B, grid * grid, C, generator=g, dtype=F64).requires_grad_(True)
    dq0 = torch.randn(B * (grid // s) ** 2, C, generator=g)
    q = orc.point_queries(x, grid, s)
    q.backward(dq0.double().reshape(q.shape))
    for inv in (1.0, 2.0 ** -9):
        ref = br.point_queries_bwd_ref(dq0, B, grid, s, inv)
        _close(ref, x.grad * inv, "dx")
        for dtype in br.GDTYPES:                                  # a move: the fp32 evaluation IS the value, one rounding
            assert torch.equal(br.cast_exact(ref, dtype), br.cast_exact(br.point_queries_bwd_ref(dq0, B, grid, s, inv, dtype=F32), dtype))
    if s > 1:                                                     # bites: the weight on a neighbouring pixel
        wrong = torch.roll(br.point_queries_bwd_ref(dq0, B, grid, s), 1, dims=1)
        assert not torch.equal(br.cast_exact(wrong, torch.float16), br.cast_exact(br.point_queries_bwd_ref(dq0, B, grid, s), torch.float16))


# ---- gelu' and the data-gradient epilogue --------------------------------------------------------------------------------------
def test_gelu_grad_equals_autograd_has_room_and_bites():
    z = br.gelu_z(64, 256, 1)
    zd = z.double().requires_grad_(True)
    F.gelu(zd).sum().backward()
    ref = br.gelu_grad_ref(z)
    _close(ref, zd.grad, "gelu'")
    bound = torch.full_like(ref, br.GELU_GRAD_ABS)
    assert br.worst_ratio(br.gelu_grad_ref(z, F32), ref, bound) <= ROOM
    assert br.worst_ratio(ref + 1e-3, ref, bound) > 1.0


@pytest.mark.parametrize("M,N,K", br.DGRAD_CASES)
def test_linear_bwd_bound_has_room_and_bites(M, N, K):
    g = torch.Generator().manual_seed(M)
    dy = torch.randn(M, K, generator=g).half()
    w = (torch.randn(N, K, generator=g) * K ** -0.5).half()
    z = br.gelu_z(M, N, 2)
    for zz, sc in ((None, 1.0), (z, 1.0), (z, 2.0 ** -6)):
        ref, bound = br.linear_bwd_ref(dy, w, zz, sc, out_dtype=F32)
        lo, _ = br.linear_bwd_ref(dy, w, zz, sc, out_dtype=F32, dtype=F32)
        assert br.worst_ratio(lo, ref, bound) <= ROOM, (M, N, K, sc)
    ref, bound = br.linear_bwd_ref(dy, w, z, 1.0, out_dtype=torch.float16)
    assert br.worst_ratio(ref.to(torch.float16), ref, bound) <= 1.0
    wrong = (dy.double() @ w.double().t()) * (br.gelu_grad_ref(z) + 1e-3)          # a gelu' off by 1e-3
    assert br.worst_ratio(wrong.to(torch.float16), ref, bound) > 1.0
    # out_scale is exact: the scaled reference is the unscaled one times 2^-6, before the one rounding
    assert torch.equal(br.linear_bwd_ref(dy, w, z, 2.0 ** -6)[0], ref * 2.0 ** -6)


# ---- moves and casts -----------------------------------------------------------------------------------------------------------
def test_cast_exact_is_torchs_rounding_with_the_fp16_clamp():
    v = torch.tensor([1.0, 65519.0, 65520.0, 1e6, -1e6, 2.0 ** -25, 3 * 2.0 ** -26, 1 + 2.0 ** -11], dtype=F64)
    h = br.cast_exact(v, torch.float16)
    assert h.tolist() == [1.0, 65504.0, 65504.0, 65504.0, -65504.0, 0.0, 2.0 ** -24, 1.0]
    assert br.cast_exact(v, torch.bfloat16)[3].item() == 999424.0
    a = torch.arange(24, dtype=F32).reshape(3, 8).half()
    ref, bound = br.transpose_ref(a, 8, torch.float16)
    assert bound is None and torch.equal(ref[:, :3], a.double().t()) and float(ref[:, 3:].abs().max()) == 0.0
    moved = br.cast_exact(ref, torch.float16).view(torch.int16).clone()
    moved[2, 1] += 2                                              # one element moved by 2 ulp: bit comparison fails
    assert not torch.equal(moved.view(torch.float16), br.cast_exact(ref, torch.float16))
