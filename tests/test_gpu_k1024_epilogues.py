"""The K = 1024 launches of the scale_factor-2 inference forward on every kernel they can be routed to: the second-moment
statistics tile (16 partial sums of squares per row, written by the waves themselves), the K launch's logits without the
softmax-invariant bias term, and the V launch's reduce-scatter with the bias added once.

Shapes: s = 2, D = 4096, fp16 and bf16 with fp32 output.  The batches are the smallest ones that reach each kernel, asked of
tp_test_gemm_route.  A batch is a handful of DISTINCT images repeated: the fp64 oracle runs once on the distinct images, and
every copy is compared with it, so every row of every tile is checked at the oracle's cost for three images."""
import ctypes

import pytest
import torch

from oracle import tokenpacker_oracle as orc
from tests.gpu_util import batch_invariant
from tests.test_gpu_forward import GATE, _module
from tokenpacker_amd import _capi, synth

pytestmark = pytest.mark.gpu

S, D, NDIST = 2, 4096, 3
ROWS = 576                                   # fine tokens per image: B = 1 is two full 256-row tiles + 64 ragged rows
CONFIGS = [(torch.float16, False), (torch.bfloat16, True)]
IDS = ["fp16", "bf16-fp32out"]
ROUTE_NAMES = {0: "128-tile", 1: "full", 2: "half", 5: "pair"}


def _route_batches():
    """Smallest batch per kernel for the two kinds of K = 1024 launch: the statistics launch (two groups, no store) and the
    K / V launches (LayerNorm fold).  (Route 3 is full rounds + a half-tile tail — the same two kernels; route 4, 192-row tiles,
    takes plain launches only: the hook cannot say that these launches carry attention epilogues, so it is ignored here — the
    pair route, the one a wrong answer could hide, is confirmed by the library's launch counter in the test itself.)"""
    lib = _capi.load_test_library()
    kinds = {"stats": (_capi.TP_LINEAR_ROW_STATS | _capi.TP_LINEAR_NO_STORE, 2), "kv": (_capi.TP_LINEAR_LN_FOLD, 1)}
    first = {}
    for B in range(1, 129):
        for kind, (flags, groups) in kinds.items():
            r = lib.tp_test_gemm_route(B * ROWS, 1024, 1024, flags, groups)
            if r in ROUTE_NAMES:
                first.setdefault((kind, r), B)
    reached = {r for _, r in first}
    assert reached == set(ROUTE_NAMES), f"routes reached below B = 129: {sorted(first)}"
    return sorted(set(first.values())), first


@pytest.fixture(scope="module")
def routes():
    return _route_batches()


@pytest.fixture(scope="module")
def inputs():
    x, xm = synth.make_inputs(41, NDIST)
    return x, xm


def _params(k_bias_scale=1.0):
    p = synth.make_params(40, D)
    if k_bias_scale != 1.0:
        b = p["clip_attn.in_proj_bias"].clone()
        b[1024:2048] *= k_bias_scale                                  # the K rows of the in-projection
        p["clip_attn.in_proj_bias"] = b
    return p


_ORACLE = {}


def _oracle(tag, params, x, xm, dtype):
    """fp64 on the same rounded operands, once per parameter set and dtype, never modified."""
    if (tag, dtype) not in _ORACLE:
        p_lp = {k: v.to(dtype) for k, v in params.items()}
        _ORACLE[(tag, dtype)] = orc.forward(p_lp, x.to(dtype), xm.to(dtype), scale_factor=S, compute_dtype=torch.float64, io_dtype=dtype)
    return _ORACLE[(tag, dtype)]


def _batch(x, xm, B, dtype):
    idx = torch.arange(B) % NDIST
    return x.to(dtype)[idx].cuda(), xm.to(dtype)[idx].cuda(), idx


@pytest.mark.parametrize("dtype,fp32_out", CONFIGS, ids=IDS)
def test_every_kernel_route_against_the_oracle(inputs, routes, dtype, fp32_out):
    x, xm = inputs
    BATCHES, FIRST = routes
    lib = _capi.load_library()
    params = _params()
    m = _module(params, S, D, dtype)
    m.output_fp32 = fp32_out
    y_ref = _oracle("plain", params, x, xm, dtype)
    print(f"\n[k1024] smallest batch per (launch, kernel): { {f'{k}/{ROUTE_NAMES[r]}': b for (k, r), b in sorted(FIRST.items())} }")
    for B in BATCHES:
        xb, xmb, idx = _batch(x, xm, B, dtype)
        n0 = lib.tp_debug_counter(_capi.TP_COUNTER_PAIR_LAUNCHES)
        with torch.no_grad():
            y = m((xb, xmb))
        torch.cuda.synchronize()
        pair = lib.tp_debug_counter(_capi.TP_COUNTER_PAIR_LAUNCHES) - n0
        if B == FIRST[("kv", 5)]:                          # statistics, K and V launches on the pair kernel, at the least
            assert pair >= 3, (B, pair)
        if B == FIRST[("kv", 0)]:
            assert pair == 0, (B, pair)
        assert torch.isfinite(y.float()).all()
        e = orc.rel_err(y, y_ref[idx])
        print(f"[k1024] B={B} {IDS[CONFIGS.index((dtype, fp32_out))]}: rel_err {e:.3e} (gate {GATE[(dtype, fp32_out)]:.2e})")
        assert e <= GATE[(dtype, fp32_out)], (B, e)
        assert m.saturated_stages() == ()


@pytest.mark.parametrize("dtype,fp32_out", CONFIGS, ids=IDS)
def test_batch_invariance_across_routes(inputs, routes, dtype, fp32_out):
    """Image 0 alone (576 rows: two full tiles and 64 ragged rows) and every copy of it inside each of the batches: bit-equal,
    whichever kernel wrote the statistics partials and the logits."""
    x, xm = inputs
    BATCHES, _ = routes
    m = _module(_params(), S, D, dtype)
    m.output_fp32 = fp32_out
    with torch.no_grad(), batch_invariant():
        alone = [m((x.to(dtype)[k:k + 1].cuda(), xm.to(dtype)[k:k + 1].cuda())) for k in range(NDIST)]
        for B in BATCHES:
            xb, xmb, idx = _batch(x, xm, B, dtype)
            y = m((xb, xmb))
            for k in range(B):
                assert torch.equal(y[k:k + 1], alone[int(idx[k])]), (B, k)
    torch.cuda.synchronize()


@pytest.mark.parametrize("dtype,fp32_out", CONFIGS, ids=IDS)
def test_large_k_bias_is_softmax_invariant(inputs, routes, dtype, fp32_out):
    """The K launch drops sum_c b_c q_c — the same number for the 4 keys of a region.  With the K in-projection bias at 50 x its
    usual scale that number dominates every logit; parity with the oracle (which adds it) stays inside the same gate."""
    x, xm = inputs
    BATCHES, _ = routes
    params = _params(50.0)
    m = _module(params, S, D, dtype)
    m.output_fp32 = fp32_out
    y_ref = _oracle("kbias50", params, x, xm, dtype)
    for B in (BATCHES[0], BATCHES[-1]):
        xb, xmb, idx = _batch(x, xm, B, dtype)
        with torch.no_grad():
            y = m((xb, xmb))
        torch.cuda.synchronize()
        e = orc.rel_err(y, y_ref[idx])
        print(f"\n[k1024] K bias x 50, B={B} {IDS[CONFIGS.index((dtype, fp32_out))]}: rel_err {e:.3e}")
        assert e <= GATE[(dtype, fp32_out)], (B, e)


@pytest.mark.parametrize("B", [1, 3])
def test_stores_stay_inside_the_workspace(inputs, B):
    """tp_forward into a workspace of exactly tp_workspace_bytes between two 64 KiB guard blocks.  The statistics partials
    ([16][rows] fp32 per group) and the logits ([8][rows] fp32, `attn_aux`) are slabs of that workspace sized to the row; rows
    past M are dropped by the buffer descriptors.  Everything behind the status block starts as 0xFF bytes (NaN in every
    format): a reader that finds a partial nobody wrote, or a writer that runs over into a neighbouring slab (the statistics
    behind `attn_aux` are written BEFORE the K launch), shows against the oracle.
    Guards intact, status word 0, parity inside the gate, and the result is the module's."""
    lib = _capi.load_library()
    dtype, GUARD = torch.float16, 64 * 1024
    x, xm = inputs
    params = _params()
    m = _module(params, S, D, dtype)
    stream = torch.cuda.current_stream().cuda_stream
    img = m._ensure_packed(dtype, torch.device("cuda", 0), stream)
    xb, xmb, idx = _batch(x, xm, B, dtype)
    d = _capi.make_desc(B, 24, S, D, _capi.TP_F16)
    nbytes = lib.tp_workspace_bytes(ctypes.byref(d))
    assert nbytes > 0 and nbytes % 256 == 0
    # the slabs in question, sized exactly: 2 groups x 16 partials and 8 heads, 4 B per row each
    assert nbytes >= _capi.TP_WORKSPACE_STATUS_BYTES + (2 * 16 + 8) * B * ROWS * 4
    buf = torch.full((GUARD + nbytes + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    ws = buf[GUARD:GUARD + nbytes]
    ws.fill_(0xFF)
    ws[:_capi.TP_WORKSPACE_STATUS_BYTES].zero_()
    out = torch.empty(B, 144, D, dtype=dtype, device="cuda")
    args = (xb.data_ptr(), _capi.strides3(xb.stride()), xmb.data_ptr(), _capi.strides3(xmb.stride()))
    for _ in range(2):
        _capi.check(lib.tp_forward(ctypes.byref(d), *args, img.data_ptr(), out.data_ptr(), ws.data_ptr(), nbytes, stream), "tp_forward")
    torch.cuda.synchronize()
    assert bool((buf[:GUARD] == 0xA5).all()) and bool((buf[GUARD + nbytes:] == 0xA5).all())
    assert int(ws[:4].view(torch.int32).item()) == 0
    e = orc.rel_err(out, _oracle("plain", params, x, xm, dtype)[idx])
    assert e <= GATE[(dtype, False)], e
    with torch.no_grad():
        y = m((xb, xmb))
    assert torch.equal(out, y)


def test_fp16_clamp_of_mlp0(inputs):
    """mlp[0]'s weights scaled until its GELU output leaves the fp16 range: the epilogue stores +65504 wherever the exact result
    would have become an fp16 inf (>= 65520), finite correctly rounded values elsewhere, on the 128-tile and the ping-pong
    kernel alike; and a forward of the module with those weights sets the stage's bit in the workspace's status word."""
    from tests.gpu_util import linear
    dtype = torch.float16
    params = _params()
    g = torch.Generator().manual_seed(7)
    A = (torch.randn(300, 1024, generator=g) * 30.0).to(dtype)
    W = (params["mlp.0.weight"] * 1000.0).to(dtype)
    b = params["mlp.0.bias"].float()
    assert torch.isfinite(W.float()).all()
    ref = torch.nn.functional.gelu(A.double() @ W.double().t() + b.double())
    over, inside = ref >= 65520.0, ref <= 65000.0
    assert int(over.sum()) > 1000 and int(inside.sum()) > 1000
    for tile in (128, 256):
        C = linear(A.cuda(), W.cuda(), b.cuda(), flags=_capi.TP_LINEAR_GELU, tile=tile).cpu()
        assert torch.isfinite(C.float()).all()
        assert bool((C[over].float() == 65504.0).all()), tile
        # fp16 rounding (2^-11) + the fp32 accumulation over K = 1024 and the GELU's 3e-7, relative to the row's scale
        err = (C.double() - ref)[inside].abs().max().item()
        assert err <= 65504.0 * 2.0 ** -10, (tile, err)
    x, xm = inputs
    # (in the module mlp[0] reads the attention output, a few tenths in magnitude, through the folded out_proj: a larger factor)
    params["mlp.0.weight"] = params["mlp.0.weight"] * 1.0e5
    assert float(params["mlp.0.weight"].abs().max()) < 65504.0
    m = _module(params, S, D, dtype)
    xb, xmb, _ = _batch(x, xm, 2, dtype)
    with torch.no_grad():
        m((xb, xmb))
    torch.cuda.synchronize()
    assert "mlp0_gelu" in m.saturated_stages(), m.saturated_stages()
    assert m.saturation_report()["A2"] > 0
