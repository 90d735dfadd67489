"""fp32 master weights read in place (TP_DESC_RAW_F32) on a real MI355X: whatever the library builds or computes from the fp32
parameters' own memory is, byte for byte, what it builds or computes from ``.to(dtype)`` copies made on the host — the packed
image field by field (inference and training pack, bf16 and fp16, with weights beyond the fp16 range and the values where roundings
differ), the forward, every parameter gradient (``.grad`` and ``main_grad``), the input gradients, and a partially frozen module.
Every comparison is ``torch.equal`` on bytes.  hidden_size 256, B = 2, scale_factor 2 and 3."""
import copy
import ctypes
from collections import OrderedDict

import pytest
import torch

from tests import pack_ref as pr
from tokenpacker_amd import TokenPacker, _capi

pytestmark = pytest.mark.gpu
DEV, D, B = "cuda", 256, 2
SEED = 9100
DTYPES = (torch.bfloat16, torch.float16)
_TP = {torch.bfloat16: _capi.TP_BF16, torch.float16: _capi.TP_F16}
_ID = lambda dt: str(dt).split(".")[-1]
# fp32 bit patterns where a rounding recipe shows: bf16 ties (to even, both ways) and just above one, fp16 ties, FLT_MAX (-> inf in
# both formats), the smallest fp32 denormal, -0, fp16's smallest denormal's half (a tie to zero) and smallest normal
SPECIAL_BITS = (0x3F808000, 0x3F818000, 0x3F808001, 0x3F801000, 0x3F803000, 0x7F7FFFFF, 0xFF7FFFFF, 0x00000001, 0x80000000,
                0x33000000, 0x38800000, 0x477FE000, 0x477FEFFF, 0x477FF000, 0xC77FF000)


def _bytes(t):
    return t.detach().contiguous().view(torch.uint8)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bytes(a), _bytes(b))


# ---- 1. the packed image ---------------------------------------------------------------------------------------------------------
def fp32_params(kind):
    """plain / offset: pack_ref's seeded sets, left in fp32.  range: the plain set with the special bit patterns in the first
    K/V layer (whose bits the image keeps as they are), weights beyond the fp16 range behind it (clamped and counted: 1e5 and -7e4
    in plain casts, 3e5 in a LayerNorm-folded row) and 65519, which fp16 still rounds to 65504 (not counted)."""
    p = pr.make_param_set("plain" if kind == "range" else kind, SEED, torch.float32, D)
    if kind == "range":
        special = torch.tensor([b - (1 << 32) if b >= 1 << 31 else b for b in SPECIAL_BITS], dtype=torch.int32).view(torch.float32)
        p["k_proj_1.0.weight"][5, 8:8 + len(special)] = special
        p["v_proj_1.0.weight"][1023, -len(special):] = special
        p["mlp.0.weight"][3, 5], p["k_proj_1.2.weight"][1000, 1], p["mlp.2.weight"][D - 1, D - 1] = 1e5, -7e4, 65519.0
        p["clip_attn.in_proj_weight"][1024 + 17, 300] = 3e5
    return p


def pack(tensors, dtype, flags):
    """-> the image as a uint8 tensor: sentinel fill, tp_pack_weights on `tensors` (in tp_weights order), tp_pack_forget."""
    lib = _capi.load_library()
    desc = _capi.make_desc(1, 24, 2, D, _TP[dtype], flags=flags)
    nbytes = lib.tp_packed_weight_bytes(ctypes.byref(desc))
    assert nbytes > 0, _capi.last_error()
    buf = torch.full((nbytes,), pr.SENTINEL_BYTE, dtype=torch.uint8, device=DEV)
    raw = _capi.tp_weights(*[t.data_ptr() for t in tensors])
    _capi.check(lib.tp_pack_weights(ctypes.byref(desc), ctypes.byref(raw), buf.data_ptr(), nbytes,
                                    torch.cuda.current_stream().cuda_stream), "tp_pack_weights")
    torch.cuda.synchronize()
    _capi.check(lib.tp_pack_forget(buf.data_ptr()), "tp_pack_forget")
    return buf


@pytest.mark.parametrize("train_pack", [False, True], ids=["inference", "train_pack"])
@pytest.mark.parametrize("dtype", DTYPES, ids=_ID)
@pytest.mark.parametrize("kind", ["plain", "offset", "range"])
def test_the_image_from_fp32_sources_is_the_image_from_host_casts(kind, dtype, train_pack):
    p32 = fp32_params(kind)
    master = [p32[n].to(DEV).contiguous() for n in _capi.WEIGHT_FIELDS]
    assert all(t.dtype == torch.float32 and t.data_ptr() % 16 == 0 for t in master)
    cast = [t.to(dtype) for t in master]
    mode = _capi.TP_DESC_TRAIN_PACK if train_pack else 0
    got = pr.slice_image(pack(master, dtype, mode | _capi.TP_DESC_RAW_F32), dtype, D)
    want = pr.slice_image(pack(cast, dtype, mode), dtype, D)
    for field in want:
        if field not in pr.SCRATCH_FIELDS:
            assert _same(got[field], want[field]), field
    status = want["status"].tolist()
    assert got["status"].tolist() == status and status[1:3] == ([0, 0] if train_pack else [1, 1])
    print(f"\n[raw-f32] {kind} {_ID(dtype)} {'train' if train_pack else 'inference'} pack: {status[0]} element(s) clamped, both ways")
    assert (status[0] > 0) == (kind == "range")                   # (equal counts, and the range set does reach the clamp)
    if kind == "range":                                           # the first layer keeps the rounded bits themselves
        row = got["w_kv0"][5, 8:8 + len(SPECIAL_BITS)]
        assert _same(row, master[1][5, 8:8 + len(SPECIAL_BITS)].to(dtype)) and bool(torch.isinf(row).any())


@pytest.mark.parametrize("dtype", DTYPES, ids=_ID)
def test_a_nan_stays_a_nan(dtype):
    p32 = fp32_params("plain")
    master = [p32[n].to(DEV).contiguous() for n in _capi.WEIGHT_FIELDS]
    nan = torch.tensor([0x7FC00000, 0x7F800001, -0x3EDCBB], dtype=torch.int32, device=DEV).view(torch.float32)   # quiet, signalling, negative
    master[1][7, 40:43] = nan                                     # k_proj_1.0.weight: the image keeps its rounded bits
    img = pr.slice_image(pack(master, dtype, _capi.TP_DESC_TRAIN_PACK | _capi.TP_DESC_RAW_F32), dtype, D)
    assert bool(torch.isnan(img["w_kv0"][7, 40:43]).all())
    clean = pr.slice_image(pack([t.to(dtype) for t in master], dtype, _capi.TP_DESC_TRAIN_PACK), dtype, D)
    keep = torch.ones_like(img["w_kv0"], dtype=torch.bool)
    keep[7, 40:43] = False                                        # (a NaN's payload is nobody's contract; everything else is)
    assert torch.equal(img["w_kv0"].view(torch.int16)[keep], clean["w_kv0"].view(torch.int16)[keep])


# ---- the module ------------------------------------------------------------------------------------------------------------------
def make_module(s, trainable=("",)):
    m = TokenPacker(hidden_size=D, scale_factor=s)
    m.load_state_dict(pr.make_param_set("plain", SEED + s, torch.float32, D))
    m = m.to(DEV)
    for name, p in m.named_parameters():
        p.requires_grad_(name.startswith(tuple(trainable)))
    return m


@pytest.fixture(scope="module")
def inputs():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, 576, 1024, generator=g).to(DEV)
    xm = torch.randn(B, 576, 4096, generator=g).to(DEV)
    w = {s: torch.randn(B, (24 // s) ** 2, D, generator=g).to(DEV) for s in (2, 3)}
    return x, xm, w


def pair(s, **kw):
    """Two modules with the same fp32 parameters: one reads them in place, the other is forced onto the host-side casts."""
    raw = make_module(s, **kw)
    host = copy.deepcopy(raw)
    host.host_cast_weights = True
    return raw, host


# ---- 2. forward, and 6. the path taken -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_ID)
@pytest.mark.parametrize("s", [2, 3])
def test_forward_under_autocast(inputs, s, dtype):
    x, xm, _ = inputs
    raw, host = pair(s)
    assert raw.last_pack_path is None and host.last_pack_path is None
    with torch.no_grad(), torch.autocast("cuda", dtype=dtype):
        y_raw, y_host = raw((x, xm)), host((x, xm))
    torch.cuda.synchronize()
    assert (raw.last_pack_path, host.last_pack_path) == ("raw_f32", "host_cast")
    assert y_raw.dtype == dtype and bool(y_raw.float().abs().max() > 0) and _same(y_raw, y_host)
    with pytest.raises(AttributeError):
        raw.last_pack_path = "host_cast"                         # read-only
    # the switch is looked at on every pack: the same module, forced, takes the old path and gives the same bytes
    raw.host_cast_weights = True
    raw.invalidate_packed()
    with torch.no_grad(), torch.autocast("cuda", dtype=dtype):
        y_again = raw((x, xm))
    assert raw.last_pack_path == "host_cast" and _same(y_again, y_raw)


def test_modules_that_are_not_all_fp32_keep_the_old_path(inputs):
    x, xm, _ = inputs
    m = make_module(2).to(torch.bfloat16)                         # a bf16 module: nothing to read as fp32
    with torch.no_grad():
        m((x.bfloat16(), xm.bfloat16()))
    assert m.last_pack_path == "host_cast"
    mixed = make_module(2)                                        # one bf16 parameter among 22 fp32 ones: mixed sets are out of scope
    mixed.ln_k_1.bias.data = mixed.ln_k_1.bias.data.to(torch.bfloat16)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        y = mixed((x, xm))
    assert mixed.last_pack_path == "host_cast" and bool(torch.isfinite(y.float()).all())
    fp32_caller = make_module(2)                                  # fp32_compute_dtype: the same fp32 parameters, outside autocast
    fp32_caller.fp32_compute_dtype = torch.float16
    with torch.no_grad():
        y = fp32_caller((x, xm))
    assert fp32_caller.last_pack_path == "raw_f32" and y.dtype == torch.float32


# ---- 3. training -----------------------------------------------------------------------------------------------------------------
def train_step(m, x, xm, w, dtype, parts=False):
    """One forward + backward under autocast -> everything a caller can read afterwards, by name."""
    x = x.clone().requires_grad_(m.input_gradients)
    if parts:
        xm = tuple(t.clone().requires_grad_(m.input_gradients) for t in xm.split(1024, dim=2))
    else:
        xm = xm.clone().requires_grad_(m.input_gradients)
    with torch.autocast("cuda", dtype=dtype):
        y = m((x, xm))
    (y.float() * w).sum().backward()
    torch.cuda.synchronize()
    out = OrderedDict(y=y.detach())
    for name, p in m.named_parameters():
        if p.grad is not None:
            out["grad:" + name] = p.grad
        if getattr(p, "main_grad", None) is not None:
            out["main_grad:" + name] = p.main_grad
    if m.input_gradients:
        out["dx"] = x.grad
        for i, t in enumerate(xm if parts else (xm,)):
            out[f"dx_multi[{i}]"] = t.grad
    return out


def compare_steps(raw, host, inputs, s, dtype, parts=False, steps=1):
    x, xm, w = inputs
    for _ in range(steps):
        a, b = train_step(raw, x, xm, w[s], dtype, parts), train_step(host, x, xm, w[s], dtype, parts)
    assert (raw.last_pack_path, host.last_pack_path) == ("raw_f32", "host_cast")
    assert list(a) == list(b)
    for name in a:
        assert a[name] is not None and _same(a[name], b[name]), name
        assert name == "y" or a[name].dtype == torch.float32, name     # fp32 parameters and inputs: fp32 gradients, as before
        assert bool(a[name].float().abs().max() > 0), name
    return a


@pytest.mark.parametrize("dtype", DTYPES, ids=_ID)
@pytest.mark.parametrize("s", [2, 3])
def test_all_23_grads(inputs, s, dtype):
    raw, host = pair(s)
    got = compare_steps(raw, host, inputs, s, dtype)
    assert sum(k.startswith("grad:") for k in got) == 23 and not any(k.startswith("main_grad:") for k in got)
    # what autograd receives stays rounded to the compute dtype, then cast to fp32
    for k, g in got.items():
        if k.startswith("grad:"):
            assert torch.equal(g, g.to(dtype).float()), k


@pytest.mark.parametrize("dtype", DTYPES, ids=_ID)
@pytest.mark.parametrize("s", [2, 3])
def test_all_23_main_grads_accumulated_over_two_steps(inputs, s, dtype):
    raw, host = pair(s)
    for m in (raw, host):
        m.use_main_grad = True
        m.init_main_grads()
    got = compare_steps(raw, host, inputs, s, dtype, steps=2)
    assert sum(k.startswith("main_grad:") for k in got) == 23 and not any(k.startswith("grad:") for k in got)


@pytest.mark.parametrize("dtype", DTYPES, ids=_ID)
@pytest.mark.parametrize("s", [2, 3])
def test_input_gradients_with_x_multi_concatenated(inputs, s, dtype):
    raw, host = pair(s)
    raw.input_gradients = host.input_gradients = True
    got = compare_steps(raw, host, inputs, s, dtype)
    assert got["dx"].shape == (B, 576, 1024) and got["dx_multi[0]"].shape == (B, 576, 4096)


def test_input_gradients_with_x_multi_as_four_parts(inputs):
    raw, host = pair(2)
    raw.input_gradients = host.input_gradients = True
    got = compare_steps(raw, host, inputs, 2, torch.bfloat16, parts=True)
    assert all(got[f"dx_multi[{i}]"].shape == (B, 576, 1024) for i in range(4))


def test_a_frozen_projector_in_front_of_a_trainable_tower(inputs):
    """No parameter gradient at all: only the first-layer and q_proj_1 transposes read the parameters in the backward."""
    raw, host = pair(3, trainable=("none",))
    raw.input_gradients = host.input_gradients = True
    got = compare_steps(raw, host, inputs, 3, torch.float16)
    assert set(got) == {"y", "dx", "dx_multi[0]"}


@pytest.mark.parametrize("main_grad", [False, True], ids=["grad", "main_grad"])
def test_a_partially_frozen_module(inputs, main_grad):
    trainable = ("mlp.", "ln_q_1.", "q_proj_1.", "clip_attn.in_proj_bias")
    raw, host = pair(2, trainable=trainable)
    for m in (raw, host):
        m.use_main_grad = main_grad
        if main_grad:
            m.init_main_grads()
    got = compare_steps(raw, host, inputs, 2, torch.bfloat16)
    key = "main_grad:" if main_grad else "grad:"
    want = [key + n for n, _ in raw.named_parameters() if n.startswith(trainable)]
    assert [k for k in got if k != "y"] == want and len(want) == 8
