"""fp32 master weights read in place (TP_DESC_RAW_F32, tp_desc_known_flags; tp_optim_hyper.dtype = TP_F32) without a GPU.

The yardstick: the rule the kernels follow — every fp32 element is first rounded to the compute dtype as ``Tensor.to(dtype)`` rounds
it, then the existing recipe runs — restated on tests/pack_ref.py's helpers for the tensors of the image that depend on nothing but
their own parameters, and, on the seeded parameter sets, each of three wrong recipes shown to differ from it in at least one byte
of every image field it is named for.  (tests/test_gpu_raw_f32.py compares the image a GPU builds from fp32 sources with the one it
builds from ``.to(dtype)`` copies, field by field: a kernel that followed one of these recipes fails there.)

The host side: the flag's value is the header's, both libraries export the symbol, and every bad call is refused through the C ABI
on fake pointers, before a device is touched."""
import ctypes
import os
import re
from collections import OrderedDict

import pytest
import torch

from tests import pack_ref as pr
from tokenpacker_amd import MainGradAdamW, TokenPacker, _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "tokenpacker.h")).read()
FAKE = 1 << 20          # a non-NULL, 256-byte aligned address that the argument checks never dereference
E = _capi.TP_ERR_INVALID_ARG
NAMES = _capi.WEIGHT_FIELDS
SEED = 9100
D = 256

# ---- the yardstick ---------------------------------------------------------------------------------------------------------------
CAST16 = {"w_kv2": ("k_proj_1.2.weight", "v_proj_1.2.weight"), "w_q1": ("q_proj_1.weight",), "w_out": ("clip_attn.out_proj.weight",),
          "w_m0": ("mlp.0.weight",), "w_m2": ("mlp.2.weight",)}
BIAS32 = {"b_kv0": ("k_proj_1.0.bias", "v_proj_1.0.bias"), "b_kv2": ("k_proj_1.2.bias", "v_proj_1.2.bias"),
          "b_out": ("clip_attn.out_proj.bias",), "b_m0": ("mlp.0.bias",), "b_m2": ("mlp.2.bias",)}
FOLD = ("w_in_kv", "c_in_kv", "b_in_kv", "w_in_q", "c_in_q", "b_in_q")
# wrong recipe -> the image fields it must show in
WRONG = {"direct_f16": tuple(CAST16),            # fp32 -> fp16 in one step for a bf16 model: the bf16 rounding is skipped
         "unrounded_fold": ("w_in_kv", "b_in_kv", "w_in_q", "b_in_q"),   # the LayerNorm fold from the fp32 gamma / beta / W
         "unrounded_bias": tuple(BIAS32)}        # the fp32 biases of the image taken as they are


def image_fields(p32, dtype, recipe="round_first"):
    """The tensors of the image that are functions of their own parameters alone, by PackedLayout field name, from FP32 parameters:
    ``round_first`` — what TP_DESC_RAW_F32 promises: ``.to(dtype)`` on every element, then tp_pack_weights' recipe as
    pack_ref.emulate states it — or one of WRONG."""
    assert recipe == "round_first" or recipe in WRONG, recipe
    r = {k: v.to(dtype) for k, v in p32.items()}                       # the rule: rounded first, as Tensor.to rounds
    stack = lambda ts: ts[0] if len(ts) == 1 else torch.stack(ts)
    img = OrderedDict()
    img["w_kv0"] = torch.cat([r["k_proj_1.0.weight"], r["v_proj_1.0.weight"]], 0)
    for field, names in CAST16.items():
        src = p32 if recipe == "direct_f16" else r
        img[field] = stack([pr.f16(src[n]) for n in names])
    for field, names in BIAS32.items():
        src = p32 if recipe == "unrounded_bias" else r
        img[field] = stack([src[n].float() for n in names])
    src = p32 if recipe == "unrounded_fold" else r
    inw, inb = src["clip_attn.in_proj_weight"].float(), src["clip_attn.in_proj_bias"].float()
    per = {}
    for m in pr.MATS:
        W, gamma, beta = inw[pr._IN_ROWS[m]], src[f"ln_{m}_1.weight"].float(), src[f"ln_{m}_1.bias"].float()
        hi = pr.f16(W * gamma)
        per[m] = (hi, hi.float().sum(1), W @ beta + inb[pr._IN_ROWS[m]])
    for i, key in enumerate(("w_in", "c_in", "b_in")):
        img[key + "_kv"] = torch.stack([per["k"][i], per["v"][i]])
        img[key + "_q"] = per["q"][i]
    return img


def _bytes(t):
    return t.contiguous().view(torch.uint8)


def _differs(a, b):
    return a.shape != b.shape or a.dtype != b.dtype or not torch.equal(_bytes(a), _bytes(b))


@pytest.fixture(scope="module")
def fp32_sets():
    return {kind: pr.make_param_set(kind, SEED, torch.float32, D) for kind in pr.SETS}


def test_the_seeded_parameters_are_not_representable_in_16_bits(fp32_sets):
    """Otherwise every recipe would agree and nothing below would show anything."""
    for kind, p in fp32_sets.items():
        for name, t in p.items():
            assert t.dtype == torch.float32
            for dt in pr.DTYPES:
                assert bool((t.to(dt).float() != t).any()), (kind, name, dt)


@pytest.mark.parametrize("dtype", pr.DTYPES, ids=["fp16", "bf16"])
def test_round_first_is_the_existing_recipe_on_rounded_parameters(fp32_sets, dtype):
    """`image_fields` restates nothing new: on the rounded parameters it is pack_ref.emulate, field for field, byte for byte."""
    p32 = fp32_sets["plain"]
    want = pr.emulate(OrderedDict((k, v.to(dtype)) for k, v in p32.items()), hidden=D)
    got = image_fields(p32, dtype)
    assert set(got) == {"w_kv0"} | set(CAST16) | set(BIAS32) | set(FOLD)
    for field, t in got.items():
        assert not _differs(t, want[field]), field


@pytest.mark.parametrize("kind", pr.SETS)
@pytest.mark.parametrize("dtype", pr.DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("recipe", list(WRONG))
def test_each_wrong_recipe_changes_a_byte_of_every_field_it_is_named_for(fp32_sets, recipe, dtype, kind):
    if recipe == "direct_f16" and dtype == torch.float16:
        # for an fp16 model fp32 -> fp16 IS the rounding to the compute dtype: the recipe is the right one, and must say so
        right, same = image_fields(fp32_sets[kind], dtype), image_fields(fp32_sets[kind], dtype, recipe)
        assert not any(_differs(right[f], same[f]) for f in right)
        return
    right, wrong = image_fields(fp32_sets[kind], dtype), image_fields(fp32_sets[kind], dtype, recipe)
    for field in right:
        if field in WRONG[recipe]:
            assert _differs(right[field], wrong[field]), f"{recipe} does not show in {field}"
        elif not (recipe == "unrounded_fold" and field in FOLD):        # (c_in follows w_in; it is not what the recipe is named for)
            assert not _differs(right[field], wrong[field]), f"{recipe} shows in {field}, which it does not touch"


def test_tensor_to_is_round_to_nearest_even_with_nan_and_overflow():
    """The rounding the kernels restate in integer arithmetic (bf16) / take from the hardware conversion (fp16), pinned on the values
    where recipes differ: ties go to even, a NaN stays a NaN, what exceeds the format becomes +-inf."""
    f = lambda bits: torch.tensor([bits], dtype=torch.int32).view(torch.float32)
    b = lambda t: int(t.to(torch.bfloat16).view(torch.int16).item()) & 0xFFFF
    assert b(f(0x3F808000)) == 0x3F80 and b(f(0x3F818000)) == 0x3F82 and b(f(0x3F808001)) == 0x3F81     # ties to even; above a tie
    assert b(f(0x7F7FFFFF)) == 0x7F80 and b(-f(0x7F7FFFFF)) == 0xFF80                                      # FLT_MAX -> inf
    for nan in (0x7FC00000, 0x7F800001, 0xFFC12345 - (1 << 32)):                                           # NaN stays NaN (any payload)
        assert b(f(nan)) & 0x7F80 == 0x7F80 and b(f(nan)) & 0x007F != 0
    h = lambda x: int(torch.tensor([x], dtype=torch.float32).to(torch.float16).view(torch.int16).item()) & 0xFFFF
    assert h(65504.0) == 0x7BFF and h(65519.0) == 0x7BFF and h(65520.0) == 0x7C00 and h(-1e6) == 0xFC00
    assert h(float("nan")) & 0x7C00 == 0x7C00 and h(float("nan")) & 0x03FF != 0


# ---- the flag and the symbol -----------------------------------------------------------------------------------------------------
def test_the_flag_has_the_headers_value_and_both_libraries_export_the_symbol():
    value = int(re.search(r"#define TP_DESC_RAW_F32 (\d+)\n", HEADER).group(1))
    assert value == _capi.TP_DESC_RAW_F32 == 4
    others = [int(re.search(rf"#define {n} (\d+)\n", HEADER).group(1)) for n in ("TP_DESC_TRAIN_PACK", "TP_DESC_MASKED")]
    assert value & (value - 1) == 0 and value == 2 * max(others), "the next free bit of tp_desc.flags"
    assert "int         tp_desc_known_flags(void);" in HEADER and "tp_desc_known_flags" in _capi.EXPORTED_SYMBOLS
    for path in (_capi.LIB_PATH, _capi.EXP_LIB_PATH):
        lib = ctypes.CDLL(path)
        assert hasattr(lib, "tp_desc_known_flags"), path
        lib.tp_desc_known_flags.restype = ctypes.c_int
        assert lib.tp_desc_known_flags() == _capi.TP_DESC_TRAIN_PACK | _capi.TP_DESC_MASKED | _capi.TP_DESC_RAW_F32, path
    assert _capi.raw_f32_supported() is True
    assert "#define TP_ABI_VERSION 6\n" in HEADER and _capi.load_library().tp_version() == 6


def test_a_flag_the_library_does_not_know_is_still_refused():
    lib = _capi.load_library()
    d = _capi.make_desc(1, 24, 2, D, _capi.TP_BF16, flags=8)
    w = _capi.tp_weights(*([FAKE] * len(NAMES)))
    assert lib.tp_pack_weights(ctypes.byref(d), ctypes.byref(w), FAKE, 1 << 40, None) == E
    assert "unknown flags" in _capi.last_error()


# ---- host-side refusals, before any launch -----------------------------------------------------------------------------------------
def _pack(ptrs, flags=_capi.TP_DESC_RAW_F32, packed_bytes=1024, dtype=_capi.TP_BF16):
    d = _capi.make_desc(1, 24, 2, D, dtype, flags=flags)
    w = _capi.tp_weights(*ptrs)
    return _capi.load_library().tp_pack_weights(ctypes.byref(d), ctypes.byref(w), FAKE, packed_bytes, None)


def _backward(ptrs, flags=_capi.TP_DESC_RAW_F32, ws_bytes=1024):
    lib = _capi.load_library()
    d = _capi.make_desc(2, 24, 2, D, _capi.TP_BF16, flags=flags)
    st = _capi.strides3((576 * 4096, 4096, 1))
    w = _capi.tp_weights(*ptrs)
    sink = _capi.tp_grad_sink(_capi.tp_grads(*([FAKE] * len(NAMES))), _capi.TP_F32, 1)
    return lib.tp_backward_sink(ctypes.byref(d), FAKE, None, st, ctypes.byref(w), FAKE, FAKE, FAKE, ctypes.byref(sink), None, None,
                                FAKE, ws_bytes, None)


@pytest.mark.parametrize("call", [_pack, _backward], ids=["tp_pack_weights", "tp_backward_sink"])
def test_the_flag_with_a_null_or_misaligned_pointer_is_refused(call):
    for i in (0, 9, 15, 22):
        ptrs = [FAKE + 64 * k for k in range(len(NAMES))]
        ptrs[i] = None
        assert call(ptrs) == E and f"pointer #{i} is NULL" in _capi.last_error(), _capi.last_error()
        for off in (2, 4, 8):                    # fp32 sources are read with 16-byte loads: no scalar detour, a refusal
            ptrs[i] = FAKE + 64 * i + off
            assert call(ptrs) == E and f"fp32 weight pointer #{i} is not 16-byte aligned" in _capi.last_error(), _capi.last_error()
            assert call(ptrs, flags=0) == _capi.TP_ERR_WORKSPACE      # (without the flag the 16-bit rules hold: not refused here)
    # well-formed: the checks pass and the call stops at the buffer that is too small, still before any launch
    assert call([FAKE + 64 * k for k in range(len(NAMES))]) == _capi.TP_ERR_WORKSPACE, _capi.last_error()


def _optim(param, dtype, ws_bytes=1 << 30, **over):
    t = (_capi.tp_optim_tensor * 2)()
    for i in range(2):
        base = FAKE + i * (1 << 16)
        t[i] = _capi.tp_optim_tensor(param if i == 1 else (None if dtype == _capi.TP_F32 else base), base + 4096, base + 8192,
                                     base + 12288, base + 16384, 1000 + i, 1e-3, 0.1)
    for k, v in over.items():
        setattr(t[1], k, v)
    h = _capi.tp_optim_hyper(0.9, 0.999, 1e-8, 1.0, dtype, _capi.TP_OPTIM_ZERO_GRAD)
    return _capi.load_library().tp_optim_step(t, 2, ctypes.byref(h), None, FAKE - 4096, FAKE - (1 << 19), ws_bytes, None)


def test_optimizer_param_pointer_rules_follow_the_dtype():
    second = FAKE + (1 << 16)
    assert _optim(second, _capi.TP_F32) == E                       # fp32 parameters are their own masters: param must be NULL
    assert all(w in _capi.last_error() for w in ("tp_optim_step", "entry #1", "param must be NULL", "TP_F32")), _capi.last_error()
    for dt in (_capi.TP_BF16, _capi.TP_F16):                       # ... and NULL stays refused for a 16-bit parameter
        assert _optim(None, dt) == E and "entry #1: param is NULL" in _capi.last_error(), _capi.last_error()
    # TP_F32 with NULL params passes every pointer check: the call stops at its workspace, before any launch
    assert _optim(None, _capi.TP_F32, ws_bytes=16) == E and "workspace" in _capi.last_error(), _capi.last_error()
    # the other rules are unchanged in the fp32 mode
    assert _optim(None, _capi.TP_F32, master=None) == E and "entry #1: master is NULL" in _capi.last_error()
    assert _optim(None, _capi.TP_F32, master=second + 4098) == E and "master" in _capi.last_error() and "aligned" in _capi.last_error()
    assert _optim(None, _capi.TP_F32, exp_avg=second + 4096) == E and "twice" in _capi.last_error()
    assert _optim(second, 3) == E and "dtype" in _capi.last_error()


def test_main_grad_adamw_refuses_mixed_dtypes():
    m = TokenPacker(hidden_size=D, scale_factor=2)                  # fp32 parameters ...
    m.mlp[2].bias.data = m.mlp[2].bias.data.to(torch.bfloat16)     # ... but one
    m.init_main_grads()
    with pytest.raises(ValueError, match=r"parameter mlp\.2\.bias is torch\.bfloat16 .* the first one torch\.float32 .* one dtype"):
        MainGradAdamW(m.parameters(), module=m)
    m = TokenPacker(hidden_size=D, scale_factor=2).to(torch.bfloat16)
    m.q_proj_1.weight.data = m.q_proj_1.weight.data.float()
    m.init_main_grads()
    with pytest.raises(ValueError, match=r"parameter k_proj_1\.0\.weight is torch\.bfloat16 .* the first one torch\.float32"):
        MainGradAdamW(m.parameters(), module=m)
    p = torch.nn.Parameter(torch.zeros(8, dtype=torch.float64))
    p.main_grad = torch.zeros(8)
    with pytest.raises(TypeError, match=r"parameter #0 is torch\.float64; .* or torch\.float32 \(their own masters\)"):
        MainGradAdamW([p])
    m = TokenPacker(hidden_size=D, scale_factor=2)                  # an all-fp32 module is accepted as far as a CPU can tell
    m.init_main_grads()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        MainGradAdamW(m.parameters(), module=m)
