"""The backward into a gradient sink (tp_grad_sink / tp_backward_sink / tp_backward_plan, an ABI 6 extension) without a GPU: the
symbols are declared, exported and bound, the struct has the header's layout, bad sinks are refused before the device is touched,
the older entry points still refuse a NULL gradient pointer, tp_backward_plan names the stages each set of wanted outputs needs, and
``module.use_main_grad`` checks its buffers before anything is launched."""
import ctypes
import os

import pytest
import torch

from tokenpacker_amd import TokenPacker, _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = _capi.WEIGHT_FIELDS
FAKE = 1 << 20          # a non-NULL, 256-byte aligned address that the argument checks never dereference
E = _capi.TP_ERR_INVALID_ARG


def test_new_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "tokenpacker.h")).read()
    lib = _capi.load_library()
    for name in ("tp_backward_sink", "tp_backward_plan"):
        assert f"{name}(" in header, name
        assert name in _capi.EXPORTED_SYMBOLS, name
        assert hasattr(lib, name) and getattr(lib, name).argtypes, name
    assert "typedef struct tp_grad_sink" in header
    for i, stage in enumerate(_capi.BWD_STAGE_NAMES):           # the header's constants are the binding's
        assert f"TP_BWD_STAGE_{stage} = 1 << {i}" in header, stage
        assert getattr(_capi, "TP_BWD_STAGE_" + stage) == 1 << i
    assert "#define TP_ABI_VERSION 6\n" in header
    assert lib.tp_version() == 6 == _capi.TP_ABI_VERSION


def test_grad_sink_struct_layout():
    assert ctypes.sizeof(_capi.tp_grads) == 23 * 8
    assert ctypes.sizeof(_capi.tp_grad_sink) == 23 * 8 + 8
    assert _capi.tp_grad_sink.grads.offset == 0
    assert _capi.tp_grad_sink.dtype.offset == 23 * 8
    assert _capi.tp_grad_sink.accumulate.offset == 23 * 8 + 4


def _sink(ptrs=None, dtype=_capi.TP_BF16, accumulate=0, **named):
    """A sink with the same pointer for every parameter (``ptrs``: an int or None), or only the named entries."""
    g = _capi.tp_grads(*([ptrs] * len(NAMES)))
    for k, v in named.items():
        setattr(g, k, v)
    return _capi.tp_grad_sink(g, dtype, accumulate)


def _call(sink, ig=None, am=None, ws_bytes=1 << 40, dtype=_capi.TP_BF16):
    lib = _capi.load_library()
    d = _capi.make_desc(2, 24, 2, 256, dtype)
    st = _capi.strides3((576 * 4096, 4096, 1))
    w = _capi.tp_weights(*([FAKE] * len(NAMES)))
    return lib.tp_backward_sink(ctypes.byref(d), FAKE, None, st, ctypes.byref(w), FAKE, FAKE, FAKE,
                                None if sink is None else ctypes.byref(sink), ig, am, FAKE, ws_bytes, None)


def test_bad_sinks_are_refused_before_any_launch():
    # accumulate needs an fp32 sink
    assert _call(_sink(FAKE, _capi.TP_BF16, 1)) == E and "accumulate" in _capi.last_error()
    assert _call(_sink(FAKE, _capi.TP_F16, 1), dtype=_capi.TP_F16) == E and "accumulate" in _capi.last_error()
    assert _call(_sink(FAKE, _capi.TP_F32, 2)) == E and "accumulate" in _capi.last_error()
    # the sink's dtype is the model's, or fp32
    for bad in (_capi.TP_F16, 3, -1):
        assert _call(_sink(FAKE, bad)) == E, bad
        assert "dtype" in _capi.last_error()
    assert _call(_sink(FAKE, _capi.TP_BF16), dtype=_capi.TP_F16) == E and "dtype" in _capi.last_error()
    # nothing asked for: no sink at all, or a sink without an entry, and no input or mask gradient
    assert _call(None) == E and "nothing requested" in _capi.last_error()
    assert _call(_sink(None)) == E and "nothing requested" in _capi.last_error()
    assert _call(_sink(None, _capi.TP_F32, 1)) == E and "nothing requested" in _capi.last_error()
    no_grad_mask = _capi.tp_attn_mask(mask=FAKE, mode=1)
    assert _call(_sink(None), am=ctypes.byref(no_grad_mask)) == E and "nothing requested" in _capi.last_error()
    assert _call(_sink(None), ig=ctypes.byref(_capi.tp_input_grads())) == E and "nothing requested" in _capi.last_error()
    # fp32 entries are 16-byte aligned (a model-dtype sink keeps tp_backward's rules)
    for off in (4, 8):
        assert _call(_sink(None, _capi.TP_F32, 0, mlp_2_weight=FAKE + off)) == E
        assert "16-byte aligned" in _capi.last_error()
        assert _call(_sink(FAKE, _capi.TP_F32, 1, ln_k_1_bias=FAKE + off)) == E
        assert "16-byte aligned" in _capi.last_error()
    # the mask and input-gradient rules of tp_backward_masked hold here too
    assert _call(_sink(FAKE), am=ctypes.byref(_capi.tp_attn_mask(mask=FAKE, mode=3))) == E and "mode" in _capi.last_error()
    assert _call(_sink(FAKE), am=ctypes.byref(_capi.tp_attn_mask(mask=FAKE, mode=1, reserved=1))) == E


def test_good_sinks_pass_the_argument_checks():
    """What is accepted gets as far as the workspace size (still before any launch: there is no device here)."""
    W = _capi.TP_ERR_WORKSPACE
    assert _call(_sink(FAKE), ws_bytes=1024) == W                                               # the full model-dtype sink
    assert _call(_sink(None, mlp_2_bias=FAKE), ws_bytes=1024) == W                              # one entry
    assert _call(_sink(FAKE, _capi.TP_F32, 0), ws_bytes=1024) == W                              # fp32, overwrite
    assert _call(_sink(FAKE + 16, _capi.TP_F32, 1), ws_bytes=1024) == W                         # fp32, accumulate
    assert _call(_sink(FAKE, _capi.TP_F32, 1), ws_bytes=1024, dtype=_capi.TP_F16) == W
    assert _call(_sink(None, mlp_2_bias=FAKE + 2), ws_bytes=1024) == W                          # (a 2-byte entry: 2-byte alignment)
    am = _capi.tp_attn_mask(mask=FAKE, mode=1, grad=FAKE)
    assert _call(_sink(None), am=ctypes.byref(am), ws_bytes=1024) == W                          # dmask alone is a request
    assert _call(None, am=ctypes.byref(am), ws_bytes=1024) == W
    assert _call(_sink(None), ig=ctypes.byref(_capi.tp_input_grads(dx=FAKE)), ws_bytes=1024) == W


def test_older_entry_points_still_refuse_a_null_gradient_pointer():
    lib = _capi.load_library()
    d = _capi.make_desc(2, 24, 2, 256, _capi.TP_BF16)
    st = _capi.strides3((576 * 4096, 4096, 1))
    w = _capi.tp_weights(*([FAKE] * len(NAMES)))
    for i in (0, 7, 22):
        ptrs = [FAKE] * len(NAMES)
        ptrs[i] = None
        g = _capi.tp_grads(*ptrs)
        assert lib.tp_backward(ctypes.byref(d), FAKE, st, ctypes.byref(w), FAKE, FAKE, FAKE, ctypes.byref(g), FAKE, 1 << 40,
                               None) == E
        assert f"pointer #{i} is NULL" in _capi.last_error()
        ig = _capi.tp_input_grads(dx=FAKE)
        assert lib.tp_backward_inputs(ctypes.byref(d), FAKE, st, ctypes.byref(w), FAKE, FAKE, FAKE, ctypes.byref(g),
                                      ctypes.byref(ig), FAKE, 1 << 40, None) == E
        am = _capi.tp_attn_mask(mask=FAKE, mode=1)
        assert lib.tp_backward_masked(ctypes.byref(d), FAKE, None, st, ctypes.byref(w), FAKE, FAKE, FAKE, ctypes.byref(g), None,
                                      ctypes.byref(am), FAKE, 1 << 40, None) == E


# ---- tp_backward_plan ----------------------------------------------------------------------------------------------------
ALL = set(_capi.BWD_STAGE_NAMES)
MLP2 = ("mlp.2.weight", "mlp.2.bias")
MLP = MLP2 + ("mlp.0.weight", "mlp.0.bias")
K_BRANCH = tuple(n for n in NAMES if n.startswith(("k_proj_1.", "ln_k_1.")))
KV = tuple(n for n in NAMES if n.startswith(("k_proj_1.", "v_proj_1.", "ln_k_1.", "ln_v_1.")))
CHAIN_DOWN_TO_ATTENTION = {"DY", "DZ2", "DA1", "DO", "ATTENTION"}


def plan(wanted=(), **kw):
    return set(_capi.backward_plan(wanted, **kw))


def test_plan_all_wanted_runs_every_stage():
    assert plan(NAMES) == ALL
    assert plan(NAMES, want_dx=True, want_dx_multi=True, want_dmask=True) == ALL
    assert _capi.load_library().tp_backward_plan((1 << 23) - 1, 0, 0, 0) == _capi.TP_BWD_STAGE_ALL
    assert _capi.load_library().tp_backward_plan(0xFFFFFFFF, 0, 0, 0) == _capi.TP_BWD_STAGE_ALL      # (bits past 22 mean nothing)


def test_plan_only_mlp2_has_no_dgrad():
    assert plan(MLP2) == {"DY", "MLP2_BIAS", "MLP2_WGRAD"}
    assert plan(("mlp.2.weight",)) == {"DY", "MLP2_WGRAD"}
    assert plan(("mlp.2.bias",)) == {"DY", "MLP2_BIAS"}


def test_plan_only_mlp_stops_before_da1():
    assert plan(MLP) == {"DY", "MLP2_BIAS", "MLP2_WGRAD", "DZ2", "MLP0_BIAS", "MLP0_WGRAD"}
    assert plan(("mlp.0.bias",)) == {"DY", "DZ2", "MLP0_BIAS"}
    assert plan(("clip_attn.out_proj.weight",)) == {"DY", "DZ2", "DA1", "OUT_WGRAD"}


def test_plan_only_q_proj_runs_the_q_chain_alone():
    assert plan(("q_proj_1.weight",)) == CHAIN_DOWN_TO_ATTENTION | {"Q_CHAIN"}
    assert plan(("ln_q_1.bias",)) == CHAIN_DOWN_TO_ATTENTION | {"Q_CHAIN"}


def test_plan_only_the_k_branch():
    assert plan(K_BRANCH) == CHAIN_DOWN_TO_ATTENTION | {"K_CHAIN", "DZ1", "KV0_WGRAD"}
    assert plan(("ln_k_1.weight", "k_proj_1.2.bias")) == CHAIN_DOWN_TO_ATTENTION | {"K_CHAIN"}
    assert plan(("v_proj_1.0.bias",)) == CHAIN_DOWN_TO_ATTENTION | {"V_CHAIN", "DZ1", "KV0_WGRAD"}


def test_plan_in_proj_weight_alone_runs_all_three_chains_without_dz1():
    assert plan(("clip_attn.in_proj_weight",)) == CHAIN_DOWN_TO_ATTENTION | {"Q_CHAIN", "K_CHAIN", "V_CHAIN"}
    assert plan(("clip_attn.in_proj_bias",)) == CHAIN_DOWN_TO_ATTENTION          # (column sums of dQ, dK, dO: no chain)


def test_plan_dmask_alone_stops_after_the_attention():
    assert plan(want_dmask=True) == CHAIN_DOWN_TO_ATTENTION


def test_plan_dx_multi_alone_runs_both_kv_chains_and_dz1_without_a_wgrad():
    got = plan(want_dx_multi=True)
    assert got == CHAIN_DOWN_TO_ATTENTION | {"K_CHAIN", "V_CHAIN", "DZ1"}
    assert not any(s.endswith(("WGRAD", "BIAS")) for s in got)
    assert plan(want_dx=True) == CHAIN_DOWN_TO_ATTENTION | {"Q_CHAIN"}


def test_plan_everything_but_the_kv_branches():
    rest = tuple(n for n in NAMES if n not in KV)
    assert plan(rest) == ALL - {"DZ1", "KV0_WGRAD"}               # (in_proj_weight keeps the K/V chains; the K/V layers drop out)
    assert plan(tuple(n for n in rest if n != "clip_attn.in_proj_weight")) == ALL - {"DZ1", "KV0_WGRAD", "K_CHAIN", "V_CHAIN"}
    assert plan() == {"DY"}


def test_plan_is_monotonic_and_closed_upwards():
    """Wanting more never runs less, and a stage that runs has every dgrad above it in the chain."""
    lib = _capi.load_library()
    up = [("DZ2", ("DY",)), ("DA1", ("DZ2",)), ("DO", ("DA1",)), ("ATTENTION", ("DO",)), ("Q_CHAIN", ("ATTENTION",)),
          ("K_CHAIN", ("ATTENTION",)), ("V_CHAIN", ("ATTENTION",)), ("DZ1", ("ATTENTION",)), ("MLP0_WGRAD", ("DZ2",)),
          ("OUT_BIAS", ("DA1",)), ("KV0_WGRAD", ("DZ1",))]
    bit = {n: 1 << i for i, n in enumerate(_capi.BWD_STAGE_NAMES)}
    g = torch.Generator().manual_seed(0)
    for _ in range(300):
        a = int(torch.randint(0, 1 << 23, (1,), generator=g))
        b = a | int(torch.randint(0, 1 << 23, (1,), generator=g))
        flags = [int(v) for v in torch.randint(0, 2, (3,), generator=g)]
        pa, pb = lib.tp_backward_plan(a, *flags), lib.tp_backward_plan(b, *flags)
        assert pa & pb == pa
        for stage, needs in up:
            if pa & bit[stage]:
                assert all(pa & bit[n] for n in needs), (a, flags, stage)
        if pa & (bit["DZ1"]):                                     # dZ1 comes from a K/V chain
            assert pa & (bit["K_CHAIN"] | bit["V_CHAIN"])


# ---- module.use_main_grad ------------------------------------------------------------------------------------------------
def _cpu_module():
    return TokenPacker(hidden_size=256, scale_factor=2)


def test_use_main_grad_defaults_off_and_survives_a_copy():
    import copy
    m = _cpu_module()
    assert m.use_main_grad is False
    m.use_main_grad = True
    assert copy.deepcopy(m).use_main_grad is True
    state = m.__getstate__()
    state.pop("use_main_grad")                                    # (a module pickled before the switch existed)
    m2 = TokenPacker.__new__(TokenPacker)
    m2.__setstate__(state)
    assert m2.use_main_grad is False


def test_init_and_zero_main_grads():
    m = _cpu_module()
    m.k_proj_1.requires_grad_(False)
    m.init_main_grads()
    for n, p in m.named_parameters():
        if n.startswith("k_proj_1"):
            assert not hasattr(p, "main_grad"), n
        else:
            assert p.main_grad.dtype == torch.float32 and p.main_grad.shape == p.shape and p.main_grad.is_contiguous(), n
            assert float(p.main_grad.abs().max()) == 0.0
    m.mlp[2].bias.main_grad.fill_(3.0)
    keep = m.mlp[2].bias.main_grad
    m.zero_main_grads()
    assert m.mlp[2].bias.main_grad is keep and float(keep.abs().max()) == 0.0
    keep.fill_(2.0)
    m.init_main_grads()                                           # a well-formed buffer is kept (and zeroed), not replaced
    assert m.mlp[2].bias.main_grad is keep and float(keep.abs().max()) == 0.0
    assert [n for n, _, mg in m.check_main_grads() if mg is None] == [n for n in NAMES if n.startswith("k_proj_1")]


def test_use_main_grad_checks_raise_before_any_launch():
    """On CPU tensors: the named error comes first — before the module's own 'no CPU fallback' refusal, so before any launch."""
    m = _cpu_module()
    m.use_main_grad = True
    x = (torch.zeros(1, 576, 1024, dtype=torch.bfloat16), torch.zeros(1, 576, 4096, dtype=torch.bfloat16))
    with pytest.raises(TypeError, match=r"use_main_grad: parameter q_proj_1\.weight requires grad but has no main_grad"):
        m(x)
    m.init_main_grads()
    m.check_main_grads()
    with pytest.raises(RuntimeError, match="no CPU fallback"):     # well-formed buffers: the module gets as far as its device check
        m(x)
    p = m.ln_q_1.weight
    good = p.main_grad
    for bad, exc, pat in ((good.to(torch.bfloat16), TypeError, r"ln_q_1\.weight\.main_grad is torch\.bfloat16"),
                          (good.double(), TypeError, "must be torch.float32"),
                          ("not a tensor", TypeError, "has no main_grad tensor"),
                          (torch.zeros(1023), ValueError, r"shape \(1023,\)"),
                          (torch.zeros(2048)[::2], ValueError, "contiguous and 16-byte aligned"),
                          (torch.zeros(1025)[1:], ValueError, "contiguous and 16-byte aligned"),     # (4 bytes past the allocation's start)
                          (torch.zeros(1024, device="meta"), ValueError, "is on meta")):
        p.main_grad = bad
        with pytest.raises(exc, match=pat):
            m.check_main_grads()
        with pytest.raises(exc, match=pat):
            m(x)
    p.main_grad = good
    m.check_main_grads()
    with torch.no_grad():                                          # inference does not look at main_grad at all
        del m.mlp[0].bias.main_grad
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            m(x)
    p.requires_grad_(False)                                        # a frozen parameter needs none
    del p.main_grad
    m.mlp[0].bias.main_grad = torch.zeros(256)
    m.check_main_grads()
