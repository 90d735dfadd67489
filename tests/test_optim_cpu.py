"""The optimizer step (tp_optim_tensor / tp_optim_hyper / tp_optim_workspace_bytes / tp_optim_step, an ABI 6 extension) without a
GPU: the symbols are declared, exported and bound, the structs have the header's layout, every bad call is refused on the host with
the offending entry named — on fake pointers, before a device is touched — and ``MainGradAdamW`` refuses CPU parameters and
parameters without a ``main_grad``."""
import ctypes
import os
import re

import pytest
import torch

from tokenpacker_amd import MainGradAdamW, TokenPacker, _capi, optim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 1 << 20          # a non-NULL, 256-byte aligned address that the argument checks never dereference
E = _capi.TP_ERR_INVALID_ARG
HEADER = open(os.path.join(ROOT, "include", "tokenpacker.h")).read()


def test_new_symbols_are_declared_exported_and_bound():
    lib = _capi.load_library()
    for name in ("tp_optim_workspace_bytes", "tp_optim_step"):
        assert f"{name}(" in HEADER, name
        assert name in _capi.EXPORTED_SYMBOLS, name
        assert hasattr(lib, name) and getattr(lib, name).argtypes, name
    for struct in ("tp_optim_tensor", "tp_optim_hyper", "tp_optim_state"):
        assert f"typedef struct {struct}" in HEADER and hasattr(_capi, struct), struct
    assert "#define TP_ABI_VERSION 6\n" in HEADER and lib.tp_version() == 6 == _capi.TP_ABI_VERSION
    assert "enum { TP_OPTIM_ZERO_GRAD = 1 }" in HEADER and _capi.TP_OPTIM_ZERO_GRAD == 1
    assert f"#define TP_OPTIM_STATE_BYTES {_capi.TP_OPTIM_STATE_BYTES}\n" in HEADER
    assert optim.MainGradAdamW is MainGradAdamW and issubclass(MainGradAdamW, torch.optim.Optimizer)


def _header_fields(struct):
    """(type, name) of the fields of a struct of the header, in order (comments dropped, `float a, b;` split, arrays kept)."""
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), HEADER, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = re.match(r"(.*?[\s*])(\w[\w\[\], ]*)$", decl).groups()
            out += [(ctype.strip(), n.strip()) for n in names.split(",")]
    return out


def test_struct_layouts_match_the_header():
    size = {"void*": 8, "float*": 8, "int64_t": 8, "float": 4, "int32_t": 4, "uint32_t": 4}
    for struct in ("tp_optim_tensor", "tp_optim_hyper", "tp_optim_state"):
        cls, offset = getattr(_capi, struct), 0
        fields = _header_fields(struct)
        assert [n.split("[")[0] for _, n in fields] == [f[0] for f in cls._fields_], struct
        for ctype, name in fields:
            count = int(name.split("[")[1].rstrip("]")) if "[" in name else 1
            width = size[ctype.replace(" ", "")]
            offset = -(-offset // width) * width                    # natural alignment, as the C compiler lays it out
            field = getattr(cls, name.split("[")[0])
            assert (field.offset, field.size) == (offset, width * count), (struct, name)
            offset += width * count
        assert ctypes.sizeof(cls) == offset, struct               # (no tail padding in any of the three)
    assert ctypes.sizeof(_capi.tp_optim_tensor) == 56 and ctypes.sizeof(_capi.tp_optim_hyper) == 24
    assert ctypes.sizeof(_capi.tp_optim_state) == _capi.TP_OPTIM_STATE_BYTES == 64
    assert [getattr(_capi.tp_optim_state, f).offset for f in ("grad_norm", "clip_coef", "found_inf", "step", "skipped", "bc1", "sqrt_bc2")] \
        == [0, 4, 8, 12, 16, 20, 24]


def _table(n=3, override=None):
    """n well-formed entries on distinct fake addresses; override: {(entry, field): value}."""
    t = (_capi.tp_optim_tensor * max(n, 1))()
    for i in range(n):
        base = FAKE + i * (1 << 16)
        t[i] = _capi.tp_optim_tensor(base, base + 4096, base + 8192, base + 12288, base + 16384, 1000 + i, 1e-3, 0.1)
    for (i, field), value in (override or {}).items():
        setattr(t[i], field, value)
    return t


def _hyper(**kw):
    args = dict(beta1=0.9, beta2=0.999, eps=1e-8, max_grad_norm=1.0, dtype=_capi.TP_BF16, flags=_capi.TP_OPTIM_ZERO_GRAD)
    args.update(kw)
    return _capi.tp_optim_hyper(**args)


def _step(t, n, h=None, ws_bytes=1 << 30, state=FAKE - 4096, ws=FAKE - (1 << 19), inv_scale=None):
    h = _hyper() if h is None else h
    return _capi.load_library().tp_optim_step(t, n, ctypes.byref(h) if h is not False else None, inv_scale, state, ws, ws_bytes, None)


def test_workspace_bytes():
    lib = _capi.load_library()
    from tests import optim_ref
    chunk = optim_ref.CHUNK
    one = _table(1, {(0, "numel"): chunk})
    two = _table(2, {(0, "numel"): chunk + 1, (1, "numel"): 1})
    state = _capi.TP_OPTIM_STATE_BYTES
    assert lib.tp_optim_workspace_bytes(one, 1) == 256 + state               # one partial, rounded up to 256 B, + the state block
    assert lib.tp_optim_workspace_bytes(two, 2) == 256 + state               # 2 + 1 chunks
    big = _table(1, {(0, "numel"): 4096 * 4096})
    assert lib.tp_optim_workspace_bytes(big, 1) == 4096 * 4096 // chunk * 4 + state
    assert lib.tp_optim_workspace_bytes(None, 0) == state
    for t, n, word in ((None, 2, "NULL table"), (one, -1, "negative"), (_table(2, {(1, "numel"): 0}), 2, "entry #1")):
        assert lib.tp_optim_workspace_bytes(t, n) == 0
        assert word in _capi.last_error(), _capi.last_error()


def test_an_empty_table_is_ok_and_launches_nothing():
    assert _step(None, 0) == _capi.TP_OK
    assert _step(_table(1), 0, ws_bytes=0, state=None, ws=None) == _capi.TP_OK


REFUSALS = [
    # (what is wrong, table overrides, hyper overrides, words the message must hold)
    ("NULL param", {(1, "param"): None}, {}, ("entry #1", "param is NULL")),
    ("NULL master", {(2, "master"): None}, {}, ("entry #2", "master is NULL")),
    ("NULL grad", {(0, "grad"): None}, {}, ("entry #0", "grad is NULL")),
    ("NULL exp_avg", {(1, "exp_avg"): None}, {}, ("entry #1", "exp_avg is NULL")),
    ("NULL exp_avg_sq", {(1, "exp_avg_sq"): None}, {}, ("entry #1", "exp_avg_sq is NULL")),
    ("numel 0", {(2, "numel"): 0}, {}, ("entry #2", "numel")),
    ("numel < 0", {(0, "numel"): -5}, {}, ("entry #0", "numel")),
    ("param off its 2-byte elements", {(1, "param"): FAKE + 70001}, {}, ("entry #1", "param", "aligned")),
    ("grad off its 4-byte elements", {(2, "grad"): FAKE + 200002}, {}, ("entry #2", "grad", "aligned")),
    ("master off its 4-byte elements", {(0, "master"): FAKE + 4097}, {}, ("entry #0", "master", "aligned")),
    ("the same address twice in one entry", {(1, "exp_avg"): FAKE + (1 << 16) + 4096}, {}, ("entry #1", "twice")),
    ("the same address in two entries", {(2, "grad"): FAKE + 8192}, {}, ("entry #", "twice")),
    ("negative lr", {(1, "lr"): -1e-3}, {}, ("entry #1", "lr")),
    ("non-finite lr", {(1, "lr"): float("inf")}, {}, ("entry #1", "lr")),
    ("NaN lr", {(0, "lr"): float("nan")}, {}, ("entry #0", "lr")),
    ("negative weight_decay", {(2, "weight_decay"): -0.1}, {}, ("entry #2", "weight_decay")),
    ("non-finite weight_decay", {(2, "weight_decay"): float("nan")}, {}, ("entry #2", "weight_decay")),
    ("beta1 = 1", {}, {"beta1": 1.0}, ("beta1",)),
    ("beta1 < 0", {}, {"beta1": -0.1}, ("beta1",)),
    ("beta2 NaN", {}, {"beta2": float("nan")}, ("beta2",)),
    ("beta2 > 1", {}, {"beta2": 1.5}, ("beta2",)),
    ("negative eps", {}, {"eps": -1e-8}, ("eps",)),
    ("non-finite eps", {}, {"eps": float("inf")}, ("eps",)),
    ("fp32 parameters", {}, {"dtype": _capi.TP_F32}, ("dtype",)),
    ("an unknown dtype", {}, {"dtype": 7}, ("dtype",)),
    ("unknown flags", {}, {"flags": 2}, ("flags",)),
]


@pytest.mark.parametrize("what,table,hyper,words", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_bad_calls_are_refused_before_any_launch(what, table, hyper, words):
    assert _step(_table(3, table), 3, _hyper(**hyper)) == E, what
    msg = _capi.last_error()
    assert msg.startswith("tp_optim_step") and all(w in msg for w in words), msg


def test_bad_counts_buffers_and_workspaces_are_refused():
    t = _table(3)
    assert _step(t, -1) == E and "negative" in _capi.last_error()
    assert _step(None, 3) == E and "NULL table" in _capi.last_error()
    assert _step(t, 3, h=False) == E and "hyper" in _capi.last_error()
    assert _step(t, 3, state=None) == E and "state" in _capi.last_error()
    assert _step(t, 3, ws=None) == E and "workspace" in _capi.last_error()
    need = _capi.load_library().tp_optim_workspace_bytes(t, 3)
    assert need > 0
    assert _step(t, 3, ws_bytes=need - 1) == E and "workspace" in _capi.last_error() and str(need) in _capi.last_error()
    assert _step(t, 3, inv_scale=FAKE + 2) == E and "inv_scale" in _capi.last_error()
    # max_grad_norm: <= 0 and +inf mean "no clipping" and are accepted by the checks; what is accepted here would go on to launch,
    # so only the refusal of a NaN can be shown without a device
    assert _step(t, 3, _hyper(max_grad_norm=float("nan"))) == E and "max_grad_norm" in _capi.last_error()


# ---- MainGradAdamW -----------------------------------------------------------------------------------------------------------
def test_main_grad_adamw_refuses_cpu_parameters():
    m = TokenPacker(hidden_size=256, scale_factor=2).to(torch.bfloat16)
    m.init_main_grads()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        MainGradAdamW(m.parameters(), module=m)


def test_main_grad_adamw_names_a_parameter_without_main_grad():
    m = TokenPacker(hidden_size=256, scale_factor=2).to(torch.bfloat16)
    with pytest.raises(TypeError, match=r"use_main_grad: parameter q_proj_1\.weight requires grad but has no main_grad"):
        MainGradAdamW(m.parameters(), module=m)
    m.init_main_grads()
    m.ln_q_1.weight.main_grad = m.ln_q_1.weight.main_grad.double()
    with pytest.raises(TypeError, match=r"ln_q_1\.weight\.main_grad is torch\.float64"):
        MainGradAdamW(m.parameters(), module=m)
    m.ln_q_1.weight.main_grad = torch.zeros(1025)[1:]
    with pytest.raises(ValueError, match=r"ln_q_1\.weight\.main_grad must be contiguous and 16-byte aligned"):
        MainGradAdamW(m.parameters(), module=m)
    p = torch.nn.Parameter(torch.zeros(8, dtype=torch.bfloat16))      # without a module the parameter is named by its index
    with pytest.raises(TypeError, match=r"parameter #0 requires grad but has no main_grad"):
        MainGradAdamW([p])


def test_main_grad_adamw_checks_its_hyper_parameters_and_leaves_frozen_parameters_alone():
    p = torch.nn.Parameter(torch.zeros(8, dtype=torch.bfloat16), requires_grad=False)
    for kw in (dict(lr=-1.0), dict(eps=-1.0), dict(betas=(1.0, 0.9)), dict(betas=(0.9, -0.1)), dict(weight_decay=-0.1)):
        with pytest.raises(ValueError):
            MainGradAdamW([p], **kw)
    opt = MainGradAdamW([p])                                           # nothing requires grad: nothing to check, nothing to step
    assert opt.step() is None and opt.state_dict()["state"] == {}
    with pytest.raises(RuntimeError, match="no state"):
        opt.grad_norm
    assert opt.param_groups[0]["lr"] == 1e-3 and opt.param_groups[0]["betas"] == (0.9, 0.999)
