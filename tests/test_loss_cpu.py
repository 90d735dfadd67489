"""Shifted cross-entropy without a GPU: the C ABI's declarations, bindings and host-side refusals, the module's own refusals,
and the test reference (tests/loss_ref.py) against F.cross_entropy on hand-made cases, the non-finite ones included."""
import ctypes
import math
import os
import re

import pytest
import torch
import torch.nn.functional as F

from tests import loss_ref
from tokenpacker_amd import _capi, loss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "tokenpacker.h")).read()
NAMES = ("tp_shift_ce_workspace_bytes", "tp_shift_ce_forward", "tp_shift_ce_backward")
INF = float("inf")


# ---- 1. the C ABI ----------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_bound():
    lib = _capi.load_library()
    for name in NAMES:
        assert re.search(r"\b%s\(" % name, HEADER), name
        assert name in _capi.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert lib.tp_shift_ce_forward.argtypes[0]._type_ is _capi.tp_shift_ce_args
    assert lib.tp_shift_ce_backward.argtypes[0]._type_ is _capi.tp_shift_ce_args
    assert lib.tp_shift_ce_workspace_bytes.restype is ctypes.c_size_t
    assert lib.tp_version() == 6 and "#define TP_ABI_VERSION 6" in HEADER


def test_struct_layout_matches_the_header():
    body = re.search(r"typedef struct tp_shift_ce_args \{(.*?)\} tp_shift_ce_args;", HEADER, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype, names = decl.rsplit(" ", 1)[0], None
        m = re.match(r"(const\s+)?(\w+)(\s*\*)?\s+(.*)", decl)
        ctype = "pointer" if m.group(3) else m.group(2)
        names = [n.strip() for n in m.group(4).split(",")]
        fields += [(n, ctype) for n in names]
    want = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t, "pointer": ctypes.c_void_p}
    assert [n for n, _ in fields] == [n for n, _ in _capi.tp_shift_ce_args._fields_]
    for (name, ctype), (_, bound) in zip(fields, _capi.tp_shift_ce_args._fields_):
        assert bound is want[ctype], name
    # six int32, five int64, four pointers and a size_t in between: no padding
    assert ctypes.sizeof(_capi.tp_shift_ce_args) == 6 * 4 + 5 * 8 + 6 * 8 == 112
    for macro, value in (("TP_SHIFT_CE_LOSS_OFFSET", 0), ("TP_SHIFT_CE_INV_N_OFFSET", 4), ("TP_SHIFT_CE_N_VALID_OFFSET", 8)):
        assert f"#define {macro} {value}" in HEADER and getattr(_capi, macro) == value
    assert "enum { TP_CE_MEAN = 0, TP_CE_SUM = 1 };" in HEADER and (_capi.TP_CE_MEAN, _capi.TP_CE_SUM) == (0, 1)


def test_workspace_bytes():
    lib = _capi.load_library()
    assert lib.tp_shift_ce_workspace_bytes(2, 64) == 2304                          # 256 + 16 * 126 = 2272, rounded up to 256
    assert lib.tp_shift_ce_workspace_bytes(1, 1) == 256                           # no row: the three results alone
    assert lib.tp_shift_ce_workspace_bytes(16, 2033) == 256 + 16 * 16 * 2032
    assert lib.tp_shift_ce_workspace_bytes(0, 5) == 0 and lib.tp_shift_ce_workspace_bytes(5, 0) == 0


def _valid_args(dtype=_capi.TP_BF16):
    """Arguments that pass validation, with pointers that address nothing (a refused call touches no memory; none of the calls
    below may pass validation, or a launch would be attempted without a GPU)."""
    a = _capi.tp_shift_ce_args()
    a.batch, a.len, a.V, a.dtype, a.reduction = 2, 5, 32003, dtype, _capi.TP_CE_MEAN
    a.row_stride, a.batch_stride = 32003, 5 * 32003
    a.d_row_stride, a.d_batch_stride = 32003, 5 * 32003
    a.ignore_index = -100
    a.logits, a.labels, a.workspace, a.grad_loss, a.dlogits = 0x10002, 0x20008, 0x30010, 0x40004, 0x50002
    a.workspace_bytes = _capi.load_library().tp_shift_ce_workspace_bytes(2, 5)
    return a


REFUSALS = [  # (what, direction: "both" or "backward", field, value, dtype of the call)
    ("NULL logits", "both", "logits", None, _capi.TP_BF16),
    ("NULL labels", "both", "labels", None, _capi.TP_BF16),
    ("NULL workspace", "both", "workspace", None, _capi.TP_BF16),
    ("NULL dlogits", "backward", "dlogits", None, _capi.TP_BF16),
    ("NULL grad_loss", "backward", "grad_loss", None, _capi.TP_BF16),
    ("unknown dtype", "both", "dtype", 3, _capi.TP_BF16),
    ("negative dtype", "both", "dtype", -1, _capi.TP_BF16),
    ("unknown reduction", "both", "reduction", 2, _capi.TP_BF16),
    ("V < 1", "both", "V", 0, _capi.TP_BF16),
    ("len < 1", "both", "len", 0, _capi.TP_BF16),
    ("batch < 1", "both", "batch", 0, _capi.TP_BF16),
    ("row stride below V", "both", "row_stride", 32002, _capi.TP_BF16),
    ("dlogits row stride below V", "backward", "d_row_stride", 32002, _capi.TP_BF16),
    ("workspace too small", "both", "workspace_bytes", 511, _capi.TP_BF16),
    ("bf16 logits at an odd address", "both", "logits", 0x10003, _capi.TP_BF16),
    ("fp32 logits at a 2-byte address", "both", "logits", 0x10002, _capi.TP_F32),
    ("labels not 8-byte aligned", "both", "labels", 0x20004, _capi.TP_BF16),
    ("workspace not 16-byte aligned", "both", "workspace", 0x30008, _capi.TP_BF16),
    ("dlogits at an odd address", "backward", "dlogits", 0x50003, _capi.TP_BF16),
    ("grad_loss not 4-byte aligned", "backward", "grad_loss", 0x40002, _capi.TP_BF16),
    ("dlogits not congruent to logits modulo 16 bytes", "backward", "dlogits", 0x50004, _capi.TP_BF16),
    ("dlogits row stride not congruent", "backward", "d_row_stride", 32004, _capi.TP_BF16),
    ("dlogits batch stride not congruent", "backward", "d_batch_stride", 5 * 32003 + 4, _capi.TP_BF16),
]


@pytest.mark.parametrize("what,direction,field,value,dtype", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_host_validation_refuses(what, direction, field, value, dtype):
    lib = _capi.load_library()
    calls = [lib.tp_shift_ce_backward] + ([lib.tp_shift_ce_forward] if direction == "both" else [])
    for call in calls:
        a = _valid_args(dtype)
        if dtype == _capi.TP_F32 and field != "logits":
            a.logits, a.dlogits = 0x10004, 0x50004
        setattr(a, field, value)
        assert call(ctypes.byref(a), None) == _capi.TP_ERR_INVALID_ARG, what
        msg = _capi.last_error()
        assert msg.startswith(call.__name__ + ": ") and len(msg) > len(call.__name__) + 10, (what, msg)


def test_in_place_needs_equal_strides_and_null_struct_is_refused():
    lib = _capi.load_library()
    a = _valid_args()
    a.dlogits = a.logits
    a.d_row_stride = a.row_stride + 8
    assert lib.tp_shift_ce_backward(ctypes.byref(a), None) == _capi.TP_ERR_INVALID_ARG
    assert "in place" in _capi.last_error()
    assert lib.tp_shift_ce_forward(None, None) == _capi.TP_ERR_INVALID_ARG
    assert lib.tp_shift_ce_backward(None, None) == _capi.TP_ERR_INVALID_ARG


# ---- 2. the module's refusals ------------------------------------------------------------------------------------------------
def test_module_raises_on_cpu_tensors_and_bad_arguments():
    x = torch.zeros(2, 3, 7, dtype=torch.bfloat16)
    y = torch.zeros(2, 3, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        loss.shifted_cross_entropy(x, y)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        loss.shifted_cross_entropy(x.requires_grad_(True), y)
    with pytest.raises(TypeError, match="bfloat16, float16 or float32"):
        loss.shifted_cross_entropy(x.detach().double(), y)
    with pytest.raises(ValueError, match="labels must be"):
        loss.shifted_cross_entropy(x, y[:, :2])
    with pytest.raises(TypeError, match="int64"):
        loss.shifted_cross_entropy(x, y.int())
    with pytest.raises(ValueError, match="stride 1"):
        loss.shifted_cross_entropy(torch.zeros(2, 7, 3, dtype=torch.bfloat16).transpose(1, 2), y)
    with pytest.raises(ValueError, match="reduction"):
        loss.shifted_cross_entropy(x, y, reduction="none")
    with pytest.raises(ValueError, match=r"\[B, L, V\]"):
        loss.shifted_cross_entropy(x[0], y[0])


def test_grad_buffer_rows_are_congruent_to_the_logits_rows():
    """The fresh gradient's rows sit at the logits rows' offsets from a 16-byte boundary (checked on CPU tensors: the layout
    arithmetic needs no device), whatever the view; it stays compact."""
    for dtype, per16 in ((torch.bfloat16, 8), (torch.float32, 4)):
        for V, pad, lead, extra_rows in ((32003, 0, 0, 0), (7, 64, 0, 0), (2049, 0, 1, 0), (64, 3, 5, 2), (1, 0, 3, 1)):
            B, L = 3, 4
            buf = torch.zeros(lead + B * (L + extra_rows) * (V + pad) + 64, dtype=dtype)
            x = buf.as_strided((B, L, V), ((L + extra_rows) * (V + pad), V + pad, 1), lead)
            g = loss._grad_buffer(x)
            assert g.shape == x.shape and g.dtype == x.dtype and g.stride(2) == 1 and g.stride(1) >= V
            assert g.stride(1) < V + per16 and g.stride(0) < L * g.stride(1) + per16
            for b in range(B):
                for t in range(L):
                    assert (g[b, t].data_ptr() - x[b, t].data_ptr()) % 16 == 0, (dtype, V, pad, lead, b, t)


# ---- 3. the test reference against F.cross_entropy ---------------------------------------------------------------------------
def _direct(x, y, dtype, reduction="mean"):
    """Row by row, without the reference's shift / view sequence: -log_softmax(x[b, t])[y[b, t + 1]] over the labelled rows."""
    x = x.to(dtype)
    rows = [F.cross_entropy(x[b, t][None], y[b, t + 1][None], reduction="sum")
            for b in range(x.shape[0]) for t in range(x.shape[1] - 1) if y[b, t + 1] != -100]
    total = torch.stack(rows).sum() if rows else torch.zeros((), dtype=dtype)
    return total / len(rows) if reduction == "mean" and rows else (total if rows else total + (math.nan if reduction == "mean" else 0))


def test_reference_on_hand_made_cases():
    # two classes, logits (0, log 3): p = (1/4, 3/4)
    x = torch.tensor([[[0.0, math.log(3.0)], [0.0, math.log(3.0)], [5.0, 5.0]]], dtype=torch.float64)
    y = torch.tensor([[1, 0, 1]])                      # row 0 -> class 0, row 1 -> class 1, row 2 has no target
    r = loss_ref.shifted_cross_entropy(x, y)
    assert r.n_valid == 2
    assert abs(float(r.loss) - 0.5 * (math.log(4.0) + math.log(4.0 / 3.0))) < 1e-15
    want = torch.tensor([[[-0.75, 0.75], [0.25, -0.25], [0.0, 0.0]]], dtype=torch.float64) / 2
    assert torch.allclose(r.grad, want, atol=1e-15)
    s = loss_ref.shifted_cross_entropy(x, y, reduction="sum", grad_out=4.0)
    assert abs(float(s.loss) - 2 * float(r.loss)) < 1e-15 and torch.allclose(s.grad, want * 8, atol=1e-14)
    # the first label is never a target; an ignored target drops its row from the count
    y2 = torch.tensor([[0, -100, 1]])
    r2 = loss_ref.shifted_cross_entropy(x, y2)
    assert r2.n_valid == 1 and abs(float(r2.loss) - math.log(4.0 / 3.0)) < 1e-15
    assert torch.equal(r2.grad[0, 0], torch.zeros(2, dtype=torch.float64)) and torch.equal(r2.grad[0, 2], torch.zeros(2, dtype=torch.float64))


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32, None])
def test_reference_equals_row_by_row_cross_entropy(dtype):
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(3, 5, 37, generator=g) * 4).to(torch.bfloat16)
    y = torch.randint(0, 37, (3, 5), generator=g)
    y[torch.rand(3, 5, generator=g) < 1 / 3] = -100
    y[0, 1] = 3
    for reduction in ("mean", "sum"):
        r = loss_ref.shifted_cross_entropy(x, y, dtype, reduction=reduction)
        cd = torch.bfloat16 if dtype is None else dtype
        assert r.loss.dtype == cd and r.grad.dtype == cd
        want = _direct(x, y, cd, reduction)
        tol = {torch.float64: 1e-14, torch.float32: 1e-6, torch.bfloat16: 2.0 ** -7}[cd]
        assert abs(float(r.loss) - float(want)) <= tol * abs(float(want))
        assert r.n_valid == int((y[:, 1:] != -100).sum())
        assert torch.equal(r.grad[:, -1], torch.zeros_like(r.grad[:, -1]))


def test_reference_on_the_non_finite_cases():
    """The five rows of the contract's table, as F.cross_entropy in fp32 answers them."""
    f32 = torch.float32
    # 1. no labelled row at all: NaN, gradient zero
    x = torch.randn(2, 3, 7)
    r = loss_ref.shifted_cross_entropy(x, torch.full((2, 3), -100), f32)
    assert math.isnan(float(r.loss)) and r.n_valid == 0 and torch.equal(r.grad, torch.zeros_like(x))
    assert float(loss_ref.shifted_cross_entropy(x, torch.full((2, 3), -100), f32, reduction="sum").loss) == 0.0
    # 2. -inf logits beside finite ones: finite loss, exact zeros at their positions
    x = torch.tensor([[[-INF, 1.0, -INF, 2.0], [0.0, 0.0, 0.0, 0.0]]])
    y = torch.tensor([[0, 3]])
    r = loss_ref.shifted_cross_entropy(x, y, f32)
    assert math.isfinite(float(r.loss)) and abs(float(r.loss) - math.log(1 + math.exp(-1.0))) < 1e-6
    assert r.grad[0, 0, 0] == 0 and r.grad[0, 0, 2] == 0 and torch.isfinite(r.grad).all()
    # 3. -inf at the target: +inf, finite gradient, -1 at the target
    r = loss_ref.shifted_cross_entropy(x, torch.tensor([[0, 2]]), f32)
    assert float(r.loss) == INF and torch.isfinite(r.grad).all() and float(r.grad[0, 0, 2]) == -1.0
    # 4. a row of -inf only: NaN, NaN in that row
    x4 = torch.stack([torch.full((4,), -INF), torch.zeros(4), torch.zeros(4)])[None]
    r = loss_ref.shifted_cross_entropy(x4, torch.tensor([[0, 1, 1]]), f32, reduction="sum")
    assert math.isnan(float(r.loss)) and torch.isnan(r.grad[0, 0]).all() and torch.isfinite(r.grad[0, 1:]).all()
    # 5. +-3e38: 3e38, gradient exactly 1 / 0 / -1
    x5 = torch.tensor([[[3e38, 0.0, -3e38, -3e38], [0.0, 0.0, 0.0, 0.0]]])
    r = loss_ref.shifted_cross_entropy(x5, torch.tensor([[0, 1]]), f32)
    assert float(r.loss) == float(torch.tensor(3e38)) and r.grad[0, 0].tolist() == [1.0, -1.0, 0.0, 0.0]
    # the same answers row by row, and in float64 wherever float64 can hold the case
    for xx, yy in ((x, y), (x, torch.tensor([[0, 2]])), (x5, torch.tensor([[0, 1]]))):
        a, b = loss_ref.shifted_cross_entropy(xx, yy, f32), _direct(xx, yy, f32)
        assert float(a.loss) == float(b)
        c = loss_ref.shifted_cross_entropy(xx, yy, torch.float64)
        assert torch.equal(torch.isfinite(c.grad), torch.isfinite(a.grad)) and math.isfinite(float(c.loss)) == math.isfinite(float(a.loss))


def test_ordered_bits_counts_units_in_the_last_place():
    for dtype in (torch.bfloat16, torch.float16):
        t = torch.tensor([0.0, -0.0, 1.0, -1.0], dtype=dtype)
        nxt = torch.nextafter(t.float(), torch.tensor(INF)).to(dtype)           # (float32 neighbours round back: equal values)
        o = loss_ref.ordered_bits(t)
        assert o[0] == o[1] == 0 and o[2] == -o[3] and torch.equal(loss_ref.ordered_bits(nxt), o)
        one = torch.tensor([1.0], dtype=dtype)
        up = (one.float() * (1 + torch.finfo(dtype).eps)).to(dtype)
        assert int(loss_ref.ordered_bits(up) - loss_ref.ordered_bits(one)) == 1
        tiny = torch.tensor([torch.finfo(dtype).smallest_normal], dtype=dtype)
        assert int(loss_ref.ordered_bits(tiny) - loss_ref.ordered_bits(tiny * 0)) == (1 << {torch.bfloat16: 7, torch.float16: 10}[dtype])
