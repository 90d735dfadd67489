"""Opt-in input gradients (tp_backward_inputs*, ABI 6) without a GPU: the symbols are declared and exported, tp_input_grads
has the header's layout, bad arguments are refused before the device is touched, the workspace size, and the fp64 oracle's
input gradients pinned against the goldens minted from the real reference (tools/make_input_grad_golden.py)."""
import ctypes
import glob
import os

import numpy as np
import pytest
import torch

from oracle import tokenpacker_oracle as orc
from tokenpacker_amd import _capi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("tp_backward_inputs_workspace_bytes", "tp_backward_inputs", "tp_backward_inputs_parts")


def test_new_symbols_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "tokenpacker.h")).read()
    lib = _capi.load_library()
    for name in NEW_SYMBOLS:
        assert f"{name}(" in header, name
        assert name in _capi.EXPORTED_SYMBOLS, name
        assert hasattr(lib, name), name
    assert "typedef struct tp_input_grads" in header
    assert _capi.TP_ABI_VERSION == 6 and lib.tp_version() == 6


def test_input_grads_struct_layout():
    P = ctypes.sizeof(ctypes.c_void_p)
    assert ctypes.sizeof(_capi.tp_input_grads) == 6 * P
    assert _capi.tp_input_grads.dx.offset == 0
    assert _capi.tp_input_grads.dx_multi.offset == P
    assert _capi.tp_input_grads.dx_multi_parts.offset == 2 * P


def _desc(B=1, grid=24, s=2, D=256, dtype=_capi.TP_BF16):
    return _capi.make_desc(B, grid, s, D, dtype)


def test_null_and_bad_arguments_are_rejected():
    lib = _capi.load_library()
    d = _desc()
    st = _capi.strides3((576 * 4096, 4096, 1))
    E = _capi.TP_ERR_INVALID_ARG
    ig = _capi.tp_input_grads()
    # every NULL
    assert lib.tp_backward_inputs(ctypes.byref(d), None, st, None, None, None, None, None, None, None, 0, None) == E
    assert lib.tp_backward_inputs_parts(ctypes.byref(d), None, st, None, None, None, None, None, None, None, 0, None) == E
    assert _capi.last_error()
    # non-NULL but fake pointers (never dereferenced: the argument checks come first)
    fake = 1 << 20
    w = _capi.tp_weights(*([fake] * len(_capi.WEIGHT_FIELDS)))
    parts = (ctypes.c_void_p * 4)(*([fake] * 4))

    def call(ig_arg, nbytes=1 << 40, grads=None, desc=d):
        return lib.tp_backward_inputs(ctypes.byref(desc), fake, st, ctypes.byref(w), fake, fake, fake, grads,
                                      ig_arg, fake, nbytes, None)

    assert call(None) == E                                           # ig is required
    assert call(ctypes.byref(ig)) == E                               # nothing requested at all
    assert "nothing requested" in _capi.last_error()
    ig_parts = _capi.tp_input_grads()
    ig_parts.dx_multi_parts[0] = fake                                # parts: all four or none ...
    assert call(ctypes.byref(ig_parts)) == E
    for i in range(4):
        ig_parts.dx_multi_parts[i] = fake
    assert call(ctypes.byref(ig_parts)) == E                         # ... and only through the _parts entry point
    ig_cat = _capi.tp_input_grads(dx_multi=fake)
    assert lib.tp_backward_inputs_parts(ctypes.byref(d), parts, st, ctypes.byref(w), fake, fake, fake, None,
                                        ctypes.byref(ig_cat), fake, 1 << 40, None) == E
    assert call(ctypes.byref(_capi.tp_input_grads(dx=fake + 8))) == E   # dx not 16-byte aligned
    # a too small workspace
    assert call(ctypes.byref(_capi.tp_input_grads(dx=fake)), nbytes=1024) == _capi.TP_ERR_WORKSPACE
    # a bad descriptor
    bad = _desc(s=5)
    assert call(ctypes.byref(_capi.tp_input_grads(dx=fake)), desc=bad) < 0
    # a gradient table with a NULL entry is refused like tp_backward refuses it
    g = _capi.tp_grads(*([fake] * len(_capi.WEIGHT_FIELDS)))
    g.mlp_2_bias = None
    assert call(ctypes.byref(_capi.tp_input_grads(dx=fake)), grads=ctypes.byref(g)) == E


@pytest.mark.parametrize("B,grid,s,D,dtype", [(1, 24, 2, 256, _capi.TP_BF16), (32, 24, 2, 4096, _capi.TP_BF16),
                                                (3, 24, 3, 256, _capi.TP_F16), (7, 8, 2, 384, _capi.TP_BF16)])
def test_workspace_bytes(B, grid, s, D, dtype):
    lib = _capi.load_library()
    d = _desc(B, grid, s, D, dtype)
    plain, inputs = lib.tp_backward_workspace_bytes(ctypes.byref(d)), lib.tp_backward_inputs_workspace_bytes(ctypes.byref(d))
    assert plain > 0 and inputs >= plain
    # the extra slabs: [Wk0; Wv0]^T, Wq1^T and dq0 (fp32 [B*M, 1024])
    assert inputs - plain >= 4096 * 2048 * 2 + 1024 * 1024 * 2 + B * (grid // s) ** 2 * 1024 * 4
    assert lib.tp_backward_inputs_workspace_bytes(ctypes.byref(_desc(s=5))) == 0
    assert lib.tp_backward_inputs_workspace_bytes(None) == 0


GOLD = sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "input_grad_s*.npz")))


def test_goldens_exist():
    assert [os.path.basename(p) for p in GOLD] == ["input_grad_s2.npz", "input_grad_s3.npz", "input_grad_s4.npz"]
    assert all(os.path.getsize(p) < 1 << 20 for p in GOLD)


@pytest.mark.parametrize("path", GOLD, ids=[os.path.basename(p)[:-4] for p in GOLD])
def test_oracle_input_gradients_match_the_reference(path):
    """The fp64 oracle's autograd dx / dx_multi (what the GPU tests gate against) is the reference module's own: pinned at fp32
    round-off when the golden was minted, and recomputed here against the stored subsample."""
    z = np.load(path)
    s, D, B = int(z["scale_factor"]), int(z["hidden_size"]), int(z["batch"])
    assert float(z["oracle_vs_ref_fp32"].max()) < 1e-4
    for tag in ("bf16", "fp16"):
        assert 0 < float(z[f"ref_{tag}_rel_l2"].max()) < 5e-2
    params = synth.make_params(int(z["param_seed"]), D)
    x, xm = synth.make_inputs(int(z["input_seed"]), B)
    w = torch.randn(B, (24 // s) ** 2, D, generator=torch.Generator().manual_seed(int(z["input_seed"]) + 1000))
    xx, mm = x.double().requires_grad_(True), xm.double().requires_grad_(True)
    (orc.forward(params, xx, mm, scale_factor=s, compute_dtype=torch.float64) * w.double()).sum().backward()
    dx_sub = xx.grad[:, torch.from_numpy(z["tok_dx"])].float()
    dxm_sub = mm.grad[:, torch.from_numpy(z["tok_dxm"]), ::4].float()
    for got, want in ((dx_sub, torch.from_numpy(z["dx_sub"])), (dxm_sub, torch.from_numpy(z["dxm_sub"]))):
        assert got.shape == want.shape
        assert float((got.double() - want.double()).norm() / want.double().norm()) < 1e-6
    # tap structure of the downsample's transpose: s = 3 receives at the centre pixel of each block only
    if s == 3:
        tok = torch.from_numpy(z["tok_dx"])
        r, c = tok // 24, tok % 24
        off = (r % 3 != 1) | (c % 3 != 1)
        assert bool((torch.from_numpy(z["dx_sub"])[0, off] == 0).all())
