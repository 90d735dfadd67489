"""Training with an attn_mask (tp_forward_train_masked / tp_forward_parts_masked / tp_backward_masked, an ABI 6 extension) without a
GPU: the symbols are declared, exported and bound, tp_attn_mask has the header's layout, bad arguments are refused before the
device is touched, the masked training forward needs no more workspace than the unmasked one, and the fp64 oracle's parameter
gradients and dL/dmask are pinned against the goldens minted from the real reference (tools/make_mask_grad_golden.py)."""
import ctypes
import glob
import os
import re

import numpy as np
import pytest
import torch

from oracle import tokenpacker_oracle as orc
from tokenpacker_amd import _capi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("tp_forward_train_masked", "tp_forward_parts_masked", "tp_backward_masked")


def test_new_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "tokenpacker.h")).read()
    lib = _capi.load_library()
    for name in NEW_SYMBOLS:
        assert f"{name}(" in header, name
        assert name in _capi.EXPORTED_SYMBOLS, name
        assert hasattr(lib, name), name
        assert getattr(lib, name).restype is ctypes.c_int and getattr(lib, name).argtypes, name
    assert "typedef struct tp_attn_mask" in header
    assert lib.tp_version() == _capi.TP_ABI_VERSION


def test_attn_mask_struct_layout():
    P = ctypes.sizeof(ctypes.c_void_p)
    assert ctypes.sizeof(_capi.tp_attn_mask) == 2 * P + 8
    assert _capi.tp_attn_mask.mask.offset == 0
    assert _capi.tp_attn_mask.mode.offset == P
    assert _capi.tp_attn_mask.reserved.offset == P + 4
    assert _capi.tp_attn_mask.grad.offset == P + 8


def _desc(B=2, grid=24, s=2, D=256, dtype=_capi.TP_BF16, flags=0):
    return _capi.make_desc(B, grid, s, D, dtype, flags=flags)


FAKE = 1 << 20          # a non-NULL, 256-byte aligned address that the argument checks never dereference


def test_backward_masked_rejects_bad_masks_before_any_launch():
    lib = _capi.load_library()
    d = _desc()
    st = _capi.strides3((576 * 4096, 4096, 1))
    w = _capi.tp_weights(*([FAKE] * len(_capi.WEIGHT_FIELDS)))
    g = _capi.tp_grads(*([FAKE] * len(_capi.WEIGHT_FIELDS)))
    E = _capi.TP_ERR_INVALID_ARG

    def call(am, grads=ctypes.byref(g), ig=None, x_multi=FAKE, parts=None):
        return lib.tp_backward_masked(ctypes.byref(d), x_multi, parts, st, ctypes.byref(w), FAKE, FAKE, FAKE, grads, ig,
                                      am, FAKE, 1 << 40, None)

    assert call(None) == E                                                          # the mask argument is required
    for mode in (-1, 3, 7):                                                         # a bad mode
        assert call(ctypes.byref(_capi.tp_attn_mask(mask=FAKE, mode=mode))) == E, mode
        assert "mode" in _capi.last_error()
    for mode in (1, 2):                                                             # a mode without a mask
        assert call(ctypes.byref(_capi.tp_attn_mask(mask=None, mode=mode))) == E, mode
    assert call(ctypes.byref(_capi.tp_attn_mask(mask=None, mode=0, grad=FAKE))) == E   # a gradient without a mask
    assert call(ctypes.byref(_capi.tp_attn_mask(mask=FAKE, mode=0))) == E          # a mask without a mode
    assert call(ctypes.byref(_capi.tp_attn_mask(mask=FAKE + 2, mode=1))) == E      # a misaligned fp32 mask
    for mode in (0, 1, 2):                                                          # reserved must be 0
        am = _capi.tp_attn_mask(mask=FAKE if mode else None, mode=mode, reserved=1)
        assert call(ctypes.byref(am)) == E, mode
        assert "reserved" in _capi.last_error()
    # nothing requested: no parameter, input or mask gradient
    assert call(ctypes.byref(_capi.tp_attn_mask(mask=FAKE, mode=1)), grads=None) == E
    # a mask gradient alone is a request (refused here by the workspace size, still before any launch)
    assert lib.tp_backward_masked(ctypes.byref(d), FAKE, None, st, ctypes.byref(w), FAKE, FAKE, FAKE, None, None,
                                  ctypes.byref(_capi.tp_attn_mask(mask=FAKE, mode=1, grad=FAKE)), FAKE, 1024,
                                  None) == _capi.TP_ERR_WORKSPACE
    # the input-gradient rules of tp_backward_inputs hold here too
    parts = (ctypes.c_void_p * 4)(*([FAKE] * 4))
    ig_cat = _capi.tp_input_grads(dx_multi=FAKE)
    assert call(ctypes.byref(_capi.tp_attn_mask(mask=FAKE, mode=1)), ig=ctypes.byref(ig_cat), x_multi=None, parts=parts) == E
    # a too small workspace
    assert lib.tp_backward_masked(ctypes.byref(d), FAKE, None, st, ctypes.byref(w), FAKE, FAKE, FAKE, ctypes.byref(g), None,
                                  ctypes.byref(_capi.tp_attn_mask(mask=FAKE, mode=1)), FAKE, 1024, None) == _capi.TP_ERR_WORKSPACE


def test_forward_entry_points_reject_bad_masks():
    lib = _capi.load_library()
    d = _desc()
    xs, st = _capi.strides3((576 * 1024, 1024, 1)), _capi.strides3((576 * 4096, 4096, 1))
    parts = (ctypes.c_void_p * 4)(*([FAKE] * 4))
    ps = _capi.strides3((576 * 1024, 1024, 1))
    E = _capi.TP_ERR_INVALID_ARG
    for mask, mode in ((FAKE, 3), (FAKE, -1), (None, 1), (None, 2)):
        assert lib.tp_forward_train_masked(ctypes.byref(d), FAKE, xs, FAKE, None, st, FAKE, FAKE, FAKE, 1 << 40, mask, mode,
                                           None) == E
        assert lib.tp_forward_parts_masked(ctypes.byref(d), FAKE, xs, parts, ps, FAKE, FAKE, FAKE, 1 << 40, mask, mode,
                                           None) == E
    assert lib.tp_forward_parts_masked(ctypes.byref(d), FAKE, xs, None, ps, FAKE, FAKE, FAKE, 1 << 40, FAKE, 1, None) == E


@pytest.mark.parametrize("B,grid,s,D", [(2, 24, 2, 256), (3, 24, 3, 256), (32, 24, 2, 4096), (2, 24, 4, 256)])
@pytest.mark.parametrize("use_parts", [False, True])
def test_masked_training_workspace_is_the_unmasked_one(B, grid, s, D, use_parts):
    """The training schedule writes K | V with or without a mask (plan_schedule): tp_forward_train_masked asks for exactly
    tp_train_workspace_bytes — one byte less is refused (before any launch) and the error names that size."""
    lib = _capi.load_library()
    d = _desc(B, grid, s, D)
    need = lib.tp_train_workspace_bytes(ctypes.byref(d))
    assert need > 0
    assert lib.tp_train_workspace_bytes(ctypes.byref(_desc(B, grid, s, D, flags=_capi.TP_DESC_MASKED))) == need
    N = grid * grid
    xs = _capi.strides3((N * 1024, 1024, 1))
    parts = (ctypes.c_void_p * 4)(*([FAKE] * 4)) if use_parts else None
    st = _capi.strides3((N * 1024, 1024, 1) if use_parts else (N * 4096, 4096, 1))
    for mode in (1, 2):
        rc = lib.tp_forward_train_masked(ctypes.byref(d), FAKE, xs, None if use_parts else FAKE, parts, st, FAKE, FAKE, FAKE,
                                         need - 1, FAKE, mode, None)
        assert rc == _capi.TP_ERR_WORKSPACE
        assert int(re.search(r"required (\d+) B", _capi.last_error()).group(1)) == need


GOLD = sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "mask_grad_s*.npz")))
KINDS = ("2d_float", "3d_bool", "3d_float")


def test_goldens_exist_and_stay_small():
    assert [os.path.basename(p) for p in GOLD] == ["mask_grad_s2.npz", "mask_grad_s3.npz", "mask_grad_s4.npz"]
    smallest_input_grad = min(os.path.getsize(p) for p in glob.glob(os.path.join(os.path.dirname(__file__), "golden",
                                                                                   "input_grad_s*.npz")))
    assert all(os.path.getsize(p) < smallest_input_grad for p in GOLD)


@pytest.mark.parametrize("path", GOLD, ids=[os.path.basename(p)[:-4] for p in GOLD])
def test_oracle_mask_gradients_match_the_reference(path):
    """The fp64 oracle's autograd with a mask — parameter gradients and dL/dmask, what the GPU tests gate against — is the
    reference module's own: pinned at fp32 round-off when the golden was minted, and dmask recomputed here against the stored
    values (2-D: all s*s entries; 3-D: every row_step-th row)."""
    z = np.load(path)
    s, D, B = int(z["scale_factor"]), int(z["hidden_size"]), int(z["batch"])
    assert len(z["names"]) == 23
    for kind in KINDS:
        assert float(z[f"oracle_vs_ref_fp32_{kind}"].max()) < 1e-4, kind
        for tag in ("bf16", "fp16"):
            assert 0 < float(z[f"ref_{tag}_grad_{kind}"].max()) < 0.1, (kind, tag)
            if kind != "3d_bool":
                assert 0 < float(z[f"ref_{tag}_dmask_{kind}"]) < 0.1, (kind, tag)
    params = synth.make_params(int(z["param_seed"]), D)
    x, xm = synth.make_inputs(int(z["input_seed"]), B)
    w = torch.randn(B, (24 // s) ** 2, D, generator=torch.Generator().manual_seed(int(z["input_seed"]) + 1000))
    masks = synth.make_train_attn_masks(int(z["input_seed"]) + 1, B, s)       # (the masks the golden was minted with)
    for kind in ("2d_float", "3d_float"):
        mk = masks[kind].double().requires_grad_(True)
        (orc.forward(params, x, xm, scale_factor=s, compute_dtype=torch.float64, attn_mask=mk) * w.double()).sum().backward()
        got = mk.grad.reshape(1, -1) if kind.startswith("2d") else mk.grad.reshape(-1, s * s)[::int(z["row_step"])]
        want = torch.from_numpy(z[f"dmask_{kind}"]).double()
        assert got.shape == want.shape
        assert float((got - want).norm() / want.norm()) < 1e-6, kind
