"""Training through the HD token splice, the parts that need no GPU: the C entry point of the assembly's backward (symbols,
argument checks), the label / attention-mask logic of hd.build_multimodal_inputs against the reference's own outputs, and the
float64 oracle's gradients against the reference's autograd (tests/golden/hd_splice_train.npz, minted by
tools/make_hd_train_golden.py from the unmodified prepare_inputs_labels_for_multimodal)."""
import ctypes
import hashlib
import os

import numpy as np
import pytest
import torch

from oracle import hd_oracle
from tokenpacker_amd import _capi, hd

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "hd_splice_train.npz")
BATCHES = ("ragged", "equal")


def load_batch(name):
    z = np.load(GOLDEN)
    b = {k[len(name) + 1:]: z[k] for k in z.files if k.startswith(name + "_")}
    t = {k: torch.from_numpy(b[k]) for k in ("ids", "feats", "table", "labels", "attention_mask", "dout")}
    h = hashlib.sha256()
    for k in ("ids", "feats", "table", "labels", "attention_mask", "dout"):
        h.update(t[k].contiguous().numpy().tobytes())
    assert h.hexdigest() == str(b["inputs_sha256"])
    t.update(hb=[int(v) for v in b["h_block"]], wb=[int(v) for v in b["w_block"]], sep_id=int(b["sep_id"]),
             ret_id=int(b["ret_id"]))
    for k in ("new_input_embeds", "new_labels", "attention_mask_out", "d_feats", "d_table"):
        t[k] = torch.from_numpy(b[k])
    return t


def test_backward_symbols_are_exported_and_declared():
    lib = _capi.load_library()
    for name in ("tp_hd_assemble_backward", "tp_hd_assemble_backward_workspace_bytes"):
        assert name in _capi.EXPORTED_SYMBOLS and hasattr(lib, name)
    src = open(os.path.join(os.path.dirname(os.path.dirname(__file__)), "include", "tokenpacker.h")).read()
    assert "int tp_hd_assemble_backward(" in src and "size_t tp_hd_assemble_backward_workspace_bytes(" in src
    assert _capi.TP_ABI_VERSION == 6 and lib.tp_version() == 6


def test_backward_workspace_size():
    lib = _capi.load_library()
    assert lib.tp_hd_assemble_backward_workspace_bytes(0, 10, 4096) == 0
    assert lib.tp_hd_assemble_backward_workspace_bytes(2, 0, 4096) == 0
    # int64 source row per token block (rounded up to 256 B) + fp32 ',' and '\n' partials per image
    assert lib.tp_hd_assemble_backward_workspace_bytes(3, 10, 4096) == 256 + 3 * 2 * 4096 * 4
    assert lib.tp_hd_assemble_backward_workspace_bytes(70, 33, 64) == 512 + 70 * 2 * 64 * 4


def test_backward_rejects_bad_arguments_without_touching_the_device():
    lib = _capi.load_library()
    E = _capi.TP_ERR_INVALID_ARG
    fake = ctypes.c_void_p(0x10000)              # 16-byte aligned, never dereferenced: validation fails first
    ws = 1 << 20

    def call(plan, n, n_crops, out_rows, n_tok, D=256, dtype=_capi.TP_BF16, cmap=None, dout=fake, dtok=fake, dsep=fake,
             dret=fake, work=fake, ws_bytes=ws):
        return lib.tp_hd_assemble_backward(plan, n, dout, out_rows, n_crops, cmap, dtok, n_tok, dsep, dret, 144, D, dtype,
                                           work, ws_bytes, None)

    one = (_capi.tp_hd_image * 1)(_capi.tp_hd_image(0, 1, 1, 0, 0))
    assert call(None, 1, 1, 145, 1) == E
    assert call(one, 0, 1, 145, 1) == E
    assert call(one, 1, 1, 145, 1, dout=None) == E
    assert call(one, 1, 1, 145, 1, dtok=None) == E
    assert call(one, 1, 1, 145, 1, dsep=None) == E
    assert call(one, 1, 1, 145, 1, dret=None) == E
    assert call(one, 1, 1, 145, 1, work=None) == E
    assert call(one, 1, 1, 145, 1, dtype=_capi.TP_F32) == E
    assert call(one, 1, 1, 145, 1, D=260) == E                                  # D % 8
    assert call(one, 1, 1, 145, 1, dsep=ctypes.c_void_p(0x10008)) == E          # 16-byte alignment
    assert call(one, 1, 1, 145, 1, work=ctypes.c_void_p(0x10004)) == E
    assert call(one, 1, 1, 145, 0) == E                                         # no token blocks
    assert call(one, 1, 2, 145, 1) == E                                         # dtokens smaller than the crops, no map
    assert call(one, 1, 1, 144, 1) == E                                         # the block needs 145 rows
    two = (_capi.tp_hd_image * 2)(_capi.tp_hd_image(0, 2, 2, 0, 0), _capi.tp_hd_image(4, 1, 1, 0, 725))   # 2x2 uses 5 crops
    assert call(two, 2, 6, 2000, 6) == E
    two = (_capi.tp_hd_image * 2)(_capi.tp_hd_image(0, 2, 2, 0, 0), _capi.tp_hd_image(5, 1, 1, 0, 700))   # rows 0..724 taken
    assert call(two, 2, 6, 2000, 6) == E
    two = (_capi.tp_hd_image * 2)(_capi.tp_hd_image(0, 2, 2, 0, 0), _capi.tp_hd_image(5, 1, 1, 0, 900))
    assert call(two, 2, 5, 2000, 6) == E                                        # crop 5 of 5
    assert call(two, 2, 6, 1000, 6) == E                                        # rows up to 1045 of 1000
    bad = (_capi.tp_hd_image * 1)(_capi.tp_hd_image(0, 0, 1, 0, 0))
    assert call(bad, 1, 1, 145, 1) == E
    need = lib.tp_hd_assemble_backward_workspace_bytes(2, 6, 256)
    assert call(two, 2, 6, 2000, 6, ws_bytes=need - 1) == _capi.TP_ERR_WORKSPACE
    assert "tp_hd_assemble_backward" in _capi.last_error()


@pytest.mark.parametrize("name", BATCHES)
def test_labels_and_mask_equal_the_reference(name):
    b = load_batch(name)
    M = b["feats"].shape[1]
    mask, labels = hd.splice_labels_and_mask(b["ids"], b["hb"], b["wb"], M, labels=b["labels"],
                                             attention_mask=b["attention_mask"])
    assert labels.dtype == b["labels"].dtype and torch.equal(labels, b["new_labels"])
    assert mask.dtype == torch.bool and torch.equal(mask, b["attention_mask_out"])
    assert labels.shape == b["new_input_embeds"].shape[:2]
    # either output is None when its input is
    mask2, labels2 = hd.splice_labels_and_mask(b["ids"], b["hb"], b["wb"], M, labels=b["labels"])
    assert mask2 is None and torch.equal(labels2, b["new_labels"])
    none = hd.splice_labels_and_mask(b["ids"], b["hb"], b["wb"], M)
    assert none == (None, None)


def test_labels_and_mask_follow_the_mask_dtype_and_the_equal_branch_without_labels():
    b = load_batch("equal")
    M = b["feats"].shape[1]
    mask, labels = hd.splice_labels_and_mask(b["ids"], b["hb"], b["wb"], M, attention_mask=b["attention_mask"].long())
    assert labels is None and mask.dtype == torch.long and torch.equal(mask, b["attention_mask_out"].long())


def test_ragged_mask_without_labels_raises_like_the_reference():
    b = load_batch("ragged")
    with pytest.raises(ValueError):
        hd.splice_labels_and_mask(b["ids"], b["hb"], b["wb"], b["feats"].shape[1], attention_mask=b["attention_mask"])


@pytest.mark.parametrize("name", BATCHES)
def test_oracle_gradients_equal_the_reference_autograd(name):
    """Autograd through hd_oracle.splice_inputs_embeds in float64 against the reference's float64 autograd: both are float64
    sums of a few dozen terms, so |diff| <= 1e-12 max|golden|.  Pins the oracle for the GPU gradient tests."""
    b = load_batch(name)
    feats = b["feats"].clone().requires_grad_(True)
    table = b["table"].clone().requires_grad_(True)
    emb = hd_oracle.splice_inputs_embeds(b["ids"], lambda t: table[t], feats, b["hb"], b["wb"], b["sep_id"], b["ret_id"])
    assert torch.equal(emb.detach(), b["new_input_embeds"])
    (emb * b["dout"]).sum().backward()
    for got, want in ((feats.grad, b["d_feats"]), (table.grad, b["d_table"])):
        err = float((got - want).abs().max())
        print(f"{name}: oracle vs reference gradient max|diff| {err:.3e} (max|golden| {float(want.abs().max()):.3e})")
        assert err <= 1e-12 * float(want.abs().max())
