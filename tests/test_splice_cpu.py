"""The one-launch token splice (tokenpacker_amd.splice), the parts that need no GPU: the C entry points (symbols, host-side
refusals, workspace size), the host layout, and the plain-torch twin tests/splice_ref.py against what the reference's own
prepare_inputs_labels_for_multimodal returned (tests/golden/splice_plain.npz, minted by tools/make_splice_golden.py with
mode=None) and, in slice mode, against hd.splice_labels_and_mask / oracle.hd_oracle on tests/golden/hd_splice_train.npz."""
import ctypes
import os

import numpy as np
import pytest
import torch

from oracle import hd_oracle
from tests import splice_ref
from tokenpacker_amd import _capi, hd, splice
import tokenpacker_amd

from tests.splice_ref import BATCHES, GOLDEN, HD_GOLDEN, INPUTS, OUTPUTS, load_batch  # noqa: F401


# ---- 1. the C surface --------------------------------------------------------------------------------------------------------
def test_symbols_are_exported_bound_and_declared():
    lib = _capi.load_library()
    for name in ("tp_splice", "tp_splice_backward", "tp_splice_backward_workspace_bytes"):
        assert name in _capi.EXPORTED_SYMBOLS and hasattr(lib, name)
        assert getattr(lib, name).argtypes is not None
    src = open(os.path.join(os.path.dirname(os.path.dirname(__file__)), "include", "tokenpacker.h")).read()
    assert "int tp_splice(" in src and "int tp_splice_backward(" in src and "size_t tp_splice_backward_workspace_bytes(" in src
    assert _capi.TP_ABI_VERSION == 6 and lib.tp_version() == 6                       # additive: the version stays
    assert tokenpacker_amd.build_multimodal_inputs is splice.build_multimodal_inputs
    assert tokenpacker_amd.splice_layout is splice.splice_layout


def test_backward_workspace_size():
    lib = _capi.load_library()
    assert lib.tp_splice_backward_workspace_bytes(0, 144) == 0
    assert lib.tp_splice_backward_workspace_bytes(4, 0) == 0
    # one int32 source row per feature row, rounded up to 256 B
    assert lib.tp_splice_backward_workspace_bytes(4, 16) == 256
    assert lib.tp_splice_backward_workspace_bytes(32, 144) == 32 * 144 * 4
    assert lib.tp_splice_backward_workspace_bytes(3, 144) == 1792


FAKE = 0x10000                    # 16-byte aligned, never dereferenced: validation fails first


def small_args(**over):
    """A valid forward call for ids [[5, IMG, 6]] with M = 2, V = 8, D = 16 (device pointers are fakes), then `over`."""
    T, F, P = 0, 2 << 30, 3 << 30
    plan = np.array([T | 0, F | 0, F | 1, T | 2, 4], dtype=np.uint32).view(np.int32)       # 4 rows | length 4
    ids = np.array([5, -200, 6], dtype=np.int64)
    a = _capi.tp_splice_args()
    a.batch, a.in_len, a.out_len, a.M, a.D, a.dtype = 1, 3, 4, 2, 16, _capi.TP_BF16
    a.V, a.n_feat_blocks, a.n_logical = 8, 1, 1
    a.plan_host, a.plan_dev, a.ids_host, a.ids_dev = plan.ctypes.data, FAKE, ids.ctypes.data, FAKE
    a.table, a.feats, a.out, a.mask_bytes, a.padding_idx = FAKE, FAKE, FAKE, 1, -1
    keep = [plan, ids]
    for k, v in over.items():
        if isinstance(v, np.ndarray):
            keep.append(v)
            v = v.ctypes.data
        setattr(a, k, v)
    return a, keep


def refused(fn, a, needle):
    rc = fn(ctypes.byref(a), None)
    assert rc == _capi.TP_ERR_INVALID_ARG, (rc, needle)
    assert needle in _capi.last_error(), (_capi.last_error(), needle)


def test_forward_refuses_bad_arguments_on_the_host():
    lib = _capi.load_library()
    f = lib.tp_splice
    assert f(None, None) == _capi.TP_ERR_INVALID_ARG
    for over, needle in (
            (dict(out=None), "NULL out"), (dict(table=None), "NULL out"), (dict(ids_dev=None), "NULL out"),
            (dict(plan_host=None), "NULL plan"), (dict(plan_dev=None), "NULL plan"),
            (dict(D=20), "multiple of 8"), (dict(D=0), "multiple of 8"),
            (dict(dtype=_capi.TP_F32), "dtype 2 unsupported"),
            (dict(out=FAKE + 8), "misaligned"), (dict(table=FAKE + 2), "misaligned"), (dict(feats=FAKE + 4), "misaligned"),
            (dict(ids_dev=FAKE + 4), "misaligned"), (dict(plan_dev=FAKE + 2), "misaligned"),
            (dict(labels=FAKE), "in pairs"), (dict(out_mask=FAKE), "in pairs"),
            (dict(labels=FAKE + 4, out_labels=FAKE), "misaligned"),
            (dict(mask=FAKE, out_mask=FAKE, mask_bytes=4), "mask_bytes"),
            (dict(batch=0), "non-positive"), (dict(M=0), "non-positive"), (dict(V=0), "non-positive"),
            (dict(n_logical=2), "n_logical"),
            (dict(feats=None), "feats is NULL"),
            (dict(n_feat_blocks=0, n_logical=0), "reads feature row"),                  # counts that do not match the plan
            (dict(V=6), "outside the table"),                                            # id 6 with a table of 6 rows
            (dict(plan_host=np.array([7, 0, 0, 0, 4], dtype=np.int32)), "outside its sample"),
            (dict(plan_host=np.array([(1 << 30) | 8, 0, 0, 0, 4], dtype=np.int32)), "names table row"),
            (dict(plan_host=np.array([0, 0, 0, 0, 5], dtype=np.int32)), "length 5"),
            (dict(plan_host=np.array([0, 0, 0, 0, 2], dtype=np.int32)), "length 2")):
        a, keep = small_args(**over)
        refused(f, a, needle)


def test_backward_refuses_bad_arguments_on_the_host():
    lib = _capi.load_library()
    f = lib.tp_splice_backward
    order = np.array([0, 3, 0, 0, 0, 0, 0, 0, 1, 2, 2], dtype=np.int32)                # rows 0 (id 5), 3 (id 6) | offsets [V + 1]
    ok = dict(dout=FAKE, dfeats=FAKE, dtable=FAKE, workspace=FAKE, workspace_bytes=256, order_host=order, order_dev=FAKE,
              n_table_rows=2)
    for over, needle in (
            (dict(dout=None), "NULL dout"), (dict(dfeats=None, dtable=None), "neither"),
            (dict(dout=FAKE + 8), "misaligned"), (dict(dtable=FAKE + 4), "misaligned"), (dict(workspace=FAKE + 8), "misaligned"),
            (dict(order_dev=FAKE + 1), "misaligned"),
            (dict(D=12), "multiple of 8"), (dict(dtype=7), "dtype 7 unsupported"),
            (dict(order_host=None), "dtable needs"), (dict(ids_host=None), "dtable needs"), (dict(order_dev=None), "dtable needs"),
            (dict(padding_idx=8), "padding_idx"),
            (dict(n_table_rows=3), "n_table_rows = 3"),
            (dict(order_host=np.array([3, 0, 0, 0, 0, 0, 0, 0, 1, 2, 2], dtype=np.int32)), "readers of table row 5"),
            (dict(order_host=np.array([0, 3, 0, 0, 0, 0, 0, 1, 1, 2, 2], dtype=np.int32)), "readers of table row 4"),
            (dict(order_host=np.array([0, 3, 0, 0, 0, 0, 0, 0, 1, 2, 1], dtype=np.int32)), "offsets"),
            (dict(order_host=np.array([0, 1, 0, 0, 0, 0, 0, 0, 1, 2, 2], dtype=np.int32)), "readers of table row 6"),
            (dict(plan_host=np.array([0, 2 << 30, 2 << 30, 2, 4], dtype=np.uint32).view(np.int32)), "read by two output rows")):
        a, keep = small_args(**{**ok, **over})
        refused(f, a, needle)
    a, keep = small_args(**{**ok, "workspace_bytes": 255})
    assert f(ctypes.byref(a), None) == _capi.TP_ERR_WORKSPACE and "tp_splice_backward" in _capi.last_error()
    a, keep = small_args(**{**ok, "workspace": None})
    assert f(ctypes.byref(a), None) == _capi.TP_ERR_WORKSPACE


# ---- 2. layout and twin against the reference's outputs ----------------------------------------------------------------------
def twin(b, **kw):
    feats = b["feats"].clone().requires_grad_(True)
    emb = torch.nn.Embedding.from_pretrained(b["table"].clone(), freeze=False, padding_idx=b.get("padding_idx"))
    mask, embeds, labels = splice_ref.build_multimodal_inputs(b["ids"], emb, feats, b["labels"], b["attention_mask"], **kw)
    embeds.backward(b["dout"])
    return mask, embeds.detach(), labels, feats.grad, emb.weight.grad


@pytest.mark.parametrize("name", BATCHES)
def test_twin_reproduces_the_reference_exactly(name):
    b = load_batch(name)
    mask, embeds, labels, d_feats, d_table = twin(b)
    assert embeds.dtype == torch.float64 and torch.equal(embeds, b["new_input_embeds"])
    assert labels.dtype == torch.int64 and torch.equal(labels, b["new_labels"])
    assert mask.dtype == torch.bool and torch.equal(mask, b["attention_mask_out"])
    assert torch.equal(d_feats, b["d_feats"]) and torch.equal(d_table, b["d_table"])


def test_the_golden_covers_what_it_claims():
    b = load_batch("ragged")
    ids, pad = b["ids"], b["padding_idx"]
    n_img = (ids == -200).sum(1).tolist()
    assert 0 in n_img and 2 in n_img and n_img.index(0) not in (len(n_img) - 1,)       # the skipped block is not the last
    text = ids[ids != -200]
    assert text.unique().numel() < text.numel() and pad in text and not bool(b["attention_mask"].all())
    assert bool((b["d_table"][pad] == 0).all()) and bool((b["table"][pad] != 0).any())
    skipped = sum(max(1, n) for n in n_img[:n_img.index(0)])
    assert bool((b["d_feats"][skipped] == 0).all()) and bool((b["d_feats"][skipped + 1] != 0).any())
    lens = {int(m.sum()) for m in b["attention_mask_out"]}
    assert len(lens) > 1                                                              # ragged: the padding branch
    e = load_batch("equal")
    assert bool(e["attention_mask_out"][1:].all()) and load_batch("one")["ids"].shape[0] == 1
    for name in BATCHES:                                  # every value is representable in bf16 and in fp16
        for k in ("feats", "table", "dout"):
            v = load_batch(name)[k]
            assert torch.equal(v.to(torch.bfloat16).double(), v) and torch.equal(v.half().double(), v)


def from_layout(lay, b, sep_id=None, ret_id=None):
    """inputs_embeds, labels, mask straight from a SpliceLayout's codes (float64, numpy indexing): what the kernel does."""
    kind, pay = torch.from_numpy(lay.kinds()), torch.from_numpy(lay.payloads())
    ids, D = b["ids"].reshape(-1), b["table"].shape[1]
    out = torch.zeros(lay.batch * lay.max_len, D, dtype=torch.float64)
    labels = torch.full((lay.batch * lay.max_len,), -100, dtype=torch.int64)
    t = kind == 0
    out[t] = b["table"][ids[pay[t]]]
    labels[t] = b["labels"].reshape(-1)[pay[t]]
    lit = kind == 1
    out[lit] = b["table"][torch.where(pay[lit] == splice.RET, ret_id or 0, sep_id or 0)]
    f = kind == 2
    out[f] = b["feats"].reshape(-1, D)[pay[f]]
    r = torch.arange(lay.max_len)[None, :] - (torch.from_numpy(lay.lengths).long()[:, None] - lay.in_len)
    given = b["attention_mask"].gather(1, r.clamp(0, lay.in_len - 1))
    mask = torch.where(r < 0, torch.ones_like(given), torch.where(r < lay.in_len, given, torch.zeros_like(given)))
    return out.view(lay.batch, lay.max_len, D), labels.view(lay.batch, lay.max_len), mask


@pytest.mark.parametrize("name", BATCHES)
def test_layout_reproduces_the_reference_exactly(name):
    b = load_batch(name)
    lay = splice.splice_layout(b["ids"], b["feats"].shape[1])
    assert lay.n_blocks == b["feats"].shape[0] and (lay.batch, lay.max_len) == tuple(b["new_labels"].shape)
    embeds, labels, mask = from_layout(lay, b)
    assert torch.equal(embeds, b["new_input_embeds"]) and torch.equal(labels, b["new_labels"])
    assert torch.equal(mask, b["attention_mask_out"])
    assert not bool((lay.kinds() == 1).any())                                         # no separator rows in the default mode


@pytest.mark.parametrize("name", ("ragged", "equal"))
def test_slice_mode_equals_the_hd_path_and_oracle(name):
    b = load_batch(name, HD_GOLDEN)
    kw = dict(mode="slice", h_block=b["hb"], w_block=b["wb"], sep_id=b["sep_id"], ret_id=b["ret_id"])
    mask, embeds, labels, d_feats, d_table = twin(b, **kw)
    M = b["feats"].shape[1]
    hd_mask, hd_labels = hd.splice_labels_and_mask(b["ids"], b["hb"], b["wb"], M, labels=b["labels"], attention_mask=b["attention_mask"])
    assert torch.equal(mask, hd_mask) and torch.equal(labels, hd_labels)
    want = hd_oracle.splice_inputs_embeds(b["ids"], lambda t: b["table"][t], b["feats"], b["hb"], b["wb"], b["sep_id"], b["ret_id"])
    assert torch.equal(embeds, want) and torch.equal(embeds, b["new_input_embeds"])
    assert torch.equal(labels, b["new_labels"]) and torch.equal(mask, b["attention_mask_out"])
    assert torch.equal(d_feats, b["d_feats"])
    assert float((d_table - b["d_table"]).abs().max()) <= 1e-12 * float(b["d_table"].abs().max())
    lay = splice.splice_layout(b["ids"], M, "slice", b["hb"], b["wb"])
    old = hd.splice_layout(b["ids"], b["hb"], b["wb"], M)
    assert lay.max_len == old[0] and lay.n_blocks == old[4]
    e2, l2, m2 = from_layout(lay, b, b["sep_id"], b["ret_id"])
    assert torch.equal(e2, want) and torch.equal(l2, hd_labels) and torch.equal(m2, hd_mask)


def test_layout_is_the_same_for_any_container_of_the_ids():
    b = load_batch("ragged")
    a = splice.splice_layout(b["ids"], 16)
    for other in (b["ids"].numpy(), b["ids"].to(torch.int32), b["ids"].t().contiguous().t()):
        o = splice.splice_layout(other, 16)
        assert o[:4] == a[:4] and np.array_equal(o.codes, a.codes) and np.array_equal(o.lengths, a.lengths) and o.n_blocks == a.n_blocks


# ---- 3. the Python refusals (all raised before any device work) --------------------------------------------------------------
def test_python_refusals():
    b = load_batch("one")
    feats, table, ids = b["feats"].to(torch.bfloat16), b["table"].to(torch.bfloat16), b["ids"]
    f = splice.build_multimodal_inputs
    with pytest.raises(TypeError, match="nn.Embedding"):
        f(ids, lambda t: table[t], feats)
    with pytest.raises(TypeError, match="max_norm"):
        f(ids, torch.nn.Embedding(24, 48, max_norm=1.0).to(torch.bfloat16), feats)
    with pytest.raises(TypeError, match="sparse"):
        f(ids, torch.nn.Embedding(24, 48, sparse=True).to(torch.bfloat16), feats)
    with pytest.raises(TypeError, match="contiguous"):
        f(ids, torch.zeros(48, 24, dtype=torch.bfloat16).t(), feats)
    with pytest.raises(TypeError, match="dtype"):
        f(ids, table.half(), feats)
    with pytest.raises(TypeError, match="bfloat16 or float16"):
        f(ids, table.float(), feats.float())
    with pytest.raises(RuntimeError, match="ZeRO-3"):
        emb = torch.nn.Embedding(24, 48).to(torch.bfloat16)
        emb.weight.data = torch.empty(0, dtype=torch.bfloat16)                       # what a partitioned parameter looks like
        f(ids, emb, feats)
    with pytest.raises(ValueError, match="outside the embedding table"):
        f(ids, table[:20], feats)                                                    # ids go up to 23
    with pytest.raises(ValueError, match="outside the embedding table"):
        f(torch.tensor([[1, -200, -3]]), table, feats)
    with pytest.raises(ValueError, match="feature blocks"):
        f(ids, table, torch.cat([feats, feats]))
    with pytest.raises(ValueError, match="feature blocks"):
        f(torch.tensor([[1, -200, 2, -200]]), table, feats)
    with pytest.raises(ValueError, match="sep_id"):
        f(ids, table, feats, mode="slice", h_block=[1], w_block=[1])
    with pytest.raises(ValueError, match="like input_ids"):
        f(ids, table, feats, labels=b["labels"][:, :-1])
    with pytest.raises(TypeError, match="attention_mask"):
        f(ids, table, feats, attention_mask=b["attention_mask"].float())
    r = load_batch("ragged")
    with pytest.raises(ValueError, match="need labels"):
        f(r["ids"], r["table"].half(), r["feats"].half(), attention_mask=r["attention_mask"])
    with pytest.raises(RuntimeError, match="no CPU fallback"):                       # valid arguments, but no device
        f(ids, table, feats)
