"""The one-launch token splice on a real MI355X: splice.build_multimodal_inputs (tp_splice / tp_splice_backward) in the default
mode against what the reference returned (tests/golden/splice_plain.npz) and in slice mode against hd.build_multimodal_inputs.

Embeds, feature gradients and the table-gradient rows of ids that occur once are copies, so they are compared bit for bit.
A table-gradient row of an id that occurs n > 1 times (',' and '\\n' of slice mode included) is an fp32 sum in a fixed order
rounded once, so it obeys the bound stated in tests/test_gpu_hd_train.py (splice_ref.check_sum restates the check_sum there):
    |got - S| <= 1/2 ulp_dtype(max(|S|, |got|)) + (n - 1) 2^-24 sum|t_i|,      S = the float64 sum of the t_i.
Nothing here reads the reference tree."""
import pytest
import torch

from tests import splice_ref
from tests.splice_ref import BATCHES, HD_GOLDEN, check_sum, load_batch
from tokenpacker_amd import hd, splice

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]


def gpu_inputs(b, dtype, table_grad=True, feats_grad=True, ids_on="cuda"):
    emb = torch.nn.Embedding.from_pretrained(b["table"].to(dtype), freeze=not table_grad, padding_idx=b.get("padding_idx")).cuda()
    feats = b["feats"].to(dtype).cuda().requires_grad_(feats_grad)
    kw = dict(labels=b["labels"].cuda(), attention_mask=b["attention_mask"].cuda())
    if "hb" in b:
        kw.update(mode="slice", h_block=b["hb"], w_block=b["wb"], sep_id=b["sep_id"], ret_id=b["ret_id"])
    return b["ids"].to(ids_on), emb, feats, kw


def table_terms(b, **kw):
    """Per table element, float64 on the CPU through the twin: (n readers, sum |t_i|)."""
    def grad(upstream):
        t = b["table"].clone().requires_grad_(True)
        _, e, _ = splice_ref.build_multimodal_inputs(b["ids"], lambda i: t[i], b["feats"], **kw)
        e.backward(upstream)
        return t.grad
    return grad(torch.ones_like(b["dout"])), grad(b["dout"].abs())


# ---- 1. forward ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", BATCHES)
def test_plain_mode_equals_the_reference_with_and_without_gradients(dtype, name):
    b = load_batch(name)
    ids, emb, feats, kw = gpu_inputs(b, dtype)
    mask, embeds, labels = splice.build_multimodal_inputs(ids, emb, feats, **kw)
    assert embeds.requires_grad and embeds.dtype == dtype
    with torch.no_grad():
        mask0, embeds0, labels0 = splice.build_multimodal_inputs(ids, emb, feats, **kw)
    assert not embeds0.requires_grad
    assert torch.equal(embeds.detach(), embeds0) and torch.equal(mask, mask0) and torch.equal(labels, labels0)
    assert torch.equal(embeds0.double().cpu(), b["new_input_embeds"])
    assert labels.dtype == torch.int64 and torch.equal(labels.cpu(), b["new_labels"])
    assert mask.dtype == torch.bool and torch.equal(mask.cpu(), b["attention_mask_out"])
    # an int64 mask comes back as int64; either output is None when its input is
    m64, _, lab64 = splice.build_multimodal_inputs(ids, emb.weight, feats, labels=kw["labels"],
                                                   attention_mask=kw["attention_mask"].long())
    assert m64.dtype == torch.int64 and torch.equal(m64.cpu(), b["attention_mask_out"].long())
    assert torch.equal(lab64.cpu(), b["new_labels"])
    none_mask, _, none = splice.build_multimodal_inputs(ids, emb.weight, feats)
    assert none is None and none_mask is None


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["ragged", "equal"])
def test_slice_mode_equals_the_hd_path(dtype, name):
    b = load_batch(name, HD_GOLDEN)
    ids, emb, feats, kw = gpu_inputs(b, dtype)
    got = splice.build_multimodal_inputs(ids, emb, feats, **kw)
    want = hd.build_multimodal_inputs(ids, emb, feats, b["hb"], b["wb"], b["sep_id"], b["ret_id"], labels=kw["labels"],
                                      attention_mask=kw["attention_mask"])
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and torch.equal(g.detach(), w.detach())
    assert torch.equal(got[1].detach().double().cpu(), b["new_input_embeds"])


@pytest.mark.parametrize("name", BATCHES)
def test_ids_on_the_cpu_give_the_same_result(name):
    b = load_batch(name)
    outs = []
    for where in ("cuda", "cpu"):
        ids, emb, feats, kw = gpu_inputs(b, torch.bfloat16, ids_on=where)
        mask, embeds, labels = splice.build_multimodal_inputs(ids, emb, feats, **kw)
        embeds.backward(b["dout"].to(torch.bfloat16).cuda())
        outs.append((mask, embeds.detach(), labels, feats.grad, emb.weight.grad))
    for a, c in zip(*outs):
        assert torch.equal(a, c)


# ---- 2. gradients --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", BATCHES)
def test_plain_mode_gradients(dtype, name):
    b = load_batch(name)
    ids, emb, feats, kw = gpu_inputs(b, dtype)
    _, embeds, _ = splice.build_multimodal_inputs(ids, emb, feats, **kw)
    embeds.backward(b["dout"].to(dtype).cuda())
    torch.cuda.synchronize()
    assert feats.grad.dtype == dtype and torch.equal(feats.grad.double().cpu(), b["d_feats"])
    n_img = (b["ids"] == -200).sum(1).tolist()
    if 0 in n_img:                                              # the block an image-less sample consumes gets zero
        skipped = sum(max(1, n) for n in n_img[:n_img.index(0)])
        assert bool((feats.grad[skipped] == 0).all())
    got = emb.weight.grad
    assert got.dtype == dtype and got.shape == emb.weight.shape
    got = got.double().cpu()
    text = b["ids"][b["ids"] != -200]
    idv, counts = text.unique(return_counts=True)
    once = idv[(counts == 1) & (idv != b["padding_idx"])]
    assert once.numel() > 0 and torch.equal(got[once], b["d_table"][once]), "rows of ids that occur once are exact copies"
    assert bool((got[b["padding_idx"]] == 0).all()), "the padding_idx row is zero"
    unread = torch.ones(got.shape[0], dtype=torch.bool)
    unread[idv] = False
    assert bool((got[unread] == 0).all()), "rows no token reads are zero"
    n, abs_sum = table_terms(b)
    n[b["padding_idx"]] = 0
    abs_sum[b["padding_idx"]] = 0
    check_sum(got, b["d_table"], n, abs_sum, dtype, f"d_table {name} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["ragged", "equal"])
def test_slice_mode_gradients_with_separator_rows(dtype, name):
    b = load_batch(name, HD_GOLDEN)
    ids, emb, feats, kw = gpu_inputs(b, dtype)
    _, embeds, _ = splice.build_multimodal_inputs(ids, emb, feats, **kw)
    embeds.backward(b["dout"].to(dtype).cuda())
    torch.cuda.synchronize()
    assert torch.equal(feats.grad.double().cpu(), b["d_feats"])
    skw = {k: v for k, v in kw.items() if k not in ("labels", "attention_mask")}
    n, abs_sum = table_terms(b, **skw)
    assert float(n[b["sep_id"]].max()) > 1 and float(n[b["ret_id"]].max()) > 1
    got = emb.weight.grad.double().cpu()
    check_sum(got, b["d_table"], n, abs_sum, dtype, f"d_table slice {name} {dtype}")
    assert bool((got[n[:, 0] == 0] == 0).all())
    once = n[:, 0] == 1
    assert torch.equal(got[once], b["d_table"][once])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("scale", [1.0, 1e-3])
def test_heavily_repeated_ids_within_the_fp32_accumulation_bound(dtype, scale):
    M, D, V, B, L_in = 8, 256, 12, 4, 96                       # ~370 text tokens over 12 ids: n ~ 30 per table row
    g = torch.Generator().manual_seed(91 + int(scale * 1000))
    ids = torch.randint(0, V, (B, L_in), generator=g)
    ids[:, 5] = -200
    ids[2, 40] = -200
    feats = torch.randn(5, M, D, generator=g).to(dtype)
    table = torch.randn(V, D, generator=g).to(dtype)
    lay = splice.splice_layout(ids, M)
    dout = (torch.randn(B * lay.max_len, D, generator=g) * scale * (1 + 10 * torch.rand(B * lay.max_len, 1, generator=g))).to(dtype)
    t = table.cuda().requires_grad_(True)
    f = feats.cuda().requires_grad_(True)
    _, embeds, _ = splice.build_multimodal_inputs(ids, t, f)
    embeds.backward(dout.view(B, lay.max_len, D).cuda())
    kind, pay = torch.from_numpy(lay.kinds()), torch.from_numpy(lay.payloads())
    row_id = torch.full((B * lay.max_len,), -1, dtype=torch.int64)
    row_id[kind == 0] = ids.reshape(-1)[pay[kind == 0]]
    S, n, abs_sum = (torch.zeros(V, D, dtype=torch.float64) for _ in range(3))
    for v in range(V):
        rows = dout[row_id == v].double()
        S[v], n[v], abs_sum[v] = rows.sum(0), float(rows.shape[0]), rows.abs().sum(0)
    assert float(n.min()) >= 10
    check_sum(t.grad, S, n, abs_sum, dtype, f"d_table n~{int(n.mean())} {dtype} scale {scale}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_unmapped_crop_map_slots_get_zero(dtype):
    b = load_batch("ragged")
    n = b["feats"].shape[0]
    cmap = [5, 0, 3, 1][:n]                                     # logical block -> slot of a 7-slot buffer; 2, 4, 6 unmapped
    padded = torch.full((7,) + tuple(b["feats"].shape[1:]), float("nan"), dtype=torch.float64)
    padded[cmap] = b["feats"]
    ids, emb, _, kw = gpu_inputs(b, dtype)
    p = padded.to(dtype).cuda().requires_grad_(True)
    cm = torch.tensor(cmap, dtype=torch.int32, device="cuda")
    mask, embeds, labels = splice.build_multimodal_inputs(ids, emb, p, crop_map=cm, **kw)
    assert torch.equal(embeds.detach().double().cpu(), b["new_input_embeds"])
    embeds.backward(b["dout"].to(dtype).cuda())
    got = p.grad.double().cpu()
    assert torch.equal(got[cmap], b["d_feats"])
    assert bool((got[[2, 4, 6]] == 0).all()), "unmapped slots must get a zero gradient"
    dup = torch.tensor([0, 0, 1, 2], dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError, match="injective"):
        splice.build_multimodal_inputs(ids, emb, p, crop_map=dup, **kw)
    with torch.no_grad():                                       # inference reads a map as it is
        splice.build_multimodal_inputs(ids, emb, p, crop_map=dup, **kw)


@pytest.mark.parametrize("dtype", DTYPES)
def test_two_backwards_are_bit_identical(dtype):
    grads = []
    for _ in range(2):
        out = []
        for name, path in (("ragged", None), ("ragged", HD_GOLDEN)):
            b = load_batch(name, path) if path else load_batch(name)
            ids, emb, feats, kw = gpu_inputs(b, dtype)
            _, embeds, _ = splice.build_multimodal_inputs(ids, emb, feats, **kw)
            embeds.backward(b["dout"].to(dtype).cuda())
            torch.cuda.synchronize()
            out += [feats.grad.cpu(), emb.weight.grad.cpu()]
        grads.append(out)
    for a, c in zip(*grads):
        assert torch.equal(a.view(torch.int16), c.view(torch.int16)), "two runs must give identical bits"


def test_a_frozen_table_launches_no_table_gradient_kernel():
    b = load_batch("ragged")
    ids, emb, feats, kw = gpu_inputs(b, torch.bfloat16, table_grad=False)
    _, embeds, _ = splice.build_multimodal_inputs(ids, emb, feats, **kw)
    node = embeds.grad_fn.next_functions[0][0]                  # the view's input: the splice node
    assert tuple(node.needs_input_grad[:2]) == (True, False)
    assert node.spec.args.n_table_rows == 0 and not node.spec.args.order_dev      # no sort, no order buffer either
    dfeats, dtable, _ = splice._SpliceFn.backward(node, b["dout"].to(torch.bfloat16).cuda().view(-1, b["dout"].shape[-1]))
    assert dtable is None and torch.equal(dfeats.double().cpu(), b["d_feats"])
    embeds.backward(b["dout"].to(torch.bfloat16).cuda())
    assert emb.weight.grad is None and torch.equal(feats.grad.double().cpu(), b["d_feats"])
    # ... and the other way round: only the table is trainable
    ids, emb, feats, kw = gpu_inputs(b, torch.bfloat16, feats_grad=False)
    _, embeds, _ = splice.build_multimodal_inputs(ids, emb, feats, **kw)
    embeds.backward(b["dout"].to(torch.bfloat16).cuda())
    assert feats.grad is None and emb.weight.grad is not None


# ---- 3. the full shape ---------------------------------------------------------------------------------------------------
def test_full_shape_matches_the_twin_on_a_sample_of_rows():
    B, M, D, V, L_in, dtype = 32, 144, 4096, 32000, 64, torch.bfloat16
    g = torch.Generator().manual_seed(2024)
    ids = torch.randint(1, V, (B, L_in), generator=g)
    ids[:, :8] = torch.randint(1, 40, (B, 8), generator=g)      # a few ids repeat across the batch
    for s in range(B):
        if s != 7:                                              # sample 7 has no image
            ids[s, int(torch.randint(1, L_in - 1, (1,), generator=g))] = -200
    ids[3, 50], ids[3, 51] = -200, 0                            # two images; an id equal to padding_idx = 0
    labels = torch.randint(0, V, (B, L_in), generator=g)
    mask = torch.rand(B, L_in, generator=g) > 0.1
    dg = torch.Generator(device="cuda").manual_seed(5)
    table = torch.randn(V, D, generator=dg, device="cuda").to(dtype)
    n_img = (ids == -200).sum(1)
    n_blocks = int(n_img.clamp(min=1).sum())                    # an image-less sample consumes one
    skipped = int(n_img[:7].clamp(min=1).sum())
    feats = torch.randn(n_blocks, M, D, generator=dg, device="cuda").to(dtype)
    emb = torch.nn.Embedding.from_pretrained(table, freeze=False, padding_idx=0)
    f = feats.clone().requires_grad_(True)
    got_mask, embeds, got_labels = splice.build_multimodal_inputs(ids.cuda(), emb, f, labels.cuda(), mask.cuda())
    L = embeds.shape[1]
    dout = torch.randn(B, L, D, generator=dg, device="cuda").to(dtype)
    embeds.backward(dout)
    torch.cuda.synchronize()
    # the twin on the CPU in the same dtype (copies only), all labels and mask, a sample of embeds rows
    table_c, feats_c = table.cpu(), feats.cpu()
    want_mask, want, want_labels = splice_ref.build_multimodal_inputs(ids, lambda t: table_c[t], feats_c, labels, mask)
    assert tuple(embeds.shape) == tuple(want.shape) and L == L_in + int(n_img.max()) * (M - 1)
    assert torch.equal(got_labels.cpu(), want_labels) and torch.equal(got_mask.cpu(), want_mask)
    rows = torch.randint(0, B * L, (4000,), generator=g)
    assert torch.equal(embeds.detach().view(B * L, D)[rows.cuda()].cpu(), want.view(B * L, D)[rows])
    assert torch.equal(embeds.detach()[7].cpu(), want[7]) and torch.equal(embeds.detach()[3].cpu(), want[3])
    # gradients from the layout (pinned to the reference by tests/test_splice_cpu.py)
    lay = splice.splice_layout(ids, M)
    kind, pay = torch.from_numpy(lay.kinds()), torch.from_numpy(lay.payloads())
    dflat = dout.view(B * L, D).cpu()
    want_df = torch.zeros(n_blocks, M, D, dtype=dtype).view(-1, D)
    want_df[pay[kind == 2]] = dflat[kind == 2]
    assert torch.equal(f.grad.cpu().view(-1, D), want_df) and bool((f.grad[skipped] == 0).all())
    row_id = torch.full((B * L,), -1, dtype=torch.int64)
    row_id[kind == 0] = ids.reshape(-1)[pay[kind == 0]]
    dt = emb.weight.grad
    assert dt.shape == (V, D) and dt.dtype == dtype and bool((dt[0] == 0).all())
    idv, counts = row_id[row_id > 0].unique(return_counts=True)
    unread = torch.ones(V, dtype=torch.bool)
    unread[idv] = False
    assert bool((dt[unread.cuda()] == 0).all())
    pick = torch.cat([idv[counts > 1][:48], idv[counts == 1][:48]])
    S, n, abs_sum = (torch.zeros(pick.numel(), D, dtype=torch.float64) for _ in range(3))
    for i, v in enumerate(pick.tolist()):
        r = dflat[row_id == v].double()
        S[i], n[i], abs_sum[i] = r.sum(0), float(r.shape[0]), r.abs().sum(0)
    assert float(n.max()) > 1
    check_sum(dt[pick.cuda()], S, n, abs_sum, dtype, "d_table full shape")
    single = (n[:, 0] == 1)
    assert torch.equal(dt[pick.cuda()].double().cpu()[single], S[single])
