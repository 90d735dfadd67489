"""Training through the HD token splice on a real MI355X: hd.assemble_hd_tokens / build_inputs_embeds / build_multimodal_inputs
with gradients live, whose backward is tp_hd_assemble_backward.

Every gradient row of the features and of the text embeddings is a copy of an incoming row, so it is checked bit for bit
against CPU autograd of the oracle (oracle/hd_oracle.py, pinned to the reference by tests/test_hd_train_cpu.py).  The ',' and
'\\n' gradients are sums of n incoming rows t_i, accumulated in fp32 and rounded once, so for every element
    |got - S| <= 1/2 ulp_dtype(max(|S|, |got|)) + (n - 1) 2^-24 sum|t_i|,      S = the float64 sum of the t_i."""
import hashlib
import os

import numpy as np
import pytest
import torch

from oracle import hd_oracle
from tokenpacker_amd import TokenPacker, hd, synth

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "hd_splice_train.npz")


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


def half_ulp(x: torch.Tensor, dtype) -> torch.Tensor:
    """1/2 ulp of |x| (float64) in `dtype` (p = 8 significant bits for bf16, 11 for fp16; subnormal floor)."""
    p, tiny = {torch.bfloat16: (8, 2.0 ** -133), torch.float16: (11, 2.0 ** -24)}[dtype]
    _, e = torch.frexp(x.abs())
    return torch.clamp(torch.ldexp(torch.ones_like(x), e - p), min=tiny) / 2


def check_sum(got, S, n, abs_sum, dtype, what, extra_half_ulps=0):
    """The fp32-accumulation bound of the module docstring, element by element (float64 CPU tensors)."""
    got = got.detach().double().cpu()
    mag = torch.maximum(S.abs(), got.abs())
    bound = (1 + extra_half_ulps) * half_ulp(mag, dtype) + (n - 1).clamp(min=0) * 2.0 ** -24 * abs_sum
    err = (got - S).abs()
    print(f"{what}: max|got - S| {float(err.max()):.3e}, worst err/bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all()), f"{what}: {int((err > bound).sum())} elements out of bound"


def rand(g, *shape, dtype):
    return torch.randn(*shape, generator=g).to(dtype)


def leaves(dtype, *ts):
    return [t.to(dtype).cuda().requires_grad_(True) for t in ts]


# ---- 1. forward values ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["ragged", "equal"])
def test_forward_values_with_gradients_live_equal_no_grad_and_the_reference(dtype, name):
    b = load_batch(name)
    emb = torch.nn.Embedding.from_pretrained(b["table"].to(dtype), freeze=False).cuda()
    feats = b["feats"].to(dtype).cuda().requires_grad_(True)
    args = (b["ids"].cuda(), emb, feats, b["hb"], b["wb"], b["sep_id"], b["ret_id"])
    kw = dict(labels=b["labels"].cuda(), attention_mask=b["attention_mask"].cuda())
    mask, embeds, labels = hd.build_multimodal_inputs(*args, **kw)
    assert embeds.requires_grad
    with torch.no_grad():
        mask0, embeds0, labels0 = hd.build_multimodal_inputs(*args, **kw)
        plain = hd.build_inputs_embeds(*args)
    assert not embeds0.requires_grad
    assert torch.equal(embeds.detach(), embeds0) and torch.equal(embeds0, plain)
    assert torch.equal(mask, mask0) and torch.equal(labels, labels0)
    assert torch.equal(embeds0.double().cpu(), b["new_input_embeds"])
    assert torch.equal(labels.cpu(), b["new_labels"]) and torch.equal(mask.cpu(), b["attention_mask_out"])


# ---- 2. copies are bit-exact ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["ragged", "equal"])
def test_feature_and_text_gradients_are_exact_copies(dtype, name):
    b = load_batch(name)
    ids = b["ids"]
    text = ids[ids != -200]
    assert text.unique().numel() == text.numel() and b["sep_id"] not in text and b["ret_id"] not in text   # no id repeats
    feats, table = leaves(dtype, b["feats"], b["table"])
    embeds = hd.build_inputs_embeds(ids.cuda(), lambda t: table[t], feats, b["hb"], b["wb"], b["sep_id"], b["ret_id"])
    embeds.backward(b["dout"].to(dtype).cuda())
    torch.cuda.synchronize()
    f64, t64 = b["feats"].clone().requires_grad_(True), b["table"].clone().requires_grad_(True)
    want = hd_oracle.splice_inputs_embeds(ids, lambda t: t64[t], f64, b["hb"], b["wb"], b["sep_id"], b["ret_id"])
    want.backward(b["dout"])
    assert feats.grad.dtype == dtype and torch.equal(feats.grad.double().cpu(), f64.grad)
    assert torch.equal(feats.grad.double().cpu(), b["d_feats"])
    rows = text.unique()
    assert torch.equal(table.grad[rows.cuda()].double().cpu(), t64.grad[rows])
    if name == "ragged":                            # sample 2 has no image: the crop index it consumes gets zero
        first = sum(hd.hd_crop_count(h, w) * int((r == -200).sum()) for r, h, w in zip(ids[:2], b["hb"][:2], b["wb"][:2]))
        assert int((ids[2] == -200).sum()) == 0 and bool((feats.grad[first] == 0).all())


@pytest.mark.parametrize("dtype", DTYPES)
def test_padding_slots_of_a_crop_map_get_zero(dtype):
    M, D = 16, 64
    g = torch.Generator().manual_seed(21)
    grids = [(2, 2), (1, 1), (1, 3)]
    hb, wb = [h for h, _ in grids], [w for _, w in grids]
    n_crops = sum(hd.hd_crop_count(h, w) for h, w in grids)               # 10 crops over 2 "ranks" of b_max = 6
    feats = rand(g, n_crops, M, D, dtype=dtype)
    sep, ret = rand(g, D, dtype=dtype), rand(g, D, dtype=dtype)
    cmap = list(range(6)) + [6 + j for j in range(4)]
    padded = torch.full((12, M, D), float("nan")).to(dtype)
    padded[cmap] = feats
    rows = sum(hd.hd_token_rows(h, w, M) for h, w in grids)
    dout = rand(g, rows, D, dtype=dtype)
    p, s, r = leaves(dtype, padded, sep, ret)
    views = hd.assemble_hd_tokens(p, hb, wb, s, r, crop_map=torch.tensor(cmap, dtype=torch.int32, device="cuda"))
    torch.cat(views).backward(dout.cuda())
    f64 = feats.double().requires_grad_(True)
    torch.cat(hd_oracle.assemble_hd_tokens(f64, hb, wb, sep.double(), ret.double())).backward(dout.double())
    got = p.grad.double().cpu()
    assert torch.equal(got[cmap], f64.grad)
    assert bool((got[[10, 11]] == 0).all()), "unmapped padding slots must get a zero gradient"


# ---- 3. separator sums ---------------------------------------------------------------------------------------------------
def sep_terms(dout, hb, wb, starts, M):
    """The incoming rows summed into dsep / dret (float64 [n, D] each)."""
    sep, ret = [], []
    for st, h, w in zip(starts, hb, wb):
        n = h * w
        for s in range(n):
            (ret if s % w == w - 1 else sep).append(dout[st + s * (M + 1) + M])
        if n > 1:
            ret.append(dout[st + n * (M + 1) + M])
    return torch.stack(sep).double(), torch.stack(ret).double()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("scale", [1.0, 1e-3])
def test_separator_sums_within_the_fp32_accumulation_bound(dtype, scale):
    M, D = 16, 256
    g = torch.Generator().manual_seed(31 + int(scale * 1000))
    grids = [(3, 3)] * 12 + [(2, 3), (1, 9), (9, 1), (1, 1)] * 3          # n(',') = 12*6 + 3*(3+8) = 105, n('\n') >= 50
    hb, wb = [h for h, _ in grids], [w for _, w in grids]
    n_crops = sum(hd.hd_crop_count(h, w) for h, w in grids)
    feats, sep, ret = rand(g, n_crops, M, D, dtype=dtype), rand(g, D, dtype=dtype), rand(g, D, dtype=dtype)
    rows = sum(hd.hd_token_rows(h, w, M) for h, w in grids)
    dout = (torch.randn(rows, D, generator=g) * scale * (1 + 10 * torch.rand(rows, 1, generator=g))).to(dtype)
    f, s, r = leaves(dtype, feats, sep, ret)
    views = hd.assemble_hd_tokens(f, hb, wb, s, r)
    torch.cat(views).backward(dout.cuda())
    starts = np.cumsum([0] + [hd.hd_token_rows(h, w, M) for h, w in grids])[:-1]
    ts, tr = sep_terms(dout, hb, wb, starts, M)
    assert ts.shape[0] >= 50 and tr.shape[0] >= 50
    for got, t, what in ((s.grad, ts, "dsep"), (r.grad, tr, "dret")):
        assert got.dtype == dtype
        check_sum(got, t.sum(0), torch.full((D,), float(t.shape[0]), dtype=torch.float64), t.abs().sum(0), dtype,
                  f"{what} n={t.shape[0]} {dtype}")


# ---- 4. through nn.Embedding ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["ragged", "equal"])
def test_build_multimodal_inputs_through_an_embedding_table(dtype, name):
    b = load_batch(name)
    emb = torch.nn.Embedding.from_pretrained(b["table"].to(dtype), freeze=False).cuda()
    feats = b["feats"].to(dtype).cuda().requires_grad_(True)
    mask, embeds, labels = hd.build_multimodal_inputs(b["ids"].cuda(), emb, feats, b["hb"], b["wb"], b["sep_id"], b["ret_id"],
                                                      labels=b["labels"].cuda(), attention_mask=b["attention_mask"].cuda())
    assert torch.equal(embeds.detach().double().cpu(), b["new_input_embeds"])
    assert torch.equal(labels.cpu(), b["new_labels"]) and torch.equal(mask.cpu(), b["attention_mask_out"])
    embeds.backward(b["dout"].to(dtype).cuda())
    torch.cuda.synchronize()
    assert torch.equal(feats.grad.double().cpu(), b["d_feats"])
    # per table element: n = the number of rows landing on it, sum|t| = the same gradient of |dout| (float64 oracle)
    def oracle_table_grad(upstream):
        t64 = b["table"].clone().requires_grad_(True)
        out = hd_oracle.splice_inputs_embeds(b["ids"], lambda t: t64[t], b["feats"], b["hb"], b["wb"], b["sep_id"], b["ret_id"])
        out.backward(upstream)
        return t64.grad
    n = oracle_table_grad(torch.ones_like(b["dout"]))
    abs_sum = oracle_table_grad(b["dout"].abs())
    check_sum(emb.weight.grad, b["d_table"], n, abs_sum, dtype, f"d_table {name} {dtype}", extra_half_ulps=1)
    # report, no gate: the reference-style loop (one embedding call per piece) on the GPU, same inputs
    emb2 = torch.nn.Embedding.from_pretrained(b["table"].to(dtype), freeze=False).cuda()
    loop = hd_oracle.splice_inputs_embeds(b["ids"].cuda(), lambda t: emb2(t.cuda()), b["feats"].to(dtype).cuda(), b["hb"],
                                          b["wb"], b["sep_id"], b["ret_id"])
    loop.backward(b["dout"].to(dtype).cuda())
    ours = float((emb.weight.grad.double().cpu() - b["d_table"]).abs().max())
    theirs = float((emb2.weight.grad.double().cpu() - b["d_table"]).abs().max())
    print(f"d_table max-norm distance from float64 ({name}, {dtype}): splice {ours:.3e}, reference-style loop {theirs:.3e}")


# ---- 5. out= semantics ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_out_behaves_like_in_place_slice_assignment(dtype):
    M, D = 8, 64
    g = torch.Generator().manual_seed(51)
    grids = [(2, 2), (1, 1), (1, 3)]
    hb, wb = [h for h, _ in grids], [w for _, w in grids]
    n_crops = sum(hd.hd_crop_count(h, w) for h, w in grids)
    rows = [hd.hd_token_rows(h, w, M) for h, w in grids]
    starts = [3, 3 + rows[0] + 7, 3 + rows[0] + 7 + rows[1] + 1]
    total = starts[-1] + rows[-1] + 5
    feats, sep, ret = rand(g, n_crops, M, D, dtype=dtype), rand(g, D, dtype=dtype), rand(g, D, dtype=dtype)
    base, w = rand(g, total, D, dtype=dtype), rand(g, total, D, dtype=dtype)
    f, s, r, b0 = leaves(dtype, feats, sep, ret, base)
    out = b0.clone()
    views = hd.assemble_hd_tokens(f, hb, wb, s, r, out=out, out_rows=starts)
    assert all(v.data_ptr() == out[st].data_ptr() for v, st in zip(views, starts))
    out.backward(w.cuda())
    # torch: out[block rows] = block under autograd, float64 on the CPU
    f2, s2, r2, b2 = (t.double().requires_grad_(True) for t in (feats, sep, ret, base))
    out2 = b2.clone()
    for st, blk in zip(starts, hd_oracle.assemble_hd_tokens(f2, hb, wb, s2, r2)):
        out2[st:st + blk.shape[0]] = blk
    out2.backward(w.double())
    assert torch.equal(out.detach().double().cpu(), out2.detach())
    assert torch.equal(b0.grad.double().cpu(), b2.grad), "the buffer's earlier content gets dout with the block rows zeroed"
    assert torch.equal(f.grad.double().cpu(), f2.grad)
    ts, tr = sep_terms(w, hb, wb, starts, M)
    for got, t, what in ((s.grad, ts, "dsep"), (r.grad, tr, "dret")):
        check_sum(got, t.sum(0), torch.full((D,), float(t.shape[0]), dtype=torch.float64), t.abs().sum(0), dtype, what)
    leaf = base.cuda().requires_grad_(True)
    with pytest.raises(RuntimeError):
        hd.assemble_hd_tokens(f, hb, wb, s, r, out=leaf, out_rows=starts)


# ---- 6. batches and refusals ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_more_than_64_images_and_two_runs_identical(dtype):
    M, D = 8, 128
    g = torch.Generator().manual_seed(61)
    grids = [(1, 1)] * 40 + [(2, 2)] * 20 + [(3, 3)] * 10
    hb, wb = [h for h, _ in grids], [w for _, w in grids]
    n_crops = sum(hd.hd_crop_count(h, w) for h, w in grids)
    feats, sep, ret = rand(g, n_crops, M, D, dtype=dtype), rand(g, D, dtype=dtype), rand(g, D, dtype=dtype)
    rows = sum(hd.hd_token_rows(h, w, M) for h, w in grids)
    dout = rand(g, rows, D, dtype=dtype)
    grads = []
    for _ in range(2):
        f, s, r = leaves(dtype, feats, sep, ret)
        torch.cat(hd.assemble_hd_tokens(f, hb, wb, s, r)).backward(dout.cuda())
        torch.cuda.synchronize()
        grads.append((f.grad.cpu(), s.grad.cpu(), r.grad.cpu()))
    for a, b in zip(*grads):
        assert torch.equal(a.view(torch.int16), b.view(torch.int16)), "two runs must give identical bits"
    f64 = feats.double().requires_grad_(True)
    torch.cat(hd_oracle.assemble_hd_tokens(f64, hb, wb, sep.double(), ret.double())).backward(dout.double())
    assert torch.equal(grads[0][0].double(), f64.grad)
    starts = np.cumsum([0] + [hd.hd_token_rows(h, w, M) for h, w in grids])[:-1]
    ts, tr = sep_terms(dout, hb, wb, starts, M)
    for got, t, what in ((grads[0][1], ts, "dsep"), (grads[0][2], tr, "dret")):
        check_sum(got, t.sum(0), torch.full((D,), float(t.shape[0]), dtype=torch.float64), t.abs().sum(0), dtype,
                  f"{what} over {len(grids)} images")


def test_duplicate_crop_map_under_grad_raises():
    M, D = 4, 32
    feats = torch.randn(3, M, D, device="cuda").to(torch.bfloat16).requires_grad_(True)
    e = torch.randn(D, device="cuda").to(torch.bfloat16)
    dup = torch.tensor([0, 0], dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError, match="injective"):
        hd.assemble_hd_tokens(feats, [1, 1], [1, 1], e, e, crop_map=dup)
    with torch.no_grad():                          # inference reads a map as it is
        hd.assemble_hd_tokens(feats, [1, 1], [1, 1], e, e, crop_map=dup)


# ---- 7. projector end to end ---------------------------------------------------------------------------------------------
def test_projector_gradients_match_the_loop_splice_bit_for_bit():
    """TokenPacker (hidden 256, bf16) training forward on HD crops -> splice -> seeded loss -> backward.  Both splices hand the
    projector the same dL/dfeatures (copies), so its 23 parameter gradients must be identical."""
    dtype, D = torch.bfloat16, 256
    params = synth.make_params(71, D)
    grids = [(2, 2), (1, 1), None, (1, 3)]                          # sample 2 has no image: it consumes one crop
    ids = torch.tensor([[1, 2, -200, 3, 4], [5, -200, 6, -200, 8], [9, 10, 12, 13, 14], [-200, 15, 16, 17, 18]])
    hb = [g[0] if g else 1 for g in grids]
    wb = [g[1] if g else 1 for g in grids]
    n_crops = sum(int((r == -200).sum()) * hd.hd_crop_count(h, w) or 1 for r, h, w in zip(ids, hb, wb))   # 5 + 2 + 1 + 4
    x, xm = synth.make_inputs(72, n_crops)
    g = torch.Generator().manual_seed(73)
    table = torch.randn(40, D, generator=g).to(dtype).cuda()

    def step(splice):
        m = TokenPacker(hidden_size=D)
        m.load_state_dict(params)
        m = m.to(device="cuda", dtype=dtype).train()
        feats = m((x.to(dtype).cuda(), xm.to(dtype).cuda()))
        emb = torch.nn.Embedding.from_pretrained(table.clone(), freeze=False)
        embeds = splice(feats, emb)
        w = torch.randn(embeds.shape, generator=torch.Generator().manual_seed(74)).cuda()
        (embeds.float() * w).sum().backward()
        torch.cuda.synchronize()
        return {k: p.grad.detach().clone() for k, p in m.named_parameters()}

    ours = step(lambda f, emb: hd.build_multimodal_inputs(ids.cuda(), emb, f, hb, wb, 7, 11)[1])
    loop = step(lambda f, emb: hd_oracle.splice_inputs_embeds(ids.cuda(), lambda t: emb(t.cuda()), f, hb, wb, 7, 11))
    assert len(ours) == 23 and ours.keys() == loop.keys()
    for k in ours:
        assert torch.equal(ours[k].view(torch.int16), loop[k].view(torch.int16)), k
