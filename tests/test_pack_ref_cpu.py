"""tests/pack_ref.py is anchored to the ALGORITHM (the oracle's layer-by-layer values), not to the kernels' comments, and its gates are
shown — without a GPU — to be passable by a correct implementation and sensitive to every named mistake: `emulate` (the recipe of
tp_pack_weights in torch fp32 / fp16) passes each gate of tests/test_gpu_pack_image.py with 2x headroom, every twin fails the gate it
is assigned to.  Both dtypes, both parameter sets; `-s` prints the table."""
import math

import pytest
import torch

from oracle import tokenpacker_oracle as orc
from tests import pack_ref as pr

E = pr.E
SEED = 9100
CASES = [(dt, kind) for dt in pr.DTYPES for kind in pr.SETS]
_ID = lambda c: f"{str(c[0]).split('.')[-1]}-{c[1]}"


def _close(got, want, what):
    err = float((got - want).abs().max())
    assert err <= 1e-10 * max(1.0, float(want.abs().max())), (what, err)


@pytest.mark.parametrize("case", [(torch.bfloat16, "offset"), (torch.float16, "plain")], ids=_ID)
def test_reference_forms_equal_the_oracle_layer_by_layer(case):
    """On a handful of random rows, in fp64: the LN fold, the plain chain, the centred chain, the triangular variance and
    out_proj o mlp[0], each evaluated from pack_ref's tensors, against oracle.linear / oracle.layer_norm applied layer by layer."""
    dtype, kind = case
    p = pr.make_param_set(kind, SEED, dtype)
    ref = pr.reference(p, kind)
    P = {k: v.double() for k, v in p.items()}
    gen = torch.Generator().manual_seed(SEED + 1)
    inw, inb = P["clip_attn.in_proj_weight"], P["clip_attn.in_proj_bias"]
    rows = {"q": slice(0, E), "k": slice(E, 2 * E), "v": slice(2 * E, 3 * E)}
    for m in pr.MATS:
        g = {"k": 0, "v": 1, "q": None}[m]
        sfx = "q" if m == "q" else "kv"
        gamma, beta = P[f"ln_{m}_1.weight"], P[f"ln_{m}_1.bias"]
        W, b = inw[rows[m]], inb[rows[m]]
        A, W2, b2 = ref.tri[m]
        hi = pr._pick(ref.bits["w_in_" + sfx], g).double()
        c, bp = ref.vec["c_in_" + sfx, g].want, ref.vec["b_in_" + sfx, g].want
        h = torch.randn(5, E, generator=gen, dtype=torch.float64) * 1.5       # rows of the layer in front (Hkv / q0)
        H2 = orc.linear(h, W2, b2 if m != "q" else None)
        mu = H2.mean(-1, keepdim=True)
        var = ((H2 - mu) ** 2).mean(-1, keepdim=True)
        rstd = 1.0 / torch.sqrt(var + orc.EPS)
        # what the ROUNDED fold computes: the LayerNorm without its shift into the weight hi / gamma, plus beta W^T + b (W unrounded)
        want_rounded = orc.linear(orc.layer_norm(H2, gamma, torch.zeros_like(beta)), hi / gamma) + orc.linear(beta[None], W, b)
        _close(rstd * (H2 @ hi.t() - mu * c) + bp, want_rounded, f"LN fold, {m}")
        d_in = ref.vec["d_in_kv", g].want if m != "q" else 0.0
        _close(rstd * (h @ ref.prod["w_c_" + sfx, g].exact.t() + d_in - mu * c) + bp, want_rounded, f"plain chain, {m}")
        # the centred chain is built from the EXACT fold: it is the reference's own layer pair
        d_cc = ref.vec["d_cc_kv", g].want if m != "q" else 0.0
        _close(rstd * (h @ ref.prod["w_cc_" + sfx, g].exact.t() + d_cc) + bp,
               orc.linear(orc.layer_norm(H2, gamma, beta), W, b), f"centred chain, {m}")
        h1 = torch.cat([h, torch.ones(5, 1, dtype=torch.float64)], 1)
        _close(((h1 @ A.t()) ** 2).sum(-1, keepdim=True) / E, var, f"triangular variance, {m}")
    o = torch.randn(5, E, generator=gen, dtype=torch.float64)
    # (the image keeps f16(parameter): a bf16 weight below fp16's normal range loses bits there, so the layers are fed those)
    want = orc.linear(orc.linear(o, ref.bits["w_out"].double(), P["clip_attn.out_proj.bias"]), ref.bits["w_m0"].double(), P["mlp.0.bias"])
    _close(o @ ref.prod["w_om", None].exact.t() + ref.vec["b_om", None].want, want, "out_proj o mlp[0]")


def _headroom_ok(row, floor=0.0):
    """2x headroom: the value uses at most half of the gate — for a product's F, half of the room above F(f16(exact)), the figure
    no implementation can be below."""
    _, _, value, gate = row
    return value - floor <= 0.5 * (gate - floor)


@pytest.mark.parametrize("case", CASES, ids=_ID)
def test_emulation_passes_every_gate_and_every_twin_fails_its_own(case):
    dtype, kind = case
    p = pr.make_param_set(kind, SEED, dtype)
    ref = pr.reference(p, kind)
    img = pr.emulate(p)
    print(f"\n[pack-ref] {_ID(case)}: the fp32 / fp16 emulation")
    for name, want in ref.bits.items():
        assert img[name].dtype == want.dtype and torch.equal(img[name].view(torch.int16 if want.element_size() == 2 else torch.int32),
                                                             want.view(torch.int16 if want.element_size() == 2 else torch.int32)), name
    groups = pr.gated_fields(ref)
    for group, fields in groups.items():
        for field, g in fields:
            rows = pr.field_rows(img, ref, field, g)
            print(pr.format_rows(rows))
            floor = pr.product_floor(ref.prod[field, g]) if group == "products" else 0.0
            for row in rows:
                assert _headroom_ok(row, floor if row[1] == "metric" else 0.0), row
    print(f"[pack-ref] {_ID(case)}: the twins (value of the gate each is assigned to)")
    for (field, g), prod in ref.prod.items():
        for name, ratio in pr.twin_separation(prod):
            assert ratio >= pr.GATE_TWIN_PRODUCT, (field, g, name, ratio)
    n_twins = 0
    for group in ("vectors", "products", "pair"):
        for field, g in groups[group]:
            holder = ref.prod["w_cc_kv", 1] if group == "pair" else (ref.vec if group == "vectors" else ref.prod)[field, g]
            for twin in holder.twins:
                metric = [r for r in pr.field_rows(pr.with_twin(img, ref, field, g, twin), ref, field, g) if r[1] == "metric"]
                print(pr.format_rows([(f"{metric[0][0]} <- {twin}",) + metric[0][1:]]))
                assert pr.failures(metric), (field, g, twin, metric)
                n_twins += 1
    assert n_twins == (43 if kind == "offset" else 37)       # every assignment of pack_ref's table was tried (rounded-c: offset only)
    # the head transposes and the pair layout invert each other the way the image is read
    hi, lo = pr.pair_tiles(img["w_cc_v3"])
    assert torch.equal(hi, img["w_cc_kv"][1]) and torch.equal(pr.head_transpose(img["w_in_kv"][0]), img["w_qt"])
    assert img["w_qt"][3, 5, 7] == img["w_in_kv"][0][3 * 128 + 7, 5] and img["w_cc_v3"][9, 2 * 64 + 5] == img["w_cc_kv"][1][9, 64 + 5]
    assert not math.isnan(float(lo.float().abs().max()))
