"""fp64 reference of the packed-weight image (tp_pack_weights, tokenpacker_amd/csrc/tp_api.hip), tensor by tensor and by
PackedLayout field name, with the WRONG recipes each tensor is told apart from ("twins") and the gates of
tests/test_gpu_pack_image.py.  Plain torch on whatever device the parameters are sent to; nothing here calls a kernel.

Conventions
  * f16(.) is round-to-nearest-even to fp16 after a clamp to +-65504 (the pack kernels saturate instead of producing inf);
  * the raw parameters are first rounded to the model dtype, as projector.py hands them to the library;
  * in_proj rows are q | k | v; every K / V pair of the image is ordered k, v; the per-matrix index m is k, v, q;
  * W' = W diag(gamma) is the LayerNorm fold.  It is EXACT in fp32 (two 16-bit floats); `hi` = f16(W') is what the image keeps
    as w_in_*, `lo` = f16(W' - hi) what the rounding dropped.  "rounded W'" is hi, "exact W'" the unrounded product.

What the image should hold
  exact-bit   w_kv0 (raw bits), b_* (fp32 widenings), w_kv2 / w_q1 / w_out / w_m0 / w_m2 = f16(parameter), w_in_* = f16(W');
              w_qt / w_qt_c / w_qt_cc and the hi K-tiles of w_cc_v3 are re-laid-out copies of OTHER IMAGE tensors and are
              compared with those (`head_transpose`, `pair_tiles`), w_r_* is exactly zero below the diagonal
  fp32 vectors    c_in = rowsum(ROUNDED W'), b_in = W beta + b (W unrounded), d_in_kv = ROUNDED W' b2,
                  d_cc_kv = EXACT W' (b2 - mean b2), b_om = f16(Wm0) b_out + b_m0
  rounded once    w_c = ROUNDED W' W2, w_cc = EXACT W' W2c (W2c: f16(W2) centred over its output index), w_om = f16(Wm0) f16(Wout)
  the V pair      hi + lo of w_cc_v3 is w_cc of the V side nearly unrounded
  triangular      T_m = [R_m | c~_m] with T^T T = A^T A, A_m = [W2c | b2c] (b2c = 0 for q)

Twins (the mistakes the end-to-end parity gate cannot see; each is assigned to the tensor it would spoil)
  hi-only       the lo product dropped: hi W2 - c_exact (x) wbar                       w_cc_*, d_cc_kv, the V pair
  rounded-c     c of the ROUNDED W' inside Wcc / dcc (offset set only: on the plain    w_cc_*, d_cc_kv, the V pair
                set wbar is too small for it to register)
  uncentred     no - c (x) wbar                                                        w_cc_*, d_cc_kv, the V pair
  exact-fold    the PLAIN chain from the unrounded W' (wrong there: the mean term      w_c_*
                must cancel against c = rowsum(rounded W'))
  exact-rowsum  c_in from the unrounded W'                                             c_in_*
  rounded-W     b_in from the W the rounded fold implies, hi / gamma.  (A parameter    b_in_*
                already is a 16-bit value: rounding W itself once more is the
                identity, so the fold is the only door a rounded W can come through.)
  exact-W'      d_in_kv from the unrounded W'                                          d_in_kv
  transposed-Wout   Wm0 Wout^T                                                         w_om
  side-swapped  K's result in V's slot and the reverse                                 every K / V pair

Gates (set by the formats and the twins, never by what a kernel gave)
  fp32 vector   max|got - want| / max|want|  <=  1/8 of the same distance from `want` to its nearest assigned twin; and per
                element |got - want| <= (n + 2) 2^-24 sum|terms| (any summation order; loose, but one garbage element fails it).
                b_om has no twin: its gate is that summation bound in the metric's own norm.
  rounded once  F(T) = ||T - exact||_F / ||exact||_F;  F(got) <= 1.1 F(f16(exact)), after checking FROM THE REFERENCES ALONE
                that every assigned twin, rounded the same way, has F >= 1.3 F(f16(exact)); and per element
                |got - exact| <= 2^-11 |exact| + 2^-25 + K 2^-23 (|A| |B|)_nk.
  the V pair    F(hi + lo) <= 1/8 of F of the nearest assigned UNROUNDED twin
  triangular    max|T^T T - A^T A| / max|A^T A| <= 2e-3;  || R h + c~ ||^2 against the centred sum of squares within 2e-4 on 512
                random h (both figures are tests/test_gpu_tri_stats.py's)
`emulate` is the recipe as tp_pack_weights states it in torch fp32 / fp16 — "a correct implementation" for
tests/test_pack_ref_cpu.py, which shows on the CPU that it passes every gate with 2x headroom and that every twin fails the
gate it is assigned to.  It is never the expectation of a GPU test."""
from __future__ import annotations

import ctypes
from collections import OrderedDict

import torch

from tokenpacker_amd import synth

E, HEADS, HEAD_DIM, C_MULTI = 1024, 8, 128, 4096
D = 384                        # the smallest hidden_size that is a multiple of 128 and no power of two: a D / E stride mix-up shows
F16_MAX = 65504.0
EPS32 = 2.0 ** -24
SENTINEL_BYTE = 0x7E           # the image is filled with it before the pack: 0x7E7E is an fp16 NaN, 0x7E7E7E7E the fp32 8.46e37
SENTINEL16, SENTINEL32 = 0x7E7E, 0x7E7E7E7E
SETS = ("plain", "offset")
DTYPES = (torch.float16, torch.bfloat16)
MATS = ("k", "v", "q")
_IN_ROWS = {"q": slice(0, E), "k": slice(E, 2 * E), "v": slice(2 * E, 3 * E)}
_W2 = {"k": "k_proj_1.2.weight", "v": "v_proj_1.2.weight", "q": "q_proj_1.weight"}
_B2 = {"k": "k_proj_1.2.bias", "v": "v_proj_1.2.bias", "q": None}

GATE_VECTOR_FRACTION = 1.0 / 8.0
GATE_PRODUCT = 1.1
GATE_TWIN_PRODUCT = 1.3
GATE_PAIR_FRACTION = 1.0 / 8.0
GATE_GRAM = 2e-3
GATE_NORM = 2e-4


# ---- the layout, by PackedLayout field name (declaration order = offset order) ----------------------------------------------------
def field_specs(hidden: int = D) -> "OrderedDict[str, tuple]":
    """name -> (element kind, shape): "io" the model dtype, "f16", "f32", "i32", or "scratch" (pack-time scratch, never inspected)."""
    f16, f32 = "f16", "f32"
    return OrderedDict([
        ("w_kv0", ("io", (2 * E, C_MULTI))), ("b_kv0", (f32, (2, E))), ("w_kv2", (f16, (2, E, E))), ("b_kv2", (f32, (2, E))),
        ("w_q1", (f16, (E, E))),
        ("w_in_kv", (f16, (2, E, E))), ("c_in_kv", (f32, (2, E))), ("b_in_kv", (f32, (2, E))),
        ("w_in_q", (f16, (E, E))), ("c_in_q", (f32, (E,))), ("b_in_q", (f32, (E,))),
        ("w_qt", (f16, (HEADS, E, HEAD_DIM))), ("w_qt_c", (f16, (HEADS, E, HEAD_DIM))),
        ("w_c_kv", (f16, (2, E, E))), ("d_in_kv", (f32, (2, E))), ("w_c_q", (f16, (E, E))),
        ("w_cc_kv", (f16, (2, E, E))), ("d_cc_kv", (f32, (2, E))), ("w_cc_q", (f16, (E, E))),
        ("w_qt_cc", (f16, (HEADS, E, HEAD_DIM))), ("w_cc_v3", (f16, (E, 2 * E))),
        ("w_r_kv", (f16, (2, E, E))), ("c_r_kv", (f32, (2, E))), ("w_r_q", (f16, (E, E))),
        ("wbar", ("scratch", None)), ("scratch_qr", ("scratch", None)),
        ("w_out", (f16, (E, E))), ("b_out", (f32, (E,))),
        ("w_m0", (f16, (hidden, E))), ("b_m0", (f32, (hidden,))), ("w_m2", (f16, (hidden, hidden))), ("b_m2", (f32, (hidden,))),
        ("w_om", (f16, (hidden, E))), ("b_om", (f32, (hidden,))),
        ("scratch_t", ("scratch", None)), ("scratch_p", ("scratch", None)),
        ("status", ("i32", (64,))),
    ])


SCRATCH_FIELDS = ("wbar", "scratch_qr", "scratch_t", "scratch_p")
# what a TP_DESC_TRAIN_PACK image does not build
INFERENCE_ONLY = ("w_qt", "w_qt_c", "w_qt_cc", "w_c_kv", "w_c_q", "d_in_kv", "w_cc_kv", "w_cc_q", "w_cc_v3", "d_cc_kv",
                  "w_r_kv", "w_r_q", "c_r_kv", "w_om", "b_om")
_ELEM = {"f16": (torch.float16, 2), "f32": (torch.float32, 4), "i32": (torch.int32, 4)}


def image_layout(hidden: int = D) -> "OrderedDict[str, tuple]":
    """name -> (offset, bytes) of every PackedLayout field, "total" last, from the library's own layout (tp_test_packed_layout)."""
    from tokenpacker_amd import _capi
    lib = _capi.load_test_library()
    out = OrderedDict()
    for name in list(field_specs(hidden)) + ["total"]:
        off, nbytes = ctypes.c_size_t(), ctypes.c_size_t()
        _capi_check(lib, lib.tp_test_packed_layout(hidden, name.encode(), ctypes.byref(off), ctypes.byref(nbytes)), name)
        out[name] = (off.value, nbytes.value)
    return out


def _capi_check(lib, rc, what):
    if rc != 0:
        raise ValueError(f"tp_test_packed_layout({what}): {lib.tp_last_error().decode('utf-8', 'replace')}")


def slice_image(buf: torch.Tensor, io_dtype: torch.dtype, hidden: int = D) -> "OrderedDict[str, torch.Tensor]":
    """Typed views of a uint8 image by field name (scratch fields: their raw bytes).  The element counts of `field_specs` must be
    what the layout reserved — a field whose size the two disagree on is an error here, not a silently short view."""
    lay = image_layout(hidden)
    out = OrderedDict()
    for name, (kind, shape) in field_specs(hidden).items():
        off, nbytes = lay[name]
        raw = buf[off:off + nbytes]
        if kind == "scratch":
            out[name] = raw
            continue
        dt, size = (io_dtype, 2) if kind == "io" else _ELEM[kind]
        numel = 1
        for d in shape:
            numel *= d
        if numel * size != nbytes:
            raise ValueError(f"{name}: the layout reserves {nbytes} B, field_specs says {shape} x {size} B")
        out[name] = raw.view(dt).view(shape)
    return out


# ---- rounding and re-layouts ------------------------------------------------------------------------------------------------------
def f16(t: torch.Tensor) -> torch.Tensor:
    """Round to fp16 (nearest even) with the kernels' clamp.  Bit-exact wherever `t` is exact in fp32 — every exact-bit tensor
    is; an fp64 product passes through fp32 first, a double rounding far below what any gate here resolves."""
    return t.to(torch.float32).clamp(-F16_MAX, F16_MAX).to(torch.float16)


def head_transpose(src: torch.Tensor) -> torch.Tensor:
    """dst[h][k][d] = src[h * 128 + d][k]: the per-head transposes w_qt* hold."""
    return src.view(HEADS, HEAD_DIM, E).transpose(1, 2).contiguous()


def pair_tiles(w3: torch.Tensor):
    """w_cc_v3 [E, 2 E] -> (hi, lo) [E, E]: K-tile 2 t is hi[:, 64 t : 64 t + 64], K-tile 2 t + 1 the matching lo."""
    t = w3.view(E, E // 64, 2, 64)
    return t[:, :, 0].reshape(E, E), t[:, :, 1].reshape(E, E)


def to_pair(hi: torch.Tensor, lo: torch.Tensor) -> torch.Tensor:
    return torch.stack([hi.view(E, E // 64, 64), lo.view(E, E // 64, 64)], dim=2).reshape(E, 2 * E).contiguous()


# ---- parameter sets ---------------------------------------------------------------------------------------------------------------
def make_param_set(kind: str, seed: int, dtype: torch.dtype, hidden: int = D):
    """plain: synth.make_params.  offset: the second layers' weights shifted by 3 * 1.5 / 32 (three of their standard deviations)
    and their biases by 3, before the cast — tests/test_gpu_tri_stats.py's shift: wbar and mean(b2) become large, so anything
    wrong in c becomes visible."""
    p = synth.make_params(seed, hidden)
    if kind == "offset":
        for name in ("k_proj_1.2.weight", "v_proj_1.2.weight", "q_proj_1.weight"):
            p[name] = p[name] + 3.0 * 1.5 / 32.0
        for name in ("k_proj_1.2.bias", "v_proj_1.2.bias"):
            p[name] = p[name] + 3.0
    elif kind != "plain":
        raise ValueError(f"unknown parameter set {kind!r}")
    return OrderedDict((k, v.to(dtype)) for k, v in p.items())


# ---- the reference ----------------------------------------------------------------------------------------------------------------
class Vec:
    """An fp32 vector of the image: `want` (fp64), sum|terms| per element, the number of terms, the assigned twins."""
    def __init__(self, want, abs_terms, n_terms, twins):
        self.want, self.abs_terms, self.n_terms, self.twins = want, abs_terms, n_terms, twins


class Prod:
    """A rounded-once product: `exact` (fp64, before the final f16), (|A| |B|) per element, K, the assigned twins (unrounded)."""
    def __init__(self, exact, abs_prod, K, twins):
        self.exact, self.abs_prod, self.K, self.twins = exact, abs_prod, K, twins


class Reference:
    """bits: field -> the exact tensor; vec / prod: (field, g) -> Vec / Prod (g: 0 / 1 of a K / V pair, None otherwise);
    tri: m -> (A [E, E + 1], W2 [E, E], b2 [E]) in fp64."""
    def __init__(self):
        self.bits, self.vec, self.prod, self.tri = OrderedDict(), OrderedDict(), OrderedDict(), OrderedDict()


def reference(params, kind: str, device="cpu") -> Reference:
    """`params`: a state dict already in the model dtype; `kind`: its parameter set (decides whether rounded-c is assigned)."""
    p = {k: v.to(device) for k, v in params.items()}
    d = lambda t: t.to(torch.float64)
    ref = Reference()
    inw, inb = p["clip_attn.in_proj_weight"], p["clip_attn.in_proj_bias"]
    # exact-bit tensors
    ref.bits["w_kv0"] = torch.cat([p["k_proj_1.0.weight"], p["v_proj_1.0.weight"]], 0)
    ref.bits["b_kv0"] = torch.stack([p["k_proj_1.0.bias"].float(), p["v_proj_1.0.bias"].float()])
    ref.bits["w_kv2"] = torch.stack([f16(p["k_proj_1.2.weight"]), f16(p["v_proj_1.2.weight"])])
    ref.bits["b_kv2"] = torch.stack([p["k_proj_1.2.bias"].float(), p["v_proj_1.2.bias"].float()])
    ref.bits["w_q1"] = f16(p["q_proj_1.weight"])
    ref.bits["w_out"], ref.bits["b_out"] = f16(p["clip_attn.out_proj.weight"]), p["clip_attn.out_proj.bias"].float()
    ref.bits["w_m0"], ref.bits["b_m0"] = f16(p["mlp.0.weight"]), p["mlp.0.bias"].float()
    ref.bits["w_m2"], ref.bits["b_m2"] = f16(p["mlp.2.weight"]), p["mlp.2.bias"].float()
    per = {}
    for m in MATS:
        W, gamma, beta = inw[_IN_ROWS[m]], p[f"ln_{m}_1.weight"], p[f"ln_{m}_1.bias"]
        hi = f16(W.float() * gamma.float())                              # the product is exact in fp32: one rounding, bit-exact
        Wx, Wr = d(W) * d(gamma), d(hi)
        W2 = d(f16(p[_W2[m]]))
        b2 = d(p[_B2[m]]) if _B2[m] else torch.zeros(E, dtype=torch.float64, device=device)
        wbar, bbar = W2.mean(0), b2.mean()
        cx, cr = Wx.sum(1), Wr.sum(1)
        Px, Pr = Wx @ W2, Wr @ W2
        absW = torch.maximum(Wx.abs(), Wr.abs())
        rowabs = absW.sum(1)
        absP = absW @ W2.abs()
        per[m] = dict(
            hi=hi,
            c_in=Vec(cr, Wr.abs().sum(1), E, {"exact-rowsum": cx}),
            b_in=Vec(d(W) @ d(beta) + d(inb[_IN_ROWS[m]]), d(W).abs() @ d(beta).abs() + d(inb[_IN_ROWS[m]]).abs(), E + 1,
                     {"rounded-W": (Wr / d(gamma)) @ d(beta) + d(inb[_IN_ROWS[m]])}),
            d_in=Vec(Wr @ b2, Wr.abs() @ b2.abs(), E, {"exact-W'": Wx @ b2}),
            d_cc=Vec(Wx @ b2 - cx * bbar, absW @ b2.abs() + rowabs * bbar.abs(), 2 * E,
                     {"hi-only": Wr @ b2 - cx * bbar, "rounded-c": Wx @ b2 - cr * bbar, "uncentred": Wx @ b2}),
            w_c=Prod(Pr, absP, E, {"exact-fold": Px}),
            w_cc=Prod(Px - torch.outer(cx, wbar), absP + torch.outer(rowabs, wbar.abs()), E,
                      {"hi-only": Pr - torch.outer(cx, wbar), "rounded-c": Px - torch.outer(cr, wbar), "uncentred": Px}))
        if kind != "offset":                                             # (on the plain set wbar and mean(b2) are too small for it)
            del per[m]["d_cc"].twins["rounded-c"], per[m]["w_cc"].twins["rounded-c"]
        ref.tri[m] = (torch.cat([W2 - wbar, (b2 - bbar)[:, None]], 1), W2, b2)
    for a, b in (("k", "v"), ("v", "k")):                                # side-swapped: the other side's result in this slot
        for key in ("c_in", "b_in", "d_in", "d_cc"):
            per[a][key].twins["side-swapped"] = per[b][key].want
        for key in ("w_c", "w_cc"):
            per[a][key].twins["side-swapped"] = per[b][key].exact
    ref.bits["w_in_kv"], ref.bits["w_in_q"] = torch.stack([per["k"]["hi"], per["v"]["hi"]]), per["q"]["hi"]
    for g, m in enumerate(("k", "v")):
        ref.vec["c_in_kv", g], ref.vec["b_in_kv", g] = per[m]["c_in"], per[m]["b_in"]
        ref.vec["d_in_kv", g], ref.vec["d_cc_kv", g] = per[m]["d_in"], per[m]["d_cc"]
        ref.prod["w_c_kv", g], ref.prod["w_cc_kv", g] = per[m]["w_c"], per[m]["w_cc"]
    ref.vec["c_in_q", None], ref.vec["b_in_q", None] = per["q"]["c_in"], per["q"]["b_in"]
    ref.prod["w_c_q", None], ref.prod["w_cc_q", None] = per["q"]["w_c"], per["q"]["w_cc"]
    Wm0, Wout = d(ref.bits["w_m0"]), d(ref.bits["w_out"])
    ref.prod["w_om", None] = Prod(Wm0 @ Wout, Wm0.abs() @ Wout.abs(), E, {"transposed-Wout": Wm0 @ Wout.t()})
    ref.vec["b_om", None] = Vec(Wm0 @ d(ref.bits["b_out"]) + d(ref.bits["b_m0"]),
                                Wm0.abs() @ d(ref.bits["b_out"]).abs() + d(ref.bits["b_m0"]).abs(), E + 1, {})
    return ref


def _pick(t: torch.Tensor, g):
    return t if g is None else t[g]


# ---- the gates: every function returns rows (label, kind, value, gate); value <= gate passes ---------------------------------------
def rel_max(a: torch.Tensor, want: torch.Tensor) -> float:
    return float((a.to(torch.float64) - want).abs().max() / want.abs().max())


def frob(a: torch.Tensor, exact: torch.Tensor) -> float:
    return float((a.to(torch.float64) - exact).norm() / exact.norm())


def _worst(err: torch.Tensor, bound: torch.Tensor) -> float:
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    r = torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)
    return float(r.max())


def vector_gate(v: Vec) -> float:
    if not v.twins:           # no named twin: the any-order summation bound, in the metric's norm
        return float(((v.n_terms + 2) * EPS32 * v.abs_terms).max() / v.want.abs().max())
    return GATE_VECTOR_FRACTION * min(rel_max(t, v.want) for t in v.twins.values())


def vector_rows(label: str, got: torch.Tensor, v: Vec):
    got = got.to(torch.float64)
    return [(label, "metric", rel_max(got, v.want), vector_gate(v)),
            (label + " per element", "elem", _worst((got - v.want).abs(), (v.n_terms + 2) * EPS32 * v.abs_terms), 1.0)]


def product_floor(pr: Prod) -> float:
    """F of the ideal result: the exact product rounded once."""
    return frob(f16(pr.exact), pr.exact)


def twin_separation(pr: Prod):
    """(twin, F(f16(twin)) / F(f16(exact))) for every assigned twin: the precondition of the product gate wants each >= 1.3."""
    f0 = product_floor(pr)
    return [(name, frob(f16(t), pr.exact) / f0) for name, t in pr.twins.items()]


def product_rows(label: str, got: torch.Tensor, pr: Prod):
    got = got.to(torch.float64)
    bound = 2.0 ** -11 * pr.exact.abs() + 2.0 ** -25 + pr.K * 2.0 ** -23 * pr.abs_prod
    return [(label, "metric", frob(got, pr.exact), GATE_PRODUCT * product_floor(pr)),
            (label + " per element", "elem", _worst((got - pr.exact).abs(), bound), 1.0)]


def pair_rows(label: str, w3: torch.Tensor, pr: Prod):
    hi, lo = pair_tiles(w3)
    total = hi.to(torch.float64) + lo.to(torch.float64)
    return [(label, "metric", frob(total, pr.exact), GATE_PAIR_FRACTION * min(frob(t, pr.exact) for t in pr.twins.values()))]


def tri_rows(label: str, r16: torch.Tensor, ctil, tri, seed: int = 4100):
    A, W2, b2 = tri
    R = r16.to(torch.float64)
    c = ctil.to(torch.float64) if ctil is not None else torch.zeros(E, dtype=torch.float64, device=R.device)
    T = torch.cat([R, c[:, None]], 1)
    gram = A.t() @ A
    h = (torch.randn(512, E, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * 1.5).to(R.device)
    y = h @ W2.t() + b2
    want = ((y - y.mean(1, keepdim=True)) ** 2).sum(1)
    got = ((h @ R.t() + c) ** 2).sum(1)
    return [(label + " gram", "metric", float((T.t() @ T - gram).abs().max() / gram.abs().max()), GATE_GRAM),
            (label + " norm", "metric", float(((got - want).abs() / want).max()), GATE_NORM)]


def field_rows(img, ref: Reference, field: str, g=None):
    """The gates of one non-bit-exact tensor of the image (`g`: which of a K / V pair)."""
    label = field if g is None else f"{field}[{'kv'[g]}]"
    if field == "w_cc_v3":
        return pair_rows(label, img[field], ref.prod["w_cc_kv", 1])
    if (field, g) in ref.vec:
        return vector_rows(label, _pick(img[field], g), ref.vec[field, g])
    if (field, g) in ref.prod:
        return product_rows(label, _pick(img[field], g), ref.prod[field, g])
    if field == "w_r_kv":
        return tri_rows(label, img["w_r_kv"][g], img["c_r_kv"][g], ref.tri["kv"[g]])
    if field == "w_r_q":
        return tri_rows(label, img["w_r_q"], None, ref.tri["q"])
    raise KeyError(field)


def gated_fields(ref: Reference):
    """(field, g) of every tensor `field_rows` has gates for, grouped as the GPU tests are."""
    return {"vectors": list(ref.vec), "products": list(ref.prod), "pair": [("w_cc_v3", None)],
            "triangular": [("w_r_kv", 0), ("w_r_kv", 1), ("w_r_q", None)]}


def format_rows(rows) -> str:
    return "\n".join(f"  {label:<28s} {value:10.3e}  <= {gate:10.3e}   {'ok' if value <= gate else 'FAIL'}"
                     for label, _, value, gate in rows)


def failures(rows):
    return [r for r in rows if not r[2] <= r[3]]


def with_twin(img, ref: Reference, field: str, g, twin: str):
    """A copy of the image dict whose tensor (field, g) holds the named twin the way the image would hold it: an fp32 vector as
    fp32, a product rounded once, the V pair as f16(twin) | f16(twin - hi)."""
    out = dict(img)
    if field == "w_cc_v3":
        t = ref.prod["w_cc_kv", 1].twins[twin]
        hi = f16(t)
        out[field] = to_pair(hi, f16(t - hi.to(torch.float64)))
        return out
    if (field, g) in ref.vec:
        t = ref.vec[field, g].twins[twin].to(torch.float32)
    else:
        t = f16(ref.prod[field, g].twins[twin])
    if g is None:
        out[field] = t
    else:
        out[field] = img[field].clone()
        out[field][g] = t
    return out


# ---- the recipe as tp_pack_weights states it, in torch fp32 / fp16 ----------------------------------------------------------------
def emulate(params, device="cpu", hidden: int = D):
    """fp32 products of fp16 operands, hi + lo, one final rounding; R by a Householder QR in fp64, rounded to fp16.  Returns the
    image as a dict by field name (no scratch fields)."""
    p = {k: v.to(device) for k, v in params.items()}
    f32 = lambda t: t.to(torch.float32)
    img = OrderedDict()
    inw, inb = p["clip_attn.in_proj_weight"], p["clip_attn.in_proj_bias"]
    img["w_kv0"] = torch.cat([p["k_proj_1.0.weight"], p["v_proj_1.0.weight"]], 0)
    img["b_kv0"] = torch.stack([f32(p["k_proj_1.0.bias"]), f32(p["v_proj_1.0.bias"])])
    img["w_kv2"] = torch.stack([f16(p["k_proj_1.2.weight"]), f16(p["v_proj_1.2.weight"])])
    img["b_kv2"] = torch.stack([f32(p["k_proj_1.2.bias"]), f32(p["v_proj_1.2.bias"])])
    img["w_q1"] = f16(p["q_proj_1.weight"])
    img["w_out"], img["b_out"] = f16(p["clip_attn.out_proj.weight"]), f32(p["clip_attn.out_proj.bias"])
    img["w_m0"], img["b_m0"] = f16(p["mlp.0.weight"]), f32(p["mlp.0.bias"])
    img["w_m2"], img["b_m2"] = f16(p["mlp.2.weight"]), f32(p["mlp.2.bias"])
    r = {}
    for m in MATS:
        W, gamma, beta = f32(inw[_IN_ROWS[m]]), f32(p[f"ln_{m}_1.weight"]), f32(p[f"ln_{m}_1.bias"])
        Wx = W * gamma                                                   # exact in fp32
        hi = f16(Wx)
        lo = (Wx - f32(hi)).to(torch.float16)
        W2h = f16(p[_W2[m]])
        W2 = f32(W2h)
        b2 = f32(p[_B2[m]]) if _B2[m] else None
        wbar = W2.double().mean(0).float()
        c_ex = Wx.sum(1)
        v = (f32(hi) @ W2 + f32(lo) @ W2) - c_ex[:, None] * wbar[None, :]
        w_cc = f16(v)
        A = torch.cat([W2.double() - W2.double().mean(0), ((b2.double() - b2.double().mean()) if b2 is not None
                                                            else torch.zeros(E, dtype=torch.float64, device=device))[:, None]], 1)
        Rfull = torch.linalg.qr(A, mode="r").R                            # [E, E + 1]: R | Q^T b2c
        r[m] = dict(hi=hi, c_in=f32(hi).sum(1), b_in=W @ beta + f32(inb[_IN_ROWS[m]]), w_c=f16(f32(hi) @ W2),
                    d_in=f32(hi) @ b2 if b2 is not None else None, w_cc=w_cc, lo3=(v - f32(w_cc)).to(torch.float16),
                    d_cc=(Wx @ b2 - c_ex * b2.double().mean().float()) if b2 is not None else None,
                    w_r=f16(torch.triu(Rfull[:, :E])), c_r=Rfull[:, E].float())
    pair = lambda key: torch.stack([r["k"][key], r["v"][key]])
    img["w_in_kv"], img["c_in_kv"], img["b_in_kv"] = pair("hi"), pair("c_in"), pair("b_in")
    img["w_in_q"], img["c_in_q"], img["b_in_q"] = r["q"]["hi"], r["q"]["c_in"], r["q"]["b_in"]
    img["w_c_kv"], img["d_in_kv"], img["w_c_q"] = pair("w_c"), pair("d_in"), r["q"]["w_c"]
    img["w_cc_kv"], img["d_cc_kv"], img["w_cc_q"] = pair("w_cc"), pair("d_cc"), r["q"]["w_cc"]
    img["w_qt"], img["w_qt_c"], img["w_qt_cc"] = (head_transpose(r["k"][key]) for key in ("hi", "w_c", "w_cc"))
    img["w_cc_v3"] = to_pair(r["v"]["w_cc"], r["v"]["lo3"])
    img["w_r_kv"], img["c_r_kv"], img["w_r_q"] = pair("w_r"), pair("c_r"), r["q"]["w_r"]
    img["w_om"] = f16(f32(img["w_m0"]) @ f32(img["w_out"]))
    img["b_om"] = f32(img["w_m0"]) @ img["b_out"] + img["b_m0"]
    status = torch.zeros(64, dtype=torch.int32, device=device)
    status[1] = status[2] = 1
    img["status"] = status
    return img
