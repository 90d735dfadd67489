"""The packed-weight image, tensor by tensor, on a real MI355X: tp_pack_weights is called directly (as projector.py calls it) into a
buffer filled with the byte 0x7E, the image is sliced with the library's own layout (tp_test_packed_layout) and every tensor is
compared with tests/pack_ref.py — bit patterns where the value is exact, fp64 references with the gates derived there otherwise
(tests/test_pack_ref_cpu.py shows on the CPU that a correct fp32 / fp16 implementation passes them and each named mistake fails).
hidden_size 384; {fp16, bf16} x {plain, offset} parameters.  `-s` prints every measured value beside its gate."""
import ctypes

import pytest
import torch

from tests import pack_ref as pr
from tokenpacker_amd import _capi

pytestmark = pytest.mark.gpu
E, D = pr.E, pr.D
SEED = 9100
CASES = [(dt, kind) for dt in pr.DTYPES for kind in pr.SETS]
_ID = lambda c: f"{str(c[0]).split('.')[-1]}-{c[1]}"
_TP = {torch.bfloat16: _capi.TP_BF16, torch.float16: _capi.TP_F16}


def _pack(params, dtype, flags=0):
    """-> the image as a uint8 tensor: sentinel fill, tp_pack_weights on the current stream, tp_pack_forget."""
    lib = _capi.load_library()
    desc = _capi.make_desc(1, 24, 2, D, _TP[dtype], flags=flags)
    nbytes = lib.tp_packed_weight_bytes(ctypes.byref(desc))
    assert nbytes == pr.image_layout(D)["total"][0] and nbytes > 0
    buf = torch.full((nbytes,), pr.SENTINEL_BYTE, dtype=torch.uint8, device="cuda")
    tensors = [params[name].to("cuda").contiguous() for name in _capi.WEIGHT_FIELDS]
    assert all(t.dtype == dtype for t in tensors)
    raw = _capi.tp_weights(*[t.data_ptr() for t in tensors])
    _capi.check(lib.tp_pack_weights(ctypes.byref(desc), ctypes.byref(raw), buf.data_ptr(), nbytes,
                                    torch.cuda.current_stream().cuda_stream), "tp_pack_weights")
    torch.cuda.synchronize()
    _capi.check(lib.tp_pack_forget(buf.data_ptr()), "tp_pack_forget")     # (the library's note about this address goes before the buffer can)
    return buf


@pytest.fixture(scope="module")
def packed():
    """(dtype, kind) -> (params, image bytes, the image by field, the fp64 reference on the GPU); one pack and one reference per
    case, shared by the tests of this module and dropped with it."""
    memo = {}

    def get(case):
        if case not in memo:
            dtype, kind = case
            params = pr.make_param_set(kind, SEED, dtype)
            buf = _pack(params, dtype)
            memo[case] = (params, buf, pr.slice_image(buf, dtype, D), pr.reference(params, kind, "cuda"))
        return memo[case]
    yield get
    memo.clear()
    torch.cuda.empty_cache()


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _holds_sentinel(t):
    return bool((_bits(t) == (pr.SENTINEL16 if t.element_size() == 2 else pr.SENTINEL32)).any())


def _report(case, title, rows):
    print(f"\n[pack-image] {_ID(case)}: {title}\n{pr.format_rows(rows)}")
    bad = pr.failures(rows)
    assert not bad, "\n" + pr.format_rows(bad)


@pytest.mark.parametrize("case", CASES, ids=_ID)
def test_exact_bit_tensors(packed, case):
    """Casts, copies and the LayerNorm-folded weights bit for bit; the re-laid-out tensors against the image's OWN sources; zeros below
    R's diagonal; the status words; no sentinel left in a built tensor, every byte of alignment padding still the sentinel."""
    _, buf, img, ref = packed(case)
    for name, want in ref.bits.items():
        assert _same_bits(img[name], want), name
    for name, src in (("w_qt", img["w_in_kv"][0]), ("w_qt_c", img["w_c_kv"][0]), ("w_qt_cc", img["w_cc_kv"][0])):
        assert _same_bits(img[name], pr.head_transpose(src)), name
    hi, _ = pr.pair_tiles(img["w_cc_v3"])
    assert _same_bits(hi, img["w_cc_kv"][1]), "w_cc_v3: the hi K-tiles"
    for name in ("w_r_kv", "w_r_q"):
        assert not bool((torch.tril(img[name].float(), diagonal=-1) != 0).any()), name
    assert img["status"][:3].tolist() == [0, 1, 1]
    for name, (kind, _) in pr.field_specs(D).items():
        if kind != "scratch":
            assert not _holds_sentinel(img[name]), name
    lay = list(pr.image_layout(D).items())
    for (name, (off, nbytes)), (_, (nxt, _)) in zip(lay[:-1], lay[1:]):
        assert bool((buf[off + nbytes:nxt] == pr.SENTINEL_BYTE).all()), f"the padding behind {name} was written"


@pytest.mark.parametrize("case", CASES, ids=_ID)
def test_fp32_vectors(packed, case):
    _, _, img, ref = packed(case)
    rows = [r for field, g in pr.gated_fields(ref)["vectors"] for r in pr.field_rows(img, ref, field, g)]
    _report(case, "fp32 vectors: max|got - want| / max|want| against 1/8 of the nearest twin's; per element against the summation bound", rows)


@pytest.mark.parametrize("case", CASES, ids=_ID)
def test_rounded_once_products(packed, case):
    _, _, img, ref = packed(case)
    for (field, g), prod in ref.prod.items():          # from the references alone: the gate separates every assigned twin
        for twin, ratio in pr.twin_separation(prod):
            assert ratio >= pr.GATE_TWIN_PRODUCT, (field, g, twin, ratio)
    rows = [r for field, g in pr.gated_fields(ref)["products"] for r in pr.field_rows(img, ref, field, g)]
    _report(case, "rounded-once products: F(got) against 1.1 F(f16(exact)); per element against rounding + accumulation", rows)


@pytest.mark.parametrize("case", CASES, ids=_ID)
def test_v_side_hi_lo_pair(packed, case):
    """hi + lo of w_cc_v3, summed in fp64, is Wcc of the V side nearly unrounded: a dropped lo product, or a lo taken from the
    already rounded value, is 8x or more beyond the gate."""
    _, _, img, ref = packed(case)
    _report(case, "the V-side pair: F(hi + lo) against 1/8 of the nearest unrounded twin's", pr.field_rows(img, ref, "w_cc_v3"))


@pytest.mark.parametrize("case", CASES, ids=_ID)
def test_triangular_factors(packed, case):
    _, _, img, ref = packed(case)
    rows = [r for field, g in pr.gated_fields(ref)["triangular"] for r in pr.field_rows(img, ref, field, g)]
    _report(case, "triangular factors: T^T T against A^T A; || R h + c~ ||^2 against the centred sum of squares", rows)


def test_training_pack_builds_the_shared_tensors_only(packed):
    """TP_DESC_TRAIN_PACK: the casts and the three LayerNorm folds bit for bit as in the inference image, status [1] = [2] = 0, and
    every inference-only region untouched — "not built" as a tested property."""
    case = (torch.bfloat16, "plain")
    params, _, img, ref = packed(case)
    buf = _pack(params, case[0], flags=_capi.TP_DESC_TRAIN_PACK)
    timg = pr.slice_image(buf, case[0], D)
    for name in list(ref.bits) + ["c_in_kv", "b_in_kv", "c_in_q", "b_in_q"]:
        assert _same_bits(timg[name], img[name]), name
    assert timg["status"][:3].tolist() == [0, 0, 0]
    lay = pr.image_layout(D)
    for name in pr.INFERENCE_ONLY:
        off, nbytes = lay[name]
        assert bool((buf[off:off + nbytes] == pr.SENTINEL_BYTE).all()), f"{name} was written by a training pack"


def test_clamp_count_of_a_cast_only_tensor():
    """Five mlp.2.weight elements of a bf16 model beyond +-65504, one of them inf (a cast-only tensor that feeds no product):
    status[0] is exactly 5, those five are +-65504, every other element of w_m2 is the plain cast."""
    dtype = torch.bfloat16
    params = pr.make_param_set("plain", SEED, dtype)
    w = params["mlp.2.weight"].clone()
    clean = pr.f16(w)
    planted = {(0, 0): 7.0e4, (17, 300): -1.0e5, (200, 383): float("inf"), (383, 1): -3.0e38, (383, 383): 65536.0}
    for (i, j), v in planted.items():
        w[i, j] = v
    params["mlp.2.weight"] = w
    img = pr.slice_image(_pack(params, dtype), dtype, D)
    assert int(img["status"][0]) == len(planted)
    got = img["w_m2"].cpu()
    for (i, j), v in planted.items():
        assert float(got[i, j]) == (pr.F16_MAX if v > 0 else -pr.F16_MAX), (i, j)
        clean[i, j] = got[i, j]
    assert _same_bits(got, clean)


def test_two_packs_give_identical_bytes(packed):
    case = (torch.float16, "offset")
    params, buf, _, _ = packed(case)
    again = _pack(params, case[0])
    lay = list(pr.image_layout(D).items())
    for (name, (off, _)), (_, (nxt, _)) in zip(lay[:-1], lay[1:]):       # each tensor with the padding behind it
        if name not in pr.SCRATCH_FIELDS:
            assert torch.equal(buf[off:nxt], again[off:nxt]), name
