"""CLIP preprocessing of the pad / square image modes (preprocess.preprocess_images / tp_clip_preprocess) without a GPU.

1. ``tp_resize_coeffs`` — the single source of coefficients — equals the model of tests/clip_preprocess_ref.py exactly.
2. The model equals Pillow on the resize alone (where PIL imports), and the golden minted from the reference's ``process_images``
   on the whole path, in both modes: digests for every case, whole arrays for two.
3. ``preprocess_plan``'s geometry.
4. Every refusal of ``tp_clip_preprocess`` through the C ABI on fake pointers, before a device is touched, and the refusals of the
   Python interface."""
import ctypes

import numpy as np
import pytest
import torch

from tests import clip_preprocess_ref as ref
from tokenpacker_amd import _capi, hd
from tokenpacker_amd import preprocess as pp

E = _capi.TP_ERR_INVALID_ARG
MODES = {0: "square", 1: "pad"}


# ---- 1. coefficients -------------------------------------------------------------------------------------------------------------
def same_tables(in_size, out_size, first, n):
    kk, bounds = pp.resize_coeffs(in_size, out_size, first, n)
    mk, mb, ksize = ref.resize_coeffs(in_size, out_size, first, n)
    assert kk.shape == (n, ksize) and kk.dtype == np.int32 and bounds.dtype == np.int32
    assert np.array_equal(bounds, mb), (in_size, out_size, first)
    assert np.array_equal(kk, mk), (in_size, out_size, first)


def test_resize_coeffs_equal_the_model_for_every_input_size_up_to_700():
    for in_size in range(1, 701):
        same_tables(in_size, 336, 0, 336)


@pytest.mark.parametrize("in_size", [1000, 1201, 1600, 2500, 4000, 8192, 16384])
def test_resize_coeffs_equal_the_model_on_large_inputs(in_size):
    same_tables(in_size, 336, 0, 336)


@pytest.mark.parametrize("in_size,out_size", [(900, 100800), (16384, 5505024), (41, 8195), (1600, 447), (39, 336)])
def test_resize_coeffs_of_a_window_of_a_long_output(in_size, out_size):
    """Only the crop window's positions are computed: at the left edge, in the centre (where the crop sits) and at the right edge."""
    n = min(336, out_size)
    for first in sorted({0, (out_size - n) // 2, out_size - n}):
        same_tables(in_size, out_size, first, n)


def test_resize_coeffs_at_scale_one_are_the_identity():
    kk, bounds = pp.resize_coeffs(336, 336, 0, 336)
    for x in range(336):
        xmin, cnt = bounds[x]
        full = np.zeros(336, dtype=np.int64)
        full[xmin:xmin + cnt] = kk[x, :cnt]
        assert full[x] == 1 << 22 and np.count_nonzero(full) == 1


def test_resize_coeffs_refusals_and_tap_count():
    lib = _capi.load_library()
    k = ctypes.c_int(0)
    assert lib.tp_resize_coeffs(16384, 336, 0, 336, None, None, ctypes.byref(k)) == _capi.TP_OK and k.value == 197
    assert lib.tp_resize_coeffs(5, 336, 0, 336, None, None, ctypes.byref(k)) == _capi.TP_OK and k.value == 5
    buf = np.zeros(4096, dtype=np.int32)
    for args, msg in (((0, 336, 0, 336), "in_size"), ((10, 0, 0, 1), "out_size"), ((10, 336, 1, 336), "lie outside"),
                      ((10, 336, -1, 2), "lie outside"), ((10, 336, 0, 0), "lie outside")):
        assert lib.tp_resize_coeffs(*args, buf.ctypes.data, buf.ctypes.data, ctypes.byref(k)) == E
        assert msg in _capi.last_error()
    assert lib.tp_resize_coeffs(10, 336, 0, 1, buf.ctypes.data, None, ctypes.byref(k)) == E and "NULL" in _capi.last_error()


# ---- 2. the model against Pillow and against the golden --------------------------------------------------------------------------
@pytest.mark.parametrize("h,w,oh,ow", [(40, 39, 344, 336), (3, 900, 336, 1000), (1000, 41, 500, 336), (1201, 1600, 336, 447),
                                       (50, 71, 336, 336), (336, 500, 336, 500), (337, 500, 336, 498), (5, 5, 336, 336)])
def test_model_resize_equals_pillow(h, w, oh, ow):
    Image = pytest.importorskip("PIL.Image")
    img = ref.test_image(h, w, 1)
    want = np.asarray(Image.fromarray(img).resize((ow, oh), Image.BICUBIC))
    assert np.array_equal(ref.resize_u8(img, oh, ow), want)
    top, left = (oh - min(oh, 336)) // 2, (ow - min(ow, 336)) // 2
    assert np.array_equal(ref.resize_u8(img, oh, ow, (top, left, 336, 336)), want[top:top + 336, left:left + 336])


def test_test_image_saturates_clip8_at_both_ends():
    """The negative lobes must push raw sums below 0 and above 255: a kernel that forgot to saturate fails the GPU cases."""
    sums = []
    ref.preprocess_bytes(ref.test_image(1201, 1600, 7), "square", sums=sums)
    ref.preprocess_bytes(ref.test_image(40, 39, 7), "pad", sums=sums)
    assert min(s[0] for s in sums) >> 22 < 0 and max(s[1] for s in sums) >> 22 > 255


def golden_cases():
    g = ref.golden()
    return [tuple(int(v) for v in c) for c in g["cases"]]


def test_golden_is_data_with_recorded_versions():
    g = ref.golden()
    assert set(g) == {"cases", "input_sha256", "output_sha256", "full_index", "full_bytes", "table", "versions"}
    assert "pillow" in str(g["versions"]) and "transformers" in str(g["versions"])
    assert len(g["cases"]) == 28 and {c[2] for c in golden_cases()} == {0, 1}
    assert g["full_bytes"].shape == (2, 3, 336, 336) and g["full_bytes"].dtype == np.uint8


def test_table_of_the_reference_is_the_library_table():
    t = ref.golden()["table"]
    assert np.array_equal(t.view(np.int32), hd.normalisation_table().numpy().view(np.int32))
    assert ref.BACKGROUND == tuple(int(m * 255) for m in hd.CLIP_MEAN)


@pytest.mark.parametrize("case", range(28))
def test_model_equals_the_golden_on_the_whole_path(case):
    g = ref.golden()
    h, w, mode, seed = golden_cases()[case]
    assert ref.digest(ref.test_image(h, w, seed)) == str(g["input_sha256"][case])
    got = ref.expected(h, w, MODES[mode], seed)
    assert got.shape == (3, 336, 336) and got.dtype == np.float32
    assert ref.digest(got) == str(g["output_sha256"][case])
    for slot, index in enumerate(g["full_index"]):
        if int(index) == case:
            assert np.array_equal(ref.expected_bytes(h, w, MODES[mode], seed).transpose(2, 0, 1), g["full_bytes"][slot])


# ---- 3. geometry ------------------------------------------------------------------------------------------------------------------
def test_preprocess_plan_geometry():
    G = pp.ClipGeometry
    sizes = [(50, 71), (71, 50), (336, 336), (1, 37), (37, 1), (1, 1), (336, 500), (500, 336), (3, 900), (1201, 1600), (335, 336)]
    pad = pp.preprocess_plan(sizes, "pad")
    assert pad[0] == G("pad", 50, 71, 71, 71, 10, 0, 336, 336, 0, 0)           # (71 - 50) // 2 = 10: odd difference, rounded down
    assert pad[1] == G("pad", 71, 50, 71, 71, 0, 10, 336, 336, 0, 0)
    assert pad[2] == G("pad", 336, 336, 336, 336, 0, 0, 336, 336, 0, 0)
    assert pad[3] == G("pad", 1, 37, 37, 37, 18, 0, 336, 336, 0, 0)
    assert pad[4] == G("pad", 37, 1, 37, 37, 0, 18, 336, 336, 0, 0)
    assert pad[5] == G("pad", 1, 1, 1, 1, 0, 0, 336, 336, 0, 0)
    sq = pp.preprocess_plan(sizes, "square")
    assert sq[0] == G("square", 50, 71, 50, 71, 0, 0, 336, 477, 0, 70)         # int(336 * 71 / 50) = 477, (477 - 336) // 2 = 70
    assert sq[1] == G("square", 71, 50, 71, 50, 0, 0, 477, 336, 70, 0)
    assert sq[2] == G("square", 336, 336, 336, 336, 0, 0, 336, 336, 0, 0)
    assert sq[3] == G("square", 1, 37, 1, 37, 0, 0, 336, 12432, 0, 6048)
    assert sq[4] == G("square", 37, 1, 37, 1, 0, 0, 12432, 336, 6048, 0)
    assert sq[5] == G("square", 1, 1, 1, 1, 0, 0, 336, 336, 0, 0)
    assert sq[6] == G("square", 336, 500, 336, 500, 0, 0, 336, 500, 0, 82)
    assert sq[7] == G("square", 500, 336, 500, 336, 0, 0, 500, 336, 82, 0)
    assert sq[8] == G("square", 3, 900, 3, 900, 0, 0, 336, 100800, 0, 50232)
    assert sq[9] == G("square", 1201, 1600, 1201, 1600, 0, 0, 336, 447, 0, 55)
    assert sq[10] == G("square", 335, 336, 335, 336, 0, 0, 336, 337, 0, 0)
    # anything but 'pad' and 'slice' is the processor alone (mm_utils.py:36-37); the model's own restatement agrees everywhere
    assert pp.preprocess_plan(sizes, "anything") == sq and pp.preprocess_plan(sizes, None) == sq
    for mode in ("pad", "square"):
        for g in pp.preprocess_plan(sizes, mode):
            assert tuple(g[3:]) == ref.geometry(g.H, g.W, mode)
    for bad in ([(0, 5)], [(5, -1)]):
        with pytest.raises(ValueError):
            pp.preprocess_plan(bad)
    with pytest.raises(ValueError, match="multiple of 8"):
        pp.preprocess_plan([(5, 5)], "pad", 100)


def test_batch_plan_tables_rows_and_workspace():
    sizes = [(1201, 1600), (50, 71), (1, 1)]
    plan = pp.clip_batch_plan(sizes, "pad", 336, ref.BACKGROUND)
    assert plan.images.dtype.itemsize == ctypes.sizeof(_capi.tp_clip_image) == 104
    word, ws, at = 0, 0, 0
    for rec, (h, w) in zip(plan.images, sizes):
        s = max(h, w)
        mk, mb, ksize = ref.resize_coeffs(s, 336)
        assert rec["ksize_h"] == rec["ksize_v"] == ksize and tuple(rec["background"]) == ref.BACKGROUND + (0,)
        assert rec["src_offset"] == at and rec["row_stride"] == 3 * w and rec["ws_offset"] == ws
        assert (rec["kk_h"], rec["bounds_h"], rec["kk_v"], rec["bounds_v"]) == (word, word + ksize * 336, word + (ksize + 2) * 336,
                                                                              word + (2 * ksize + 2) * 336)
        c = plan.coeffs
        assert np.array_equal(c[rec["kk_h"]:rec["bounds_h"]].reshape(ksize, 336), mk.T)             # tap-major
        assert np.array_equal(c[rec["bounds_h"]:rec["kk_v"]].reshape(336, 2), mb)
        assert np.array_equal(c[rec["kk_v"]:rec["bounds_v"]].reshape(336, ksize), mk)
        assert rec["row0"] == mb[0, 0] and rec["rows"] == mb[-1, 0] + mb[-1, 1] - mb[0, 0]
        word += (2 * ksize + 4) * 336
        ws += -(-int(rec["rows"]) * 336 * 3 // 16) * 16
        at += -(-h * w * 3 // 16) * 16
    assert plan.coeffs.size == word and plan.workspace_bytes == ws and plan.pixel_bytes == at
    # square mode: only the rows under the crop window's vertical taps are resampled horizontally
    rec = pp.clip_batch_plan([(2000, 500)], "square").images[0]
    assert rec["crop_top"] == 504 and 0 < rec["row0"] and rec["rows"] < 520 and rec["row0"] + rec["rows"] < 2000


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------------
FAKE = 0x10000          # a 16-byte aligned "device pointer" — never dereferenced: every call below fails on the host first


def call(plan, **over):
    lib = _capi.load_library()
    a = dict(plan_host=plan.images.ctypes.data, plan_dev=FAKE, n=len(plan.images), pixels=FAKE, pixel_bytes=plan.pixel_bytes, lut=FAKE,
             coeffs_host=plan.coeffs.ctypes.data, coeffs_dev=FAKE, coeff_words=plan.coeffs.size, workspace=FAKE,
             workspace_bytes=plan.workspace_bytes, out=FAKE, size=336, out_dtype=_capi.TP_F32)
    a.update(over)
    return lib.tp_clip_preprocess(a["plan_host"], a["plan_dev"], a["n"], a["pixels"], a["pixel_bytes"], a["lut"], a["coeffs_host"],
                                  a["coeffs_dev"], a["coeff_words"], a["workspace"], a["workspace_bytes"], a["out"], a["size"],
                                  a["out_dtype"], None)


def fresh(mode="pad"):
    return pp.clip_batch_plan([(50, 71), (1201, 1600)], mode, 336, ref.BACKGROUND)


def refused(msg, plan=None, **over):
    assert call(plan or fresh(), **over) == E
    assert msg in _capi.last_error(), _capi.last_error()


def test_capi_refuses_bad_pointers_and_sizes_before_any_launch():
    for name in ("plan_host", "plan_dev", "pixels", "lut", "coeffs_host", "coeffs_dev", "workspace", "out"):
        refused("NULL pointer", **{name: None})
    for name, bad in (("plan_dev", FAKE + 4), ("lut", FAKE + 2), ("coeffs_dev", FAKE + 2), ("workspace", FAKE + 8), ("out", FAKE + 8)):
        refused("aligned", **{name: bad})
    refused("n_images = 0", n=0)
    refused("n_images = 70000", n=70000)
    refused("pixel_bytes = 3 must be at least 4", pixel_bytes=3)
    refused("coeff_words = 0", coeff_words=0)
    refused("workspace_bytes = 0", workspace_bytes=0)
    for size in (0, -8, 100, 340):
        refused(f"size = {size} must be a multiple of 8", size=size)
    refused("out_dtype 9", out_dtype=9)


def mutated(field, value, image=0, mode="pad"):
    plan = fresh(mode)
    plan.images[image][field] = value
    return plan


def test_capi_refuses_every_bad_plan_entry_by_name():
    refused("H = 0, W = 71 must be positive", mutated("H", 0))
    refused("W = -1 must be positive", mutated("W", -1))
    refused("exceeds the supported maximum of 16384 pixels per side", mutated("H", 16385))
    refused("exceeds the supported maximum of 16384 pixels per side", mutated("W", 20000, 1))
    refused("mode 2", mutated("mode", 2))
    refused("does not describe a 50 x 71 image", mutated("in_h", 70))
    refused("does not describe a 50 x 71 image", mutated("pad_top", 22))
    refused("does not describe a 50 x 71 image", mutated("pad_left", 1, mode="square"))
    refused("crop window", mutated("crop_top", 1))
    refused("crop window", mutated("out_w", 335))
    refused("taps", mutated("ksize_h", 7))
    refused("workspace rows [0, 0 + 72) lie outside [0, 71)", mutated("rows", 72))
    refused("row_stride 212 < 3 * W = 213", mutated("row_stride", 212))
    refused("lie outside pixels", mutated("src_offset", -1))
    refused("lie outside pixels", pixel_bytes=fresh().pixel_bytes - 1)          # the last image ends exactly at the buffer's end
    assert call(fresh(), pixel_bytes=fresh().pixel_bytes, size=336, out_dtype=9) == E and "out_dtype" in _capi.last_error()
    # tables: in plan order, none overlapping the one before it, all inside coeffs
    p = fresh()
    refused("table bounds_h at word", mutated("bounds_h", int(p.images[0]["bounds_h"]) - 1))
    refused("table kk_h at word", mutated("kk_h", int(p.images[1]["kk_h"]) - 1, 1))
    refused("table kk_v at word", mutated("kk_v", 0, 1))
    refused("table bounds_v, words", mutated("bounds_v", p.coeffs.size - 671, 1))
    refused("lies outside coeffs", coeff_words=p.coeffs.size - 1)
    # workspace slices: aligned, in plan order, none overlapping the one before it, all inside the workspace
    refused("ws_offset 8 must be a multiple of 16", mutated("ws_offset", 8))
    refused("workspace slice at", mutated("ws_offset", int(p.images[1]["ws_offset"]) - 16, 1))
    refused("lies outside workspace", workspace_bytes=p.workspace_bytes - 16)
    refused("lies outside workspace", mutated("ws_offset", -16))


def test_capi_refuses_tap_ranges_outside_the_source():
    for table, which, value, msg in (("bounds_h", 0, -1, "horizontal taps"), ("bounds_h", 0, 70, "horizontal taps"),
                                     ("bounds_h", 1, 6, "horizontal taps"), ("bounds_h", 1, -1, "horizontal taps"),
                                     ("bounds_v", 0, 71, "vertical taps"), ("bounds_v", 1, 6, "vertical taps"),
                                     ("bounds_v", 0, -1, "vertical taps")):
        plan = fresh()
        plan.coeffs[int(plan.images[0][table]) + 2 * 200 + which] = value
        refused(msg, plan)
    # square mode resamples a band of rows only: a vertical tap above the band is outside the workspace
    plan = pp.clip_batch_plan([(2000, 500)], "square")
    plan.coeffs[int(plan.images[0]["bounds_v"])] -= 1
    refused("lie outside the workspace rows", plan)


def test_workspace_bytes_through_the_capi():
    lib = _capi.load_library()
    plan = fresh()
    assert lib.tp_clip_preprocess_workspace_bytes(plan.images.ctypes.data, 2, 336) == plan.workspace_bytes
    assert plan.workspace_bytes == -(-71 * 336 * 3 // 16) * 16 + -(-1600 * 336 * 3 // 16) * 16
    assert lib.tp_clip_preprocess_workspace_bytes(None, 2, 336) == 0 and "NULL" in _capi.last_error()
    assert lib.tp_clip_preprocess_workspace_bytes(plan.images.ctypes.data, 2, 12) == 0 and "multiple of 8" in _capi.last_error()
    assert lib.tp_clip_preprocess_workspace_bytes(mutated("H", 16385).images.ctypes.data, 2, 336) == 0
    assert "supported maximum" in _capi.last_error()


class FakeDeviceImage(torch.Tensor):
    """A CPU tensor that claims to live on a device: enough for the placement check, which runs before anything touches a GPU."""
    is_cuda = True


def test_python_interface_refusals():
    assert _capi.clip_preprocess_supported()
    img = np.zeros((4, 5, 3), dtype=np.uint8)
    with pytest.raises(ValueError, match="hd.slice_images"):
        pp.preprocess_images([img], "slice")
    with pytest.raises(ValueError, match="hd.slice_images"):
        pp.preprocess_plan([(4, 5)], "slice")
    with pytest.raises(ValueError, match="supported maximum of 16384"):
        pp.preprocess_images([np.zeros((1, 16385, 3), dtype=np.uint8)], "pad")
    with pytest.raises(ValueError, match="supported maximum of 16384"):
        pp.preprocess_images([np.zeros((16385, 1, 3), dtype=np.uint8)])
    with pytest.raises(ValueError, match="all be on the CPU or all on one device"):
        pp.preprocess_images([torch.zeros(4, 5, 3, dtype=torch.uint8), torch.zeros(4, 5, 3, dtype=torch.uint8).as_subclass(FakeDeviceImage)])
    with pytest.raises(TypeError):
        pp.preprocess_images(img)
    with pytest.raises(TypeError):
        pp.preprocess_images([img.astype(np.float32)])
    with pytest.raises(TypeError):
        pp.preprocess_images([img], dtype=torch.float64)
    with pytest.raises(ValueError):
        pp.preprocess_images([])
    with pytest.raises(ValueError):
        pp.preprocess_images([img[:, :, :2]])
    with pytest.raises(ValueError, match="multiple of 8"):
        pp.preprocess_images([img], size=100)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            pp.preprocess_images([img])
