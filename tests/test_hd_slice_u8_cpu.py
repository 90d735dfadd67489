"""HD slicing from uint8 images (hd.slice_images / tp_hd_slice_u8) without a GPU.

The yardstick for the normalisation: ``Compose([ToTensor(), Normalize(mean, std)])`` as tests/hd_slice_ref.py restates it — true
fp32 divisions, in that order.  ``hd.normalisation_table`` must equal it on all 768 (channel, byte) pairs, bit for bit, and each of
two wrong recipes is shown to differ from it: a kernel (or a table) built on one of them fails the bit-exact GPU cases of
tests/test_gpu_hd_slice_u8.py.  The reference helper itself is shown exact on the identity cases those tests rely on.

The host side: the batch plan (offsets, strides, crop ranges, the crop-to-image index), the argument errors of ``slice_images``, and
every refusal of ``tp_hd_slice_u8`` through the C ABI on fake pointers, before a device is touched."""
import ctypes

import numpy as np
import pytest
import torch

from tests import hd_slice_ref as ref
from tokenpacker_amd import _capi, hd

E = _capi.TP_ERR_INVALID_ARG


# ---- the normalisation table -----------------------------------------------------------------------------------------------------
def all_bytes_image() -> torch.Tensor:
    """[1, 256, 3] uint8: byte value u in every channel of pixel u."""
    return torch.arange(256, dtype=torch.uint8).view(1, 256, 1).expand(1, 256, 3).contiguous()


def table(recipe: str = "true_division", mean=hd.CLIP_MEAN, std=hd.CLIP_STD) -> torch.Tensor:
    """[3, 256] fp32 by one of the named recipes; ``true_division`` is the reference's."""
    u = torch.arange(256)
    m, s = torch.tensor(mean, dtype=torch.float32), torch.tensor(std, dtype=torch.float32)
    if recipe == "true_division":
        return ref.to_tensor_normalize(all_bytes_image(), mean, std)[:, 0, :]
    if recipe == "reciprocal":                   # u * fl(1 / 255) and * fl(1 / std): what a kernel that "does no division" would do
        return (u.to(torch.float32) * torch.tensor(1.0, dtype=torch.float32).div(255)).sub(m[:, None]) * (1.0 / s)[:, None]
    if recipe == "fp64_then_round":              # the exact quotient rounded once
        return ((u.double() / 255 - m.double()[:, None]) / s.double()[:, None]).float()
    raise AssertionError(recipe)


WRONG = ("reciprocal", "fp64_then_round")


def test_normalisation_table_is_the_reference_arithmetic_on_all_768_entries():
    t = hd.normalisation_table()
    assert t.shape == (3, 256) and t.dtype == torch.float32 and t.is_contiguous()
    assert torch.equal(t.view(torch.int32), table().view(torch.int32))
    other = ((0.5, 0.25, 0.125), (0.3, 0.7, 1.9))
    assert torch.equal(hd.normalisation_table(*other).view(torch.int32), table("true_division", *other).view(torch.int32))
    with pytest.raises(ValueError):
        hd.normalisation_table((0.5, 0.5), (1.0, 1.0, 1.0))
    with pytest.raises(ValueError):
        hd.normalisation_table((0.5, 0.5, 0.5), (1.0, 0.0, 1.0))


@pytest.mark.parametrize("recipe", WRONG)
def test_each_wrong_recipe_differs_from_the_table(recipe):
    """Otherwise the bit-exact GPU cases could not tell the recipes apart.  Each differs in every channel, by at most a few ulps."""
    right, wrong = table(), table(recipe)
    for c in range(3):
        assert bool((right[c].view(torch.int32) != wrong[c].view(torch.int32)).any()), f"{recipe} does not show in channel {c}"
    assert float((right - wrong).abs().max()) < 2e-6


def test_the_restated_to_tensor_divides_truly():
    """``div(255)`` on the CPU is a true division: fl(u / 255), the correctly rounded quotient."""
    u = torch.arange(256)
    assert torch.equal(u.to(torch.float32).div(255), (u.double() / 255).float())


# ---- the reference helper on the identity cases ----------------------------------------------------------------------------------
IDENTITY = [(336, 336, 1, 1), (336, 1008, 1, 3), (672, 1008, 2, 3), (1008, 1008, 3, 3)]


def identity_expectation(u8: torch.Tensor, hb: int, wb: int, block: int = 336) -> torch.Tensor:
    """What the loader makes of an image that needs no resize: tiles of the normalised image, and — more than one crop — the
    stride-3 pick ``n[:, 1::3, 1::3]`` (``src = 3 d + 1``, weight exactly 1) in the top-left corner of a zero block."""
    n = ref.to_tensor_normalize(u8)
    tiles = [n[:, block * i:block * (i + 1), block * j:block * (j + 1)] for i in range(hb) for j in range(wb)]
    if len(tiles) > 1:
        view = torch.zeros(3, block, block)
        pick = n[:, 1::3, 1::3]
        view[:, :pick.shape[1], :pick.shape[2]] = pick
        tiles.append(view)
    return torch.stack(tiles)


@pytest.mark.parametrize("h,w,hb,wb", IDENTITY)
def test_reference_helper_is_exact_on_the_identity_cases(h, w, hb, wb):
    u8 = ref.random_image(h, w)
    want, got_hb, got_wb = ref.slice_reference(u8)
    assert (got_hb, got_wb) == (hb, wb)
    assert hd.slice_plan(h, w)[2:4] == (h, w)                                   # no resize
    assert torch.equal(want.view(torch.int32), identity_expectation(u8, hb, wb).view(torch.int32))


# ---- the batch plan --------------------------------------------------------------------------------------------------------------
def test_plan_record_has_the_c_struct_layout():
    assert hd._PLAN_IMAGE.itemsize == ctypes.sizeof(_capi.tp_hd_slice_image) == 48
    for name, _ in _capi.tp_hd_slice_image._fields_:
        assert hd._PLAN_IMAGE.fields[name][1] == getattr(_capi.tp_hd_slice_image, name).offset, name


def test_batch_plan_offsets_strides_and_crop_ranges():
    sizes = [(336, 336), (500, 700), (37, 2000), (1, 1), (2000, 37)]
    plan = hd.slice_batch_plan(sizes)
    first = at = 0
    for i, ((H, W), rec) in enumerate(zip(sizes, plan.images)):
        hb, wb, h_res, w_res, hg, wg = hd.slice_plan(H, W)
        assert tuple(rec)[1:] == (H, W, 3 * W, hb, wb, h_res, w_res, hg, wg, first)
        assert rec["src_offset"] == at and at % 16 == 0
        count = hd.hd_crop_count(hb, wb)
        assert list(plan.crop_image[first:first + count]) == [i] * count
        assert (plan.h_block[i], plan.w_block[i]) == (hb, wb)
        first += count
        at += -(-H * W * 3 // 16) * 16
    assert plan.n_crops == first == plan.crop_image.size and plan.pixel_bytes == at and plan.crop_image.dtype == np.int32
    assert plan.words().size == 48 * len(sizes) + 4 * first
    # given strides and offsets (images read in place): kept as given, the buffer ends behind the last byte addressed
    plan = hd.slice_batch_plan([(10, 20), (5, 5)], row_strides=[100, 15], offsets=[7, 2000])
    assert [int(r["src_offset"]) for r in plan.images] == [7, 2000] and [int(r["row_stride"]) for r in plan.images] == [100, 15]
    assert plan.pixel_bytes >= 2000 + 4 * 15 + 15
    with pytest.raises(ValueError):
        hd.slice_batch_plan([(10, 20)], row_strides=[59])
    with pytest.raises(ValueError):
        hd.slice_batch_plan([])
    with pytest.raises(ValueError):
        hd.slice_batch_plan([(0, 5)])
    with pytest.raises(ValueError, match="elongated"):                         # the global view would be 24 x 0: F.interpolate refuses it
        hd.slice_batch_plan([(100, 1)], block=24)


def test_batch_plan_of_70_images_passes_the_library_validation_as_far_as_a_host_can_tell():
    """70 small images, block 24: the plan the Python side builds is one the C validation accepts — the call gets past every plan
    check and is refused only for the one thing made wrong on purpose (out_dtype), named in the message."""
    g = torch.Generator().manual_seed(70)
    sizes = [(int(h), int(w)) for h, w in torch.randint(3, 101, (70, 2), generator=g)]     # (3: no resized side rounds to 0)
    plan = hd.slice_batch_plan(sizes, patch_num=9, block=24)
    assert len(plan.images) == 70 and plan.n_crops == sum(hd.hd_crop_count(h, w) for h, w in zip(plan.h_block, plan.w_block))
    assert len({(h, w) for h, w in zip(plan.h_block, plan.w_block)}) > 5               # many different grids
    ends = [int(r["first_crop"]) for r in plan.images] + [plan.n_crops]
    assert all(b - a == hd.hd_crop_count(h, w) for a, b, h, w in zip(ends, ends[1:], plan.h_block, plan.w_block))
    words = plan.words()
    lib = _capi.load_library()
    fake = ctypes.c_void_p(4096)
    rc = lib.tp_hd_slice_u8(words.ctypes.data, fake, 70, fake, plan.pixel_bytes, fake, fake, plan.n_crops, 24, 7, None)
    assert rc == E and "out_dtype" in _capi.last_error()
    rc = lib.tp_hd_slice_u8(words.ctypes.data, fake, 70, fake, plan.pixel_bytes - 16, fake, fake, plan.n_crops, 24, _capi.TP_BF16, None)
    assert rc == E and "image 69" in _capi.last_error() and "outside pixels" in _capi.last_error()


# ---- slice_images' argument errors -----------------------------------------------------------------------------------------------
def test_slice_images_argument_errors_come_before_the_device():
    ok = np.zeros((4, 5, 3), dtype=np.uint8)
    with pytest.raises(ValueError, match="empty"):
        hd.slice_images([])
    with pytest.raises(TypeError):
        hd.slice_images(ok)                                                        # one image, not a sequence
    with pytest.raises(TypeError):
        hd.slice_images(["picture.png"])
    with pytest.raises(TypeError, match="uint8"):
        hd.slice_images([ok.astype(np.float32)])
    with pytest.raises(TypeError, match="uint8"):
        hd.slice_images([torch.zeros(4, 5, 3)])
    with pytest.raises(ValueError, match=r"\[H, W, 3\]"):
        hd.slice_images([np.zeros((3, 4, 5), dtype=np.uint8)])                     # channels first
    with pytest.raises(ValueError, match=r"\[H, W, 3\]"):
        hd.slice_images([np.zeros((4, 5), dtype=np.uint8)])                        # grey
    with pytest.raises(ValueError, match=r"\[H, W, 3\]"):
        hd.slice_images([np.zeros((4, 5, 4), dtype=np.uint8)])                     # RGBA
    with pytest.raises(ValueError):
        hd.slice_images([np.zeros((0, 5, 3), dtype=np.uint8)])
    with pytest.raises(TypeError, match="dtype"):
        hd.slice_images([ok], dtype=torch.float64)
    with pytest.raises(ValueError, match="multiple of 8"):
        hd.slice_images([ok], block=20)
    with pytest.raises(ValueError):
        hd.slice_images([ok], mean=(0.5, 0.5))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            hd.slice_images([ok])


# ---- the C ABI refuses bad calls on the host -------------------------------------------------------------------------------------
def _image(**kw):
    """A valid one-image plan entry (500 x 700 in a 2 x 3 grid of 336-pixel blocks), with fields replaced."""
    d = dict(src_offset=0, H=500, W=700, row_stride=2100, h_block=2, w_block=3, h_res=672, w_res=941, hg=240, wg=336, first_crop=0)
    d.update(kw)
    return _capi.tp_hd_slice_image(**d)


def _plan(images, owners):
    """The plan words: records, then the crop-to-image index."""
    buf = ctypes.create_string_buffer(48 * len(images) + 4 * len(owners))
    for i, im in enumerate(images):
        ctypes.memmove(ctypes.addressof(buf) + 48 * i, ctypes.byref(im), 48)
    idx = (ctypes.c_int32 * len(owners))(*owners)
    ctypes.memmove(ctypes.addressof(buf) + 48 * len(images), idx, 4 * len(owners))
    return buf


def test_library_loads_and_declares_the_symbol_without_a_gpu():
    lib = _capi.load_library()
    assert _capi.hd_slice_u8_supported() and "tp_hd_slice_u8" in _capi.EXPORTED_SYMBOLS and hasattr(lib, "tp_hd_slice_u8")
    assert hasattr(_capi.load_test_library(), "tp_hd_slice_u8")


def test_tp_hd_slice_u8_refuses_every_invalid_argument_on_the_host():
    lib = _capi.load_library()
    p, odd = 4096, 4100                                   # fake device pointers: aligned | 4 bytes off; never dereferenced
    nbytes = 499 * 2100 + 2100
    one = _plan([_image()], [0] * 7)

    def call(plan=one, plan_dev=p, n_images=1, pixels=p, pixel_bytes=nbytes, lut=p, crops=p, n_crops=7, block=336,
             dt=_capi.TP_BF16):
        return lib.tp_hd_slice_u8(plan, plan_dev, n_images, pixels, pixel_bytes, lut, crops, n_crops, block, dt, None)

    def refused(match, **kw):
        assert call(**kw) == E, kw
        assert match in _capi.last_error(), (_capi.last_error(), kw)

    # pointers, sizes, block, dtype
    for name in ("plan", "plan_dev", "pixels", "lut", "crops"):
        refused("NULL", **{name: None})
    refused("aligned", plan_dev=odd)
    refused("aligned", crops=4096 + 8)
    refused("aligned", lut=4096 + 2)
    refused("positive", n_images=0)
    refused("positive", n_crops=0)
    refused("pixel_bytes", pixel_bytes=0)
    refused("pixel_bytes", pixel_bytes=7)
    for block in (0, -8, 20, 4):
        refused("block", block=block)
    for dt in (-1, 3, 7):
        refused("out_dtype", dt=dt)
    # the image inside pixels: src_offset + (H - 1) * row_stride + 3 W <= pixel_bytes
    refused("outside pixels", pixel_bytes=nbytes - 1)
    refused("outside pixels", plan=_plan([_image(src_offset=1)], [0] * 7))
    refused("outside pixels", plan=_plan([_image(src_offset=-1)], [0] * 7))
    refused("outside pixels", plan=_plan([_image(row_stride=2101)], [0] * 7))
    refused("row_stride", plan=_plan([_image(row_stride=2099)], [0] * 7))
    refused("positive", plan=_plan([_image(H=0)], [0] * 7))
    refused("positive", plan=_plan([_image(W=-1)], [0] * 7))
    # sizes against the grid
    refused("grid", plan=_plan([_image(h_block=0)], [0] * 7))
    refused("does not fit", plan=_plan([_image(h_res=673)], [0] * 7))
    refused("does not fit", plan=_plan([_image(w_res=1009)], [0] * 7))
    refused("does not fit", plan=_plan([_image(h_res=0)], [0] * 7))
    refused("global view", plan=_plan([_image(hg=337)], [0] * 7))
    refused("global view", plan=_plan([_image(wg=337)], [0] * 7))
    refused("global view", plan=_plan([_image(hg=0, wg=0)], [0] * 7))                                   # several crops need one
    single = dict(H=336, W=336, row_stride=1008, h_block=1, w_block=1, h_res=336, w_res=336, hg=0, wg=0)
    assert call(plan=_plan([_image(**single)], [0]), n_crops=1, dt=9) == E and "out_dtype" in _capi.last_error()   # (the entry itself is fine)
    refused("global view", plan=_plan([_image(**dict(single, hg=336, wg=336))], [0]), n_crops=1)     # one crop has none
    # crop ranges: in order, disjoint, summing to n_crops; the index agrees with them
    two = [_image(), _image(**dict(single, first_crop=7))]
    assert call(plan=_plan(two, [0] * 7 + [1]), n_images=2, n_crops=8, dt=9) == E and "out_dtype" in _capi.last_error()
    refused("overlaps", plan=_plan([_image(), _image(**dict(single, first_crop=6))], [0] * 7 + [1]), n_images=2, n_crops=8)
    refused("gap", plan=_plan([_image(), _image(**dict(single, first_crop=8))], [0] * 7 + [1, 1]), n_images=2, n_crops=9)
    refused("gap", plan=_plan([_image(first_crop=1)], [0] * 8), n_crops=8)
    refused("crops up to 8 of 7", plan=_plan(two, [0] * 7 + [1]), n_images=2, n_crops=7)
    refused("describes 7 crops", n_crops=8, plan=_plan([_image()], [0] * 8))
    refused("mapped to image", plan=_plan(two, [0] * 6 + [1, 1]), n_images=2, n_crops=8)
    refused("mapped to image", plan=_plan([_image()], [0] * 6 + [-1]))
