"""HD slicing from uint8 images on a real MI355X: hd.slice_images / tp_hd_slice_u8 against the reference's loader as
tests/hd_slice_ref.py restates it (ToTensor + Normalize in torch on the CPU, then oracle.hd_oracle.slice_image).

Bit-exact where the loader's own arithmetic is exact (images that need no resize: every weight is 0 or 1, the global view a
stride-3 pick), within the bar tests/test_gpu_hd.py sets for the resize arithmetic elsewhere, and bit-identical between a batch and
its images sliced one by one.  References and fp32 device results are computed once per size and shared."""
from functools import lru_cache

import numpy as np
import pytest
import torch

from tests import hd_slice_ref as ref
from tokenpacker_amd import hd

pytestmark = pytest.mark.gpu

IDENTITY = [(336, 336), (336, 1008), (672, 1008), (1008, 1008)]
GENERAL = [(500, 700), (901, 413), (300, 1400), (37, 2000), (2000, 37), (200, 150), (1, 1), (3, 5), (1, 640), (640, 1)]
SMALL_BLOCK = dict(patch_num=9, block=24)


@lru_cache(maxsize=None)
def want(h, w, block=336):
    """(image, reference crops fp32, h_block, w_block) — never modified by a test."""
    u8 = ref.random_image(h, w)
    crops, hb, wb = ref.slice_reference(u8, 9, block)
    return u8, crops, hb, wb


@lru_cache(maxsize=None)
def got_f32(h, w, block=336):
    """The fp32-mode result of the single-image call, on the CPU."""
    crops, hb, wb = hd.slice_images([want(h, w, block)[0]], patch_num=9, block=block, dtype=torch.float32)
    torch.cuda.synchronize()
    assert (hb, wb) == ([want(h, w, block)[2]], [want(h, w, block)[3]])
    return crops.cpu()


def bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def within_the_resize_bar(got, expect):
    """tests/test_gpu_hd.py:52 — a few fp32 ulps of the pixel range (torch's vectorised CPU kernel contracts a*b + c*d
    differently from the device), and the identical zero pattern."""
    assert got.shape == expect.shape and got.dtype == torch.float32
    err = (got - expect).abs().max().item()
    print(f"max |got - want| = {err:.3e}  bound = {4e-6 * max(1.0, expect.abs().max().item()):.3e}")
    assert err <= 4e-6 * max(1.0, expect.abs().max().item()), err
    assert torch.equal(got == 0, expect == 0)


# ---- 1. bit-exact identity cases -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", IDENTITY)
def test_identity_cases_are_bit_exact_in_every_dtype(h, w):
    """No resize: crops are tiles of the normalised image, the global view is n[:, 1::3, 1::3] plus zeros — fp32 output equals the
    helper bit for bit (a table built on another recipe, a wrong tap or a wrong channel fails here), 16-bit output its .to(dtype)."""
    u8, expect, hb, wb = want(h, w)
    assert hd.slice_plan(h, w)[2:4] == (h, w)
    assert torch.equal(bits(got_f32(h, w)), bits(expect))
    for dtype in (torch.bfloat16, torch.float16):
        crops, ghb, gwb = hd.slice_images([u8], dtype=dtype)
        torch.cuda.synchronize()
        assert crops.dtype == dtype and (ghb, gwb) == ([hb], [wb])
        assert torch.equal(bits(crops.cpu()), bits(expect.to(dtype)))


# ---- 2. general sizes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", GENERAL)
def test_general_sizes_against_the_reference_helper(h, w):
    within_the_resize_bar(got_f32(h, w), want(h, w)[1])


@pytest.mark.parametrize("h,w", GENERAL)
def test_general_sizes_equal_slice_image_on_the_normalised_image(h, w):
    """The same taps and the same blend on the same fp32 values as tp_hd_slice, under the same bar.  Measured: the two are NOT
    bit-equal — the compiler contracts the blend's products and sums into other fused multiply-adds in the two kernels; the largest
    difference on these cases is one fp32 ulp of the pixel range (2.4e-7), as against the helper — so the bar is what is asserted."""
    u8 = want(h, w)[0]
    old, hb, wb = hd.slice_image(ref.to_tensor_normalize(u8).cuda())
    torch.cuda.synchronize()
    assert (hb, wb) == want(h, w)[2:]
    within_the_resize_bar(got_f32(h, w), old.cpu())


# ---- 3. 16-bit output ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("h,w", GENERAL)
def test_16_bit_output_is_the_fp32_output_rounded_once(h, w, dtype):
    crops, _, _ = hd.slice_images([want(h, w)[0]], dtype=dtype)
    torch.cuda.synchronize()
    assert crops.dtype == dtype and torch.equal(bits(crops.cpu()), bits(got_f32(h, w).to(dtype)))


# ---- 4. batches ------------------------------------------------------------------------------------------------------------------
def ranges_equal_single_calls(batch_crops, sizes, block=336):
    first = 0
    for h, w in sizes:
        single = got_f32(h, w, block)
        assert torch.equal(bits(batch_crops[first:first + single.shape[0]]), bits(single)), (h, w)
        first += single.shape[0]
    assert first == batch_crops.shape[0]


def test_mixed_grids_in_one_call():
    sizes = [(336, 336), (37, 2000), (2000, 37), (500, 700), (1008, 1008)]
    imgs = [want(h, w)[0] for h, w in sizes]
    crops, hb, wb = hd.slice_images(imgs, dtype=torch.float32)
    again, _, _ = hd.slice_images(imgs, dtype=torch.float32)
    torch.cuda.synchronize()
    assert list(zip(hb, wb)) == [(1, 1), (1, 9), (9, 1), (2, 3), (3, 3)]
    ranges_equal_single_calls(crops.cpu(), sizes)
    assert torch.equal(bits(crops), bits(again))                                  # two runs, identical bits
    lp, _, _ = hd.slice_images(imgs)                                              # the default dtype: bf16, one rounding
    torch.cuda.synchronize()
    assert lp.dtype == torch.bfloat16 and torch.equal(bits(lp.cpu()), bits(crops.cpu().to(torch.bfloat16)))


@lru_cache(maxsize=None)
def small_sizes():
    g = torch.Generator().manual_seed(24)
    return tuple((int(h), int(w)) for h, w in torch.randint(3, 101, (70, 2), generator=g))


def test_70_small_images_in_one_call():
    """block = 24 with patch_num = 9 on images of at most 100 pixels a side: several crops, padding inside a crop and a global view
    at the smallest size; 70 images in one plan."""
    sizes = small_sizes()
    imgs = [want(h, w, 24)[0] for h, w in sizes]
    crops, hb, wb = hd.slice_images(imgs, dtype=torch.float32, **SMALL_BLOCK)
    again, _, _ = hd.slice_images(imgs, dtype=torch.float32, **SMALL_BLOCK)
    torch.cuda.synchronize()
    assert len(set(zip(hb, wb))) > 5 and crops.shape[1:] == (3, 24, 24)
    ranges_equal_single_calls(crops.cpu(), sizes, 24)
    assert torch.equal(bits(crops), bits(again))


@pytest.mark.parametrize("h,w", [(50, 100), (100, 50), (100, 100), (7, 99), (24, 216), (61, 61)])
def test_small_block_against_the_reference_helper(h, w):
    expect = want(h, w, 24)[1]
    assert expect.shape[0] > 1 or (h, w) == (24, 24)
    within_the_resize_bar(got_f32(h, w, 24), expect)


def test_rows_with_a_stride_and_device_resident_inputs():
    """A column slice of a wider array (row_stride > 3 W) from the CPU and on the device, numpy arrays and tensors, and device inputs
    in a batch: all equal the dense CPU image's result, bit for bit."""
    sizes = [(200, 150), (3, 5), (500, 700)]
    wide = [torch.cat([ref.random_image(h, 7, 1), want(h, w)[0], ref.random_image(h, 4, 2)], dim=1) for h, w in sizes]
    views = [x[:, 7:7 + w] for x, (h, w) in zip(wide, sizes)]
    assert all(not v.is_contiguous() and torch.equal(v, want(h, w)[0]) for v, (h, w) in zip(views, sizes))
    for imgs in (views, [v.numpy() for v in views], [x.cuda()[:, 7:7 + w] for x, (h, w) in zip(wide, sizes)],
                 [want(h, w)[0].cuda() for h, w in sizes], [want(h, w)[0].cuda().permute(1, 0, 2).contiguous().permute(1, 0, 2) for h, w in sizes]):
        crops, _, _ = hd.slice_images(imgs, dtype=torch.float32)
        torch.cuda.synchronize()
        ranges_equal_single_calls(crops.cpu(), sizes)
    tiny, _, _ = hd.slice_images([want(1, 1)[0].cuda()], dtype=torch.float32)     # 3 bytes on the device: the buffer is padded to 8
    torch.cuda.synchronize()
    assert torch.equal(bits(tiny.cpu()), bits(got_f32(1, 1)))
    with pytest.raises(ValueError):
        hd.slice_images([want(3, 5)[0], want(3, 5)[0].cuda()])                    # mixed CPU / device


# ---- 5. the existing path --------------------------------------------------------------------------------------------------------
def test_slice_image_is_unchanged_by_the_new_path():
    """hd.slice_image before and after slice_images calls in the same process: the same bits (the two paths share no state), and
    still the oracle's values within the bar of tests/test_gpu_hd.py."""
    img = torch.randn(3, 300, 1400, generator=torch.Generator().manual_seed(300 * 7 + 1400))
    before, hb, wb = hd.slice_image(img.cuda())
    hd.slice_images([want(300, 1400)[0]])
    after, _, _ = hd.slice_image(img.cuda())
    torch.cuda.synchronize()
    assert torch.equal(bits(before), bits(after))
    from oracle import hd_oracle
    within_the_resize_bar(after.cpu(), hd_oracle.slice_image(img.unsqueeze(0), hb, wb))
