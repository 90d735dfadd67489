"""CLIP preprocessing of the pad / square image modes on a real MI355X: preprocess.preprocess_images / tp_clip_preprocess against
the model of tests/clip_preprocess_ref.py (shown equal to Pillow and to the reference's ``process_images`` by the CPU tests) and,
directly, against the digests of the reference's ``pixel_values`` in tests/golden/clip_preprocess.npz.

Everything here is bit for bit — there is no tolerance in this file: Pillow's 8-bit resize is integer arithmetic, and a wrongly
rounded coefficient moves a byte by one.  Needs neither PIL nor transformers.  Expected values and the fp32 device results of the
single-image calls are computed once per case and shared."""
from functools import lru_cache

import numpy as np
import pytest
import torch

from tests import clip_preprocess_ref as ref
from tokenpacker_amd import hd
from tokenpacker_amd import preprocess as pp

pytestmark = pytest.mark.gpu

# the smallest sizes at which each part can go wrong: no pass at all; crop only; barely resized (5 and 7 taps); upscale; both paste
# directions with an odd offset; one-pixel sides; a 100 800-pixel resized width with the window in its middle; a narrow tall image; a
# 4.8-fold (23 taps) and a 7.4-fold (about 33 taps) downscale
SIZES = [(336, 336), (336, 500), (337, 500), (335, 336), (40, 39), (5, 5), (50, 71), (71, 50), (1, 37), (37, 1), (3, 900), (1000, 41),
         (1201, 1600), (2500, 700)]
MODES = ("square", "pad")
SEED = 7                              # the golden's seed: every (size, mode) here is a golden case


def image(h, w):
    return ref.test_image(h, w, SEED)


def want(h, w, mode):
    return torch.tensor(ref.expected(h, w, mode, SEED))                 # (a copy: the cached array is read-only)


@lru_cache(maxsize=None)
def got_f32(h, w, mode):
    """The fp32 result of the single-image call, on the CPU — never modified by a test."""
    out = pp.preprocess_images([image(h, w)], mode, dtype=torch.float32)
    torch.cuda.synchronize()
    assert out.shape == (1, 3, 336, 336) and out.dtype == torch.float32
    return out[0].cpu()


def bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def golden_digest(h, w, mode):
    g = ref.golden()
    for case, d in zip(g["cases"], g["output_sha256"]):
        if tuple(int(v) for v in case) == (h, w, MODES.index(mode), SEED):
            return str(d)
    raise AssertionError((h, w, mode))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("h,w", SIZES)
def test_fp32_output_is_the_reference_bit_for_bit(h, w, mode):
    got = got_f32(h, w, mode)
    assert torch.equal(bits(got), bits(want(h, w, mode)))
    assert ref.digest(got.numpy()) == golden_digest(h, w, mode)          # the reference's own pixel_values


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("h,w", SIZES)
def test_16_bit_output_is_the_reference_rounded_once(h, w, mode):
    for dtype in (torch.bfloat16, torch.float16):
        out = pp.preprocess_images([image(h, w)], mode, dtype=dtype)
        torch.cuda.synchronize()
        assert out.dtype == dtype and out.shape == (1, 3, 336, 336)
        assert torch.equal(bits(out[0].cpu()), bits(want(h, w, mode).to(dtype)))


@pytest.mark.parametrize("mode", MODES)
def test_a_batch_of_all_sizes_equals_the_single_image_calls(mode):
    """Two launches for the whole batch; images of 1 to 2500 rows share the grid."""
    out = pp.preprocess_images([image(h, w) for h, w in SIZES], mode, dtype=torch.float32)
    torch.cuda.synchronize()
    assert out.shape == (len(SIZES), 3, 336, 336)
    out = out.cpu()
    for i, (h, w) in enumerate(SIZES):
        assert torch.equal(bits(out[i]), bits(got_f32(h, w, mode))), (h, w)


def test_the_two_modes_back_to_back_on_one_stream():
    """The mode is per call: two calls in a row without a synchronise between them (each owns its workspace) equal the single calls."""
    some = [(50, 71), (1201, 1600), (3, 900), (336, 336)]
    a = pp.preprocess_images([image(h, w) for h, w in some], "pad", dtype=torch.float32)
    b = pp.preprocess_images([image(h, w) for h, w in some], "square", dtype=torch.float32)
    c = pp.preprocess_images([image(h, w) for h, w in some], None, dtype=torch.float32)     # train.py's default: not 'pad'
    torch.cuda.synchronize()
    for i, (h, w) in enumerate(some):
        assert torch.equal(bits(a[i].cpu()), bits(got_f32(h, w, "pad")))
        assert torch.equal(bits(b[i].cpu()), bits(got_f32(h, w, "square")))
        assert torch.equal(bits(c[i].cpu()), bits(got_f32(h, w, "square")))


PLACED = [(71, 50), (337, 500), (1000, 41), (1, 37), (37, 1)]                  # the last one: 111 bytes, an odd count


@pytest.mark.parametrize("mode", MODES)
def test_device_resident_and_strided_input_equal_the_dense_cpu_input(mode):
    dev = torch.device("cuda", torch.cuda.current_device())
    dense = [torch.from_numpy(image(h, w)).to(dev) for h, w in PLACED]
    wide = []
    for h, w in PLACED:                                                         # rows of a view into a wider buffer
        buf = np.full((h, w + 5, 3), 77, dtype=np.uint8)
        buf[:, 2:2 + w] = image(h, w)
        wide.append(buf)
    legs = dict(device=dense,
                device_strided=[torch.from_numpy(b).to(dev)[:, 2:2 + w] for b, (h, w) in zip(wide, PLACED)],
                cpu_strided_numpy=[b[:, 2:2 + w] for b, (h, w) in zip(wide, PLACED)],
                cpu_strided_torch=[torch.from_numpy(b)[:, 2:2 + w] for b, (h, w) in zip(wide, PLACED)])
    assert not legs["device_strided"][0].is_contiguous() and not legs["cpu_strided_numpy"][0].flags["C_CONTIGUOUS"]
    for name, imgs in legs.items():
        out = pp.preprocess_images(imgs, mode, dtype=torch.float32)
        torch.cuda.synchronize()
        assert out.device == dev
        for i, (h, w) in enumerate(PLACED):
            assert torch.equal(bits(out[i].cpu()), bits(got_f32(h, w, mode))), (name, h, w)


@pytest.mark.parametrize("mode", MODES)
def test_an_image_that_ends_exactly_at_the_end_of_the_pixel_buffer(mode):
    """Device images are packed byte by byte, so the last one — (37, 1), 111 bytes — ends where `pixels` ends and the 4-byte load
    of its last pixel is the one that is moved down; staged CPU images end on the buffer's end when their size is a multiple of 16."""
    dev = torch.device("cuda", torch.cuda.current_device())
    order = [(40, 39), (37, 1)]
    out = pp.preprocess_images([torch.from_numpy(image(h, w)).to(dev) for h, w in order], mode, dtype=torch.float32)
    staged = [(5, 5), (336, 336)]
    plan = pp.clip_batch_plan(staged, mode)
    assert int(plan.images[-1]["src_offset"]) + 336 * 336 * 3 == plan.pixel_bytes
    out2 = pp.preprocess_images([image(h, w) for h, w in staged], mode, dtype=torch.float32)
    torch.cuda.synchronize()
    for got, sizes in ((out, order), (out2, staged)):
        for i, (h, w) in enumerate(sizes):
            assert torch.equal(bits(got[i].cpu()), bits(got_f32(h, w, mode))), (h, w)


def test_result_is_what_the_tower_call_takes():
    out = pp.preprocess_images([image(50, 71), image(40, 39)], "pad")
    torch.cuda.synchronize()
    assert out.shape == (2, 3, 336, 336) and out.dtype == torch.bfloat16 and out.is_cuda and out.is_contiguous()
    assert out[1].shape == (3, 336, 336) and out[1].is_contiguous() and out[1].data_ptr() % 16 == 0
    other = pp.preprocess_images([image(5, 5)], "pad", size=24, dtype=torch.float16, mean=(0.5, 0.5, 0.5), std=(0.5, 0.25, 1.0),
                                 background=(1, 2, 3))
    torch.cuda.synchronize()
    assert other.shape == (1, 3, 24, 24) and other.dtype == torch.float16
    table = hd.normalisation_table((0.5, 0.5, 0.5), (0.5, 0.25, 1.0)).numpy()
    expect = torch.from_numpy(ref.normalise(ref.preprocess_bytes(image(5, 5), "pad", 24, (1, 2, 3)), table)).to(torch.float16)
    assert torch.equal(bits(other[0].cpu()), bits(expect))
