"""The model the CLIP-preprocessing tests compare against: Pillow's 8-bit bicubic resize restated in numpy / Python integers and
doubles (coefficients, the horizontal and the vertical uint8 pass), the reference's pad (``expand2square``), the processor's
shortest-edge resize and centre crop, and the normalisation as a table lookup.  No PIL, no transformers, no GPU: the CPU tests check
this model against Pillow and against ``tests/golden/clip_preprocess.npz`` (minted from the reference's ``process_images``), the
GPU tests check the kernels against this model.

Every floating-point step is an elementwise IEEE-double numpy operation in Pillow's order (numpy fuses nothing), the normalising
sum runs left to right over the taps, ``astype(int64)`` truncates towards zero as C's ``(int)`` does."""
import functools
import hashlib
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "clip_preprocess.npz")
PRECISION_BITS = 22
BACKGROUND = (122, 116, 104)          # tuple(int(m * 255) for m in CLIP mean)


def cubic(x):
    a = -0.5
    x = np.abs(x)
    inner = ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    outer = (((x - 5) * x + 8) * x - 4) * a
    return np.where(x < 1.0, inner, np.where(x < 2.0, outer, 0.0))


def resize_coeffs(in_size, out_size, first_out=0, n_out=None):
    """-> (kk int32 [n_out, ksize], bounds int32 [n_out, 2] = (xmin, xcount), ksize) for output positions
    [first_out, first_out + n_out) of Pillow's bicubic resize of ``in_size`` to ``out_size``."""
    n_out = out_size - first_out if n_out is None else n_out
    scale = np.float64(in_size) / np.float64(out_size)
    fs = max(scale, np.float64(1.0))
    support = 2.0 * fs
    ksize = int(np.ceil(support)) * 2 + 1
    xx = np.arange(first_out, first_out + n_out, dtype=np.float64)
    center = (xx + 0.5) * scale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)
    xmax = np.minimum((center + support + 0.5).astype(np.int64), in_size) - xmin
    ss = 1.0 / fs
    t = np.arange(ksize, dtype=np.int64)[None, :]
    live = t < xmax[:, None]
    w = np.where(live, cubic(((t + xmin[:, None]).astype(np.float64) - center[:, None] + 0.5) * ss), 0.0)
    ww = np.zeros(n_out, dtype=np.float64)
    for j in range(ksize):                                      # left to right (adding the 0.0 of a dead tap changes nothing)
        ww = ww + w[:, j]
    w = np.where((ww != 0.0)[:, None], w / np.where(ww != 0.0, ww, 1.0)[:, None], w)
    scaled = w * 4194304.0
    kk = np.where(w < 0, scaled - 0.5, scaled + 0.5).astype(np.int64)
    kk = np.where(live, kk, 0).astype(np.int32)
    return kk, np.stack([xmin, xmax], axis=1).astype(np.int32), ksize


def clip8(acc):
    return np.clip(acc >> PRECISION_BITS, 0, 255)               # numpy's >> on int64 is arithmetic


def resample_axis(src, kk, bounds, axis, sums=None):
    """One uint8 pass along ``axis`` (0: vertical, 1: horizontal) of ``src [h, w, 3]``; ``sums`` (a list) collects the raw
    accumulators' minimum and maximum, for the saturation check."""
    src = src.astype(np.int64)
    n = kk.shape[0]
    shape = (n, src.shape[1], 3) if axis == 0 else (src.shape[0], n, 3)
    out = np.empty(shape, dtype=np.uint8)
    for i in range(n):
        xmin, cnt = int(bounds[i, 0]), int(bounds[i, 1])
        k = kk[i, :cnt].astype(np.int64)
        if axis == 0:
            acc = (1 << (PRECISION_BITS - 1)) + np.tensordot(k, src[xmin:xmin + cnt], axes=(0, 0))
            out[i] = clip8(acc)
        else:
            acc = (1 << (PRECISION_BITS - 1)) + np.tensordot(src[:, xmin:xmin + cnt], k, axes=(1, 0))
            out[:, i] = clip8(acc)
        if sums is not None:
            sums.append((int(acc.min()), int(acc.max())))
    return out


def resize_u8(img, out_h, out_w, window=None, sums=None):
    """Pillow's ``Image.resize((out_w, out_h), BICUBIC)`` of ``img [h, w, 3]`` uint8, or only its ``window = (top, left, n_rows,
    n_cols)``: horizontal pass over the rows the vertical taps touch, rounded to uint8, then the vertical pass."""
    h, w = img.shape[:2]
    top, left, nr, nc = (0, 0, out_h, out_w) if window is None else window
    kh, bh, _ = resize_coeffs(w, out_w, left, nc)
    kv, bv, _ = resize_coeffs(h, out_h, top, nr)
    r0, r1 = int(bv[0, 0]), int(bv[-1, 0] + bv[-1, 1])
    mid = resample_axis(img[r0:r1], kh, bh, 1, sums)
    bv = bv.copy()
    bv[:, 0] -= r0
    return resample_axis(mid, kv, bv, 0, sums)


def expand2square(img, background=BACKGROUND):
    h, w = img.shape[:2]
    if h == w:
        return img
    s = max(h, w)
    out = np.empty((s, s, 3), dtype=np.uint8)
    out[:] = np.asarray(background, dtype=np.uint8)
    top, left = ((w - h) // 2, 0) if w > h else (0, (h - w) // 2)
    out[top:top + h, left:left + w] = img
    return out


def geometry(h, w, mode, size=336):
    """-> (in_h, in_w, pad_top, pad_left, out_h, out_w, crop_top, crop_left), restated from the reference independently of
    ``preprocess.preprocess_plan``."""
    if mode == "pad":
        s = max(h, w)
        top, left = ((w - h) // 2, 0) if w > h else (0, (h - w) // 2)
        return s, s, top, left, size, size, 0, 0
    if h <= w:
        oh, ow = size, int(size * w / h)
    else:
        oh, ow = int(size * h / w), size
    return h, w, 0, 0, oh, ow, (oh - size) // 2, (ow - size) // 2


def preprocess_bytes(img, mode, size=336, background=BACKGROUND, sums=None):
    """The uint8 ``[size, size, 3]`` picture the processor rescales and normalises."""
    if mode == "pad":
        img = expand2square(img, background)
    h, w = img.shape[:2]
    _, _, _, _, oh, ow, top, left = geometry(h, w, "square", size)
    return resize_u8(img, oh, ow, (top, left, size, size), sums)


def normalise(u8, table):
    """``u8 [size, size, 3]`` -> fp32 ``[3, size, size]`` through ``table [3, 256]`` (numpy fp32)."""
    return np.stack([table[c][u8[:, :, c]] for c in range(3)]).astype(np.float32)


def test_image(h, w, seed):
    """Seeded uint8 ``[h, w, 3]``: noise with hard black and white blocks laid over it, so that the bicubic filter's negative
    lobes overshoot at the block edges and drive clip8 into saturation at both ends."""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    bh, bw = max(1, h // 6), max(1, w // 6)
    for n in range(12):
        y, x = int(rng.integers(0, h)), int(rng.integers(0, w))
        img[y:y + bh, x:x + bw] = 255 if n % 2 else 0
    return img
test_image.__test__ = False           # (a helper, not a test, whatever its name)


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def expected_bytes(h, w, mode, seed):
    """The model's uint8 ``[336, 336, 3]`` result for ``test_image(h, w, seed)``: computed once, shared, read-only."""
    out = preprocess_bytes(test_image(h, w, seed), mode)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def expected(h, w, mode, seed):
    """fp32 ``[3, 336, 336]`` through the table the reference produced (stored in the golden)."""
    out = normalise(expected_bytes(h, w, mode, seed), golden()["table"])
    out.setflags(write=False)
    return out
