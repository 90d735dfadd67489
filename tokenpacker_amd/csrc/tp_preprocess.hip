// tp_preprocess.hip — CLIP preprocessing of a BATCH of raw RGB uint8 images for the reference's 'pad' and default ('square') image
// modes (llava/mm_utils.py:14-37, train.py:679-694, 732-734): expand2square + CLIPImageProcessor.preprocess — PIL's 8-bit bicubic
// resize, centre crop, rescale and normalise — bit for bit, in the tower's dtype, as TWO launches per batch.  See
// include/tokenpacker.h ("CLIP preprocessing") for the contract.
//
// Pillow's 8-bit resize is integer arithmetic: per axis a table of int32 coefficients (22 fractional bits) and, per output
// position, the tap range [xmin, xmin + xcount); a sample is clip8((2^21 + sum k[t] src[xmin + t]) >> 22).  It resamples
// horizontally first, rounds to uint8, then vertically and rounds again.  tp_resize_coeffs (host, IEEE double, Pillow's order of
// operations) is the single source of the tables; the kernels do integer multiply-adds only:
//   pass H  every source row the crop window's vertical taps touch x every output column of the window -> uint8 workspace
//           [rows][size][3]; in pad mode a coordinate outside the pasted content reads the background bytes (the padded square is
//           never materialised)
//   pass V  workspace -> out [n, 3, size, size]: the second resample, then lut[c][byte] (hd.normalisation_table, kept in LDS) and
//           one rounding to the output dtype
// An axis whose size does not change needs no special case: at scale 1 the coefficients are exactly {0, 2^22, 0, 0}.
#include "tp_internal.h"
#include <math.h>

using namespace tp;

namespace {

constexpr int kMaxSide = 16384;                 // H, W: 197 taps at size 336; |sum k * 255| stays near 1.25e9 < 2^31 for any tap count
constexpr int kHalf = 1 << 21;                  // Pillow: ss = 1 << (PRECISION_BITS - 1), PRECISION_BITS = 32 - 8 - 2
constexpr int kRowsPerWave = 2;                 // pass H: a wave resamples this many source rows with one read of the coefficients
constexpr int kRowsPerBlockH = 4 * kRowsPerWave;

__host__ __device__ __forceinline__ int clip8(int acc) {
    acc >>= 22;                                  // arithmetic shift, as Pillow's table lookup of `in >> PRECISION_BITS`
    return acc < 0 ? 0 : (acc > 255 ? 255 : acc);
}

// taps of a resize in_size -> out_size (Pillow's precompute_coeffs); also what tp_resize_coeffs reports
int resize_ksize(int in_size, int out_size) {
    const double scale = (double)in_size / (double)out_size;
    const double fs = scale < 1.0 ? 1.0 : scale;
    return (int)ceil(2.0 * fs) * 2 + 1;
}

// What a validated plan entry guarantees the kernels; they check their own copy again (the device words are the caller's) and
// treat an image that fails as empty: its outputs are zeros, no address is formed from it.  The tap ranges inside the tables are
// checked where they are read (per column in pass H, per row in pass V).
__host__ __device__ __forceinline__ bool image_addressable(const tp_clip_image& im, long long pixel_bytes, long long coeff_words,
                                                           long long workspace_bytes, int size) {
    if (im.H < 1 || im.W < 1 || im.H > kMaxSide || im.W > kMaxSide || im.src_offset < 0 || pixel_bytes < 4) return false;
    if ((long long)im.row_stride < 3LL * im.W) return false;
    const long long last = (long long)(im.H - 1) * im.row_stride + 3LL * im.W;       // < 2^46
    if (im.src_offset > pixel_bytes - last) return false;
    if (im.mode == TP_CLIP_SQUARE) {
        if (im.in_h != im.H || im.in_w != im.W || im.pad_top != 0 || im.pad_left != 0) return false;
    } else if (im.mode == TP_CLIP_PAD) {
        const int S = im.H > im.W ? im.H : im.W;
        if (im.in_h != S || im.in_w != S || im.pad_top < 0 || im.pad_left < 0 || im.pad_top > S - im.H || im.pad_left > S - im.W) return false;
    } else {
        return false;
    }
    if (im.ksize_h < 1 || im.ksize_v < 1 || im.row0 < 0 || im.rows < 1 || im.rows > im.in_h - im.row0) return false;
    const long long kh = (long long)im.ksize_h * size, kv = (long long)im.ksize_v * size, nb = 2LL * size;
    if (im.kk_h < 0 || im.bounds_h < 0 || im.kk_v < 0 || im.bounds_v < 0) return false;
    if (im.kk_h > coeff_words - kh || im.kk_v > coeff_words - kv || im.bounds_h > coeff_words - nb || im.bounds_v > coeff_words - nb) return false;
    if (im.ws_offset < 0 || (im.ws_offset & 15) != 0) return false;
    return im.ws_offset <= workspace_bytes - (long long)im.rows * size * 3;
}

// The packed R | G << 8 | B << 16 bytes of the pixel at byte offset `off`: ONE 4-byte load, moved down by one byte where it would
// end past pixel_bytes (>= 4), so it always lies inside pixels[0, pixel_bytes) — off + 3 <= pixel_bytes holds for every pixel of
// a validated image (the load_taps discipline of tp_hd_slice.hip).
__device__ __forceinline__ unsigned load_pixel(const uint8_t* __restrict__ pixels, long long pixel_bytes, long long off) {
    const long long lim = pixel_bytes - 4;
    int shift = 0;
    if (off > lim) { shift = (int)(off - lim); off = lim; }
    unsigned v;
    __builtin_memcpy(&v, pixels + off, 4);
    return (v >> (8 * shift)) & 0xffffffu;
}

// Pass H.  grid (ceil(max rows / 8), n_images), 4 waves; a wave owns kRowsPerWave source rows (wave-uniform: so is "this row lies
// in the pasted content"), its lanes adjacent output columns — they read adjacent words of the tap-major table [ksize][size].
__global__ void __launch_bounds__(256)
clip_resize_h_kernel(const tp_clip_image* __restrict__ plan, const uint8_t* __restrict__ pixels, long long pixel_bytes,
                     const int32_t* __restrict__ coeffs, long long coeff_words, uint8_t* __restrict__ workspace, long long workspace_bytes,
                     int size) {
    const tp_clip_image im = plan[blockIdx.y];
    if (!image_addressable(im, pixel_bytes, coeff_words, workspace_bytes, size)) return;
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), lane = (int)threadIdx.x & 63;
    const int r0 = ((int)blockIdx.x * 4 + wave) * kRowsPerWave;                     // <= 2^16 * 8
    if (r0 >= im.rows) return;
    const int32_t* kk = coeffs + im.kk_h;
    const int32_t* bounds = coeffs + im.bounds_h;
    const unsigned bg = (unsigned)im.background[0] | (unsigned)im.background[1] << 8 | (unsigned)im.background[2] << 16;
    bool row_in[kRowsPerWave];
    long long row_off[kRowsPerWave];
#pragma unroll
    for (int j = 0; j < kRowsPerWave; ++j) {
        const int y = im.row0 + r0 + j - im.pad_top;                                  // row of the stored image
        row_in[j] = y >= 0 && y < im.H;
        row_off[j] = im.src_offset + (long long)(row_in[j] ? y : 0) * im.row_stride;
    }
    for (int x = lane; x < size; x += 64) {
        const int xmin = bounds[2 * x];
        int xcount = bounds[2 * x + 1];
        const bool ok = xmin >= 0 && xcount >= 0 && xcount <= im.ksize_h && xmin <= im.in_w - xcount;
        if (!ok) xcount = 0;
        int acc[kRowsPerWave][3];
#pragma unroll
        for (int j = 0; j < kRowsPerWave; ++j) acc[j][0] = acc[j][1] = acc[j][2] = kHalf;
        for (int t = 0; t < xcount; ++t) {
            const int k = kk[(long long)t * size + x];
            const int sx = xmin + t - im.pad_left;                                    // column of the stored image
            const bool col_in = sx >= 0 && sx < im.W;
#pragma unroll
            for (int j = 0; j < kRowsPerWave; ++j) {
                unsigned p = bg;
                if (col_in && row_in[j]) p = load_pixel(pixels, pixel_bytes, row_off[j] + 3LL * sx);
                acc[j][0] += k * (int)(p & 255u);
                acc[j][1] += k * (int)((p >> 8) & 255u);
                acc[j][2] += k * (int)(p >> 16);
            }
        }
#pragma unroll
        for (int j = 0; j < kRowsPerWave; ++j) {
            if (r0 + j >= im.rows) continue;
            uint8_t* dst = workspace + im.ws_offset + ((long long)(r0 + j) * size + x) * 3;
            dst[0] = ok ? (uint8_t)clip8(acc[j][0]) : (uint8_t)0;
            dst[1] = ok ? (uint8_t)clip8(acc[j][1]) : (uint8_t)0;
            dst[2] = ok ? (uint8_t)clip8(acc[j][2]) : (uint8_t)0;
        }
    }
}

// eight consecutive fp32 values -> T, one rounding (Tensor.to: round to nearest even), stored as 16 bytes (2 x 16 for fp32)
template <typename T>
__device__ __forceinline__ void store8(T* __restrict__ dst, const float* v) {
    if constexpr (std::is_same<T, float>::value) {
        reinterpret_cast<float4*>(dst)[0] = make_float4(v[0], v[1], v[2], v[3]);
        reinterpret_cast<float4*>(dst)[1] = make_float4(v[4], v[5], v[6], v[7]);
    } else {
        typename Vec<T>::x8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = round_param<T>(v[j]);
        *reinterpret_cast<uint4*>(dst) = __builtin_bit_cast(uint4, o);
    }
}

// Pass V.  grid (ceil(size / 4), n_images), 4 waves; a wave owns one output row — its coefficients and tap range are wave-uniform
// (scalar loads) — and a lane 8 consecutive pixels of it for all three channels: 24 contiguous workspace bytes per tap.
template <typename T>
__global__ void __launch_bounds__(256)
clip_resize_v_kernel(const tp_clip_image* __restrict__ plan, const int32_t* __restrict__ coeffs, long long coeff_words,
                     long long pixel_bytes, const uint8_t* __restrict__ workspace, long long workspace_bytes,
                     const float* __restrict__ lut_global, T* __restrict__ out, int size) {
    __shared__ float lut[768];
    for (int i = threadIdx.x; i < 768; i += blockDim.x) lut[i] = lut_global[i];
    __syncthreads();
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), lane = (int)threadIdx.x & 63;
    const int row = (int)blockIdx.x * 4 + wave;
    if (row >= size) return;
    const tp_clip_image im = plan[blockIdx.y];
    bool ok = image_addressable(im, pixel_bytes, coeff_words, workspace_bytes, size);
    int ymin = 0, ycount = 0;
    if (ok) {
        ymin = coeffs[im.bounds_v + 2LL * row];
        ycount = coeffs[im.bounds_v + 2LL * row + 1];
        ok = ycount >= 0 && ycount <= im.ksize_v && ymin >= im.row0 && ymin - im.row0 <= im.rows - ycount;
    }
    if (!ok) ymin = ycount = 0;
    const int32_t* k = coeffs + (ok ? im.kk_v + (long long)row * im.ksize_v : 0);
    const uint8_t* src = workspace + (ok ? im.ws_offset + (long long)(ymin - im.row0) * size * 3 : 0);
    const long long plane = (long long)size * size;
    T* dst_row = out + ((long long)blockIdx.y * 3 * size + row) * size;
    for (int x8 = lane * 8; x8 < size; x8 += 512) {
        int acc[24];
#pragma unroll
        for (int e = 0; e < 24; ++e) acc[e] = kHalf;
        for (int t = 0; t < ycount; ++t) {
            const int kt = k[t];
            const uint2* p = reinterpret_cast<const uint2*>(src + ((long long)t * size + x8) * 3);   // 8-byte aligned: size % 8 == 0
            const uint2 a = p[0], b = p[1], c = p[2];
            const unsigned w[6] = {a.x, a.y, b.x, b.y, c.x, c.y};
#pragma unroll
            for (int e = 0; e < 24; ++e) acc[e] += kt * (int)((w[e >> 2] >> (8 * (e & 3))) & 255u);
        }
        float r[8], g[8], b[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            r[j] = ok ? lut[clip8(acc[3 * j])] : 0.f;
            g[j] = ok ? lut[256 + clip8(acc[3 * j + 1])] : 0.f;
            b[j] = ok ? lut[512 + clip8(acc[3 * j + 2])] : 0.f;
        }
        store8<T>(dst_row + x8, r);
        store8<T>(dst_row + plane + x8, g);
        store8<T>(dst_row + 2 * plane + x8, b);
    }
}


#define CLIP_FAIL(...) do { set_error(__VA_ARGS__); return TP_ERR_INVALID_ARG; } while (0)

int validate_image_records(const char* who, const tp_clip_image* plan, int n_images, int size) {
    if (!plan) CLIP_FAIL("%s: NULL pointer (plan_host)", who);
    if (n_images < 1 || n_images > 65535) CLIP_FAIL("%s: n_images = %d must lie in 1 .. 65535 (one grid row per image)", who, n_images);
    if (size < 8 || size % 8 != 0 || size > 4096) CLIP_FAIL("%s: size = %d must be a multiple of 8 in 8 .. 4096", who, size);
    for (int i = 0; i < n_images; ++i) {
        const tp_clip_image& im = plan[i];
        if (im.H < 1 || im.W < 1) CLIP_FAIL("%s: image %d: H = %d, W = %d must be positive", who, i, im.H, im.W);
        if (im.H > kMaxSide || im.W > kMaxSide)
            CLIP_FAIL("%s: image %d: %d x %d exceeds the supported maximum of %d pixels per side", who, i, im.H, im.W, kMaxSide);
        if (im.mode != TP_CLIP_SQUARE && im.mode != TP_CLIP_PAD) CLIP_FAIL("%s: image %d: mode %d (TP_CLIP_SQUARE or TP_CLIP_PAD)", who, i, im.mode);
        const int S = im.H > im.W ? im.H : im.W;
        if (im.mode == TP_CLIP_SQUARE ? (im.in_h != im.H || im.in_w != im.W || im.pad_top != 0 || im.pad_left != 0)
                                      : (im.in_h != S || im.in_w != S || im.pad_top < 0 || im.pad_left < 0 || im.pad_top > S - im.H ||
                                         im.pad_left > S - im.W))
            CLIP_FAIL("%s: image %d: resampled area %d x %d with the content at (%d, %d) does not describe a %d x %d image in mode %d", who, i,
                      im.in_h, im.in_w, im.pad_top, im.pad_left, im.H, im.W, im.mode);
        if (im.out_h < size || im.out_w < size || im.crop_top < 0 || im.crop_left < 0 || im.crop_top > im.out_h - size ||
            im.crop_left > im.out_w - size)
            CLIP_FAIL("%s: image %d: crop window (%d, %d) + %d lies outside the resized %d x %d", who, i, im.crop_top, im.crop_left, size,
                      im.out_h, im.out_w);
        const int kh = resize_ksize(im.in_w, im.out_w), kv = resize_ksize(im.in_h, im.out_h);
        if (im.ksize_h != kh || im.ksize_v != kv)
            CLIP_FAIL("%s: image %d: ksize %d (horizontal), %d (vertical); resizing %d x %d to %d x %d takes %d and %d taps", who, i,
                      im.ksize_h, im.ksize_v, im.in_h, im.in_w, im.out_h, im.out_w, kh, kv);
        if (im.row0 < 0 || im.rows < 1 || im.rows > im.in_h - im.row0)
            CLIP_FAIL("%s: image %d: workspace rows [%d, %d + %d) lie outside [0, %d)", who, i, im.row0, im.row0, im.rows, im.in_h);
    }
    return TP_OK;
}

int validate_plan(const tp_clip_image* plan, int n_images, long long pixel_bytes, const int32_t* coeffs, long long coeff_words,
                  long long workspace_bytes, int size) {
    const char* who = "tp_clip_preprocess";
    long long next_word = 0, next_ws = 0;
    for (int i = 0; i < n_images; ++i) {
        const tp_clip_image& im = plan[i];
        if ((long long)im.row_stride < 3LL * im.W) CLIP_FAIL("%s: image %d: row_stride %d < 3 * W = %lld", who, i, im.row_stride, 3LL * im.W);
        const long long last = (long long)(im.H - 1) * im.row_stride + 3LL * im.W;
        if (im.src_offset < 0 || im.src_offset > pixel_bytes - last)
            CLIP_FAIL("%s: image %d: bytes [%lld, %lld + %lld) lie outside pixels[0, %lld)", who, i, (long long)im.src_offset,
                      (long long)im.src_offset, last, pixel_bytes);
        // the four tables, in the order kk_h, bounds_h, kk_v, bounds_v, each behind the one before (and behind the previous image's)
        const struct { const char* name; long long at, words; } tables[4] = {
            {"kk_h", im.kk_h, (long long)im.ksize_h * size}, {"bounds_h", im.bounds_h, 2LL * size},
            {"kk_v", im.kk_v, (long long)im.ksize_v * size}, {"bounds_v", im.bounds_v, 2LL * size}};
        for (const auto& t : tables) {
            if (t.at < 0 || t.at > coeff_words - t.words)
                CLIP_FAIL("%s: image %d: table %s, words [%lld, %lld + %lld), lies outside coeffs[0, %lld)", who, i, t.name, t.at, t.at, t.words, coeff_words);
            if (t.at < next_word) CLIP_FAIL("%s: image %d: table %s at word %lld overlaps the table before it (which ends at %lld)", who, i, t.name, t.at, next_word);
            next_word = t.at + t.words;
        }
        const long long ws = (long long)im.rows * size * 3;
        if ((im.ws_offset & 15) != 0) CLIP_FAIL("%s: image %d: ws_offset %lld must be a multiple of 16", who, i, (long long)im.ws_offset);
        if (im.ws_offset < 0 || im.ws_offset > workspace_bytes - ws)
            CLIP_FAIL("%s: image %d: workspace slice [%lld, %lld + %lld) lies outside workspace[0, %lld)", who, i, (long long)im.ws_offset,
                      (long long)im.ws_offset, ws, workspace_bytes);
        if (im.ws_offset < next_ws) CLIP_FAIL("%s: image %d: workspace slice at %lld overlaps the slice before it (which ends at %lld)", who, i, (long long)im.ws_offset, next_ws);
        next_ws = im.ws_offset + ws;
        const int32_t* bh = coeffs + im.bounds_h;
        const int32_t* bv = coeffs + im.bounds_v;
        for (int x = 0; x < size; ++x) {
            if (bh[2 * x] < 0 || bh[2 * x + 1] < 0 || bh[2 * x + 1] > im.ksize_h || bh[2 * x] > im.in_w - bh[2 * x + 1])
                CLIP_FAIL("%s: image %d: horizontal taps [%d, %d + %d) of column %d lie outside [0, %d) or exceed ksize %d", who, i, bh[2 * x],
                          bh[2 * x], bh[2 * x + 1], x, im.in_w, im.ksize_h);
            if (bv[2 * x + 1] < 0 || bv[2 * x + 1] > im.ksize_v || bv[2 * x] < im.row0 || bv[2 * x] - im.row0 > im.rows - bv[2 * x + 1])
                CLIP_FAIL("%s: image %d: vertical taps [%d, %d + %d) of row %d lie outside the workspace rows [%d, %d) or exceed ksize %d", who, i,
                          bv[2 * x], bv[2 * x], bv[2 * x + 1], x, im.row0, im.row0 + im.rows, im.ksize_v);
        }
    }
    return TP_OK;
}

// Pillow's bicubic filter (a = -0.5) and coefficient arithmetic: IEEE double, this order, no contraction
double cubic(double x) {
#pragma clang fp contract(off)
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

}  // namespace

extern "C" {

int tp_resize_coeffs(int in_size, int out_size, int first_out, int n_out, int32_t* kk, int32_t* bounds, int* ksize_out) {
#pragma clang fp contract(off)
    if (in_size < 1 || out_size < 1 || in_size > (1 << 24) || out_size > (1 << 24))
        CLIP_FAIL("tp_resize_coeffs: in_size = %d, out_size = %d must lie in 1 .. 2^24", in_size, out_size);
    const double scale = (double)in_size / (double)out_size;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = 2.0 * fs;
    const int ksize = (int)ceil(support) * 2 + 1;
    if (ksize_out) *ksize_out = ksize;
    if (!kk && !bounds) return TP_OK;                                                  // the tap count alone
    if (!kk || !bounds) CLIP_FAIL("tp_resize_coeffs: NULL pointer (kk and bounds go together)");
    if (first_out < 0 || n_out < 1 || n_out > out_size - first_out)
        CLIP_FAIL("tp_resize_coeffs: positions [%d, %d + %d) lie outside [0, %d)", first_out, first_out, n_out, out_size);
    const double ss = 1.0 / fs;
    for (int i = 0; i < n_out; ++i) {
        const int xx = first_out + i;
        const double center = (xx + 0.5) * scale;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in_size) xmax = in_size;
        xmax -= xmin;
        double ww = 0.0;                                                               // left to right, as Pillow sums it
        for (int t = 0; t < xmax; ++t) ww += cubic((t + xmin - center + 0.5) * ss);
        int32_t* k = kk + (long long)i * ksize;
        for (int t = 0; t < xmax; ++t) {                                               // (the weight again: no scratch, no allocation)
            double w = cubic((t + xmin - center + 0.5) * ss);
            if (ww != 0.0) w /= ww;
            k[t] = w < 0 ? (int32_t)(w * 4194304.0 - 0.5) : (int32_t)(w * 4194304.0 + 0.5);
        }
        for (int t = xmax; t < ksize; ++t) k[t] = 0;
        bounds[2 * i] = xmin;
        bounds[2 * i + 1] = xmax;
    }
    return TP_OK;
}

size_t tp_clip_preprocess_workspace_bytes(const tp_clip_image* plan_host, int n_images, int size) {
    if (validate_image_records("tp_clip_preprocess_workspace_bytes", plan_host, n_images, size) != TP_OK) return 0;
    long long need = 0;
    for (int i = 0; i < n_images; ++i) {
        const tp_clip_image& im = plan_host[i];
        if (im.ws_offset < 0 || (im.ws_offset & 15) != 0) {
            set_error("tp_clip_preprocess_workspace_bytes: image %d: ws_offset %lld must be a non-negative multiple of 16", i, (long long)im.ws_offset);
            return 0;
        }
        const long long end = im.ws_offset + (long long)im.rows * size * 3;
        if (end > need) need = end;
    }
    return (size_t)((need + 15) / 16 * 16);
}

int tp_clip_preprocess(const tp_clip_image* plan_host, const void* plan_dev, int n_images, const uint8_t* pixels, int64_t pixel_bytes,
                       const float* lut, const int32_t* coeffs_host, const int32_t* coeffs_dev, int64_t coeff_words, void* workspace,
                       int64_t workspace_bytes, void* out, int size, int out_dtype, void* stream) {
    const char* who = "tp_clip_preprocess";
    if (!plan_host || !plan_dev || !pixels || !lut || !coeffs_host || !coeffs_dev || !workspace || !out) CLIP_FAIL("%s: NULL pointer", who);
    if (((uintptr_t)plan_dev & 7) != 0 || ((uintptr_t)lut & 3) != 0 || ((uintptr_t)coeffs_dev & 3) != 0 || ((uintptr_t)workspace & 15) != 0 ||
        ((uintptr_t)out & 15) != 0)
        CLIP_FAIL("%s: plan_dev must be 8-byte, lut and coeffs_dev 4-byte, workspace and out 16-byte aligned", who);
    if (pixel_bytes < 4 || coeff_words < 1 || workspace_bytes < 1)
        CLIP_FAIL("%s: pixel_bytes = %lld must be at least 4, coeff_words = %lld and workspace_bytes = %lld positive", who, (long long)pixel_bytes,
                  (long long)coeff_words, (long long)workspace_bytes);
    int rc = validate_image_records(who, plan_host, n_images, size);
    if (rc != TP_OK) return rc;
    rc = validate_plan(plan_host, n_images, pixel_bytes, coeffs_host, coeff_words, workspace_bytes, size);
    if (rc != TP_OK) return rc;
    if (out_dtype != TP_F32 && out_dtype != TP_BF16 && out_dtype != TP_F16) CLIP_FAIL("%s: out_dtype %d", who, out_dtype);
    int max_rows = 0;
    for (int i = 0; i < n_images; ++i) max_rows = plan_host[i].rows > max_rows ? plan_host[i].rows : max_rows;
    const tp_clip_image* plan = (const tp_clip_image*)plan_dev;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid_h((unsigned)((max_rows + kRowsPerBlockH - 1) / kRowsPerBlockH), (unsigned)n_images);
    const dim3 grid_v((unsigned)((size + 3) / 4), (unsigned)n_images);
    hipLaunchKernelGGL(clip_resize_h_kernel, grid_h, dim3(256), 0, st, plan, pixels, (long long)pixel_bytes, coeffs_dev, (long long)coeff_words,
                       (uint8_t*)workspace, (long long)workspace_bytes, size);
    rc = check_launch("clip_resize_h_kernel");
    if (rc != TP_OK) return rc;
    if (out_dtype == TP_F32)
        hipLaunchKernelGGL(clip_resize_v_kernel<float>, grid_v, dim3(256), 0, st, plan, coeffs_dev, (long long)coeff_words, (long long)pixel_bytes,
                           (const uint8_t*)workspace, (long long)workspace_bytes, lut, (float*)out, size);
    else if (out_dtype == TP_BF16)
        hipLaunchKernelGGL(clip_resize_v_kernel<bf16_t>, grid_v, dim3(256), 0, st, plan, coeffs_dev, (long long)coeff_words, (long long)pixel_bytes,
                           (const uint8_t*)workspace, (long long)workspace_bytes, lut, (bf16_t*)out, size);
    else
        hipLaunchKernelGGL(clip_resize_v_kernel<f16_t>, grid_v, dim3(256), 0, st, plan, coeffs_dev, (long long)coeff_words, (long long)pixel_bytes,
                           (const uint8_t*)workspace, (long long)workspace_bytes, lut, (f16_t*)out, size);
    return check_launch("clip_resize_v_kernel");
}

}  // extern "C"
