// tp_hd_slice.hip — TokenPacker-HD slicing of a BATCH of raw RGB uint8 images (reference llava/train/train.py:696-731 and the
// driver's `.to(dtype)`): ToTensor + Normalize, resize, zero-pad, tile and global view of every image, in the tower's dtype, as
// ONE launch.  See include/tokenpacker.h ("HD slicing from uint8 images") for the contract.
//
// Normalisation is a table lookup: fl(fl(fl(u / 255) - mean_c) / std_c) depends on (c, u) only, the host builds the 768 fp32
// values with torch's own CPU ops and the kernel keeps them in LDS — bit-exact by construction, no division on the device.
// The resize arithmetic is tp_hd_slice's (bilinear_taps, the same blend) on table values; the global view is computed from the
// canvas's fp32 values (canvas_pixel below), never from crops already rounded to 16 bits.
//
// The plan (host copy for validation, device copy for the kernel — the same words): tp_hd_slice_image [n_images], then one
// int32 per crop, the index of its image, so that a workgroup finds its image in O(1) whatever the batch.
#include "tp_internal.h"

using namespace tp;

namespace {

struct Rgb { float r, g, b; };

constexpr long long kMaxCanvas = 1 << 30;      // canvas side in pixels: its coordinates and an image's crop count stay 32-bit

// The packed R | G << 8 | B << 16 bytes of the taps x0 and x1 (x1 = x0 + 1 when `two`, else x0) of one source row: the six
// bytes are adjacent, so ONE 8-byte load fetches both taps.  `off` is the byte offset of tap x0 in `pixels`; the load is
// moved down by up to 5 bytes where it would end past pixel_bytes (>= 8), so it always lies inside pixels[0, pixel_bytes):
// off + 3 (one tap) or off + 6 (two) <= pixel_bytes holds for every tap of a validated image.
__host__ __device__ __forceinline__ void load_taps(const uint8_t* __restrict__ pixels, long long pixel_bytes, long long off, bool two,
                                                   unsigned& a, unsigned& b) {
    const long long lim = pixel_bytes - 8;
    int shift = 0;
    if (off > lim) { shift = (int)(off - lim); off = lim; }
    unsigned long long v;
    __builtin_memcpy(&v, pixels + off, 8);
    v >>= 8 * shift;
    a = (unsigned)v & 0xffffffu;
    b = two ? (unsigned)(v >> 24) & 0xffffffu : a;
}

// What a validated plan entry guarantees the kernel; the kernel checks it again on its own copy (the device words are the
// caller's) and treats an image that fails as empty: all its crops are zeros, no address is formed from it.
__host__ __device__ __forceinline__ bool image_addressable(const tp_hd_slice_image& im, long long pixel_bytes, int block) {
    if (im.H < 1 || im.W < 1 || im.h_block < 1 || im.w_block < 1 || im.src_offset < 0 || im.row_stride < 0) return false;
    if ((long long)im.h_block * block > kMaxCanvas || (long long)im.w_block * block > kMaxCanvas) return false;
    if ((long long)im.row_stride < 3LL * im.W) return false;
    if (im.h_res < 1 || im.w_res < 1 || (long long)im.h_res > (long long)im.h_block * block ||
        (long long)im.w_res > (long long)im.w_block * block) return false;
    if (im.hg < 0 || im.wg < 0 || im.hg > block || im.wg > block) return false;
    if (pixel_bytes < 8) return false;
    const long long last = (long long)(im.H - 1) * im.row_stride + 3LL * im.W;       // < 2^62
    return im.src_offset <= pixel_bytes - last;
}

// One pixel (Y, X) of an image's canvas, all three channels in fp32: zero outside (h_res, w_res), else the bilinear blend of
// the normalised source (F.interpolate's arithmetic, align_corners = False).  `lut` is the [3][256] table.
__host__ __device__ __forceinline__ Rgb canvas_pixel(const tp_hd_slice_image& im, const uint8_t* __restrict__ pixels, long long pixel_bytes,
                                                     const float* lut, int Y, int X) {
    Rgb out{0.f, 0.f, 0.f};
    if (Y >= im.h_res || X >= im.w_res) return out;
    int y0, y1, x0, x1; float ly0, ly1, lx0, lx1;
    bilinear_taps((float)im.H / (float)im.h_res, Y, im.H, y0, y1, ly0, ly1);
    bilinear_taps((float)im.W / (float)im.w_res, X, im.W, x0, x1, lx0, lx1);
    const long long col = im.src_offset + 3LL * x0;
    unsigned a, b, c, d;
    load_taps(pixels, pixel_bytes, col + (long long)y0 * im.row_stride, x1 != x0, a, b);
    load_taps(pixels, pixel_bytes, col + (long long)y1 * im.row_stride, x1 != x0, c, d);
    const float* lg = lut + 256;
    const float* lb = lut + 512;
    out.r = ly0 * (lx0 * lut[a & 255u] + lx1 * lut[b & 255u]) + ly1 * (lx0 * lut[c & 255u] + lx1 * lut[d & 255u]);
    out.g = ly0 * (lx0 * lg[(a >> 8) & 255u] + lx1 * lg[(b >> 8) & 255u]) + ly1 * (lx0 * lg[(c >> 8) & 255u] + lx1 * lg[(d >> 8) & 255u]);
    out.b = ly0 * (lx0 * lb[a >> 16] + lx1 * lb[b >> 16]) + ly1 * (lx0 * lb[c >> 16] + lx1 * lb[d >> 16]);
    return out;
}

// Pixel (row, x) of crop `s` of an image: a tile of the canvas, or — s == h_block * w_block — the global view: the canvas
// (padding included, train.py:710,728) resized to (hg, wg), zero elsewhere.
__host__ __device__ __forceinline__ Rgb crop_pixel(const tp_hd_slice_image& im, const uint8_t* __restrict__ pixels, long long pixel_bytes,
                                                   const float* lut, int s, int row, int x, int block) {
    if (s < im.h_block * im.w_block)
        return canvas_pixel(im, pixels, pixel_bytes, lut, (s / im.w_block) * block + row, (s % im.w_block) * block + x);
    Rgb out{0.f, 0.f, 0.f};
    if (row >= im.hg || x >= im.wg) return out;
    const int CH = im.h_block * block, CW = im.w_block * block;
    int y0, y1, x0, x1; float ly0, ly1, lx0, lx1;
    bilinear_taps((float)CH / (float)im.hg, row, CH, y0, y1, ly0, ly1);
    bilinear_taps((float)CW / (float)im.wg, x, CW, x0, x1, lx0, lx1);
    const Rgb a = canvas_pixel(im, pixels, pixel_bytes, lut, y0, x0), b = canvas_pixel(im, pixels, pixel_bytes, lut, y0, x1);
    const Rgb c = canvas_pixel(im, pixels, pixel_bytes, lut, y1, x0), d = canvas_pixel(im, pixels, pixel_bytes, lut, y1, x1);
    out.r = ly0 * (lx0 * a.r + lx1 * b.r) + ly1 * (lx0 * c.r + lx1 * d.r);
    out.g = ly0 * (lx0 * a.g + lx1 * b.g) + ly1 * (lx0 * c.g + lx1 * d.g);
    out.b = ly0 * (lx0 * a.b + lx1 * b.b) + ly1 * (lx0 * c.b + lx1 * d.b);
    return out;
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

// `wgs_per_crop` workgroups per crop; a lane produces 8 consecutive pixels of one output row for all three channels.
template <typename T>
__global__ void __launch_bounds__(256)
hd_slice_u8_kernel(const tp_hd_slice_image* __restrict__ plan, const int* __restrict__ crop_image, int n_images,
                   const uint8_t* __restrict__ pixels, long long pixel_bytes, const float* __restrict__ lut_global,
                   T* __restrict__ crops, int block, int wgs_per_crop) {
    __shared__ float lut[768];
    for (int i = threadIdx.x; i < 768; i += blockDim.x) lut[i] = lut_global[i];
    __syncthreads();
    const long long crop = blockIdx.x / (unsigned)wgs_per_crop;                     // < n_crops: the grid is n_crops * wgs_per_crop
    const int lanes_per_row = block / 8;
    const int item = (int)(blockIdx.x % (unsigned)wgs_per_crop) * (int)blockDim.x + (int)threadIdx.x;
    if (item >= block * lanes_per_row) return;
    const int row = item / lanes_per_row, x8 = (item - row * lanes_per_row) * 8;
    const int i = crop_image[crop];
    tp_hd_slice_image im{};                                                           // (all zeros: an empty image, every pixel zero)
    int s = 0;
    if (i >= 0 && i < n_images) {
        im = plan[i];
        const long long rel = crop - im.first_crop;
        const long long n = (long long)im.h_block * im.w_block;
        if (!image_addressable(im, pixel_bytes, block) || rel < 0 || rel > n || (rel == n && n == 1)) im = tp_hd_slice_image{};
        else s = (int)rel;
    }
    float r[8], g[8], b[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        Rgb p{0.f, 0.f, 0.f};
        if (im.H > 0) p = crop_pixel(im, pixels, pixel_bytes, lut, s, row, x8 + j, block);
        r[j] = p.r; g[j] = p.g; b[j] = p.b;
    }
    const long long plane = (long long)block * block;
    T* dst = crops + (crop * 3 * block + row) * block + x8;
    store8<T>(dst, r);
    store8<T>(dst + plane, g);
    store8<T>(dst + 2 * plane, b);
}

int validate_plan(const tp_hd_slice_image* plan, int n_images, long long pixel_bytes, long long n_crops, int block) {
    const int32_t* crop_image = reinterpret_cast<const int32_t*>(plan + n_images);
    long long next = 0;
    for (int i = 0; i < n_images; ++i) {
        const tp_hd_slice_image& im = plan[i];
        if (im.H < 1 || im.W < 1) { set_error("tp_hd_slice_u8: image %d: H = %d, W = %d must be positive", i, im.H, im.W); return TP_ERR_INVALID_ARG; }
        if (im.h_block < 1 || im.w_block < 1 || (long long)im.h_block * block > kMaxCanvas || (long long)im.w_block * block > kMaxCanvas) {
            set_error("tp_hd_slice_u8: image %d: grid %d x %d of %d-pixel blocks", i, im.h_block, im.w_block, block);
            return TP_ERR_INVALID_ARG;
        }
        if ((long long)im.row_stride < 3LL * im.W) {
            set_error("tp_hd_slice_u8: image %d: row_stride %d < 3 * W = %lld", i, im.row_stride, 3LL * im.W);
            return TP_ERR_INVALID_ARG;
        }
        const long long last = (long long)(im.H - 1) * im.row_stride + 3LL * im.W;
        if (im.src_offset < 0 || im.src_offset > pixel_bytes - last) {
            set_error("tp_hd_slice_u8: image %d: bytes [%lld, %lld + %lld) lie outside pixels[0, %lld)", i, (long long)im.src_offset,
                      (long long)im.src_offset, last, pixel_bytes);
            return TP_ERR_INVALID_ARG;
        }
        const long long n = (long long)im.h_block * im.w_block;
        if (im.h_res < 1 || im.w_res < 1 || im.h_res > (long long)im.h_block * block || im.w_res > (long long)im.w_block * block) {
            set_error("tp_hd_slice_u8: image %d: resized size %d x %d does not fit the %d x %d grid of %d-pixel blocks", i, im.h_res,
                      im.w_res, im.h_block, im.w_block, block);
            return TP_ERR_INVALID_ARG;
        }
        if (n == 1 ? (im.hg != 0 || im.wg != 0) : (im.hg < 1 || im.wg < 1 || im.hg > block || im.wg > block)) {
            set_error("tp_hd_slice_u8: image %d: global view %d x %d (0 x 0 exactly when there is one crop, else within 1 .. %d)", i,
                      im.hg, im.wg, block);
            return TP_ERR_INVALID_ARG;
        }
        if (im.first_crop != next) {
            set_error("tp_hd_slice_u8: image %d: first_crop %d %s (the previous image ends at %lld)", i, im.first_crop,
                      im.first_crop < next ? "overlaps the previous image's crops" : "leaves a gap", next);
            return TP_ERR_INVALID_ARG;
        }
        const long long count = n + (n > 1 ? 1 : 0);
        if (next + count > n_crops) { set_error("tp_hd_slice_u8: image %d: crops up to %lld of %lld", i, next + count, n_crops); return TP_ERR_INVALID_ARG; }
        for (long long c = next; c < next + count; ++c)
            if (crop_image[c] != i) { set_error("tp_hd_slice_u8: crop %lld is mapped to image %d, the plan puts it in image %d", c, crop_image[c], i); return TP_ERR_INVALID_ARG; }
        next += count;
    }
    if (next != n_crops) { set_error("tp_hd_slice_u8: the plan describes %lld crops, n_crops = %lld", next, n_crops); return TP_ERR_INVALID_ARG; }
    return TP_OK;
}

}  // namespace

extern "C" {

int tp_hd_slice_u8(const tp_hd_slice_image* plan_host, const void* plan_dev, int n_images, const uint8_t* pixels, int64_t pixel_bytes,
                   const float* lut, void* crops, int64_t n_crops, int block, int out_dtype, void* stream) {
    if (!plan_host || !plan_dev || !pixels || !lut || !crops) { set_error("tp_hd_slice_u8: NULL pointer"); return TP_ERR_INVALID_ARG; }
    if (((uintptr_t)plan_dev & 7) != 0 || ((uintptr_t)lut & 3) != 0 || ((uintptr_t)crops & 15) != 0) {
        set_error("tp_hd_slice_u8: plan_dev must be 8-byte, lut 4-byte and crops 16-byte aligned");
        return TP_ERR_INVALID_ARG;
    }
    if (n_images < 1 || n_crops < 1 || pixel_bytes < 8) {
        set_error("tp_hd_slice_u8: n_images = %d, n_crops = %lld must be positive and pixel_bytes = %lld at least 8", n_images,
                  (long long)n_crops, (long long)pixel_bytes);
        return TP_ERR_INVALID_ARG;
    }
    if (block < 8 || block % 8 != 0 || block > 32768) { set_error("tp_hd_slice_u8: block = %d must be a multiple of 8 in 8 .. 32768", block); return TP_ERR_INVALID_ARG; }
    const int rc = validate_plan(plan_host, n_images, pixel_bytes, n_crops, block);
    if (rc != TP_OK) return rc;
    if (out_dtype != TP_F32 && out_dtype != TP_BF16 && out_dtype != TP_F16) { set_error("tp_hd_slice_u8: out_dtype %d", out_dtype); return TP_ERR_INVALID_ARG; }
    const long long items = (long long)block * (block / 8);
    const long long wgs_per_crop = (items + 255) / 256;
    if (n_crops * wgs_per_crop > 0x7fffffffLL) { set_error("tp_hd_slice_u8: %lld crops of %d pixels exceed one launch", (long long)n_crops, block); return TP_ERR_INVALID_ARG; }
    const tp_hd_slice_image* plan = (const tp_hd_slice_image*)plan_dev;
    const int* crop_image = (const int*)(plan + n_images);
    const dim3 grid((unsigned)(n_crops * wgs_per_crop));
    hipStream_t st = (hipStream_t)stream;
    if (out_dtype == TP_F32)
        hipLaunchKernelGGL(hd_slice_u8_kernel<float>, grid, dim3(256), 0, st, plan, crop_image, n_images, pixels, (long long)pixel_bytes,
                           lut, (float*)crops, block, (int)wgs_per_crop);
    else if (out_dtype == TP_BF16)
        hipLaunchKernelGGL(hd_slice_u8_kernel<bf16_t>, grid, dim3(256), 0, st, plan, crop_image, n_images, pixels, (long long)pixel_bytes,
                           lut, (bf16_t*)crops, block, (int)wgs_per_crop);
    else
        hipLaunchKernelGGL(hd_slice_u8_kernel<f16_t>, grid, dim3(256), 0, st, plan, crop_image, n_images, pixels, (long long)pixel_bytes,
                           lut, (f16_t*)crops, block, (int)wgs_per_crop);
    return check_launch("hd_slice_u8_kernel");
}

}  // extern "C"
