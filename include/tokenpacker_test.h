/* tokenpacker_test.h — test hooks and probe builds of the TokenPacker HIP library.  NOT part of the product ABI
 * (include/tokenpacker.h): these entry points exist only in libtokenpacker_exp.so (`make -C tokenpacker_amd/csrc exp`, built by
 * __graft_entry__.build() beside the product library from the same sources + csrc/tp_test_hooks.hip and the GEMM kernels' timing-probe
 * instantiations (-DTP_BUILD_PROBES: TP_TUNE_PAIR_DEBUG)).  All of them are stateless: a test may call them
 * in libtokenpacker_exp.so while the module under test runs on libtokenpacker_hip.so. */
#ifndef TOKENPACKER_TEST_H
#define TOKENPACKER_TEST_H
#include "tokenpacker.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- test hook: occupy `workgroups` CUs for ~`microseconds` on `stream` (100 KiB LDS each; `scratch_int`: any
 * device int).  Stands in for another stream's kernels when the GEMM tile queue is measured (tools/hog_bench.py). */
int tp_test_occupy_cus(int workgroups, int microseconds, void* scratch_int, void* stream);
/* ---- test hook: workgroups of the pair kernel the runtime admits per CU (hipOccupancyMaxActiveBlocksPerMultiprocessor;
 * the design needs 2); negative on error */
int tp_test_pair_occupancy(void);
/* ---- test hook (host logic only, no GPU needed): where tp_linear would send a plain fp16 launch of this shape under the tuning
 * of the moment — 0 the 128-tile kernel | 1 full 256 x 256 tiles | 2 all 128 x 256 half tiles | 3 full rounds + a half-tile tail
 * launch | 4 192 x 256 tiles | 5 the pair kernel; -1: bad shape.  (256 CUs are assumed when no device is visible.) */
int tp_test_gemm_route(int M, int N, int K, int flags, int groups);
/* ---- test hook: the pack-time factorisation behind TP_TUNE_TRI_STATS on ONE layer.  w2 [1024][1024] fp16 and b2 [1024] fp32
 * (or NULL) in; r [1024][1024] fp16 (upper triangular), c_tilde [1024] fp32 and wbar [1025] fp32 (column means of w2, then
 * mean(b2)) out, with  sum_n ((w2 h + b2)_n - mean)^2 = || r h + c_tilde ||^2  for every h.  scratch: device memory of
 * tp_test_pack_qr_scratch_bytes() bytes. */
size_t tp_test_pack_qr_scratch_bytes(void);
int tp_test_pack_qr(const void* w2_f16, const float* b2, void* r_f16, float* c_tilde, float* wbar, void* scratch, void* stream);

/* ---- test hook (host logic only, no GPU needed): where tp_pack_weights puts one tensor of the packed image.  `name` is a field of
 * PackedLayout (csrc/tp_internal.h: "w_kv0" .. "status", in the order of their offsets; "total": the image's size, 0 bytes);
 * *offset = its byte offset in the image, *bytes = the size the layout reserved for it before the 256-byte alignment.  An unknown
 * name or a hidden_size that is not a positive multiple of 128: TP_ERR_INVALID_ARG (tp_last_error() says why).
 * tests/test_gpu_pack_image.py slices the image with it. */
int tp_test_packed_layout(int hidden_size, const char* name, size_t* offset, size_t* bytes);

/* ---- test hooks: the FORWARD's two attention kernels one at a time, WITH the additive mask the public tp_region_attention /
 * tp_region_attention_absorbed do not take (tests/test_gpu_attention_masks.py).  Pass-throughs to the launchers tp_forward* calls
 * (csrc/tp_internal.h: region_attention_launch, region_attention_absorbed_launch), after the host checks described below: NULL
 * pointers, 16-byte alignment (mr_k / mr_v: 8, mask: 4), B > 0, s dividing grid <= 1024, mask_mode 0 (mask NULL) / 1 / 2 (mask given).
 * mask: fp32, mode 1 [s*s], mode 2 [(M B) 8, s*s] with batch index region * B + image; -inf allowed at any key position as long as
 * one key of the row stays finite. */
/* o [B M, 1024] = softmax(q k^T / sqrt(128) + mask) v per head, fp16; q [B M, 1024], k / v [B grid^2, 1024] in raster order
 * (region_major 0) or with the rows of region m at m * s*s + key inside each image (region_major 1). */
int tp_test_region_attention(const void* q, const void* k, const void* v, void* o, int B, int grid, int s, const float* mask,
                             int mask_mode, int region_major, void* stream);
/* The absorbed schedule's attention in its plain (not RAW) form: qt [B M, 8, 1024] fp16, h2k / h2v [B grid^2, 1024] fp16 with their
 * per-row (mean, rstd) mr_k / mr_v (fp32 [B grid^2][2]) -> u [B M, 8, 1024] fp16.  s*s > 64: the launcher's TP_ERR_INVALID_ARG. */
int tp_test_region_attention_absorbed(const void* qt, const void* h2k, const void* h2v, const float* mr_k, const float* mr_v, void* u,
                                      int B, int grid, int s, const float* mask, int mask_mode, void* stream);

/* ---- test hooks: the BACKWARD's kernels one at a time (tests/test_gpu_bwd_kernels.py compares each with fp64 math on the same
 * rounded operands, tests/bwd_ref.py).  Each is a pass-through to the launcher tp_backward itself calls (csrc/tp_internal.h:
 * bw_*_launch, point_queries_bwd_launch, gemm_launch): same objects, same kernels.  Every hook checks on the HOST what its launcher
 * leaves to its caller — NULL pointers, 16-byte alignment, element counts / strides that must be multiples of 8 or 4, scratch
 * sizes — and returns TP_ERR_INVALID_ARG (tp_last_error() says why) before anything is enqueued; otherwise the launcher's status.
 * All pointers are device pointers unless stated; dtypes are TP_BF16 / TP_F16 (/ TP_F32 where stated); sizes in elements. */

/* dst[c][r] = cast(f(src[r][c])), r < R; exact zeros for R <= r < Rpad; dst is [C][ldd], ldd >= Rpad.  f = identity, or with
 * `mean_rstd` (fp32 [R][2]) the LayerNorm (v - mean_r) rstd_r gamma_c + beta_c (gamma / beta fp32 [C]).  Source row r lives at
 * src + (r / rows_per_batch) batch_stride + (r % rows_per_batch) ld (rows_per_batch <= 0 or >= R: contiguous rows, ld apart).
 * colsum_part (optional, `colsum_floats` floats available, >= ceil(Rpad / 64) * C): [ceil(Rpad / 64)][C] column sums of the SOURCE
 * values of each 64-row block, the last partial block included.  C, ld, ldd, Rpad, batch_stride: multiples of 8. */
int tp_test_bw_transpose(int src_dtype, int dst_dtype, const void* src, int64_t ld, int rows_per_batch, int64_t batch_stride,
                         int R, int C, void* dst, int64_t ldd, int Rpad, const float* mean_rstd, const float* gamma,
                         const float* beta, float* colsum_part, size_t colsum_floats, void* stream);
/* `count` (1 .. 8) plain transposes dst_i [C_i][Rpad_i] = cast(src_i [R_i][C_i], rows ld_i apart) in ONE launch.  The six arrays
 * are HOST arrays of `count` entries. */
int tp_test_bw_transpose_batch(int src_dtype, int dst_dtype, int count, const void* const* src, const int64_t* ld, const int* R,
                               const int* C, void* const* dst, const int* Rpad, void* stream);
/* part[slice][c] = sum over the slice's rows of src[r][c] (fp32; src [R][ld], C % 8 == 0) — RETURNS the number of slices written
 * (>= 1; a fixed function of R and C), or a negative status.  `part_floats` >= min(512, max(1, R / 64)) * C.  amax_part (optional,
 * `amax_floats` >= 4096): max |v| per workgroup, NaN sticks; *amax_count (HOST int) = the number of entries written. */
int tp_test_bw_colsum_rows(int dtype, const void* src, int64_t ld, int64_t R, int C, float* part, size_t part_floats,
                           float* amax_part, size_t amax_floats, int* amax_count, void* stream);
/* out[i] = cast(out_scale[0] * sum_k part[k * part_stride + i]), i < n, k in part order; out dtype TP_BF16 / TP_F16 / TP_F32;
 * out_scale optional (device fp32). */
int tp_test_bw_reduce_parts(int dst_dtype, const float* part, int64_t part_stride, int nparts, int64_t n, void* out,
                            const float* out_scale, void* stream);
/* The same sum in two stages (up to 32 slices of parts, then the slices): n and part_stride multiples of 4, `scratch_floats` >=
 * 32 * n; n_out (-1: n) = the number of leading columns written. */
int tp_test_bw_reduce_many_parts(int dst_dtype, const float* part, int64_t part_stride, int nparts, int n, void* out, float* scratch,
                                 size_t scratch_floats, const float* out_scale, int n_out, void* stream);
/* scale[0] = S = 2^k with max(amax_part) * S in [16, 32), |k| <= 60; S = 1 for a maximum of 0 / inf / NaN; scale[1] = 1 / S. */
int tp_test_bw_dynamic_scale(const float* amax_part, int nparts, float* scale, void* stream);
/* dst_f16[i] = saturate(src[i] * scale[0]), n % 8 == 0; sat_flag (optional device int32): 1 (bit 0) is ORed in when some
 * |src[i] * scale[0]| >= 65520 or is NaN. */
int tp_test_bw_scale_cast(int src_dtype, const void* src, int64_t n, const float* scale, void* dst_f16, int* sat_flag, void* stream);
/* LayerNorm backward over `rows` rows of 1024 on `nblocks` workgroups (four rows each per sweep): dx (gdtype) from dy (gdtype),
 * x (fp16), mean_rstd (fp32 [rows][2]) and gamma (fp32 [1024]); part [nblocks][3][1024] (`part_floats` >= nblocks * 3072) = every
 * workgroup's partial sums of dgamma, dbeta and the column sums of the ROUNDED dx — every workgroup writes its slab, also one
 * without rows.  xn (optional, needs beta) = the LayerNorm's output in gdtype.  sat_flag (optional): 2 (bit 1 of
 * tp_backward's status word) is ORed in when an fp16 dx reaches 65520 and is clamped. */
int tp_test_bw_ln_backward(int gdtype, const void* dy, const void* x_f16, const float* mean_rstd, const float* gamma, void* dx,
                           float* part, size_t part_floats, int nblocks, int64_t rows, const float* beta, void* xn, int* sat_flag,
                           void* stream);
/* Region-attention backward: q [B M, 1024], k / v [B grid^2, 1024] fp16; dout, dq [B M, 1024], dk, dv [B grid^2, 1024] gdtype.
 * mask_mode 0: the unmasked launch (mask, dmask NULL).  1 / 2: the additive fp32 mask ([s*s] | [(M B) 8, s*s]) enters the
 * recomputed logits; dmask (optional, fp32, the mask's layout) = dL/dmask times inv_scale[0] (optional).  A mode-1 dmask needs
 * part (`part_bytes` >= B M ceil4(s*s) * 4) and redscratch (`redscratch_floats` >= 32 * ceil4(s*s)).  sat_flag: 4 (bit 2)
 * when an fp16 dq / dk clamps. */
int tp_test_bw_region_attention(int gdtype, const void* q, const void* k, const void* v, const void* dout, void* dq, void* dk,
                                void* dv, int B, int grid, int s, const float* mask, int mask_mode, float* dmask,
                                const float* inv_scale, float* part, size_t part_bytes, float* redscratch, size_t redscratch_floats,
                                int* sat_flag, void* stream);
/* dx [B, grid^2, 1024] (dtype, contiguous) = downsample^T(dq0 fp32 [B (grid/s)^2, 1024]) * inv_scale[0] (optional). */
int tp_test_point_queries_bwd(int dtype, const float* dq0, const float* inv_scale, void* dx, int B, int grid, int s, void* stream);
/* C [M, ldc] = cast(out_scale[0] * (A [M, lda] · W [N, K]^T) * gelu'(Z [M, ldz])) — the data-gradient GEMM of tp_backward with its
 * training epilogue: flags 0 or TP_LINEAR_GELU_BWD (then Z, fp16, is required), out_scale optional, tile 0 (auto) / 128 / 256.
 * N % 128 == 0, K % 64 == 0; the training epilogue exists for 16-bit outputs only (TP_F32 with Z or out_scale: TP_ERR_INVALID_ARG). */
int tp_test_linear_bwd(int M, int N, int K, int dtype, int out_dtype, int flags, const void* A, int64_t lda, const void* W, void* C,
                       int64_t ldc, const void* Z, int64_t ldz, const float* out_scale, int tile, void* stream);

/* ---- test hooks: the weight-gradient contraction dW [n_out, k_in] = dY^T · X over `rows` token rows, as tp_backward launches it
 * (tests/test_gpu_wgrad_edges.py).  The public tp_wgrad fixes half of the launchers' options; these do not. */

/* Host logic only, no GPU needed: the split the launchers would use for this shape — *splits = S groups of *rows_per_split = Ks
 * contraction rows each (Ks a multiple of 64; S * n_out * k_in * 4 bytes of `part` are written).  It CALLS the launchers' rule
 * (csrc/tp_internal.h: wgrad_plan), it is no copy of it.  transposed 0: the in-place form (rpad ignored); 1: the transposed form,
 * whose split follows rpad (a multiple of 1024, >= rows).  rows > 0, n_out % 8 == 0, k_in % 256 == 0, else TP_ERR_INVALID_ARG. */
int tp_test_wgrad_plan(int64_t rows, int n_out, int k_in, int transposed, int64_t rpad, int* splits, long long* rows_per_split);

/* Pass-through to wgrad_tt_launch (transposed 0) / wgrad_tn_launch (transposed 1): same objects, same kernels as tp_backward.
 *   dy [rows, ldy] (dtype), read in place; only columns 0 .. n_out - 1 of rows 0 .. rows - 1 may reach the result.
 *   transposed 0:  x [rows, ldx] (dtype) read in place; row r lives at x + (r / rows_per_batch) batch_stride + (r % rows_per_batch)
 *       ldx (rows_per_batch 0 or >= rows: contiguous; else a multiple of 64, >= 128 — the launcher refuses others).  OR the four
 *       x_part pointers with x NULL: k_in = 4 n_part columns from four tensors with the same ldx / rows_per_batch / batch_stride.
 *   transposed 1:  x = X^T [k_in, ldx] with ldx = rpad (a multiple of 1024, >= rows) and ZEROS in columns rows .. rpad - 1 (the
 *       caller's contract); no parts, no rows_per_batch / batch_stride, no split_row.
 *   grad_out (out_dtype: TP_BF16 / TP_F16 / TP_F32) = cast(out_scale[0] * dW) (out_scale: device fp32, optional), added to what
 *       grad_out holds when accumulate = 1 (TP_F32 only).  0 < split_row < n_out: rows [0, split_row) of dW go to grad_out, rows
 *       [split_row, n_out) to grad_out_hi; either side (not both) may be NULL — it is not reduced and nothing is written through it.
 *   counters (optional): ONE tile-queue slot as tp_backward hands one to every launch — `counter_ints` >= 32 device ints
 *       ([4 groups][8 XCDs] queue heads), ZEROED by the caller before EVERY launch (the launch leaves its draws in them).  The
 *       launchers pass the slot on only when S <= 4; with more splits it is ignored and comes back untouched.
 *   part: `part_bytes` >= S * n_out * k_in * 4 (tp_wgrad_workspace_bytes always suffices), 256-byte aligned; all of it is scratch.
 * Checked on the host before anything is enqueued (TP_ERR_INVALID_ARG, tp_last_error() says why): NULL pointers, 16-byte alignment
 * of dy / x / parts / grad_out / grad_out_hi (256 of part, 4 of out_scale / counters), accumulate with a 16-bit out_dtype, parts /
 * split_row / batch strides together with the transposed form, ldy < n_out, strides shorter than a row.  Shapes the launchers
 * themselves refuse (k_in % 256, n_out % 8, strides % 8, rows_per_batch) come back with the launcher's message ("tp wgrad: ..."),
 * a part too small with TP_ERR_WORKSPACE. */
int tp_test_wgrad(const void* dy, int64_t ldy, const void* x, int64_t ldx, int rows_per_batch, int64_t batch_stride,
                  const void* x_part0, const void* x_part1, const void* x_part2, const void* x_part3, int n_part,
                  int64_t rows, int n_out, int k_in, int dtype, int out_dtype, void* grad_out, void* grad_out_hi, int split_row,
                  const float* out_scale, int accumulate, int* counters, size_t counter_ints, void* part, size_t part_bytes,
                  int transposed, void* stream);

#ifdef __cplusplus
}
#endif
#endif
