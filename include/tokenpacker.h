/*
 * tokenpacker.h — C ABI of libtokenpacker_hip.so (MI355X / gfx950).
 *
 * Drop-in boundary for ONE hot path: the TokenPacker region-to-point visual projector of
 * CircleRadon/TokenPacker, reference `llava/model/multimodal_projector/builder.py:39-137`
 * (class TokenPacker; called from `llava/model/llava_arch.py:97`).  The reference has no FFI of
 * its own (it is 100 % eager PyTorch); the entry points below are what a binding for this path
 * has to offer, and each one names the reference code it replaces.  The Python side
 * (`tokenpacker_amd/_capi.py`) binds them with ctypes; INTEGRATION.md shows the stub a
 * maintainer of the reference would add.
 *
 * Conventions
 *  - Plain C types only: device pointers, sizes, element strides, an opaque stream handle
 *    (`hipStream_t` passed as `void*`; NULL = the legacy default stream).
 *  - The caller owns every buffer.  The library allocates nothing on the device; its only global state is a
 *    thread-local error string, the tuning table of tp_set_tuning() and, per caller stream, one side stream +
 *    event pair that tp_forward forks from / joins back into `stream` for the query side of the path.
 *  - Every call only ENQUEUES work (on `stream` and that side stream); it never synchronises the device.
 *  - Return value: 0 on success, a negative tp_status otherwise; tp_last_error() describes the
 *    failure for the calling thread.  Nothing throws across the ABI.
 *  - All tensors are row-major.  `dtype` is the element type of activations AND weights.
 */
#ifndef TOKENPACKER_H_
#define TOKENPACKER_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI 5 (round 6): tp_linear_args.reserved1 became `ldw` and the packed-weight image's layout changed (w_cc_v3: interleaved
 * hi_t | lo_t K-tile pairs) — both already in round 5 under a stale 4 —, TP_TUNE_DECOUPLE_K and TP_TUNE_BWD_CHAIN (18 knobs), the probe instantiations
 * and test hooks left the product library (tokenpacker_test.h / libtokenpacker_exp.so), tp_debug_counter. */
/* ABI 6: additive — tp_input_grads, tp_backward_inputs_workspace_bytes, tp_backward_inputs and tp_backward_inputs_parts (opt-in
 * gradients with respect to x / x_multi).  Every ABI 5 entry point, struct and workspace size is unchanged, and so are its results. */
/* ABI 6, extended (detected by symbol; the version stays 6): tp_attn_mask, tp_forward_train_masked, tp_forward_parts_masked and
 * tp_backward_masked (training with an attn_mask, and its gradient).  Nothing else changes. */
/* ABI 6, extended again (by symbol, the version stays 6): tp_grad_sink, tp_backward_sink and tp_backward_plan (a backward that skips
 * the gradients of frozen parameters and can accumulate into fp32 buffers).  Every older entry point keeps its behaviour and its bits. */
/* ABI 6, extended a third time (by symbol, the version stays 6): tp_optim_tensor, tp_optim_hyper, tp_optim_state,
 * tp_optim_workspace_bytes and tp_optim_step (gradient clipping and AdamW on those fp32 buffers).  Nothing else changes. */
/* ABI 6, extended a fourth time (by symbol, the version stays 6): tp_desc_known_flags, TP_DESC_RAW_F32 (the raw parameters handed to
 * tp_pack_weights / tp_backward* may be fp32 master weights, read in place) and tp_optim_hyper.dtype = TP_F32 (AdamW on fp32
 * parameters that are their own masters).  Without the flag / with a 16-bit optimizer dtype nothing changes, bits included. */
/* ABI 6, extended a fifth time (by symbol, the version stays 6): tp_optim_sumsq and tp_optim_apply — tp_optim_step cut in two with
 * room for a collective in between, for an optimizer whose state is sharded across ranks.  tp_optim_step is unchanged, bits included. */
/* ABI 6, extended again (by symbol, the version stays 6): tp_shift_ce_args, tp_shift_ce_workspace_bytes, tp_shift_ce_forward and
 * tp_shift_ce_backward — the LLM's shifted cross-entropy on given logits.  Nothing else changes. */
#define TP_ABI_VERSION 6

typedef enum tp_status {
    TP_OK = 0,
    TP_ERR_INVALID_ARG = -1,   /* NULL pointer, bad shape, unsupported dtype ...                  */
    TP_ERR_BAD_SCALE = -2,     /* raw_grid % scale_factor != 0 (reference builder.py:51-52)       */
    TP_ERR_WORKSPACE = -3,     /* workspace / packed buffer too small                             */
    TP_ERR_LAUNCH = -4         /* HIP reported an error when enqueueing                           */
} tp_status;

typedef enum tp_dtype {
    TP_BF16 = 0,
    TP_F16 = 1,
    TP_F32 = 2                 /* only valid as tp_desc.out_dtype (fp32-output validation mode)   */
} tp_dtype;

/* Problem descriptor.  Mirrors the constructor arguments of the reference module
 * (builder.py:40-49: raw_grid=24, embed_dim=1024, num_heads=8, kv_dim=1024, hidden_size,
 * scale_factor) plus the batch.  embed_dim / kv_dim / the 4096-wide multi-level input are fixed
 * by the reference (builder.py:61,67 hard-code nn.Linear(4096,1024)). */
typedef struct tp_desc {
    int32_t batch;         /* B: images or HD crops                                               */
    int32_t raw_grid;      /* g: 24 for CLIP-L/14 @ 336 px; tokens per image N = g*g              */
    int32_t scale_factor;  /* s: must divide raw_grid; M = (g/s)^2 coarse queries                 */
    int32_t hidden_size;   /* D: LLM width (multiple of 128)                                      */
    int32_t dtype;         /* tp_dtype of x, x_multi and all weights: TP_BF16 or TP_F16           */
    int32_t out_dtype;     /* tp_dtype of `out`: == dtype, or TP_F32                              */
    float   ln_eps;        /* 1e-6 (builder.py:48)                                                */
    int32_t flags;         /* 0 | TP_DESC_TRAIN_PACK (tp_pack_weights) | TP_DESC_MASKED (sizes of a masked forward) |
                            * TP_DESC_RAW_F32 (tp_pack_weights, tp_backward*); other bits 0 */
    const struct tp_tuning* tuning;    /* ABI 4: the tuning context this call reads its knobs from; NULL: the process-wide table */
} tp_desc;
/* tp_pack_weights only: the image will serve tp_forward_train / tp_backward — the weights that only the inference
 * schedules read (Wc / d of the fused LayerNorm chain, the per-head transposes of the absorbed schedule, the out_proj fold)
 * are not built.  A training step re-packs every step (the parameters just changed) and must not pay for them. */
#define TP_DESC_TRAIN_PACK 1
/* tp_workspace_bytes / tp_forward_masked: the forward carries an attn_mask.  The mask-less scale_factor-2 schedule never
 * writes K | V (attention runs in the in-projections' epilogues) and its workspace has no room for them; a masked forward
 * runs the plain schedule, which does — size its workspace with this flag set (tp_forward_masked checks). */
#define TP_DESC_MASKED 2
/* tp_pack_weights and every tp_backward* entry point (tp_backward_sink included): EVERY pointer of the tp_weights handed over as
 * `raw` addresses fp32 elements — the fp32 master weights of a module that runs under autocast — instead of desc.dtype elements;
 * desc.dtype stays the compute dtype (bf16 / fp16).  Each fp32 element is first rounded to desc.dtype exactly as Tensor.to(dtype)
 * rounds it (to nearest even, NaN stays NaN, overflow becomes +-inf), on load, inside the kernel that reads it; from there the code
 * does what it does with a 16-bit source.  The packed image (status word and clamp count included), every dgrad operand and every
 * gradient are byte-identical to those of 16-bit copies made on the host, and nothing — not the LayerNorm fold, not the fp32
 * biases — ever reads the unrounded value.  Every pointer must be 16-byte aligned (TP_ERR_INVALID_ARG otherwise: there is no
 * scalar path).  Other entry points ignore the flag.  A library that predates it answers with its "unknown flags" error; a binding
 * asks tp_desc_known_flags (detected by symbol). */
#define TP_DESC_RAW_F32 4

/* The 23 tensors of the reference state dict, all of element type desc.dtype (all fp32 under
 * TP_DESC_RAW_F32), each contiguous, nn.Linear layout [out_features, in_features]. */
typedef struct tp_weights {
    const void* q_proj_1_weight;        /* [1024,1024]  builder.py:59 (no bias)                   */
    const void* k_proj_1_0_weight;      /* [1024,4096]  builder.py:61                             */
    const void* k_proj_1_0_bias;        /* [1024]                                                 */
    const void* k_proj_1_2_weight;      /* [1024,1024]  builder.py:64                             */
    const void* k_proj_1_2_bias;        /* [1024]                                                 */
    const void* v_proj_1_0_weight;      /* [1024,4096]  builder.py:67                             */
    const void* v_proj_1_0_bias;
    const void* v_proj_1_2_weight;      /* [1024,1024]  builder.py:70                             */
    const void* v_proj_1_2_bias;
    const void* ln_q_1_weight;          /* [1024]       builder.py:73                             */
    const void* ln_q_1_bias;
    const void* ln_k_1_weight;          /* [1024]       builder.py:74                             */
    const void* ln_k_1_bias;
    const void* ln_v_1_weight;          /* [1024]       builder.py:75                             */
    const void* ln_v_1_bias;
    const void* clip_attn_in_proj_weight;   /* [3072,1024]  builder.py:77 (q,k,v stacked)         */
    const void* clip_attn_in_proj_bias;     /* [3072]                                             */
    const void* clip_attn_out_proj_weight;  /* [1024,1024]                                        */
    const void* clip_attn_out_proj_bias;    /* [1024]                                             */
    const void* mlp_0_weight;           /* [D,1024]     builder.py:79                             */
    const void* mlp_0_bias;             /* [D]                                                    */
    const void* mlp_2_weight;           /* [D,D]        builder.py:82                             */
    const void* mlp_2_bias;             /* [D]                                                    */
} tp_weights;

/* ---- library info ---------------------------------------------------------------------------- */
int         tp_version(void);                 /* == TP_ABI_VERSION                                 */
const char* tp_last_error(void);              /* thread-local, never NULL                          */
/* ABI 6 extension (detected by symbol): the OR of every tp_desc.flags bit this library accepts. */
int         tp_desc_known_flags(void);

/* ---- sizes ----------------------------------------------------------------------------------- */
/* Bytes of the packed-weight buffer for (hidden_size, dtype); 0 on invalid arguments. */
size_t tp_packed_weight_bytes(const tp_desc* desc);
/* Byte offset, inside the packed-weight buffer, of an int32[64] status block written by tp_pack_weights():
 * [0] = number of weight elements that did not fit the fp16 range the kernels keep every post-first-layer weight in
 *       and were clamped to +-65504 (a bf16 model can hold such values; results would silently differ from the
 *       reference, so the Python wrapper raises OverflowError when it is non-zero),
 * [1] = 1 when the out_proj∘mlp[0] fold was built (TP_TUNE_FOLD_OUT_PROJ set at pack time),
 * [2] = 1 when the fused LayerNorm chain's Wc = W'·W2 / d = W'·b2 were built (TP_TUNE_FUSE_KV_LN at pack time).
 * 0 on invalid args. */
size_t tp_packed_status_offset(const tp_desc* desc);
/* Bytes of scratch tp_forward() needs for this descriptor (depends on batch); 0 on invalid args. */
size_t tp_workspace_bytes(const tp_desc* desc);
/* The first TP_WORKSPACE_STATUS_BYTES of every workspace are a STATUS BLOCK the caller zeroes once (after allocating):
 *   int32[0]  sticky fp16-saturation bits.  Every activation between the kernels is fp16 and every epilogue CLAMPS to +-65504
 *             where the reference's fp16 / bf16 arithmetic would have produced inf or a larger finite value; an inference
 *             forward that clamps anything ORs bit k into this word (k = 1 + index of the stage in tp_forward_staged's list,
 *             bit 0 = the query side).  The library never clears it: read it back whenever convenient (a 4-byte copy),
 *             nonzero = some forward since the last clear differs from what the reference would have computed.
 *             Covered: every fp16 epilogue of the GEMM kernels and the K-split reduction of small batches (ABI 4).  NOT covered: a
 *             NaN inside a GEMM epilogue (the running max that tracks |v| is a v_max3, which drops NaN operands; the K-split
 *             reduction does report NaN), and training forwards (their epilogues have no register to spare) — scan those
 *             with tp_debug_count_saturated, which counts values at the bound AND NaNs. */
#define TP_WORKSPACE_STATUS_BYTES 256

/* ---- one-time weight preparation -------------------------------------------------------------
 * Replaces what `TokenPacker.__init__` + `load_state_dict` leave in the nn.Parameters
 * (builder.py:59-83, llava_arch.py:78-83): re-lays the 23 tensors out for the kernels — K/V first
 * layers concatenated into one [2048,4096] operand, the three LayerNorm affines folded into the
 * attention in-projection (W' = W·diag(gamma), c = rowsum(W'), b' = W·beta + b), out_proj folded into
 * mlp[0] (W = Wm0·Wout, b = Wm0·bout + bm0), biases widened to fp32.  Must be re-run whenever a parameter changes.  `packed` needs tp_packed_weight_bytes(). */
int tp_pack_weights(const tp_desc* desc, const tp_weights* raw, void* packed, size_t packed_bytes,
                    void* stream);
/* The library keeps a HOST-side note of what tp_pack_weights wrote at an address (hidden size, dtype, TP_DESC_TRAIN_PACK) and
 * refuses a forward the image cannot serve.  The note describes the address, not the bytes: before the memory of an image is
 * freed / reused for anything but a re-pack in place, drop it with tp_pack_forget (an unknown address is accepted unchecked). */
int tp_pack_forget(const void* packed);

/* ---- the hot path ------------------------------------------------------------------------------
 * Replaces `TokenPacker.forward((x, x_multi))` (builder.py:107-137).
 *   x        [B, g*g, 1024]  element strides x_strides[3]  (innermost stride must be 1)
 *   x_multi  [B, g*g, 4096]  element strides xm_strides[3] (innermost stride must be 1)
 *            — strides because the CLIP tower hands over `[:, 1:]` slices of CLS-prefixed
 *              buffers (clip_encoder.py:37-38,62); base pointers must be 16-byte aligned and row
 *              strides multiples of 8 elements.
 *   out      [B, M, D] contiguous, element type desc.out_dtype.
 * `attn_mask` of the reference signature is always None on the real path (llava_arch.py:97): tp_forward is the
 * mask-less call, tp_forward_masked below honours one.
 *
 * Schedules (same function, same parity gates; what differs is which intermediates exist):
 *   training (tp_forward_train)     : every layer as its own GEMM — the backward needs H2, K and V;
 *   inference, scale_factor 2       : fused LayerNorm chain (TP_TUNE_FUSE_KV_LN): the K/V second layer is computed for its
 *                                     LayerNorm statistics only, the in-projection reads Hkv through Wc = W'·W2, and region
 *                                     attention runs in the epilogues of those two GEMMs (TP_TUNE_FUSE_ATTN): K, V are not written;
 *   inference, scale_factor >= 3    : K/V in-projections absorbed into the query side (TP_TUNE_ABSORB_KV, see
 *                                     tp_region_attention_absorbed) — on the fused LayerNorm chain too: the second K/V layer is
 *                                     computed for its statistics only and the attention kernel walks Hkv. */
int tp_forward(const tp_desc* desc,
               const void* x, const int64_t x_strides[3],
               const void* x_multi, const int64_t xm_strides[3],
               const void* packed_weights,
               void* out,
               void* workspace, size_t workspace_bytes,
               void* stream);

/* tp_forward with the `attn_mask` argument of `TokenPacker.forward(x, attn_mask)` (builder.py:107,130), as
 * nn.MultiheadAttention applies it: an ADDITIVE fp32 mask on the scaled logits (a boolean mask is the caller's
 * 0 / -inf).  mask_mode 1: attn_mask [s*s] — the reference's 2-D (L=1, S=s*s) form, shared by every image, region
 * and head; mask_mode 2: attn_mask [(M*B)*8, s*s] — its 3-D (N*num_heads, L=1, S) form with the reference's batch
 * index N = region * B + image (divide_feature's order, builder.py:96-105); mask_mode 0: none.  Key index inside a
 * region: a*s + b for fine token (i*s + a, j*s + b).  Inference; training with a mask: tp_forward_train_masked /
 * tp_backward_masked (below). */
int tp_forward_masked(const tp_desc* desc,
                      const void* x, const int64_t x_strides[3],
                      const void* x_multi, const int64_t xm_strides[3],
                      const void* packed_weights, void* out, void* workspace, size_t workspace_bytes,
                      const float* attn_mask, int mask_mode, void* stream);

/* tp_forward with x_multi given as its FOUR [B, g*g, 1024] sources — the CLIP hidden states 12, 16, 22, 23 that
 * `CLIPVisionTower.feature_select` concatenates (clip_encoder.py:28-32) — each with the element strides
 * `part_strides` (e.g. the `[:, 1:]` slice of a [B, 577, 1024] hidden state).  The first GEMM walks the four
 * sources as K-ranges, so the tower's torch.cat (1.2 GB written and read again at B = 256) never happens.
 * Bit-identical to tp_forward on the concatenated tensor. */
int tp_forward_parts(const tp_desc* desc,
                     const void* x, const int64_t x_strides[3],
                     const void* const xm_parts[4], const int64_t part_strides[3],
                     const void* packed_weights,
                     void* out,
                     void* workspace, size_t workspace_bytes,
                     void* stream);

/* Same as tp_forward, additionally recording caller-owned HIP events (hipEvent_t, created with
 * timing enabled) on `stream` at the TP_NUM_STAGES+1 stage boundaries, so a benchmark can time each
 * kernel of the schedule inside the real forward (bench.py's `roofline` object).  Stages, in order:
 * point_queries, kv_layer0(+GELU), kv_layer2(+stats), kv_inproj(LN-fold), q_proj_1(+stats),
 * q_inproj(LN-fold), region_attention, out_proj, mlp0(+GELU), mlp2.
 * (The staged forward runs on ONE stream.  With attention in the in-projections' epilogues — TP_TUNE_FUSE_ATTN, the
 * scale_factor-2 default — the K launch needs Q: the whole query side then runs inside the first stage, the two q stages are
 * empty, `kv_inproj` is the K launch (logits) and `region_attention` the V launch (softmax-weighted sums -> O).) */
#define TP_NUM_STAGES 10
int tp_forward_staged(const tp_desc* desc,
                      const void* x, const int64_t x_strides[3],
                      const void* x_multi, const int64_t xm_strides[3],
                      const void* packed_weights,
                      void* out,
                      void* workspace, size_t workspace_bytes,
                      void* stream,
                      void* const* stage_events, int n_events);

/* ---- per-kernel entry points (used by the parity tests; same kernels tp_forward launches) ---- */

/* NUMERICS NOTE for the per-kernel entry points: activations BETWEEN kernels are always fp16,
 * whatever desc.dtype is (bf16 models: weights/inputs widen to fp16 exactly; keeping fp16
 * intermediates is what brings the bf16 path within 1e-3 of exact math, DESIGN.md "Numerics").
 *
 * Coarse point queries: fp32 bilinear (align_corners=False) g*g -> (g/s)^2, rounded once to
 * desc.dtype (the reference's cast, builder.py:117-118) and stored as fp16.
 * x has element type desc.dtype; q0 is fp16 [B, M, 1024] contiguous. */
int tp_point_queries(const tp_desc* desc, const void* x, const int64_t x_strides[3], void* q0,
                     void* stream);

/* Region-to-point attention core on projected tensors (post in-proj, pre out-proj), all fp16:
 *   q [B, M, 1024], k and v [B, g*g, 1024] contiguous; o [B, M, 1024].
 * 8 heads x d=128, logits scaled by 1/sqrt(128), softmax over the s*s tokens of the query's own
 * region.  Replaces divide_feature (builder.py:96-105, 122-124) + the bmm/softmax/bmm of
 * nn.MultiheadAttention (builder.py:126-130; torch/nn/functional.py:6576-6594). */
int tp_region_attention(const tp_desc* desc, const void* q, const void* k, const void* v, void* o,
                        void* stream);

/* The same attention with the K/V in-projections ABSORBED into the query side — what tp_forward runs for
 * scale_factor >= 3 (TP_TUNE_ABSORB_KV): with one query per region, Q_h·(W'k n_t + b'k)_h = (W'k_h^T Q_h)·n_t + const and
 * sum_t p_t (W'v n_t + b'v)_h = W'v_h (sum_t p_t n_t) + b'v_h, so the two [B·576,1024]x[1024,1024] in-projection GEMMs
 * shrink to query-sized work (1/s^2).  All fp16:
 *   qt [B, M, 8, 1024] = per-head Q_h · W'k_h (W' = LayerNorm-folded in_proj rows of k),
 *   h2k / h2v [B, g*g, 1024] = the PRE-LayerNorm second-layer outputs, normalised on load with
 *   mr_k / mr_v [B*g*g][2] = their per-row (mean, rstd) from tp_ln_finalize;
 *   u [B, M, 8, 1024] = per head sum_t softmax_t(qt_h·n^k_t / sqrt(128)) n^v_t   (then O_h = u_h·W'v_h^T + b'v_h).
 * s*s <= 64. */
int tp_region_attention_absorbed(const tp_desc* desc, const void* qt, const void* h2k, const void* h2v,
                                 const float* mr_k, const float* mr_v, void* u, void* stream);

/* Generic fused linear used for every dense contraction of the path (11 nn.Linear calls of
 * builder.py:112,113,120,126-130,136):  C[M,N] = epilogue(A[M,K] · W[N,K]^T).
 * flags: TP_LINEAR_* below.  `bias` fp32 [N] or NULL.  With TP_LINEAR_LN_FOLD the epilogue applies
 * a LayerNorm that precedes the linear: C = rstd_m·(acc − mu_m·colsum_n) + bias_n, with
 * `row_mean_rstd` = fp32 [M][2] (mean, rstd) per row of A, produced by tp_ln_finalize().
 * With TP_LINEAR_ROW_STATS the kernel writes, per 128 output columns, the (mean, M2) of ITS rounded output — M2 = sum of
 * squared deviations from that slab's own mean; merged by Chan's formula, accurate even when |mean| >> std — to
 * `row_stats_out` ([N/128][M][2]: one slab per 128 output columns; tp_linear_stats_parts() returns N/128).
 * One call addresses at most 4 GiB of output, (M + 256) * ldc * sizeof(element) < 2^32 (the stores go through a
 * range-checked 32-bit buffer descriptor); larger problems are rejected with TP_ERR_INVALID_ARG.  tp_forward /
 * tp_forward_parts split a batch beyond that bound (about 1800 images at hidden_size 4096) into consecutive chunks
 * themselves — no operation mixes images, the result is bit-identical; the training entry points reject it. */
enum {
    TP_LINEAR_GELU = 1,        /* exact erf GELU after bias (nn.GELU(), builder.py:63,69,81)      */
    TP_LINEAR_LN_FOLD = 2,
    TP_LINEAR_ROW_STATS = 4,
    TP_LINEAR_OUT_F32 = 8,     /* retired: use tp_linear_args.out_dtype = TP_F32                    */
    /* The next two belong to the TRAINING entry points (tp_forward_train* / tp_backward*), which own the pre-activation buffer both
     * need; tp_linear_args has no field for it and tp_linear() refuses either flag with TP_ERR_INVALID_ARG before anything is enqueued. */
    TP_LINEAR_SAVE_PRE = 16,   /* with GELU: also store the pre-activation (training forward; not through tp_linear)       */
    TP_LINEAR_GELU_BWD = 32,   /* multiply the result by gelu'(z), z = fp16 pre-activations (backward; not through tp_linear) */
    TP_LINEAR_NO_STORE = 64    /* with ROW_STATS: compute the row statistics of the (unrounded) result and store NOTHING else
                                  — C may be NULL (the LayerNorm statistics of a tensor nobody needs to materialise)     */
};
typedef struct tp_linear_args {
    int32_t M, N, K;           /* N % 128 == 0, K % 64 == 0                                        */
    int32_t dtype;             /* element type of A and W: TP_BF16 / TP_F16                        */
    int32_t out_dtype;         /* element type of C: TP_BF16 / TP_F16 / TP_F32                     */
    int32_t flags;
    int32_t rows_per_batch;    /* A row r lives at A + (r / rpb)*a_batch_stride + (r % rpb)*lda   */
    int32_t a_k_dup;           /* (ABI 5; was reserved0) 0, or a multiple of 64 <= K / 2: the first a_k_dup K-elements of A are each used for
                                * TWO consecutive 64-wide K-tiles of W, the rest once (A is K - a_k_dup wide) — the per-head V GEMM of the absorbed
                                * schedule (u against weight rows laid out as K-tile pairs hi_t | lo_t).  Contiguous A, N % 128 == 0; served by the
                                * pair kernel or the 128-tile kernel by launch size (TP_TUNE_PAIR_GEMM), bit-identical either way */
    int64_t a_batch_stride;    /* elements; ignored when rows_per_batch >= M                       */
    int64_t lda;               /* elements between consecutive rows of A                           */
    int64_t ldc;               /* elements between consecutive rows of C                           */
    const void* A;
    const void* W;             /* [N,K], rows ldw elements apart (ldw = 0: contiguous)             */
    const float* bias;
    void* C;
    const float* row_mean_rstd;/* LN_FOLD: fp32 [M][2]                                             */
    const float* colsum;       /* LN_FOLD: fp32 [N]                                                */
    int32_t tile;              /* 0 = auto, 128 or 256: force the block tile                       */
    int32_t ldw;               /* elements between consecutive rows of W; 0 = K (contiguous).  (ABI 5; round 5: the field was
                                * reserved1.  It exists for tools/stride_ab.py: an isolated LDS-DMA stream over rows a power of two
                                * apart runs at 28 GB/s per CU against 123 with +64 elements of padding — tools/probes/
                                * operand_fetch_probe.hip — but INSIDE the GEMMs, where an XCD's 32 tiles share their operands,
                                * padded A / W / C strides measure +-0.5 %, profiles/r05f_stride_ab.json; nothing is padded) */
    float*  row_stats_out;     /* ROW_STATS                                                        */
} tp_linear_args;
int tp_linear(const tp_linear_args* args, void* stream);
/* (mean, M2) slabs [parts][M][2] written by a TP_LINEAR_ROW_STATS call -> per-row (mean, rstd)
 * [M][2] of nn.LayerNorm(ln_dim, eps) (biased variance), for a TP_LINEAR_LN_FOLD call.  ln_dim == parts * 128. */
int tp_ln_finalize(const float* row_stats, int parts, int64_t M, int ln_dim, float eps,
                   float* row_mean_rstd, void* stream);
/* Number of row-stat slabs a TP_LINEAR_ROW_STATS call with these M,N (and args->tile) writes. */
int tp_linear_stats_parts(const tp_linear_args* args);

/* ---- training: forward that keeps the backward's operands, and the backward pass ---------------------------
 * Stage-1 training of the reference updates ONLY the projector (llava/train/train.py:950-953); the CLIP features
 * come from a frozen, no_grad tower (clip_encoder.py:46).  tp_backward therefore produces the gradients of the
 * 23 parameters (tp_grads mirrors tp_weights, each tensor contiguous, element type desc.dtype) and none for
 * x / x_multi; tp_backward_inputs (below) adds those on request.  Replaces what autograd records for builder.py:107-137.
 *   tp_forward_train : tp_forward + the fp16 pre-GELU activations, into a caller-owned `train_workspace`
 *                      (tp_train_workspace_bytes) that must stay untouched until tp_backward has run.
 *   tp_backward      : dy [B, M, D] contiguous (desc.dtype) -> grads; `raw` = the model's current parameters
 *                      (the same tensors tp_pack_weights packed), `bw_workspace` = scratch
 *                      (tp_backward_workspace_bytes).  Gradients travel in desc.dtype, accumulate in fp32;
 *                      no atomics: results are deterministic. */
typedef struct tp_grads {
    void* q_proj_1_weight;
    void* k_proj_1_0_weight;  void* k_proj_1_0_bias;  void* k_proj_1_2_weight;  void* k_proj_1_2_bias;
    void* v_proj_1_0_weight;  void* v_proj_1_0_bias;  void* v_proj_1_2_weight;  void* v_proj_1_2_bias;
    void* ln_q_1_weight;  void* ln_q_1_bias;  void* ln_k_1_weight;  void* ln_k_1_bias;
    void* ln_v_1_weight;  void* ln_v_1_bias;
    void* clip_attn_in_proj_weight;   void* clip_attn_in_proj_bias;
    void* clip_attn_out_proj_weight;  void* clip_attn_out_proj_bias;
    void* mlp_0_weight;  void* mlp_0_bias;  void* mlp_2_weight;  void* mlp_2_bias;
} tp_grads;
size_t tp_train_workspace_bytes(const tp_desc* desc);
size_t tp_backward_workspace_bytes(const tp_desc* desc);
int tp_forward_train(const tp_desc* desc, const void* x, const int64_t x_strides[3], const void* x_multi,
                     const int64_t xm_strides[3], const void* packed_weights, void* out, void* train_workspace,
                     size_t workspace_bytes, void* stream);
int tp_backward(const tp_desc* desc, const void* x_multi, const int64_t xm_strides[3], const tp_weights* raw,
                const void* packed_weights, const void* train_workspace, const void* dy, const tp_grads* grads,
                void* bw_workspace, size_t bw_workspace_bytes, void* stream);
/* the same two with x_multi as its four sources (see tp_forward_parts) */
int tp_forward_train_parts(const tp_desc* desc, const void* x, const int64_t x_strides[3],
                           const void* const xm_parts[4], const int64_t part_strides[3], const void* packed_weights,
                           void* out, void* train_workspace, size_t workspace_bytes, void* stream);
int tp_backward_parts(const tp_desc* desc, const void* const xm_parts[4], const int64_t part_strides[3],
                      const tp_weights* raw, const void* packed_weights, const void* train_workspace, const void* dy,
                      const tp_grads* grads, void* bw_workspace, size_t bw_workspace_bytes, void* stream);

/* ABI 6: the backward with gradients with respect to the CLIP features (opt-in: a trainable or LoRA-tuned tower, attribution over
 * the features).  Same arguments as tp_backward / tp_backward_parts plus `ig`, the input gradients wanted (each output contiguous,
 * element type desc.dtype, 16-byte aligned; NULL = not wanted):
 *   dx                 [B, N, 1024]: the transpose of the point queries' bilinear downsample applied to dQ1 · Wq1 (fp32, rounded once)
 *   dx_multi           [B, N, 4096]: dZ1 · [Wk0; Wv0] (tp_backward_inputs only)
 *   dx_multi_parts[4]  four [B, N, 1024]: the same product's column slices, bit for bit (tp_backward_inputs_parts only; all or none)
 * `grads` may be NULL: no parameter gradient is computed (a frozen projector in front of a trainable tower).  The workspace is
 * tp_backward_inputs_workspace_bytes (>= tp_backward_workspace_bytes; 0 on a bad descriptor), and its status word has the bits
 * tp_backward's has.  Deterministic like tp_backward; the parameter gradients are those tp_backward computes, bit for bit. */
typedef struct tp_input_grads {
    void* dx;                  /* [B, N, 1024] contiguous, desc.dtype; NULL = not wanted                        */
    void* dx_multi;            /* [B, N, 4096] contiguous; NULL = not wanted (concatenated form)                */
    void* dx_multi_parts[4];   /* four [B, N, 1024] contiguous (the _parts entry point); NULL = none            */
} tp_input_grads;
size_t tp_backward_inputs_workspace_bytes(const tp_desc* desc);
int tp_backward_inputs(const tp_desc* desc, const void* x_multi, const int64_t xm_strides[3], const tp_weights* raw,
                       const void* packed_weights, const void* train_workspace, const void* dy, const tp_grads* grads,
                       const tp_input_grads* ig, void* bw_workspace, size_t bw_workspace_bytes, void* stream);
int tp_backward_inputs_parts(const tp_desc* desc, const void* const xm_parts[4], const int64_t part_strides[3],
                             const tp_weights* raw, const void* packed_weights, const void* train_workspace, const void* dy,
                             const tp_grads* grads, const tp_input_grads* ig, void* bw_workspace, size_t bw_workspace_bytes,
                             void* stream);

/* ABI 6 extension (a binding detects it by symbol): training with the `attn_mask` of tp_forward_masked.  The masked training
 * forward runs the training schedule (which writes K | V anyway: its workspace is tp_train_workspace_bytes, mask or not) with the
 * mask in the attention logits; the masked backward adds the mask to the logits it recomputes, and — when `grad` is non-NULL —
 * returns dL/dmask, the gradient of an additive float mask that is a learnable region bias in the reference (an ordinary
 * autograd leaf there).
 *   mask   fp32 additive mask, laid out as tp_forward_masked takes it (mode 1: [s*s]; mode 2: [(M*B)*8, s*s], batch index
 *          region * B + image) — the SAME values the training forward of this step was given
 *   mode   1 or 2 (0 with mask == NULL and grad == NULL: no mask — the call is then tp_backward_inputs' / tp_backward's)
 *   grad   NULL, or fp32 in the mask's layout: dL/dmask_j = p_j (dP_j - D) summed over whatever shares entry j (mode 1: every
 *          image, query and head; mode 2: nothing — each entry is written once).  Unscaled: the fp16 gradient chain's dynamic
 *          scale is taken out on the device.  Deterministic (mode 1 sums per-query partials in a fixed order), no atomics.
 * -inf may sit at ANY key position, the leading keys included, as long as one key of the row (one head of one query) is finite:
 * every attention kernel, forward and backward, then gives the reference's softmax (tests/test_gpu_attention_masks.py).
 * A FULLY masked row (every key of some head of some query at -inf) is NOT the reference's NaN row.  The attention itself gives NaN
 * for that head (128 elements of O; under the absorbed schedule the head's u, and -65504 in O behind the per-head V GEMM), but every
 * fp16 GEMM epilogue behind it clamps to +-65504 and a clamp turns NaN into -65504 without setting that stage's status bit.  So the
 * query's OUTPUT ROW IS FINITE IN EVERY ELEMENT AND MEANINGLESS; the first stage whose finite result then leaves fp16's range sets
 * its status bit (mlp0_gelu at hidden_size 256), which is how a caller notices: the status word / tp_debug_count_saturated (O: 128
 * elements, then whole rows of A1 / A2).  In training (bf16 model) dL/dmask of that row is NaN in every element, the gradient of
 * out_proj.weight is NaN in the head's 128 input columns, every other parameter gradient and the query's dx / dx_multi / other
 * dmask rows are finite and meaningless, and tp_backward's status word has bits 0 and 2 set.  Every OTHER output row, dx / dx_multi
 * outside that query's region and the dmask rows of other queries keep their bits (tests/test_gpu_mask_train.py::
 * test_fully_masked_row).  A caller that can produce such rows must test for them itself.
 * A per-head mask (mode 2) needs the whole batch in one launch, as in inference.
 *   tp_forward_train_masked  xm_parts NULL: x_multi concatenated (xm_strides its strides); non-NULL: the four sources of
 *                            tp_forward_train_parts (xm_strides their common strides; x_multi ignored)
 *   tp_forward_parts_masked  inference: tp_forward_parts with a mask (workspace sized with TP_DESC_MASKED)
 *   tp_backward_masked       tp_backward_inputs(_parts) with the mask: `grads` and `ig` are both nullable (at least one of them
 *                            or mask->grad must be asked for); `ig` non-NULL takes tp_backward_inputs_workspace_bytes, NULL
 *                            tp_backward_workspace_bytes — no further scratch.  xm_parts as for tp_forward_train_masked.
 * Without a mask (mode 0) every result is tp_backward's / tp_backward_inputs', bit for bit. */
typedef struct tp_attn_mask {
    const float* mask;         /* fp32 additive mask (tp_forward_masked's layout); NULL iff mode == 0            */
    int32_t mode;              /* 1: [s*s] shared by everything; 2: [(M*B)*8, s*s]; 0: none                       */
    int32_t reserved;          /* must be 0 (anything else: TP_ERR_INVALID_ARG)                                   */
    float* grad;               /* NULL, or dL/dmask in the mask's layout (fp32)                                  */
} tp_attn_mask;
int tp_forward_train_masked(const tp_desc* desc, const void* x, const int64_t x_strides[3], const void* x_multi,
                            const void* const xm_parts[4], const int64_t xm_strides[3], const void* packed_weights, void* out,
                            void* train_workspace, size_t workspace_bytes, const float* attn_mask, int mask_mode, void* stream);
int tp_forward_parts_masked(const tp_desc* desc, const void* x, const int64_t x_strides[3], const void* const xm_parts[4],
                            const int64_t part_strides[3], const void* packed_weights, void* out, void* workspace,
                            size_t workspace_bytes, const float* attn_mask, int mask_mode, void* stream);
int tp_backward_masked(const tp_desc* desc, const void* x_multi, const void* const xm_parts[4], const int64_t xm_strides[3],
                       const tp_weights* raw, const void* packed_weights, const void* train_workspace, const void* dy,
                       const tp_grads* grads, const tp_input_grads* ig, const tp_attn_mask* mask, void* bw_workspace,
                       size_t bw_workspace_bytes, void* stream);

/* ABI 6 extension (a binding detects it by symbol): the backward into a GRADIENT SINK.  tp_backward* computes all 23 parameter
 * gradients in the model dtype and overwrites their destination; a partially frozen projector (LoRA-style runs that freeze the K/V
 * branches — 4 x the rows of the query side, a first-layer weight gradient that contracts over K = 4096) pays for gradients nobody
 * reads, and micro-batch accumulation rounds twice per micro-step (bf16 .grad += bf16 g).  The sink says, per parameter, whether its
 * gradient is wanted, and lets every wanted one leave as fp32 — optionally ADDED to what the buffer holds (the fp32 `main_grad`
 * of Megatron / Apex / Transformer Engine).
 *   grads       one pointer per parameter (tp_grads); NULL = not wanted: nothing is computed for it alone, nothing is written
 *   dtype       element type of every non-NULL entry: desc.dtype, or TP_F32 (then every entry 16-byte aligned).  An fp32 entry is
 *               the fp32 sum the model-dtype gradient is rounded from (times the fp16 chain's exact 1 / S): rounding it to desc.dtype
 *               gives tp_backward's value bit for bit; nothing is clamped
 *   accumulate  0: overwrite; 1 (TP_F32 only): out += gradient — one plain load, add and store per element in a fixed order, no
 *               atomics: deterministic
 * tp_backward_sink takes tp_backward_masked's arguments with `sink` in place of `grads`; `sink`, `ig` and `mask` are each nullable
 * (mask NULL = no mask), and at least one output must be asked for: a non-NULL sink entry, an input gradient or mask->grad.
 * Workspace: tp_backward_workspace_bytes, or tp_backward_inputs_workspace_bytes when `ig` is given.  The status word keeps its
 * meaning.  TP_ERR_INVALID_ARG, before anything is enqueued: accumulate with a dtype other than TP_F32 (or a value other than 0 / 1),
 * a dtype that is neither desc.dtype nor TP_F32, a misaligned fp32 entry, nothing asked for.  With every entry non-NULL, dtype =
 * desc.dtype and accumulate = 0 the call IS tp_backward / _inputs / _masked: the same launches in the same order, the same bits.
 * Every wanted gradient of a partial sink has the bits the full backward gives it.
 *
 * tp_backward_plan: which stages a backward runs for what is wanted — pure host logic, no device; tp_backward_sink decides its
 * launches with this same function.  Bit i of `wanted_params` is field i of tp_grads (q_proj_1_weight = bit 0 .. mlp_2_bias =
 * bit 22); the result is an OR of TP_BWD_STAGE_*.  A stage runs if and only if something wanted lies at or below it in the chain
 * (dy -> mlp[2] -> mlp[0] -> out_proj -> attention -> the q | k | v chains -> the K/V layers):
 *   DY          the pass over dy (column sums, max |dy| and scale, the fp16 copy): always (a model-dtype chain that does not want
 *               mlp.2.bias has nothing to take from it and launches nothing); MLP2_BIAS: the reduction into mlp.2.bias
 *   MLP2_WGRAD, MLP0_BIAS, MLP0_WGRAD, OUT_BIAS, OUT_WGRAD    that parameter alone
 *   DZ2, DA1, DO   the dgrads dy -> dZ2 -> dA1 -> dO: anything below the layer, or that layer's own parameters for the dgrad in front
 *   ATTENTION   in_proj_*, any ln_*, q_proj_1, any k_proj_1.* / v_proj_1.*, dx, dx_multi, dmask
 *   Q_CHAIN     dgrad dQ -> dq1 and the LayerNorm-q backward: ln_q_1.*, in_proj_weight (its q third reads the LayerNorm output that
 *               backward writes), q_proj_1.weight, dx
 *   K_CHAIN / V_CHAIN   the same for a K/V branch: its ln_*, *_proj_1.2.* (the bias is the column sum of the LayerNorm backward's dx),
 *               *_proj_1.0.*, in_proj_weight, dx_multi
 *   DZ1         the dgrads dH2 -> dZ1: any k_proj_1.0.* / v_proj_1.0.*, or dx_multi (each half where its chain ran)
 *   KV0_WGRAD   the first K/V layer's column sums and its ONE joint contraction: any of its four parameters; a member that is not
 *               wanted has its reduction skipped
 * in_proj_weight / in_proj_bias are single tensors: wanting one means all three of its thirds (the bias thirds are column sums of
 * dQ, dK and dO: they need the attention backward, not the chains). */
enum { TP_BWD_STAGE_DY = 1 << 0, TP_BWD_STAGE_MLP2_BIAS = 1 << 1, TP_BWD_STAGE_MLP2_WGRAD = 1 << 2, TP_BWD_STAGE_DZ2 = 1 << 3,
       TP_BWD_STAGE_MLP0_BIAS = 1 << 4, TP_BWD_STAGE_MLP0_WGRAD = 1 << 5, TP_BWD_STAGE_DA1 = 1 << 6,
       TP_BWD_STAGE_OUT_BIAS = 1 << 7, TP_BWD_STAGE_OUT_WGRAD = 1 << 8, TP_BWD_STAGE_DO = 1 << 9, TP_BWD_STAGE_ATTENTION = 1 << 10,
       TP_BWD_STAGE_Q_CHAIN = 1 << 11, TP_BWD_STAGE_K_CHAIN = 1 << 12, TP_BWD_STAGE_V_CHAIN = 1 << 13, TP_BWD_STAGE_DZ1 = 1 << 14,
       TP_BWD_STAGE_KV0_WGRAD = 1 << 15, TP_BWD_STAGE_ALL = (1 << 16) - 1 };
typedef struct tp_grad_sink {
    tp_grads grads;      /* NULL entry = this parameter's gradient is not wanted                  */
    int32_t  dtype;      /* element type of every non-NULL entry: desc.dtype or TP_F32            */
    int32_t  accumulate; /* 0: overwrite; 1: out += gradient (TP_F32 only)                        */
} tp_grad_sink;
int tp_backward_sink(const tp_desc* desc, const void* x_multi, const void* const xm_parts[4], const int64_t xm_strides[3],
                     const tp_weights* raw, const void* packed_weights, const void* train_workspace, const void* dy,
                     const tp_grad_sink* sink, const tp_input_grads* ig, const tp_attn_mask* mask, void* bw_workspace,
                     size_t bw_workspace_bytes, void* stream);
uint32_t tp_backward_plan(uint32_t wanted_params, int want_dx, int want_dx_multi, int want_dmask);

/* ---- optimizer step: clip + AdamW on the fp32 gradient buffers (ABI 6 extension, detected by symbol) ----------------------
 * The consumer of what tp_backward_sink accumulates (sink dtype TP_F32, accumulate 1): the reference's stage-1 recipe —
 * `optim = "adamw_torch"` (train.py:81) behind HF's max_grad_norm clipping, per-group lr / weight_decay (llava_trainer.py:164-222) —
 * as three launches per table of up to 32 tensors: the global L2 norm of grad * inv_scale, the clipping coefficient and overflow
 * guard, then torch.optim.AdamW's update (no amsgrad, no maximize) on fp32 master weights with the model-dtype write-back and the
 * zeroing of the gradient buffers.  Per element, with g = grad * inv_scale * clip_coef, in fp32:
 *     p <- p * (1 - lr * weight_decay);  m <- beta1 * m + (1 - beta1) * g;  v <- beta2 * v + (1 - beta2) * g * g;
 *     p <- p - (lr / bc1) * m / (sqrt(v) / sqrt(bc2) + eps),      bc_i = 1 - beta_i ^ step
 * master, exp_avg and exp_avg_sq are stored in fp32, param as the round-to-nearest-even cast of the stored master (no clamp: what
 * Tensor.to does).  Work is cut into chunks of a fixed number of elements and every sum runs in a fixed order: no atomics, results
 * do not depend on the device's CU count, two runs give the same bits.  A table longer than 32 entries is served by consecutive
 * launches.  Enqueue-only, reentrant, allocates nothing.
 *
 *   tp_optim_tensor  one tensor: param (hyper.dtype), master / grad / exp_avg / exp_avg_sq (fp32), all of numel elements, and the
 *                    lr / weight_decay of its parameter group.  The 16-byte vector path needs all five pointers 16-byte aligned
 *                    and numel % 4 == 0; everything else (element alignment is the minimum) takes a scalar path.
 *   tp_optim_hyper   beta1, beta2 in [0, 1); eps >= 0; max_grad_norm <= 0 or +inf: no clipping (the norm and found_inf are
 *                    computed all the same); dtype TP_BF16 / TP_F16, or TP_F32; flags 0 | TP_OPTIM_ZERO_GRAD (grad is zeroed
 *                    behind the update — on a skipped step too).
 *                    dtype TP_F32: the parameters are fp32 and their own masters (a module that keeps fp32 weights under autocast):
 *                    every entry's `master` points at the parameter and `param` must be NULL (a non-NULL one is TP_ERR_INVALID_ARG,
 *                    as a NULL one is for bf16 / fp16).  The update, the skipped step, the zeroing and the vector / scalar paths are
 *                    the same; there is no second copy and no write-back.
 *   inv_scale        device float (the reciprocal of a loss scale; read by the kernels, never by the host), or NULL: 1.
 *   state            tp_optim_state, a device block of TP_OPTIM_STATE_BYTES the caller zeroes ONCE and keeps across steps:
 *                      grad_norm  the norm of grad * inv_scale before clipping, summed in fp32 per chunk, in fp64 across chunks
 *                      clip_coef  min(1, max_grad_norm / (grad_norm + 1e-6)) in fp32 (clip_grad_norm_'s formula); 1 without
 *                                 clipping, 0 on a skipped step
 *                      found_inf  1 when grad_norm is not finite: THIS step was skipped — master, exp_avg, exp_avg_sq and param
 *                                 keep their bits (gradients whose fp32 sum of squares overflows count as non-finite)
 *                      step       steps applied so far; a skipped step does not advance it (torch's fused AdamW under a GradScaler)
 *                      skipped    steps skipped so far
 *                      bc1, sqrt_bc2   1 - beta1^step and sqrt(1 - beta2^step) of the step being applied, computed on the device
 *                                 in fp64 from `step`, stored as fp32
 *   workspace        tp_optim_workspace_bytes bytes, 16-byte aligned: one fp32 partial sum per chunk, plus room for a state block
 *                    behind them (a caller may place `state` in the last TP_OPTIM_STATE_BYTES of the same allocation); 0 with
 *                    the error set on a bad table.
 * TP_ERR_INVALID_ARG before anything is enqueued, the message naming the entry: n < 0, a NULL pointer, numel <= 0, a pointer not
 * aligned to its element size, the same address twice among all pointers of the table, a beta outside [0, 1), negative or
 * non-finite eps / lr / weight_decay, a dtype other than bf16 / fp16 / fp32, unknown flags, a workspace that is too small.  n == 0 is
 * TP_OK and launches nothing. */
enum { TP_OPTIM_ZERO_GRAD = 1 };
typedef struct tp_optim_tensor {
    void* param; float* master; float* grad; float* exp_avg; float* exp_avg_sq;
    int64_t numel;
    float lr; float weight_decay;
} tp_optim_tensor;
typedef struct tp_optim_hyper {
    float beta1, beta2, eps, max_grad_norm;
    int32_t dtype;
    uint32_t flags;
} tp_optim_hyper;
#define TP_OPTIM_STATE_BYTES 64
typedef struct tp_optim_state {
    float   grad_norm;     /* byte  0 */
    float   clip_coef;     /* byte  4 */
    int32_t found_inf;     /* byte  8 */
    int32_t step;          /* byte 12 */
    int32_t skipped;       /* byte 16 */
    float   bc1;           /* byte 20 */
    float   sqrt_bc2;      /* byte 24 */
    int32_t reserved[9];   /* stays zero */
} tp_optim_state;
size_t tp_optim_workspace_bytes(const tp_optim_tensor* t, int n);
int tp_optim_step(const tp_optim_tensor* t, int n, const tp_optim_hyper* h, const float* inv_scale, void* state, void* workspace,
                  size_t workspace_bytes, void* stream);

/* ---- sharded optimizer step: tp_optim_step in two calls (ABI 6 extension, detected by symbol) ------------------------------
 * For an optimizer whose moments, masters and update are sharded across W ranks (ZeRO-1): every rank holds a table over ITS shard of
 * the reduced gradients, and the global norm needs one collective between the two calls:
 *     tp_optim_sumsq (this rank's sum of squares -> one device double)  ->  all-gather of the W doubles, in rank order
 *     ->  tp_optim_apply (the W doubles -> the state block -> AdamW on this rank's table)
 * Both multiply every gradient by s = (inv_scale ? inv_scale[0] : 1) * grad_scale, one fp32 product, before anything else;
 * grad_scale is a HOST float, finite and > 0: the 1 / W of gradient averaging behind a summing reduce-scatter (1: the bits of
 * inv_scale alone).  tp_optim_step is these two calls with grad_scale = 1 and nsums = 1, bit for bit.
 *
 *   tp_optim_sumsq   the fp32 sum of (grad * s)^2 per chunk into `workspace` (one float per chunk: tp_optim_workspace_bytes is
 *                    enough, 16-byte aligned), exactly tp_optim_step's first launches; then ONE workgroup adds the chunks' sums in
 *                    fp64 in tp_optim_step's fixed order (a contiguous run per lane, then the neighbour tree) into sumsq_out[0]
 *                    (a device double, 8-byte aligned).  Only `grad` and `numel` of each entry are read.  n == 0 is legal — a rank
 *                    whose shard is all padding still takes part — and writes 0.0; its workspace may be NULL.
 *   tp_optim_apply   one workgroup adds sums[0 .. nsums) (device doubles, 8-byte aligned, nsums >= 1) in index order in fp64 and
 *                    derives the whole state block from the total exactly as tp_optim_step does (norm, clip_coef, found_inf, the
 *                    step / skipped counters, bc1, sqrt_bc2: same formulas, same fp32 roundings); the AdamW kernel then runs over
 *                    the table.  n == 0 still runs the first kernel: the counters advance on every rank alike.  A non-finite
 *                    total skips the update of EVERY shard, also on a rank whose own gradients are finite.
 * Determinism: the results depend on the table and on nsums, never on the grid or the device's CU count; every rank that is given
 * the same `sums` writes the same state block.  TP_ERR_INVALID_ARG before anything is enqueued, under tp_optim_step's rules (the
 * named entry, alignment, the same address twice, dtype, param == NULL for TP_F32; tp_optim_sumsq holds only `grad` to them), and
 * for grad_scale <= 0 / NaN / inf, nsums < 1, a NULL or misaligned sums / sumsq_out.  A table longer than 32 entries is served by
 * consecutive launches.  Enqueue-only, reentrant, no atomics, allocates nothing. */
int tp_optim_sumsq(const tp_optim_tensor* t, int n, const float* inv_scale, float grad_scale, double* sumsq_out, void* workspace,
                   size_t workspace_bytes, void* stream);
int tp_optim_apply(const tp_optim_tensor* t, int n, const tp_optim_hyper* h, const float* inv_scale, float grad_scale,
                   const double* sums, int nsums, void* state, void* stream);

/* The backward's weight-gradient contraction on its own (what autograd computes for every nn.Linear of
 * builder.py:59-83):  dw[n_out, k_in] = sum over the `rows` token rows of dy[r, n] * x[r, k], read from the ROW-MAJOR
 * activations — no transposed copies.  dy [rows, n_out] and x [rows, k_in] are `dtype` with row strides ldy / ldx
 * (elements, multiples of 8); x may be batch-strided like x_multi (x_rows_per_batch a multiple of 64 and >= 128, or 0).
 * dw is `out_dtype` (TP_BF16 / TP_F16 / TP_F32), contiguous; fp32 accumulation, deterministic.
 * Needs k_in % 256 == 0 and n_out % 8 == 0.  workspace: tp_wgrad_workspace_bytes(n_out, k_in) bytes, 256-byte aligned.
 * With TP_WGRAD_X_TRANSPOSED the activation operand is given transposed instead, x = X^T [k_in, ldx] with ldx a
 * multiple of 1024 and zeros in columns rows .. ldx - 1 (an operand a cast or LayerNorm pass rewrote anyway);
 * dy is still read in place. */
enum { TP_WGRAD_X_TRANSPOSED = 1 };
size_t tp_wgrad_workspace_bytes(int n_out, int k_in);
int tp_wgrad(const void* dy, int64_t ldy, const void* x, int64_t ldx, int x_rows_per_batch, int64_t x_batch_stride,
             int64_t rows, int n_out, int k_in, int dtype, void* dw, int out_dtype, int flags, void* workspace,
             size_t workspace_bytes, void* stream);

/* ---- TokenPacker-HD token assembly (the step right after the projector) --------------------------------
 * Replaces the Python loop + torch.cat of `prepare_inputs_labels_for_multimodal` in mode 'slice'
 * (llava_arch.py:140-154): per image, the h_block x w_block crops in row-major order, the ',' embedding after
 * every crop that is not the last of its row, the '\n' embedding after every row, then (more than one crop)
 * the global-view crop and '\n'.  tokens [n_crops, M, D], sep / ret [D], out [out_rows, D]; all of `dtype`.
 * Image i reads crops first_crop .. and writes rows out_row .. out_row + tp_hd_rows(h, w, M).  Images are listed in
 * order; their crop and row ranges must not overlap and must lie inside `tokens` / `out` (validated).  Rows of `out`
 * between two images are left untouched, so `out` can be the `inputs_embeds` buffer itself with the text embeddings
 * already in place (llava_arch.py:172-191) — the visual tokens then land where the LLM reads them.
 * `crop_map` (device int32[n_crops], or NULL): logical crop c lives in row block crop_map[c] of `tokens` — lets the
 * kernel read the b_max-strided buffer of a RAGGED all-gather in place (tokenpacker_amd.shard.GatheredTokens); the
 * caller guarantees the mapped blocks exist (values are not readable from the host side).
 *
 * tp_hd_assemble_backward is its transpose, for training (the same plan, M, D, dtype and crop_map conventions):
 * from dout [out_rows, D] it writes
 *   dtokens [n_token_crops, M, D], the WHOLE buffer: every crop row that a block reads gets its dout row (a copy, bit-exact);
 *     every other row is zero (crops no image reads, e.g. those of image-less samples, and unmapped slots of a ragged gather);
 *   dsep [D] / dret [D]: the sums of dout over all ',' rows / all '\n' rows of every image of the call, accumulated in fp32
 *     in a fixed order (no atomics: two runs give identical bits) and rounded once to `dtype`.
 * Without crop_map, logical crop c is block c (n_token_crops >= n_crops); with it, the map must be injective and its values
 * inside [0, n_token_crops) (entries outside are ignored).  Enqueues only: no host synchronisation, no allocation; the
 * fp32 partials live in `workspace` (16-byte aligned) of tp_hd_assemble_backward_workspace_bytes(n_images, n_token_crops, D)
 * bytes.  Any number of images (launches of 64). */
typedef struct tp_hd_image {
    int32_t first_crop;
    int32_t h_block;
    int32_t w_block;
    int32_t reserved;
    int64_t out_row;
} tp_hd_image;
int64_t tp_hd_rows(int h_block, int w_block, int M);
int tp_hd_assemble(const tp_hd_image* plan, int n_images, const void* tokens, int64_t n_crops, const int32_t* crop_map,
                   const void* sep, const void* ret, void* out, int64_t out_rows, int M, int D, int dtype, void* stream);
size_t tp_hd_assemble_backward_workspace_bytes(int n_images, int64_t n_token_crops, int D);
int tp_hd_assemble_backward(const tp_hd_image* plan, int n_images, const void* dout, int64_t out_rows, int64_t n_crops,
                            const int32_t* crop_map, void* dtokens, int64_t n_token_crops, void* dsep, void* dret, int M, int D,
                            int dtype, void* workspace, size_t workspace_bytes, void* stream);

/* ---- token splice: text and visual tokens into inputs_embeds, labels and attention_mask (one launch) -------------------
 * What `prepare_inputs_labels_for_multimodal` (llava_arch.py:100-233) builds with a Python walk per sample, in any mode:
 * ONE gather writes every row of out [batch * out_len, D] exactly once, plus out_labels and out_mask [batch, out_len].
 * The caller describes each output row by one int32 code, kind << 30 | payload:
 *   TP_SPLICE_TEXT     payload = flat position b * in_len + pos: the row is table[ids_dev[position]] (the id is read on the
 *                      device), its label is labels[position];
 *   TP_SPLICE_LITERAL  payload = a table row (the ',' and '\n' rows of mode 'slice'); label -100;
 *   TP_SPLICE_FEATURE  payload = k * M + m: token m of logical feature block k of feats [n_feat_blocks, M, D] — block
 *                      crop_map[k] with a `crop_map` (device int32 [n_logical], as in tp_hd_assemble); label -100;
 *   TP_SPLICE_PAD      a zero row; label -100.
 * The plan is batch * out_len codes followed by one int32 per sample, its length before padding; `plan_host` is read by the
 * call's validation, `plan_dev` is the caller's device copy of the same words.  out_mask[b, r] is 1 for r < len_b - in_len
 * (the rows the images added), then mask[b, r - (len_b - in_len)], then 0 (llava_arch.py:214-221, :228-230); `mask_bytes`
 * is 1 (bool) or 8 (int64).  labels / out_labels (int64) and mask / out_mask may be NULL in pairs.  `ids_host` (the ids as
 * the host knows them, or NULL) lets the validation refuse an id outside [0, V); the kernel never forms an address from
 * an id or a crop_map value outside its buffer (such a row is written as zeros).
 *
 * tp_splice_backward is the transpose, from dout [batch * out_len, D], with the same struct and plan:
 *   dfeats [n_feat_blocks, M, D] (NULL = not wanted), the WHOLE buffer: a feature row that an output row reads gets that
 *     dout row (a copy); every other row is zero (the block an image-less sample consumes, unmapped crop_map slots).  A
 *     feature row read twice is refused.  Needs `workspace` of tp_splice_backward_workspace_bytes(n_feat_blocks, M) =
 *     n_feat_blocks * M * 4 bytes rounded up to 256.
 *   dtable [V, D] (NULL = not wanted: nothing is launched for it), dense like nn.Embedding's gradient: row t is the sum
 *     of the dout rows whose source is table row t (TEXT and LITERAL alike), accumulated in fp32 in increasing row order
 *     and rounded once — no atomics, two runs give the same bits; a row read once is a copy, a row never read and the
 *     `padding_idx` row (-1: none) are zero.  The caller sorts: order_host / order_dev hold n_table_rows int32 output rows
 *     (those that read the table), stably sorted by table row, followed by V + 1 int32 offsets (table row t's readers are
 *     order[offsets[t] .. offsets[t + 1])); needs ids_host.
 * Both entries validate on the host first (TP_ERR_INVALID_ARG: NULL or misaligned pointers, D % 8, dtype, a code outside
 * its buffer, counts that do not match the plan), then only enqueue: no allocation, no synchronisation.  The plan belongs
 * to one batch, so a call cannot be replayed from a captured graph for another. */
enum { TP_SPLICE_TEXT = 0, TP_SPLICE_LITERAL = 1, TP_SPLICE_FEATURE = 2, TP_SPLICE_PAD = 3 };
typedef struct tp_splice_args {
    int32_t batch, in_len, out_len, M, D, dtype;
    int64_t V, n_feat_blocks, n_logical;      /* n_logical: crop_map's length; n_feat_blocks without a crop_map */
    const int32_t* plan_host;                 /* codes [batch * out_len] | lengths [batch] */
    const int32_t* plan_dev;
    const int64_t* ids_host;                  /* [batch * in_len], or NULL (forward) */
    const int64_t* ids_dev;
    const void* table;                        /* [V, D] */
    const void* feats;                        /* [n_feat_blocks, M, D] */
    const int32_t* crop_map;
    const int64_t* labels;
    const void* mask;
    int32_t mask_bytes, reserved;
    void* out;
    int64_t* out_labels;
    void* out_mask;
    /* backward only */
    const void* dout;
    void* dfeats;
    void* dtable;
    int64_t padding_idx, n_table_rows;
    const int32_t* order_host;                /* order [n_table_rows] | offsets [V + 1] */
    const int32_t* order_dev;
    void* workspace;
    size_t workspace_bytes;
} tp_splice_args;
int tp_splice(const tp_splice_args* args, void* stream);
size_t tp_splice_backward_workspace_bytes(int64_t n_feat_blocks, int M);
int tp_splice_backward(const tp_splice_args* args, void* stream);

/* ---- shifted cross-entropy over the labelled rows (ABI 6 extension) ------------------------------------------------------
 * The loss of the reference's LLM wrapper on GIVEN logits (llava/model/language_model/llava_llama.py:95-106):
 *     shift_logits = logits[..., :-1, :].contiguous();  shift_labels = labels[..., 1:].contiguous()
 *     loss = CrossEntropyLoss()(shift_logits.view(-1, V), shift_labels.view(-1))
 * without the shifted copy, the log-softmax and (in place) the gradient buffer, and without reading a row whose target is
 * `ignore_index` — after the splice most rows are (images, separators, prompt, padding).  No GEMM is part of it.
 *
 * logits [batch, len, V], dtype TP_BF16 / TP_F16 / TP_F32, last-dimension stride 1, `row_stride` (>= V) and `batch_stride`
 * (any value) in ELEMENTS: a padded-vocabulary view buf[..., :V] qualifies.  The base pointer and every row need only the
 * alignment of one element; the kernels go element by element up to the first 16-byte boundary of a row and after its last
 * whole 16-byte vector, and never access 16 bytes wide at another address.  All addressing is 64-bit (a 64-bit row base plus a
 * 32-bit offset inside the row).  labels [batch, len] int64, contiguous.
 *
 * tp_shift_ce_forward: row (b, t), t < len - 1, has the target labels[b, t + 1].  One workgroup per row; a labelled row is
 * read from memory once (online maximum and rescaled sum, fp32) and leaves lse, its loss -log_softmax(x)[target], its maximum
 * and the log of its rescaled sum in the workspace.  A second launch of one workgroup sums the row losses (fp64) and counts
 * the labelled rows in a fixed order, no atomics — two runs give the same bits — and writes, at the head of the workspace:
 *     byte TP_SHIFT_CE_LOSS_OFFSET     float    sum / n_valid (TP_CE_MEAN, the reference's reduction) or sum (TP_CE_SUM)
 *     byte TP_SHIFT_CE_INV_N_OFFSET    float    1 / n_valid
 *     byte TP_SHIFT_CE_N_VALID_OFFSET  int64    n_valid, the rows whose target is not ignore_index
 * followed at byte 256 by four fp32 arrays of batch * (len - 1) words, row b * (len - 1) + t: lse | loss | max | log(sum).
 * tp_shift_ce_workspace_bytes(batch, len) = 256 + 16 * batch * (len - 1) rounded up to 256 (0 for sizes < 1).
 *
 * tp_shift_ce_backward (same struct, after the forward on the same workspace): one launch writes the whole of dlogits
 * [batch, len, V] (d_row_stride, d_batch_stride, the logits' dtype):
 *     dlogits[b, t, v] = g * w * (exp(x - lse) - [v == target]),   g = *grad_loss (read on the device),
 *     w = 1 / n_valid (TP_CE_MEAN) or 1 (TP_CE_SUM),
 * and zeros in every unlabelled row and in row len - 1 of every sample.  A labelled row is read once and written once.
 * dlogits may equal logits (in place; the strides must then be equal).  Otherwise every dlogits row must sit at the same
 * offset from a 16-byte boundary as its logits row: the base pointers and both pairs of strides congruent modulo 16 bytes.
 *
 * Non-finite inputs behave as F.cross_entropy on the logits upcast to fp32: no labelled row -> loss NaN (mean), gradient
 * zero; -inf logits beside finite ones -> finite loss, exact zeros in the gradient; -inf at the target -> loss +inf, finite
 * gradient; a row of -inf only -> NaN loss and NaN in that row's gradient.  A target outside [0, V) that is not
 * ignore_index counts as labelled and makes its row's loss, hence the loss, NaN; its gradient row is zeros; no address is
 * ever formed from a target and there is no device assert.
 *
 * Both calls validate on the host first (TP_ERR_INVALID_ARG: NULL pointers, an unknown dtype or reduction, V / len / batch
 * < 1, a row stride below V, a workspace that is too small, a pointer not aligned to its element size — labels 8, workspace
 * 16, grad_loss 4 bytes —, dlogits not congruent to logits), then only enqueue: no allocation, no synchronisation. */
enum { TP_CE_MEAN = 0, TP_CE_SUM = 1 };
#define TP_SHIFT_CE_LOSS_OFFSET 0
#define TP_SHIFT_CE_INV_N_OFFSET 4
#define TP_SHIFT_CE_N_VALID_OFFSET 8
typedef struct tp_shift_ce_args {
    int32_t batch, len, V, dtype, reduction, reserved;
    int64_t row_stride, batch_stride;         /* logits, in elements */
    int64_t d_row_stride, d_batch_stride;     /* dlogits, in elements (backward) */
    int64_t ignore_index;
    const void* logits;
    const int64_t* labels;
    void* workspace;
    size_t workspace_bytes;
    const float* grad_loss;                   /* backward: the incoming 0-dim fp32 gradient, on the device */
    void* dlogits;                            /* backward */
} tp_shift_ce_args;
size_t tp_shift_ce_workspace_bytes(int batch, int len);
int tp_shift_ce_forward(const tp_shift_ce_args* args, void* stream);
int tp_shift_ce_backward(const tp_shift_ce_args* args, void* stream);

/* ---- TokenPacker-HD image slicing (the step before the CLIP tower) ---------------------------------------------
 * Replaces the resize / zero-pad / tile code of the data loader and the eval drivers (llava/train/train.py:695-731):
 * image [3, H, W] fp32 (already normalised) -> crops [h_block*w_block (+1), 3, block, block] fp32: the image resized
 * (F.interpolate bilinear, align_corners = False) to (h_res, w_res) in the top-left of a zero canvas of
 * h_block x w_block blocks, cut row-major; with more than one crop, the canvas resized to (hg, wg) and
 * zero-padded to block x block as the last crop.  The sizes follow the reference's rounding rules
 * (tokenpacker_amd.hd.slice_plan). */
int tp_hd_slice(const float* image, int H, int W, int h_block, int w_block, int h_res, int w_res, int hg, int wg,
                float* crops, int block, void* stream);

/* ---- HD slicing from uint8 images: a batch per launch, normalised on the device ------------------------------------
 * (An ABI 6 extension, detected by symbol: an older ABI 6 build lacks tp_hd_slice_u8.)
 * Everything the reference's loader does between the decoded picture and the tower (train.py:696-731 and the driver's
 * `.to(dtype)`), for a whole batch of raw RGB uint8 images of different sizes, as ONE launch: ToTensor + Normalize,
 * resize, zero-pad, tile and global view, stored in `out_dtype` (TP_F32, TP_BF16 or TP_F16) with one rounding
 * (round to nearest even, Tensor.to).
 *   pixels [pixel_bytes]  device bytes; image i is HWC uint8, pixel (y, x) at src_offset + y * row_stride + 3 * x.
 *                         pixel_bytes >= 8: a tap is fetched by one 8-byte load, moved down where it would end past the
 *                         buffer — no address outside pixels[0, pixel_bytes) is ever formed.
 *   lut [3][256] fp32     device table: lut[c][u] = fl(fl(fl(u / 255) - mean_c) / std_c), built on the host (true
 *                         divisions, tokenpacker_amd.hd.normalisation_table); the kernel keeps it in LDS and does no
 *                         division of its own — the normalisation is bit-exact by construction.
 *   crops [n_crops, 3, block, block]   16-byte aligned; block % 8 == 0 (a lane stores 8 consecutive pixels, 16 bytes per
 *                         channel plane).  Image i owns crops [first_crop, first_crop + h_block * w_block (+ 1)), row-major,
 *                         the global view last; the ranges are in image order, disjoint, and cover [0, n_crops).
 * Resize arithmetic: tp_hd_slice's taps and blend on table values, zero outside (h_res, w_res); the global view is the
 * canvas (padding included) resized to (hg, wg), computed from the canvas's fp32 values, not from rounded crops.
 * The plan — the same words on the host (read by the validation) and on the device (read by the kernel) — is
 * tp_hd_slice_image [n_images] followed by int32 [n_crops], the image index of every crop (a workgroup finds its image in
 * O(1)).  plan_dev is 8-byte aligned.  The call validates on the host first (TP_ERR_INVALID_ARG: NULL or misaligned
 * pointers, non-positive sizes, an image outside `pixels`, sizes that do not fit the grid, (hg, wg) != (0, 0) with one crop
 * or 0 with several, crop ranges out of order / overlapping / not summing to n_crops, a crop mapped to another image,
 * block, out_dtype), then only enqueues: no allocation, no atomics, no synchronisation.  The kernel checks the device copy
 * of an entry again and writes zeros for one that fails. */
typedef struct tp_hd_slice_image {
    int64_t src_offset;            /* byte offset of pixel (0,0) in `pixels` */
    int32_t H, W, row_stride;      /* row_stride in bytes, >= 3*W */
    int32_t h_block, w_block, h_res, w_res, hg, wg;   /* hd.slice_plan's sizes; hg = wg = 0 iff one crop */
    int32_t first_crop;
} tp_hd_slice_image;
int tp_hd_slice_u8(const tp_hd_slice_image* plan_host, const void* plan_dev, int n_images,
                   const uint8_t* pixels, int64_t pixel_bytes, const float* lut /* device [3][256] */,
                   void* crops, int64_t n_crops, int block, int out_dtype /* TP_F32 | TP_BF16 | TP_F16 */, void* stream);

/* ---- CLIP preprocessing: the 'pad' and default ('square') image modes from uint8 images, bit-exact to PIL ------------
 * (An ABI 6 extension, detected by symbol: an older ABI 6 build lacks tp_clip_preprocess.)
 * What the reference's loader and drivers do to a decoded picture when image_aspect_ratio is not 'slice'
 * (llava/mm_utils.py:14-37, train.py:679-694, 732-734): optionally expand2square with a background colour, then
 * CLIPImageProcessor.preprocess — PIL's 8-bit bicubic resize (shortest edge to `size`, or the padded square to size x size),
 * centre crop to size x size, rescale by 1/255, normalise — and the driver's `.to(dtype)`; for a whole batch of raw RGB
 * uint8 images of different sizes, as TWO launches, with results that equal the reference's bit for bit.
 *
 * Pillow's 8-bit resize is integer arithmetic.  Per axis: int32 coefficients k with 22 fractional bits and, per output
 * position, the taps [xmin, xmin + xcount); a sample is clip8((2^21 + sum_t k[t] * src[xmin + t]) >> 22) (arithmetic shift,
 * saturated to 0 .. 255).  The horizontal pass runs first and ROUNDS to uint8, then the vertical one: the intermediate
 * rounding is part of the result.
 *
 * tp_resize_coeffs (host only, no GPU needed) is the single source of the tables: Pillow's precompute_coeffs /
 * normalize_coeffs_8bpc for the bicubic filter, evaluated in IEEE double in Pillow's order without contraction, for the
 * output positions [first_out, first_out + n_out) of a resize of in_size to out_size — only the `size` positions inside the
 * crop window are ever needed, however long the resized side.  *ksize = the taps per position; kk [n_out][ksize] (zero
 * behind xcount), bounds [n_out][2] = (xmin, xcount).  With kk == bounds == NULL only *ksize is written. */
int tp_resize_coeffs(int in_size, int out_size, int first_out, int n_out, int32_t* kk, int32_t* bounds, int* ksize);

/* One image of tp_clip_preprocess's plan.  The resize reads a virtual in_h x in_w picture: the stored H x W image itself
 * (TP_CLIP_SQUARE; in_h = H, in_w = W, pad_top = pad_left = 0) or the square of side max(H, W) filled with `background` in
 * which the image sits at (pad_top, pad_left) (TP_CLIP_PAD; never materialised).  It is resized to out_h x out_w, of which the
 * window (crop_top, crop_left) + size x size is the result (tokenpacker_amd.preprocess.preprocess_plan has the reference's
 * rules).  Tables, as int32 word offsets into `coeffs`, for the `size` positions of the window:
 *   kk_h [ksize_h][size]  TAP-MAJOR (the transpose of what tp_resize_coeffs writes: adjacent lanes are adjacent columns)
 *   bounds_h [size][2], kk_v [size][ksize_v], bounds_v [size][2]  as tp_resize_coeffs writes them
 * The horizontal pass covers the virtual rows [row0, row0 + rows) — every row a vertical tap of the window touches — and
 * leaves them as uint8 [rows][size][3] at workspace + ws_offset. */
#define TP_CLIP_SQUARE 0
#define TP_CLIP_PAD 1
typedef struct tp_clip_image {
    int64_t src_offset;            /* byte offset of pixel (0,0) in `pixels` */
    int64_t ws_offset;             /* byte offset of the image's workspace slice, a multiple of 16 */
    int32_t H, W, row_stride;      /* row_stride in bytes, >= 3*W */
    int32_t mode;                  /* TP_CLIP_SQUARE | TP_CLIP_PAD */
    int32_t in_h, in_w, pad_top, pad_left;
    int32_t out_h, out_w, crop_top, crop_left;
    int32_t ksize_h, ksize_v;      /* tp_resize_coeffs' tap counts of in_w -> out_w and in_h -> out_h */
    int32_t row0, rows;
    int32_t kk_h, bounds_h, kk_v, bounds_v;
    uint8_t background[4];         /* R, G, B, 0: what TP_CLIP_PAD reads outside the content */
    int32_t reserved;
} tp_clip_image;

/* The workspace a plan needs: the end of its furthest slice (ws_offset + rows * size * 3), rounded up to 16.  Host only.
 * 0 + tp_last_error() for a plan whose records are invalid. */
size_t tp_clip_preprocess_workspace_bytes(const tp_clip_image* plan_host, int n_images, int size);

/*   pixels [pixel_bytes]  device bytes; image i is HWC uint8, pixel (y, x) at src_offset + y * row_stride + 3 * x.
 *                         pixel_bytes >= 4: a pixel is fetched by one 4-byte load, moved down where it would end past the
 *                         buffer — no address outside pixels[0, pixel_bytes) is ever formed.
 *   lut [3][256] fp32     device table lut[c][u] = fl(fl(fl(u / 255) - mean_c) / std_c) (tokenpacker_amd.hd.normalisation_table)
 *   coeffs [coeff_words]  the int32 tables of all images, the same words on the host (validated) and on the device (read)
 *   workspace             caller-owned device bytes, 16-byte aligned, at least tp_clip_preprocess_workspace_bytes
 *   out [n_images, 3, size, size] in out_dtype (TP_F32, TP_BF16 or TP_F16; one rounding, Tensor.to's), 16-byte aligned
 * The plan is the same words on the host (plan_host, read by the validation) and on the device (plan_dev, 8-byte aligned, read
 * by the kernels).  The call validates on the host first (TP_ERR_INVALID_ARG, each with its own message: NULL or misaligned
 * pointers; sizes below 1; a side beyond the supported maximum of 16384 pixels — refused, never truncated; a geometry that
 * does not describe the image; an image outside `pixels`; size not a multiple of 8; tables or workspace slices that overlap
 * the one before them or fall outside their buffers — both must come in plan order; a tap range outside [0, in_size) or
 * outside the workspace rows; out_dtype), then only enqueues two launches, whatever n_images: no allocation, no atomics, no
 * synchronisation, no division and no floating-point arithmetic on the device other than the final rounding.  The kernels
 * check the device copy of an entry again, write zeros for one that fails and form no address from it. */
int tp_clip_preprocess(const tp_clip_image* plan_host, const void* plan_dev, int n_images,
                       const uint8_t* pixels, int64_t pixel_bytes, const float* lut /* device [3][256] */,
                       const int32_t* coeffs_host, const int32_t* coeffs_dev, int64_t coeff_words,
                       void* workspace, int64_t workspace_bytes, void* out, int size,
                       int out_dtype /* TP_F32 | TP_BF16 | TP_F16 */, void* stream);

/* ---- debug: fp16 saturation scan ---------------------------------------------------------------------------------
 * Every activation between the kernels of tp_forward is fp16 and every epilogue CLAMPS to +-65504 instead of producing
 * inf.  After a tp_forward on `stream` with the same desc / workspace, this scans the nine intermediate
 * buffers — q0, Hkv, H2, KV (qt | u under the absorbed schedule), Q1pre, Q, O, A1, A2 in this order — and writes into counts[i] (device int32[9]) the
 * number of elements at the clamp bound (or NaN).  All zeros = no activation of that forward left the fp16 range. */
#define TP_NUM_DEBUG_BUFFERS 9
int tp_debug_count_saturated(const tp_desc* desc, const void* workspace, size_t workspace_bytes, int32_t* counts,
                             void* stream);

/* The first TP_WORKSPACE_STATUS_BYTES of tp_backward's workspace are a status block like the forward workspace's: int32 word 0 holds
 * the sticky saturation bits of THAT backward (zeroed by the call itself): bit 0 — the incoming dy was not finite, or a GEMM epilogue of
 * the fp16 gradient chain clamped a value to +-65504; bit 1 — the LayerNorm backward did; bit 2 — the attention backward did.  Non-zero
 * means the parameter gradients of that call are not trustworthy (TP_TUNE_BWD_CHAIN = 1 carries the gradients in bf16 instead). */

/* ---- diagnostics counters of this process (read-only; ABI 5: the round-3/4 test hooks tp_test_side_cache_size /
 * tp_test_pair_launch_count under one entry — the other, stateless test hooks and the timing-probe instantiations of the GEMM
 * kernels are NOT in this library: include/tokenpacker_test.h, libtokenpacker_exp.so):
 *   TP_COUNTER_SIDE_STREAMS  entries of the per-caller-stream side-stream cache (tp_release_stream, LRU eviction)
 *   TP_COUNTER_PAIR_LAUNCHES launches of the pair GEMM kernel (tp_gemm_pair.hip) issued so far
 * -1: unknown counter. */
enum { TP_COUNTER_SIDE_STREAMS = 0, TP_COUNTER_PAIR_LAUNCHES = 1 };
long long tp_debug_counter(int which);

/* ---- tuning knobs (benchmarks / deployment policy; defaults are what tp_forward ships with) --------------------
 * Two places hold them (ABI 4):
 *   - a TUNING CONTEXT (tp_tuning_create): a private copy of the table.  Every entry point that takes a tp_desc reads its
 *     knobs from desc->tuning for the whole call — plan, workspace layout, every launch — whatever other threads do to
 *     other contexts or to the process-wide table meanwhile.  This is what a serving worker uses (the reference runs
 *     `generate` on a thread per request, llava/serve/model_worker.py:174): one context per model instance, set once.
 *   - the PROCESS-WIDE table (tp_set_tuning / tp_get_tuning): what a descriptor with tuning == NULL, the per-kernel entry
 *     points (tp_linear ...) and tp_tuning_create's initial copy read.  One array of atomics, NOT scoped to a stream, a
 *     call or a thread: benchmarks and tests flip it between calls; concurrent forwards that rely on it see each
 *     other's changes (several knobs change the summation order, i.e. low bits).
 * Everything else in this header is reentrant (state is per call, per thread (error string) or per caller stream (the
 * forked query-side stream; at most 64 distinct caller streams per device get one, later ones run the query side on the
 * caller's stream)). */
enum { TP_TUNE_GEMM_TILE = 0,   /* 0 auto (full tiles, half-tile tail, all half tiles or all 192-row tiles by CU rounds) | 128 | 256 |
                                   2: every tile of the ping-pong kernel a 128 x 256 half tile | 3: a 192 x 256 tile (plain launches) |
                                   4: auto without 192-row tiles (tests, A/Bs; same bits whatever the tile) */
       TP_TUNE_XCD_SWIZZLE = 1, /* 1 (default) | 0 | 2 = A/B: W-half-resident blocking of an XCD's tiles (measured null) */
       TP_TUNE_FOLD_OUT_PROJ = 2, /* out_proj folded into mlp[0] (W = Wm0·Wout, one GEMM less): 0 (default) auto = on the absorbed
                                     schedule and on the scale_factor-2 schedule with attention in the in-projection epilogues
                                     (TP_TUNE_FUSE_ATTN 0) | 1 always | 2 never; read at PACK time (tp_pack_weights builds the
                                     folded weight only then) and at forward time */
       TP_TUNE_DYNAMIC_TILES = 3, /* 1 (default): persistent GEMMs draw tiles from per-XCD queues | 0: static striding */
       TP_TUNE_Q_SIDE_STREAM = 4, /* 1 (default): the query side runs on a forked side stream | 0: one stream */
       TP_TUNE_RESERVE_CUS = 5,   /* r in 0 .. CUs/8 - 1 (default 0): persistent GEMMs launch (CUs/8 - r) workgroups per XCD, leaving
                                     r CUs per XCD to kernels of other streams (RCCL's all-gather overlapping the next forward) */
       TP_TUNE_ABSORB_KV = 6,     /* K/V in-projection absorbed into the query side (see tp_forward): 0 auto (scale_factor >= 3),
                                     1 never, 2 always */
       TP_TUNE_FUSE_KV_LN = 7,    /* 1 (default): inference: the layer in front of every LayerNorm is computed for its row statistics
                                     only and the in-projection behind it reads that layer's INPUT through a pre-multiplied weight
                                     (K/V side: Wc = W'·W2, no H2 written — on the plain schedule through the in-projection GEMM, on
                                     the absorbed schedule through qt and the per-head V GEMM, the attention kernel walking Hkv; query
                                     side: W'q·Wq1, no Q1pre written) | 0: the pre-LayerNorm activations are written and read back.
                                     Read at PACK time (the pre-multiplied weights are built only then) and at forward time */
       TP_TUNE_LN_MERGE = 8,      /* 0 (default): inference, a LayerNorm's consumer on the 128-tile kernel (small batches) merges the
                                     producer's (mean, M2) slabs itself — no ln_finalize launch | 1: always the separate launch */
       TP_TUNE_FUSE_ATTN = 9,    /* inference, scale_factor 2, fused LayerNorm chain, no attn_mask: 0 (default) the first K/V layer reads
                                     the tower's rows in REGION-MAJOR order (a region's 4 tokens = 4 consecutive rows of every K/V-side
                                     tensor) and region attention runs inside the epilogues of the K and V in-projection GEMMs — K, V
                                     are never written, no attention kernel | 1 off (raster rows, tp_region_attention's kernel) |
                                     2 region-major rows + the separate attention kernel (A/B, tests) */
       TP_TUNE_SPLIT_K = 10,      /* small batches (B <= 3 at the shipped shapes), inference: the two K = 4096 GEMMs of the path (first
                                     K/V layer, mlp[2]) — 80 and 64 workgroups walking 64 K-slabs each at B = 1, a serial chain of
                                     ~0.65 us steps — are split over K into up to 8 groups of the 128-tile kernel with fp32 partials
                                     and a fixed-order reduction kernel that applies the epilogue (B = 1: 0.157 -> 0.137 ms).
                                     0 (default since round 3) / 1: on where at least 4 K-groups fit | 2: off.  Deterministic, but NOT
                                     the summation order of the unsplit kernels: with 0 / 1 the low bits of a batch of <= 3 images
                                     differ from the same images inside a larger batch; 2 keeps an image's bits independent of the
                                     batch it travels in (what rounds 1-2 shipped; the reference's eager PyTorch does not have that
                                     property either). */
       TP_TUNE_SMALL_GEMM_WAVES = 11, /* the 128 x 128-tile kernel as 4 waves of 64 x 64 or 8 waves of 32 x 64 (bit-identical): 0 (default)
                                     auto by the number of workgroups of the launch | 4 | 8.  A launch of the 8-wave form with at
                                     most one workgroup per CU keeps FOUR K-slabs in its LDS ring (three in flight, counted vmcnt;
                                     round 3: a one-image forward 0.132 -> 0.128 ms) | 9: 8 waves with the double buffer (A/B) */
       TP_TUNE_TRI_STATS = 12,    /* inference, fused LayerNorm chain: 0 (default, round 3) the layer in front of a LayerNorm is replaced, for
                                     its statistics, by the UPPER-TRIANGULAR factor R of its centred weight (W2c = Q R, Householder QR at
                                     pack time): var = ||R h + c~||^2 / E, a sum of squares, on 40 of the 64 (N-tile, K-tile) pairs; the
                                     consumers use centred chain weights (W'·W2c, W'·b2c) and need no mean at all | 1: the full
                                     statistics GEMM on W2 with (mean, M2), as rounds 1-2 shipped */
       TP_TUNE_PAIR_GEMM = 13,    /* the 256 x 128-tile "pair" kernel (tp_gemm_pair.hip: two co-resident 4-wave workgroups per CU, a tile's
                                     epilogue under the other workgroup's MFMAs; bit-identical to the other GEMM kernels): 0 (default) for
                                     the short-K launches of 1.5 .. 2.5 rounds of its 512 workgroups, where it measured faster — on
                                     full-chip launches its 1.5 x operand traffic loses 12-17 % | 1 never | 2 wherever it is supported */
       TP_TUNE_PAIR_STAGGER = 14, /* percent (default 100) of half a tile period by which the second workgroup of each CU starts late in
                                     a pair-kernel launch (0: both start together — their epilogues then coincide for ever) */
       TP_TUNE_PAIR_DEBUG = 15,   /* libtokenpacker_exp.so ONLY (`make exp`; this library refuses a non-zero value: the probe instantiations are
                                     not built into it).  Timing probes of the pair kernel (fp16 -> fp16 plain launches; results are GARBAGE with 1..4): low 3 bits 1 no
                                     DMA in the K loop | 2 no fragment reads | 3 no barriers | 4 no MFMAs; + 8: one workgroup per CU;
                                     bits 4.. (value >> 4): the same kind of probe of the ping-pong kernel's K loop (tools/loop_probe.py:
                                     1 / 3 / 15 no b0 / W / any fragment reads, 16 no DMA, 31 neither, 64 no MFMAs, 79, 80) */
       TP_TUNE_DECOUPLE_K = 16,   /* scale_factor 2, attention in the in-projection epilogues, centred chain (all defaults): 0 (default) the K
                                     launch behind the statistics, LayerNorm fold in its epilogue (the round-5 form) | 1 the K launch writes
                                     RAW logits Q·(Hkv·Wcc^T + dcc) — the K rows' rstd is applied by the V launch, the K bias is
                                     softmax-invariant — so it does not wait for the row statistics and runs on the side stream BESIDE the
                                     statistics launch | 2 raw logits on the caller's stream (same bits as 1: the A/B of the placement
                                     alone).  Measured null at B = 32 .. 256 (profiles/r06b_decouple_k_ab.txt): kept as the record of
                                     that A/B, parity-tested (tests/test_gpu_round6.py) */
       TP_TUNE_BWD_CHAIN = 17,    /* tp_backward of a bf16 model: 0 (default) gradients travel between the backward's kernels in FP16 behind a
                                     dynamic power-of-two scale (S = 2^k brings amax(dy) to (16, 32], computed on the device per call; every
                                     parameter gradient is multiplied by 1 / S — exact — when its fp32 sum is cast to bf16): the weight gradients
                                     read the forward's saved fp16 activations in place instead of through a bf16 copy each (6 of 9 cast passes
                                     gone), and the chain keeps 11 mantissa bits instead of 8 | 1 gradients travel in bf16 (rounds 1-5).  fp16
                                     models are not affected (their gradients travel in fp16, unscaled, as before) */
       TP_TUNE_COUNT_ = 18 };
int tp_set_tuning(int key, int value);
int tp_get_tuning(int key);                  /* the library's current value (not a binding's shadow copy); -1: bad key */
typedef struct tp_tuning tp_tuning;          /* opaque; host memory owned by the library until tp_tuning_destroy */
tp_tuning* tp_tuning_create(void);           /* a copy of the process-wide table of the moment; NULL: out of memory */
void tp_tuning_destroy(tp_tuning* t);        /* (no call that was handed `t` may still be running) */
int tp_tuning_set(tp_tuning* t, int key, int value);
int tp_tuning_get(const tp_tuning* t, int key);          /* -1: bad key / NULL */

/* Per-caller-stream state: tp_forward forks the query side onto a side stream it keeps per (device, caller stream).
 * A caller that destroys a stream it has passed to tp_forward releases that state first — a later stream the runtime
 * hands out at the same address would otherwise inherit it.  Synchronises the side stream; a stream the library has
 * never seen is not an error.  The cache holds 64 entries per process; beyond that the least recently used one is
 * released the same way. */
int tp_release_stream(void* stream);

/* ---- CU-free all-gather of the projected tokens ("one all-gather ... before the LLM") ----------------
 * One process per GPU.  Every rank's projector writes its shard into rows [lo, hi) of a receive buffer [total, M, D]
 * (tp_forward's `out`), and the shard travels to the same rows of every peer's buffer by ONE hipMemcpyAsync per peer —
 * SDMA engines over that peer's xGMI link, no compute unit — instead of RCCL's all-gather kernels, which need the CUs the
 * next forward's persistent GEMMs own.  The reference has no counterpart (it never calls torch.distributed); this is the
 * data-path step the north_star prescribes.  tokenpacker_amd/shard.py (DirectGather) drives it; INTEGRATION.md §4 shows
 * the protocol.  Everything below only enqueues; buffers, flags, streams and events are the caller's.
 *
 *   tp_gather_export  IPC handle of the ALLOCATION `ptr` lives in + ptr's offset inside it (hipMemGetAddressRange +
 *                     hipIpcGetMemHandle): what a peer process needs to address `ptr`.
 *   tp_gather_open    maps a peer's allocation into this process (peer access enabled lazily); tp_gather_close unmaps it.
 *   tp_gather_push    for each of n_peers: copy `bytes` from `src` to dst[j], then the 4-byte sequence number in
 *                     *seq_cell to dst_flag[j], both on streams[j] (stream order: the flag cannot land before the data).
 *                     use_cus = 0: hipMemcpyDeviceToDeviceNoCU (SDMA) | 1: the runtime's choice (A/B).
 *   tp_gather_sync    ONE-wave kernel on `stream`: waits until flags[p] has reached wait_seq for every p != rank
 *                     (wrap-safe signed distance), then stores publish_seq to *seq_cell (NULL: nothing).  A wait longer than
 *                     timeout_ms (<= 0: 30 s) sets bit 0 of *status (device int32, may be NULL) and gives up — the caller
 *                     reads status when it synchronises.  flags: device uint32[world] in THIS rank's memory, zeroed
 *                     once, slot p written only by rank p's tp_gather_push.
 *   tp_gather_alloc_flags  the flag array as FINE-GRAINED device memory (hipExtMallocWithFlags), zeroed: it is written by
 *                     other devices' copy engines while a kernel of this device polls it, and ordinary device memory is only
 *                     coherent across agents at kernel boundaries.  The one allocation the library performs (on request, a few
 *                     hundred bytes; tp_gather_free_flags releases it) — the caller's framework allocator cannot provide it. */
#define TP_IPC_HANDLE_BYTES 64
int tp_gather_alloc_flags(void** flags, size_t bytes);
int tp_gather_free_flags(void* flags);
int tp_gather_export(const void* ptr, void* handle /* [TP_IPC_HANDLE_BYTES] */, uint64_t* offset);
int tp_gather_open(const void* handle, void** base);
int tp_gather_close(void* base);
int tp_gather_push(int n_peers, void* const* dst, const void* src, size_t bytes, void* const* dst_flag,
                   const uint32_t* seq_cell, void* const* streams, int use_cus);
int tp_gather_sync(const uint32_t* flags, int world, int rank, uint32_t wait_seq, uint32_t* seq_cell,
                   uint32_t publish_seq, int32_t* status, int timeout_ms, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TOKENPACKER_H_ */
