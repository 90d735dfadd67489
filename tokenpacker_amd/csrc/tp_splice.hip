// tp_splice.hip — the splice of text and visual tokens between the projector and the LLM (what the reference's
// prepare_inputs_labels_for_multimodal builds with a Python walk per sample, llava_arch.py:100-233), as ONE gather launch,
// and its backward.  See include/tokenpacker.h ("token splice") for the contract.
//
// The host describes every output row by one int32 code (tp_splice_args.plan_host / plan_dev):
//     kind = code >> 30 (unsigned), payload = code & 0x3fffffff
//     TP_SPLICE_TEXT     payload = flat position b * L_in + pos of input_ids: the row is table[input_ids[position]]
//     TP_SPLICE_LITERAL  payload = a table row (',' and '\n' of slice mode)
//     TP_SPLICE_FEATURE  payload = k * M + m: token m of logical feature block k (through crop_map when there is one)
//     TP_SPLICE_PAD      a zero row
// followed by one int32 per sample: its length before padding (the attention mask's left / right fill follows from it).
// Forward and backward read the same plan, and validate_splice() below is the one host-side check of both.
#include "tp_internal.h"

#include <vector>

using namespace tp;

namespace {

constexpr unsigned kPayloadMask = 0x3fffffffu;

__device__ __forceinline__ void splice_copy_row(uint4* __restrict__ dst, const uint4* __restrict__ src, int vecs) {
    for (int v = threadIdx.x; v < vecs; v += blockDim.x) dst[v] = src[v];
}

__device__ __forceinline__ void splice_zero_row(uint4* __restrict__ dst, int vecs) {
    for (int v = threadIdx.x; v < vecs; v += blockDim.x) dst[v] = make_uint4(0u, 0u, 0u, 0u);
}

// One workgroup per output row of D 16-bit elements, 16 B per lane; lane 0 also writes the row's label and mask element.
// Every source index is checked against its buffer (ids and crop_map values live on the device: the host has validated
// its own copy, the kernel never trusts them for an address) — a row whose source is out of range is written as zeros.
__global__ void __launch_bounds__(256)
splice_kernel(const int* __restrict__ codes, const int* __restrict__ lengths, const long long* __restrict__ ids,
              const uint4* __restrict__ table, long long V, const uint4* __restrict__ feats, long long n_feat_blocks,
              const int* __restrict__ crop_map, long long n_logical, const long long* __restrict__ labels,
              const void* __restrict__ mask, int mask_bytes, uint4* __restrict__ out, long long* __restrict__ out_labels,
              void* __restrict__ out_mask, int L_in, int L_out, int M, int vecs) {
    const long long row = blockIdx.x;
    const unsigned code = (unsigned)codes[row];
    const unsigned kind = code >> 30, payload = code & kPayloadMask;
    const uint4* src = nullptr;
    if (kind == TP_SPLICE_TEXT || kind == TP_SPLICE_LITERAL) {
        const long long t = kind == TP_SPLICE_TEXT ? ids[payload] : (long long)payload;
        if (t >= 0 && t < V) src = table + t * vecs;
    } else if (kind == TP_SPLICE_FEATURE) {
        const long long k = payload / (unsigned)M, m = payload - k * M;
        if (k < n_logical) {
            const long long blk = crop_map ? (long long)crop_map[k] : k;
            if (blk >= 0 && blk < n_feat_blocks) src = feats + (blk * M + m) * vecs;
        }
    }
    uint4* dst = out + row * vecs;
    if (src) splice_copy_row(dst, src, vecs);
    else splice_zero_row(dst, vecs);
    if (threadIdx.x == 0) {
        if (out_labels) out_labels[row] = kind == TP_SPLICE_TEXT ? labels[payload] : -100LL;      // IGNORE_INDEX
        if (out_mask) {
            // llava_arch.py:214-221 / :228-230: True for the len - L_in rows the images added, the given mask, False padding
            const int b = (int)(row / L_out), r = (int)(row - (long long)b * L_out);
            const int s = r - (lengths[b] - L_in);
            if (mask_bytes == 1) {
                const unsigned char* m = (const unsigned char*)mask;
                ((unsigned char*)out_mask)[row] = s < 0 ? 1 : (s < L_in ? m[(long long)b * L_in + s] : 0);
            } else {
                const long long* m = (const long long*)mask;
                ((long long*)out_mask)[row] = s < 0 ? 1 : (s < L_in ? m[(long long)b * L_in + s] : 0);
            }
        }
    }
}

// ---- backward with respect to the features ----------------------------------------------------------------------------------
// src_row[feature row] = the output row that read it (or -1: memset), then one workgroup per dfeats row copies or zeroes.
__global__ void __launch_bounds__(256)
splice_bwd_map_kernel(const int* __restrict__ codes, long long rows, const int* __restrict__ crop_map, long long n_logical,
                      long long n_feat_blocks, int* __restrict__ src_row, int M) {
    const long long row = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= rows) return;
    const unsigned code = (unsigned)codes[row];
    if ((code >> 30) != TP_SPLICE_FEATURE) return;
    const unsigned payload = code & kPayloadMask;
    const long long k = payload / (unsigned)M, m = payload - k * M;
    if (k >= n_logical) return;
    const long long blk = crop_map ? (long long)crop_map[k] : k;
    if (blk >= 0 && blk < n_feat_blocks) src_row[blk * M + m] = (int)row;
}

__global__ void __launch_bounds__(256)
splice_bwd_feats_kernel(const uint4* __restrict__ dout, const int* __restrict__ src_row, uint4* __restrict__ dfeats, int vecs) {
    const long long row = blockIdx.x;
    const int s = src_row[row];
    uint4* dst = dfeats + row * vecs;
    if (s < 0) splice_zero_row(dst, vecs);
    else splice_copy_row(dst, dout + (long long)s * vecs, vecs);
}

// ---- backward with respect to the table -------------------------------------------------------------------------------------
// order [n_table_rows]: the output rows whose source is a table row, stably sorted by table row; offsets [V + 1]: where table
// row t's run begins.  One workgroup per table row: zero (no reader, or padding_idx), a copy (one reader), or the fp32 sum of
// its readers in `order`'s order, rounded once.  No atomics, so two runs give the same bits.
template <typename T>
__device__ __forceinline__ void splice_acc8(float* acc, const uint4 v) {
    using X8 = typename Vec<T>::x8;
    const X8 x = __builtin_bit_cast(X8, v);
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] += (float)x[j];
}

template <typename T>
__global__ void __launch_bounds__(256)
splice_bwd_table_kernel(const uint4* __restrict__ dout, const int* __restrict__ order, const int* __restrict__ offsets,
                        long long padding_idx, uint4* __restrict__ dtable, int vecs) {
    using X8 = typename Vec<T>::x8;
    const long long t = blockIdx.x;
    const int beg = offsets[t], n = offsets[t + 1] - beg;
    uint4* dst = dtable + t * vecs;
    if (n <= 0 || t == padding_idx) { splice_zero_row(dst, vecs); return; }
    if (n == 1) { splice_copy_row(dst, dout + (long long)order[beg] * vecs, vecs); return; }
    for (int v = threadIdx.x; v < vecs; v += blockDim.x) {
        float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        int i = 0;
        for (; i + 16 <= n; i += 16) {               // a row with many readers (a pad id, ',' or '\n'): sixteen loads in flight
            uint4 x[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) x[j] = dout[(long long)order[beg + i + j] * vecs + v];
#pragma unroll
            for (int j = 0; j < 16; ++j) splice_acc8<T>(acc, x[j]);      // added in order: the same sum as one by one
        }
        for (; i + 4 <= n; i += 4) {                 // four loads in flight, added in order
            const uint4 x0 = dout[(long long)order[beg + i] * vecs + v], x1 = dout[(long long)order[beg + i + 1] * vecs + v];
            const uint4 x2 = dout[(long long)order[beg + i + 2] * vecs + v], x3 = dout[(long long)order[beg + i + 3] * vecs + v];
            splice_acc8<T>(acc, x0); splice_acc8<T>(acc, x1); splice_acc8<T>(acc, x2); splice_acc8<T>(acc, x3);
        }
        for (; i < n; ++i) splice_acc8<T>(acc, dout[(long long)order[beg + i] * vecs + v]);
        X8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = (T)acc[j];
        dst[v] = __builtin_bit_cast(uint4, o);
    }
}

size_t splice_bwd_workspace_bytes(long long n_feat_blocks, int M) {
    return ((size_t)n_feat_blocks * M * sizeof(int) + 255) & ~(size_t)255;
}

// The one host-side check of a plan, for the forward (backward = 0) and the backward.  Touches host memory only.
int validate_splice(const char* what, const tp_splice_args* a, int backward) {
    if (!a) { set_error("%s: NULL argument struct", what); return TP_ERR_INVALID_ARG; }
    if (a->batch <= 0 || a->in_len <= 0 || a->out_len <= 0 || a->M <= 0 || a->V <= 0 || a->n_feat_blocks < 0 || a->n_logical < 0) {
        set_error("%s: non-positive size (batch %d, in_len %d, out_len %d, M %d, V %lld)", what, a->batch, a->in_len, a->out_len,
                  a->M, (long long)a->V);
        return TP_ERR_INVALID_ARG;
    }
    if (a->dtype != TP_BF16 && a->dtype != TP_F16) { set_error("%s: dtype %d unsupported (bf16 / fp16)", what, a->dtype); return TP_ERR_INVALID_ARG; }
    if (a->D <= 0 || a->D % 8 != 0) { set_error("%s: D = %d must be a positive multiple of 8", what, a->D); return TP_ERR_INVALID_ARG; }
    if (!a->plan_host || !a->plan_dev) { set_error("%s: NULL plan (plan_host / plan_dev)", what); return TP_ERR_INVALID_ARG; }
    const long long rows = (long long)a->batch * a->out_len, positions = (long long)a->batch * a->in_len;
    if (rows > 0x7fffffffLL || positions > (long long)kPayloadMask || a->V > (long long)kPayloadMask + 1 ||
        a->n_logical * a->M > (long long)kPayloadMask || a->n_feat_blocks * a->M > 0x7fffffffLL) {
        set_error("%s: %lld rows / %lld positions / %lld feature rows exceed one launch", what, rows, positions,
                  (long long)(a->n_logical * a->M));
        return TP_ERR_INVALID_ARG;
    }
    if (a->crop_map ? a->n_logical <= 0 : a->n_logical != a->n_feat_blocks) {
        set_error("%s: n_logical = %lld (the crop_map's length; without a crop_map it equals n_feat_blocks = %lld)", what,
                  (long long)a->n_logical, (long long)a->n_feat_blocks);
        return TP_ERR_INVALID_ARG;
    }
    if (a->mask_bytes != 1 && a->mask_bytes != 8 && (a->mask || a->out_mask)) {
        set_error("%s: mask_bytes = %d (1: bool, 8: int64)", what, a->mask_bytes);
        return TP_ERR_INVALID_ARG;
    }
    if (!backward) {
        if (!a->out || !a->table || !a->ids_dev) { set_error("%s: NULL out / table / ids_dev", what); return TP_ERR_INVALID_ARG; }
        if ((a->labels == nullptr) != (a->out_labels == nullptr) || (a->mask == nullptr) != (a->out_mask == nullptr)) {
            set_error("%s: labels / out_labels and mask / out_mask come in pairs", what);
            return TP_ERR_INVALID_ARG;
        }
        if (((uintptr_t)a->out & 15) || ((uintptr_t)a->table & 15) || ((uintptr_t)a->feats & 15) || ((uintptr_t)a->plan_dev & 3) ||
            ((uintptr_t)a->ids_dev & 7) || ((uintptr_t)a->labels & 7) || ((uintptr_t)a->out_labels & 7) ||
            (a->mask_bytes == 8 && (((uintptr_t)a->mask & 7) || ((uintptr_t)a->out_mask & 7))) || ((uintptr_t)a->crop_map & 3)) {
            set_error("%s: misaligned pointer (out / table / feats 16 B, ids / labels / int64 mask 8 B, plan / crop_map 4 B)", what);
            return TP_ERR_INVALID_ARG;
        }
    } else {
        if (!a->dout || (!a->dfeats && !a->dtable)) { set_error("%s: NULL dout, or neither dfeats nor dtable wanted", what); return TP_ERR_INVALID_ARG; }
        if (((uintptr_t)a->dout & 15) || ((uintptr_t)a->dfeats & 15) || ((uintptr_t)a->dtable & 15) || ((uintptr_t)a->plan_dev & 3) ||
            ((uintptr_t)a->workspace & 15) || ((uintptr_t)a->order_dev & 3) || ((uintptr_t)a->crop_map & 3)) {
            set_error("%s: misaligned pointer (dout / dfeats / dtable / workspace 16 B, plan / order / crop_map 4 B)", what);
            return TP_ERR_INVALID_ARG;
        }
        if (a->dfeats && a->n_feat_blocks <= 0) { set_error("%s: dfeats wanted but n_feat_blocks = 0", what); return TP_ERR_INVALID_ARG; }
        if (a->dtable && (!a->order_host || !a->order_dev || !a->ids_host)) {
            set_error("%s: dtable needs order_host, order_dev and ids_host", what);
            return TP_ERR_INVALID_ARG;
        }
        if (a->dtable && a->padding_idx >= a->V) { set_error("%s: padding_idx %lld outside the table", what, (long long)a->padding_idx); return TP_ERR_INVALID_ARG; }
    }
    // the codes, row by row
    const int32_t* codes = a->plan_host;
    const int32_t* lengths = a->plan_host + rows;
    long long n_table = 0, n_feat = 0;
    for (long long row = 0; row < rows; ++row) {
        const unsigned code = (unsigned)codes[row], kind = code >> 30, payload = code & kPayloadMask;
        if (kind == TP_SPLICE_TEXT) {
            if (payload >= positions || payload / (unsigned)a->in_len != row / a->out_len) {
                set_error("%s: plan row %lld reads position %u outside its sample", what, row, payload);
                return TP_ERR_INVALID_ARG;
            }
            if (a->ids_host && (a->ids_host[payload] < 0 || a->ids_host[payload] >= a->V)) {
                set_error("%s: input id %lld at position %u is outside the table [0, %lld)", what, (long long)a->ids_host[payload],
                          payload, (long long)a->V);
                return TP_ERR_INVALID_ARG;
            }
            ++n_table;
        } else if (kind == TP_SPLICE_LITERAL) {
            if (payload >= a->V) { set_error("%s: plan row %lld names table row %u of %lld", what, row, payload, (long long)a->V); return TP_ERR_INVALID_ARG; }
            ++n_table;
        } else if (kind == TP_SPLICE_FEATURE) {
            if (!a->feats && !backward) { set_error("%s: the plan reads features but feats is NULL", what); return TP_ERR_INVALID_ARG; }
            if ((long long)payload >= a->n_logical * a->M) {
                set_error("%s: plan row %lld reads feature row %u of %lld", what, row, payload, (long long)(a->n_logical * a->M));
                return TP_ERR_INVALID_ARG;
            }
            ++n_feat;
        }
    }
    for (int b = 0; b < a->batch; ++b)
        if (lengths[b] < a->in_len || lengths[b] > a->out_len) {
            set_error("%s: sample %d has length %d outside [in_len %d, out_len %d]", what, b, lengths[b], a->in_len, a->out_len);
            return TP_ERR_INVALID_ARG;
        }
    if (!backward) return TP_OK;
    if (a->dfeats) {
        // every feature row feeds at most one output row: its gradient is a copy, not a sum
        std::vector<unsigned char> seen((size_t)(a->n_logical * a->M), 0);
        for (long long row = 0; row < rows; ++row) {
            const unsigned code = (unsigned)codes[row];
            if ((code >> 30) != TP_SPLICE_FEATURE) continue;
            if (seen[code & kPayloadMask]++) {
                set_error("%s: feature row %u is read by two output rows (dfeats is a copy, not a sum)", what, code & kPayloadMask);
                return TP_ERR_INVALID_ARG;
            }
        }
        const size_t need = splice_bwd_workspace_bytes(a->n_feat_blocks, a->M);
        if (!a->workspace || a->workspace_bytes < need) {
            set_error("%s: workspace %zu B < %zu B", what, a->workspace ? a->workspace_bytes : (size_t)0, need);
            return TP_ERR_WORKSPACE;
        }
    }
    if (a->dtable) {
        if (a->n_table_rows != n_table) {
            set_error("%s: n_table_rows = %lld, the plan has %lld rows that read the table", what, (long long)a->n_table_rows, n_table);
            return TP_ERR_INVALID_ARG;
        }
        const int32_t* order = a->order_host;
        const int32_t* offsets = a->order_host + n_table;
        if (offsets[0] != 0 || offsets[a->V] != n_table) {
            set_error("%s: offsets must run from 0 to n_table_rows = %lld", what, n_table);
            return TP_ERR_INVALID_ARG;
        }
        for (long long t = 0; t < a->V; ++t) {
            if (offsets[t + 1] < offsets[t] || offsets[t + 1] > n_table) {
                set_error("%s: offsets[%lld] is not monotone", what, t + 1);
                return TP_ERR_INVALID_ARG;
            }
            for (int i = offsets[t]; i < offsets[t + 1]; ++i) {
                const long long row = order[i];
                bool ok = row >= 0 && row < rows && (i == offsets[t] || order[i - 1] < row);
                if (ok) {
                    const unsigned code = (unsigned)codes[row], kind = code >> 30, payload = code & kPayloadMask;
                    ok = (kind == TP_SPLICE_TEXT && a->ids_host[payload] == t) || (kind == TP_SPLICE_LITERAL && (long long)payload == t);
                }
                if (!ok) {
                    set_error("%s: order[%d] does not list the readers of table row %lld in increasing row order", what, i, t);
                    return TP_ERR_INVALID_ARG;
                }
            }
        }
    }
    (void)n_feat;
    return TP_OK;
}

}  // namespace

extern "C" {

int tp_splice(const tp_splice_args* a, void* stream) {
    const int rc = validate_splice("tp_splice", a, 0);
    if (rc != TP_OK) return rc;
    const long long rows = (long long)a->batch * a->out_len;
    const int* plan = (const int*)a->plan_dev;
    hipLaunchKernelGGL(splice_kernel, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, plan, plan + rows,
                       (const long long*)a->ids_dev, (const uint4*)a->table, (long long)a->V, (const uint4*)a->feats,
                       (long long)a->n_feat_blocks, (const int*)a->crop_map, (long long)a->n_logical, (const long long*)a->labels,
                       a->mask, a->mask_bytes, (uint4*)a->out, (long long*)a->out_labels, a->out_mask, a->in_len, a->out_len, a->M,
                       a->D / 8);
    return check_launch("splice_kernel");
}

size_t tp_splice_backward_workspace_bytes(int64_t n_feat_blocks, int M) {
    if (n_feat_blocks <= 0 || M <= 0) return 0;
    return splice_bwd_workspace_bytes(n_feat_blocks, M);
}

int tp_splice_backward(const tp_splice_args* a, void* stream_) {
    int rc = validate_splice("tp_splice_backward", a, 1);
    if (rc != TP_OK) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    const long long rows = (long long)a->batch * a->out_len;
    const int vecs = a->D / 8;
    if (a->dfeats) {
        int* src_row = (int*)a->workspace;
        const long long feat_rows = a->n_feat_blocks * a->M;
        hipError_t e = hipMemsetAsync(src_row, 0xff, (size_t)feat_rows * sizeof(int), stream);
        if (e != hipSuccess) { set_error("tp_splice_backward: hipMemsetAsync: %s", hipGetErrorString(e)); return TP_ERR_LAUNCH; }
        hipLaunchKernelGGL(splice_bwd_map_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, stream, (const int*)a->plan_dev,
                           rows, (const int*)a->crop_map, (long long)a->n_logical, (long long)a->n_feat_blocks, src_row, a->M);
        if ((rc = check_launch("splice_bwd_map_kernel")) != TP_OK) return rc;
        hipLaunchKernelGGL(splice_bwd_feats_kernel, dim3((unsigned)feat_rows), dim3(256), 0, stream, (const uint4*)a->dout,
                           (const int*)src_row, (uint4*)a->dfeats, vecs);
        if ((rc = check_launch("splice_bwd_feats_kernel")) != TP_OK) return rc;
    }
    if (a->dtable) {
        auto kernel = a->dtype == TP_BF16 ? splice_bwd_table_kernel<bf16_t> : splice_bwd_table_kernel<f16_t>;
        const int* order = (const int*)a->order_dev;
        hipLaunchKernelGGL(kernel, dim3((unsigned)a->V), dim3(256), 0, stream, (const uint4*)a->dout, order, order + a->n_table_rows,
                           (long long)a->padding_idx, (uint4*)a->dtable, vecs);
        if ((rc = check_launch("splice_bwd_table_kernel")) != TP_OK) return rc;
    }
    return TP_OK;
}

}  // extern "C"
