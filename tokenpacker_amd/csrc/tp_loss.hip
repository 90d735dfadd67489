// tp_loss.hip — the LLM's loss (llava_llama.py:95-106: logits[..., :-1, :] against labels[..., 1:], CrossEntropyLoss) on given
// logits, over the labelled rows only: one forward launch per row + one fixed-order reduction, one backward launch.
// See include/tokenpacker.h ("shifted cross-entropy") for the contract.
//
// Row (b, t), t < len - 1, has the target labels[b, t + 1].  A row whose target is ignore_index is never read.  A labelled row
// is streamed once with an online maximum / rescaled sum in fp32; the row leaves four fp32 words in the workspace:
//     lse = m + log(s),  loss = log(s) - (x[target] - m),  m (the row maximum)  and  log(s), s = sum exp(x - m).
// The backward recomputes the probabilities as exp((x - m) - log(s)) — the two halves of the lse kept apart, as torch's
// log_softmax does, so that a probability near 1 does not inherit the rounding of an lse of 20.
//
// THREAD-TO-ELEMENT MAP of a row of V elements starting at address p (forward and backward alike; tests build on it):
//     E    = 16 / sizeof(element): 8 for bf16 / fp16, 4 for fp32
//     head = min(V, the elements in front of the first 16-byte boundary at or after p) = ((16 - p % 16) % 16) / sizeof(element)
//     nvec = (V - head) / E whole 16-byte vectors, tail = V - head - nvec * E
//     thread i of 256 reads   element i                               if i < head
//                             elements head + E * v .. head + E * v + E - 1   for v = i, i + 256, i + 512, ... < nvec
//                             element  head + E * nvec + i            if i < tail
// Only those whole vectors are accessed 16 bytes wide, each at a 16-byte aligned address; head and tail go element by element.
//
// -inf: a running maximum of -inf (all a thread, or the whole workgroup, has seen so far is -inf) must not produce
// exp(-inf - (-inf)); every rescale subtracts max_or_zero() instead, which turns that term into exp(-inf) = 0.
#include "tp_internal.h"

using namespace tp;

namespace {

constexpr int kCeThreads = 256;
constexpr int kCeUnroll = 4;                      // 16-byte loads in flight per thread
constexpr size_t kCeHeaderBytes = 256;            // loss | 1 / n_valid | n_valid (int64) | padding
constexpr int kCeRowWords = 4;                    // lse | loss | m | log(s): four fp32 arrays of `rows` words behind the header

template <typename T> struct CeVec { static constexpr int E = 16 / (int)sizeof(T); };

__device__ __forceinline__ float ce_neg_inf() { return -__builtin_inff(); }
__device__ __forceinline__ float max_or_zero(float m) { return m == ce_neg_inf() ? 0.f : m; }

template <typename T> __device__ __forceinline__ void ce_load_vec(const T* p, float* f) {
    if constexpr (sizeof(T) == 4) {
        const f32x4 v = *(const f32x4*)p;
#pragma unroll
        for (int j = 0; j < 4; ++j) f[j] = v[j];
    } else {
        const typename Vec<T>::x8 v = *(const typename Vec<T>::x8*)p;
#pragma unroll
        for (int j = 0; j < 8; ++j) f[j] = (float)v[j];
    }
}

template <typename T> __device__ __forceinline__ void ce_store_vec(T* p, const float* f) {
    if constexpr (sizeof(T) == 4) {
        f32x4 v;
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = f[j];
        *(f32x4*)p = v;
    } else {
        typename Vec<T>::x8 v;
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = (T)f[j];
        *(typename Vec<T>::x8*)p = v;
    }
}

// head / nvec / tail of the map above
template <typename T> __device__ __forceinline__ void ce_split_row(const void* p, int V, int& head, int& nvec, int& tail) {
    constexpr int E = CeVec<T>::E;
    head = (int)(((16u - (unsigned)((uintptr_t)p & 15u)) & 15u) / (unsigned)sizeof(T));
    head = head < V ? head : V;
    nvec = (V - head) / E;
    tail = V - head - nvec * E;
}

// (m, s) += N more logits
template <int N> __device__ __forceinline__ void ce_online_add(float& m, float& s, const float* x) {
    float cm = x[0];
#pragma unroll
    for (int j = 1; j < N; ++j) cm = fmaxf(cm, x[j]);
    const float mn = fmaxf(m, cm), ref = max_or_zero(mn);
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < N; ++j) acc += __expf(x[j] - ref);
    s = s * __expf(m - ref) + acc;
    m = mn;
}

__device__ __forceinline__ void ce_online_merge(float& m, float& s, float m2, float s2) {
    const float mn = fmaxf(m, m2), ref = max_or_zero(mn);
    s = s * __expf(m - ref) + s2 * __expf(m2 - ref);
    m = mn;
}

// One workgroup per row (b, t), t < len - 1.
template <typename T>
__global__ void __launch_bounds__(kCeThreads)
shift_ce_fwd_kernel(const T* __restrict__ logits, long long row_stride, long long batch_stride, const long long* __restrict__ labels,
                    long long ignore_index, float* __restrict__ row_words, long long rows, int len, int V) {
    constexpr int E = CeVec<T>::E;
    __shared__ float sh_m[kCeThreads / 64], sh_s[kCeThreads / 64], sh_xt;
    const long long r = blockIdx.x;
    const int b = (int)(r / (len - 1)), t = (int)(r - (long long)b * (len - 1));
    const long long tgt = labels[(long long)b * len + t + 1];
    float* lse = row_words;
    float* loss = lse + rows;
    float* rmax = loss + rows;
    float* logs = rmax + rows;
    if (tgt == ignore_index) {                       // not labelled: the row is not read
        if (threadIdx.x == 0) { lse[r] = 0.f; loss[r] = 0.f; rmax[r] = 0.f; logs[r] = 0.f; }
        return;
    }
    // a target outside [0, V) matches no element: x[target] stays NaN and so does the row's loss.  No address comes from it.
    const unsigned tgt_u = (tgt >= 0 && tgt < V) ? (unsigned)tgt : 0xffffffffu;
    if (threadIdx.x == 0) sh_xt = __builtin_nanf("");
    __syncthreads();

    const T* row = logits + (long long)b * batch_stride + (long long)t * row_stride;      // 64-bit row base, 32-bit inside
    int head, nvec, tail;
    ce_split_row<T>(row, V, head, nvec, tail);
    const int tid = threadIdx.x;
    float m = ce_neg_inf(), s = 0.f;
    if (tid < head) {
        const float x = (float)row[tid];
        ce_online_add<1>(m, s, &x);
        if ((unsigned)tid == tgt_u) sh_xt = x;
    }
    const T* body = row + head;
    for (int v0 = tid; v0 < nvec; v0 += kCeThreads * kCeUnroll) {
        float x[kCeUnroll * E];
#pragma unroll
        for (int u = 0; u < kCeUnroll; ++u) {
            const int v = v0 + u * kCeThreads;
            if (v < nvec) {
                ce_load_vec<T>(body + (size_t)v * E, x + u * E);
            } else {
#pragma unroll
                for (int j = 0; j < E; ++j) x[u * E + j] = ce_neg_inf();
            }
        }
#pragma unroll
        for (int u = 0; u < kCeUnroll; ++u) {
            const unsigned d = tgt_u - (unsigned)(head + (v0 + u * kCeThreads) * E);
            if (d < (unsigned)E && v0 + u * kCeThreads < nvec) {
#pragma unroll
                for (int j = 0; j < E; ++j) if (d == (unsigned)j) sh_xt = x[u * E + j];
            }
        }
        ce_online_add<kCeUnroll * E>(m, s, x);
    }
    if (tid < tail) {
        const int i = head + nvec * E + tid;
        const float x = (float)row[i];
        ce_online_add<1>(m, s, &x);
        if ((unsigned)i == tgt_u) sh_xt = x;
    }
    // the 64 lanes of a wave, then the waves in order: a fixed tree
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float m2 = __shfl_xor(m, off, 64), s2 = __shfl_xor(s, off, 64);
        ce_online_merge(m, s, m2, s2);
    }
    if ((tid & 63) == 0) { sh_m[tid >> 6] = m; sh_s[tid >> 6] = s; }
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int w = 1; w < kCeThreads / 64; ++w) ce_online_merge(m, s, sh_m[w], sh_s[w]);
        const float ls = logf(s);
        lse[r] = m + ls;
        loss[r] = ls - (sh_xt - m);                  // = -log_softmax(x)[target], in torch's order of operations
        rmax[r] = m;
        logs[r] = ls;
    }
}

// One workgroup: the row losses summed in fp64 and the labelled rows counted, each thread over rows tid, tid + 1024, ... in
// order, then a fixed tree.  No atomics: two runs give the same bits.
__global__ void __launch_bounds__(1024)
shift_ce_reduce_kernel(const long long* __restrict__ labels, long long ignore_index, const float* __restrict__ row_loss,
                       long long rows, int len, int mean, float* __restrict__ header) {
    __shared__ double sh_sum[1024];
    __shared__ long long sh_cnt[1024];
    double sum = 0.0;
    long long cnt = 0;
    for (long long r0 = threadIdx.x; r0 < rows; r0 += 1024 * 4) {
        long long lab[4];
        float l[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {                // four independent pairs of loads in flight; rows < 2^31 (the host checks)
            const long long r = r0 + u * 1024;
            const bool in = r < rows;
            const unsigned b = in ? (unsigned)r / (unsigned)(len - 1) : 0u;
            lab[u] = in ? labels[r + b + 1] : ignore_index;              // b * len + t + 1 with r = b * (len - 1) + t
            l[u] = in ? row_loss[r] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (lab[u] != ignore_index) { sum += (double)l[u]; ++cnt; }
    }
    sh_sum[threadIdx.x] = sum;
    sh_cnt[threadIdx.x] = cnt;
    __syncthreads();
    for (int half = 512; half > 0; half >>= 1) {
        if ((int)threadIdx.x < half) {
            sh_sum[threadIdx.x] += sh_sum[threadIdx.x + half];
            sh_cnt[threadIdx.x] += sh_cnt[threadIdx.x + half];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double n = (double)sh_cnt[0];
        header[0] = (float)(mean ? sh_sum[0] / n : sh_sum[0]);      // no labelled row: 0 / 0 = NaN, as the reference's mean
        header[1] = (float)(1.0 / n);
        *(long long*)(header + 2) = sh_cnt[0];
    }
}

// One workgroup per row (b, t) of dlogits, t < len: g * w * (softmax - onehot) for a labelled row, zeros for every other row
// (unlabelled, t = len - 1, a target outside [0, V)).  dlogits may be the logits themselves: every thread reads what it
// overwrites and nothing else.  The host has checked that a dlogits row sits at the same offset from a 16-byte boundary as
// its logits row, so one split serves both.
template <typename T>
__global__ void __launch_bounds__(kCeThreads)
shift_ce_bwd_kernel(const T* logits, long long row_stride, long long batch_stride, T* dlogits, long long d_row_stride,
                    long long d_batch_stride, const long long* __restrict__ labels, long long ignore_index,
                    const float* __restrict__ row_words, long long rows, const float* __restrict__ header,
                    const float* __restrict__ grad_loss, int mean, int len, int V) {
    constexpr int E = CeVec<T>::E;
    const long long r = blockIdx.x;
    const int b = (int)(r / len), t = (int)(r - (long long)b * len);
    T* dst = dlogits + (long long)b * d_batch_stride + (long long)t * d_row_stride;
    int head, nvec, tail;
    ce_split_row<T>(dst, V, head, nvec, tail);
    const int tid = threadIdx.x;
    long long tgt = ignore_index;
    if (t < len - 1) tgt = labels[(long long)b * len + t + 1];
    if (t == len - 1 || tgt == ignore_index || tgt < 0 || tgt >= V) {
        float z[E];
#pragma unroll
        for (int j = 0; j < E; ++j) z[j] = 0.f;
        if (tid < head) dst[tid] = (T)0.f;
        for (int v = tid; v < nvec; v += kCeThreads) ce_store_vec<T>(dst + head + (size_t)v * E, z);
        if (tid < tail) dst[head + nvec * E + tid] = (T)0.f;
        return;
    }
    const T* src = logits + (long long)b * batch_stride + (long long)t * row_stride;
    const long long fr = (long long)b * (len - 1) + t;
    const float m = row_words[2 * rows + fr], ls = row_words[3 * rows + fr];
    float gw = grad_loss[0];
    if (mean) gw = gw / (float)*(const long long*)(header + 2);
    const unsigned tgt_u = (unsigned)tgt;
    if (tid < head) {
        const float p = __expf(((float)src[tid] - m) - ls);
        dst[tid] = (T)(((unsigned)tid == tgt_u ? p - 1.f : p) * gw);
    }
    for (int v0 = tid; v0 < nvec; v0 += kCeThreads * kCeUnroll) {
        float x[kCeUnroll * E];
#pragma unroll
        for (int u = 0; u < kCeUnroll; ++u) {
            const int v = v0 + u * kCeThreads;
            if (v < nvec) ce_load_vec<T>(src + head + (size_t)v * E, x + u * E);
        }
#pragma unroll
        for (int u = 0; u < kCeUnroll; ++u) {
            const int v = v0 + u * kCeThreads;
            if (v < nvec) {
                float* xu = x + u * E;
#pragma unroll
                for (int j = 0; j < E; ++j) xu[j] = __expf((xu[j] - m) - ls);
                const unsigned d = tgt_u - (unsigned)(head + v * E);
                if (d < (unsigned)E) {
#pragma unroll
                    for (int j = 0; j < E; ++j) if (d == (unsigned)j) xu[j] -= 1.f;
                }
#pragma unroll
                for (int j = 0; j < E; ++j) xu[j] *= gw;
                ce_store_vec<T>(dst + head + (size_t)v * E, xu);
            }
        }
    }
    if (tid < tail) {
        const int i = head + nvec * E + tid;
        const float p = __expf(((float)src[i] - m) - ls);
        dst[i] = (T)(((unsigned)i == tgt_u ? p - 1.f : p) * gw);
    }
}

size_t shift_ce_workspace_bytes(long long batch, long long len) {
    const size_t rows = (size_t)batch * (size_t)(len - 1);
    return kCeHeaderBytes + ((rows * kCeRowWords * sizeof(float) + 255) & ~(size_t)255);
}

int elem_bytes(int dtype) { return dtype == TP_F32 ? 4 : 2; }

// The one host-side check of both directions.  Touches no device memory.
int validate_shift_ce(const char* what, const tp_shift_ce_args* a, int backward) {
    if (!a) { set_error("%s: NULL argument struct", what); return TP_ERR_INVALID_ARG; }
    if (a->batch < 1 || a->len < 1 || a->V < 1) {
        set_error("%s: batch %d, len %d, V %d must each be >= 1", what, a->batch, a->len, a->V);
        return TP_ERR_INVALID_ARG;
    }
    if (a->dtype != TP_BF16 && a->dtype != TP_F16 && a->dtype != TP_F32) {
        set_error("%s: dtype %d unsupported (bf16 / fp16 / fp32)", what, a->dtype);
        return TP_ERR_INVALID_ARG;
    }
    if (a->reduction != TP_CE_MEAN && a->reduction != TP_CE_SUM) {
        set_error("%s: reduction %d unknown (TP_CE_MEAN / TP_CE_SUM)", what, a->reduction);
        return TP_ERR_INVALID_ARG;
    }
    if ((long long)a->batch * a->len > 0x7fffffffLL) {
        set_error("%s: %lld rows exceed one launch", what, (long long)a->batch * a->len);
        return TP_ERR_INVALID_ARG;
    }
    if (!a->logits || !a->labels || !a->workspace) { set_error("%s: NULL logits / labels / workspace", what); return TP_ERR_INVALID_ARG; }
    if (a->row_stride < a->V) {
        set_error("%s: row_stride %lld < V %d", what, (long long)a->row_stride, a->V);
        return TP_ERR_INVALID_ARG;
    }
    const size_t need = shift_ce_workspace_bytes(a->batch, a->len);
    if (a->workspace_bytes < need) { set_error("%s: workspace %zu B < %zu B", what, a->workspace_bytes, need); return TP_ERR_INVALID_ARG; }
    const uintptr_t es = (uintptr_t)elem_bytes(a->dtype);
    if (((uintptr_t)a->logits & (es - 1)) || ((uintptr_t)a->labels & 7) || ((uintptr_t)a->workspace & 15)) {
        set_error("%s: misaligned pointer (logits: its element size, labels 8 B, workspace 16 B)", what);
        return TP_ERR_INVALID_ARG;
    }
    if (!backward) return TP_OK;
    if (!a->dlogits || !a->grad_loss) { set_error("%s: NULL dlogits / grad_loss", what); return TP_ERR_INVALID_ARG; }
    if (((uintptr_t)a->dlogits & (es - 1)) || ((uintptr_t)a->grad_loss & 3)) {
        set_error("%s: misaligned pointer (dlogits: its element size, grad_loss 4 B)", what);
        return TP_ERR_INVALID_ARG;
    }
    if (a->d_row_stride < a->V) {
        set_error("%s: d_row_stride %lld < V %d", what, (long long)a->d_row_stride, a->V);
        return TP_ERR_INVALID_ARG;
    }
    if (a->dlogits == a->logits && (a->d_row_stride != a->row_stride || a->d_batch_stride != a->batch_stride)) {
        set_error("%s: in place (dlogits == logits) the strides of dlogits must be those of logits", what);
        return TP_ERR_INVALID_ARG;
    }
    // every dlogits row at the same offset from a 16-byte boundary as its logits row: one head / body / tail split for both
    const long long per16 = 16 / (long long)es;
    if ((((uintptr_t)a->dlogits - (uintptr_t)a->logits) & 15) || (a->len > 1 && (a->d_row_stride - a->row_stride) % per16 != 0) ||
        (a->batch > 1 && (a->d_batch_stride - a->batch_stride) % per16 != 0)) {
        set_error("%s: dlogits and its strides must be congruent to logits and its strides modulo 16 bytes", what);
        return TP_ERR_INVALID_ARG;
    }
    return TP_OK;
}

template <typename T> int launch_fwd(const tp_shift_ce_args* a, hipStream_t stream) {
    const long long rows = (long long)a->batch * (a->len - 1);
    float* header = (float*)a->workspace;
    float* row_words = (float*)((char*)a->workspace + kCeHeaderBytes);
    if (rows > 0) {                                  // (len = 1: no row, and an empty grid is not a launch)
        hipLaunchKernelGGL(shift_ce_fwd_kernel<T>, dim3((unsigned)rows), dim3(kCeThreads), 0, stream, (const T*)a->logits,
                           (long long)a->row_stride, (long long)a->batch_stride, (const long long*)a->labels,
                           (long long)a->ignore_index, row_words, rows, a->len, a->V);
        const int rc = check_launch("shift_ce_fwd_kernel");
        if (rc != TP_OK) return rc;
    }
    hipLaunchKernelGGL(shift_ce_reduce_kernel, dim3(1), dim3(1024), 0, stream, (const long long*)a->labels, (long long)a->ignore_index,
                       (const float*)(row_words + rows), rows, a->len, a->reduction == TP_CE_MEAN ? 1 : 0, header);
    return check_launch("shift_ce_reduce_kernel");
}

template <typename T> int launch_bwd(const tp_shift_ce_args* a, hipStream_t stream) {
    const long long rows = (long long)a->batch * (a->len - 1);
    const float* header = (const float*)a->workspace;
    const float* row_words = (const float*)((const char*)a->workspace + kCeHeaderBytes);
    hipLaunchKernelGGL(shift_ce_bwd_kernel<T>, dim3((unsigned)((long long)a->batch * a->len)), dim3(kCeThreads), 0, stream,
                       (const T*)a->logits, (long long)a->row_stride, (long long)a->batch_stride, (T*)a->dlogits,
                       (long long)a->d_row_stride, (long long)a->d_batch_stride, (const long long*)a->labels,
                       (long long)a->ignore_index, row_words, rows, header, a->grad_loss, a->reduction == TP_CE_MEAN ? 1 : 0, a->len,
                       a->V);
    return check_launch("shift_ce_bwd_kernel");
}

}  // namespace

extern "C" {

size_t tp_shift_ce_workspace_bytes(int batch, int len) {
    if (batch < 1 || len < 1) return 0;
    return shift_ce_workspace_bytes(batch, len);
}

int tp_shift_ce_forward(const tp_shift_ce_args* a, void* stream) {
    const int rc = validate_shift_ce("tp_shift_ce_forward", a, 0);
    if (rc != TP_OK) return rc;
    if (a->dtype == TP_BF16) return launch_fwd<bf16_t>(a, (hipStream_t)stream);
    if (a->dtype == TP_F16) return launch_fwd<f16_t>(a, (hipStream_t)stream);
    return launch_fwd<float>(a, (hipStream_t)stream);
}

int tp_shift_ce_backward(const tp_shift_ce_args* a, void* stream) {
    const int rc = validate_shift_ce("tp_shift_ce_backward", a, 1);
    if (rc != TP_OK) return rc;
    if (a->dtype == TP_BF16) return launch_bwd<bf16_t>(a, (hipStream_t)stream);
    if (a->dtype == TP_F16) return launch_bwd<f16_t>(a, (hipStream_t)stream);
    return launch_bwd<float>(a, (hipStream_t)stream);
}

}  // extern "C"
