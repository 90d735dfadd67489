// Fused clip + AdamW step on the fp32 main_grad buffers (tp_optim_step, include/tokenpacker.h "optimizer step"): the consumer of
// what tp_backward_sink accumulates.  Three launches for a table of up to kOptimTable tensors, no host synchronisation, no atomics:
//   optim_sumsq_kernel    one workgroup per chunk of kOptimChunk elements: the fp32 sum of (grad * inv_scale)^2 -> partials[chunk]
//   optim_prepare_kernel  one workgroup: the partials summed in index order in fp64 -> the state block (norm, coefficient,
//                         found_inf, the step counters, the bias corrections of the step being applied)
//   optim_adamw_kernel    one workgroup per chunk: the AdamW update on the fp32 masters, the model-dtype write-back, the zeroing
//                         (T = float: the fp32 parameter IS the master — no write-back, `param` is NULL)
// A chunk is a fixed number of elements and every sum has a fixed order (a serial chain of kOptimChain terms per lane, then a
// fixed tree over the workgroup; the partials in index order): results do not depend on the grid or on the number of CUs, and two
// runs give the same bits.  The table travels by value as a kernel argument (pack_batch_kernel's style); a longer list is
// served by consecutive launches over the same partials array.
//
// The sharded step (tp_optim_sumsq / tp_optim_apply, "sharded optimizer step" in the header) is the same work cut in two, with room
// for a collective in between: tp_optim_sumsq = optim_sumsq_kernel + optim_reduce_kernel (the partials summed in fp64, in
// optim_prepare_kernel's order, into one double); tp_optim_apply = optim_prepare_sums_kernel (the ranks' doubles added in index
// order, then optim_prepare_kernel's state block) + optim_adamw_kernel.  Both read the gradient through s = inv_scale * grad_scale
// (grad_scale: the host's 1 / world size of gradient averaging; tp_optim_step passes 1, which changes no bit).
//
// These are bandwidth kernels (34 B per parameter + 4 B for the norm): 16-byte loads, all of a lane's loads issued before the
// first use, 16-byte stores; a tensor whose pointers or length do not allow that takes the scalar path.
#include "tp_internal.h"

#include <algorithm>
#include <cmath>
#include <utility>
#include <vector>

using namespace tp;

namespace {

constexpr int kOptimThreads = 256;
constexpr int kOptimVecs = 4;                                  // 16-byte vectors per lane and array
constexpr int kOptimChain = 4 * kOptimVecs;                    // terms of a lane's serial chain (tests/optim_ref.py: CHAIN)
constexpr int kOptimChunk = kOptimThreads * kOptimChain;       // elements per workgroup (tests/optim_ref.py: CHUNK)
constexpr int kOptimTreeDepth = 8;                             // log2(kOptimThreads): additions of the workgroup's tree (TREE_DEPTH)
constexpr int kOptimTable = 32;                                // tensors of one launch
static_assert(kOptimThreads == 1 << kOptimTreeDepth && kOptimThreads / 64 == 4, "optim_block_sum's tree is written for 4 waves of 64");

struct OptimEntry {
    void* param; float* master; float* grad; float* exp_avg; float* exp_avg_sq;
    long long numel;
    float lr, weight_decay;
    int first_chunk;                                           // index of the tensor's first chunk among ALL chunks of the call
    int pad_;
};
struct OptimTable {
    OptimEntry e[kOptimTable];
    int count;
    int chunk_base;                                            // first chunk of this launch: workgroup b owns chunk chunk_base + b
};

// the entry that owns chunk c (entries are in chunk order; wave-uniform)
__device__ __forceinline__ int optim_entry_of(const OptimTable& tab, int c) {
    int i = 0;
    for (int k = 1; k < tab.count; ++k)
        if (tab.e[k].first_chunk <= c) i = k;
    return i;
}

// Sum over the workgroup in a fixed tree: 6 levels inside each wave, 2 over the 4 waves.  A NaN / inf term survives.
__device__ __forceinline__ float optim_block_sum(float v, float* lds) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off, 64);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) lds[wave] = v;
    __syncthreads();
    return (lds[0] + lds[1]) + (lds[2] + lds[3]);
}

// what a gradient is multiplied by before anything else: one fp32 product (by 1 when grad_scale == 1: the bits of inv_scale alone)
__device__ __forceinline__ float optim_scale(const float* __restrict__ inv_scale, float grad_scale) {
#pragma clang fp contract(off)
    return (inv_scale ? inv_scale[0] : 1.0f) * grad_scale;
}

__global__ void __launch_bounds__(kOptimThreads)
optim_sumsq_kernel(const OptimTable tab, const float* __restrict__ inv_scale, float grad_scale, float* __restrict__ partials) {
    __shared__ float lds[kOptimThreads / 64];
    const int c = tab.chunk_base + (int)blockIdx.x;
    const OptimEntry e = tab.e[optim_entry_of(tab, c)];
    const long long base = (long long)(c - e.first_chunk) * kOptimChunk;
    const long long left = e.numel - base;
    const int n = left < kOptimChunk ? (int)left : kOptimChunk;
    const float s = optim_scale(inv_scale, grad_scale);
    const int t = threadIdx.x;
    const float* g = e.grad + base;
    float acc = 0.f;
    if ((e.numel & 3) == 0 && ((uintptr_t)e.grad & 15) == 0) {
        f32x4 v[kOptimVecs];
#pragma unroll
        for (int j = 0; j < kOptimVecs; ++j) {
            const int i = j * kOptimThreads + t;
            v[j] = i * 4 < n ? *((const f32x4*)g + i) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int j = 0; j < kOptimVecs; ++j)
#pragma unroll
            for (int k = 0; k < 4; ++k) { const float x = v[j][k] * s; acc = fmaf(x, x, acc); }
    } else {
        float v[kOptimChain];
#pragma unroll
        for (int j = 0; j < kOptimChain; ++j) {
            const int i = j * kOptimThreads + t;
            v[j] = i < n ? g[i] : 0.f;
        }
#pragma unroll
        for (int j = 0; j < kOptimChain; ++j) { const float x = v[j] * s; acc = fmaf(x, x, acc); }
    }
    acc = optim_block_sum(acc, lds);
    if (t == 0) partials[c] = acc;
}

// The partials summed in fp64 in index order: lane t sums its contiguous run (16-byte loads where the run allows, the additions in
// index order all the same), the tree then joins neighbouring runs.  The sum is lane 0's return value; nparts == 0 gives 0.0.
__device__ __forceinline__ double optim_sum_partials(const float* __restrict__ partials, int nparts, double* lds) {
    const int t = threadIdx.x;
    const int per = (nparts + kOptimThreads - 1) / kOptimThreads;
    const int lo = t * per < nparts ? t * per : nparts, hi = lo + per < nparts ? lo + per : nparts;
    double a = 0.0;
    int i = lo;
    for (; i < hi && (i & 3); ++i) a += (double)partials[i];
    for (; i + 4 <= hi; i += 4) {                                      // (partials is 16-byte aligned: the workspace's contract)
        const f32x4 v = *(const f32x4*)(partials + i);
        a += (double)v[0]; a += (double)v[1]; a += (double)v[2]; a += (double)v[3];
    }
    for (; i < hi; ++i) a += (double)partials[i];
    lds[t] = a;
    __syncthreads();
    for (int off = 1; off < kOptimThreads; off <<= 1) {
        if ((t & (2 * off - 1)) == 0) lds[t] += lds[t + off];
        __syncthreads();
    }
    return lds[0];
}

// The state block from the fp64 sum of squares (one lane): norm, coefficient, found_inf, the counters, the bias corrections
__device__ __forceinline__ void optim_write_state(double sumsq, float beta1, float beta2, float max_norm, tp_optim_state* __restrict__ st) {
#pragma clang fp contract(off)
    const float norm = (float)sqrt(sumsq);
    const bool bad = !(fabsf(norm) <= 3.402823466e+38f);           // inf or NaN (an fp32 sum of squares that overflowed included)
    float coef = bad ? 0.f : 1.f;
    if (!bad && max_norm > 0.f && max_norm <= 3.402823466e+38f) {
        const float q = max_norm / (norm + 1e-6f);                  // clip_grad_norm_'s formula, in fp32
        coef = q < 1.f ? q : 1.f;
    }
    st->grad_norm = norm;
    st->clip_coef = coef;
    st->found_inf = bad ? 1 : 0;
    if (bad) {
        st->skipped += 1;
    } else {
        const int step = st->step + 1;
        st->step = step;
        st->bc1 = (float)(1.0 - pow((double)beta1, (double)step));
        st->sqrt_bc2 = (float)sqrt(1.0 - pow((double)beta2, (double)step));
    }
}

__global__ void __launch_bounds__(kOptimThreads)
optim_prepare_kernel(const float* __restrict__ partials, int nparts, float beta1, float beta2, float max_norm,
                     tp_optim_state* __restrict__ st) {
    __shared__ double lds[kOptimThreads];
    const double total = optim_sum_partials(partials, nparts, lds);
    if (threadIdx.x == 0) optim_write_state(total, beta1, beta2, max_norm, st);
}

// tp_optim_sumsq's second launch: this rank's partials -> one double (optim_prepare_kernel's sum, stored instead of used)
__global__ void __launch_bounds__(kOptimThreads)
optim_reduce_kernel(const float* __restrict__ partials, int nparts, double* __restrict__ sumsq_out) {
    __shared__ double lds[kOptimThreads];
    const double total = optim_sum_partials(partials, nparts, lds);
    if (threadIdx.x == 0) sumsq_out[0] = total;
}

// tp_optim_apply's first launch: the ranks' sums added in index order by one lane (nsums is a world size), then the state block.
// 0.0 + sums[0] is sums[0]: one rank gives optim_prepare_kernel's bits.
__global__ void __launch_bounds__(64)
optim_prepare_sums_kernel(const double* __restrict__ sums, int nsums, float beta1, float beta2, float max_norm,
                          tp_optim_state* __restrict__ st) {
    if (threadIdx.x != 0) return;
    double total = 0.0;
    for (int i = 0; i < nsums; ++i) total += sums[i];
    optim_write_state(total, beta1, beta2, max_norm, st);
}

struct AdamScalars { float s, coef, decay, step_size, beta1, omb1, beta2, omb2, sqrt_bc2, eps; };

// torch.optim.AdamW's update (no amsgrad, no maximize) of one element, every operation rounded once as written
// (tests/optim_ref.py derives its error bound from this sequence)
__device__ __forceinline__ void adamw_update(const AdamScalars& k, float g_raw, float& p, float& m, float& v) {
#pragma clang fp contract(off)
    const float g = (g_raw * k.s) * k.coef;
    p = p * k.decay;
    m = fmaf(k.beta1, m, k.omb1 * g);
    v = fmaf(k.beta2, v, (k.omb2 * g) * g);
    const float denom = sqrtf(v) / k.sqrt_bc2 + k.eps;
    p = p - (k.step_size * m) / denom;
}

template <typename T>
__global__ void __launch_bounds__(kOptimThreads)
optim_adamw_kernel(const OptimTable tab, const float* __restrict__ inv_scale, float grad_scale, const tp_optim_state* __restrict__ st,
                   float beta1, float beta2, float eps, unsigned flags) {
    constexpr bool kWriteBack = !std::is_same<T, float>::value;    // fp32 parameters are their own masters: nothing to write back
    using T4 = typename std::conditional<kWriteBack, Vec<T>, Vec<f16_t>>::type::x4;
    const int c = tab.chunk_base + (int)blockIdx.x;
    const OptimEntry e = tab.e[optim_entry_of(tab, c)];
    const long long base = (long long)(c - e.first_chunk) * kOptimChunk;
    const long long left = e.numel - base;
    const int n = left < kOptimChunk ? (int)left : kOptimChunk;
    const int t = threadIdx.x;
    const bool skip = st->found_inf != 0, zero = (flags & TP_OPTIM_ZERO_GRAD) != 0;
    if (skip && !zero) return;
    float* g = e.grad + base;
    float* pm = e.master + base;
    float* m = e.exp_avg + base;
    float* v = e.exp_avg_sq + base;
    T* pp = kWriteBack ? (T*)e.param + base : nullptr;
    const bool vec = (e.numel & 3) == 0 &&
                     (((uintptr_t)e.grad | (uintptr_t)e.master | (uintptr_t)e.exp_avg | (uintptr_t)e.exp_avg_sq | (uintptr_t)e.param) & 15) == 0;
    // (T = float: e.param is NULL — it adds nothing to the alignment test, and pp is never dereferenced)
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    if (skip) {                                        // a skipped step: master, exp_avg, exp_avg_sq and param keep their bits
        if (vec) {
#pragma unroll
            for (int j = 0; j < kOptimVecs; ++j) {
                const int i = j * kOptimThreads + t;
                if (i * 4 < n) *((f32x4*)g + i) = zero4;
            }
        } else {
#pragma unroll
            for (int j = 0; j < kOptimChain; ++j) {
                const int i = j * kOptimThreads + t;
                if (i < n) g[i] = 0.f;
            }
        }
        return;
    }
    AdamScalars k;
    {
#pragma clang fp contract(off)
        k.s = optim_scale(inv_scale, grad_scale);
        k.coef = st->clip_coef;
        k.decay = 1.0f - e.lr * e.weight_decay;
        k.step_size = e.lr / st->bc1;
        k.beta1 = beta1; k.omb1 = 1.0f - beta1;
        k.beta2 = beta2; k.omb2 = 1.0f - beta2;
        k.sqrt_bc2 = st->sqrt_bc2;
        k.eps = eps;
    }
    if (vec) {
        f32x4 gv[kOptimVecs], pv[kOptimVecs], mv[kOptimVecs], vv[kOptimVecs];
#pragma unroll
        for (int j = 0; j < kOptimVecs; ++j) {
            const int i = j * kOptimThreads + t;
            const bool in = i * 4 < n;
            gv[j] = in ? *((const f32x4*)g + i) : zero4;
            pv[j] = in ? *((const f32x4*)pm + i) : zero4;
            mv[j] = in ? *((const f32x4*)m + i) : zero4;
            vv[j] = in ? *((const f32x4*)v + i) : zero4;
        }
#pragma unroll
        for (int j = 0; j < kOptimVecs; ++j) {
            const int i = j * kOptimThreads + t;
            if (i * 4 >= n) continue;
            T4 out;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                float p_ = pv[j][q], m_ = mv[j][q], v_ = vv[j][q];
                adamw_update(k, gv[j][q], p_, m_, v_);
                pv[j][q] = p_; mv[j][q] = m_; vv[j][q] = v_;
                if constexpr (kWriteBack) out[q] = (T)p_;   // round to nearest even, no clamp (Tensor.to)
            }
            *((f32x4*)m + i) = mv[j];
            *((f32x4*)v + i) = vv[j];
            *((f32x4*)pm + i) = pv[j];
            if constexpr (kWriteBack) *((T4*)pp + i) = out;
            if (zero) *((f32x4*)g + i) = zero4;
        }
    } else {
        float gv[kOptimChain], pv[kOptimChain], mv[kOptimChain], vv[kOptimChain];
#pragma unroll
        for (int j = 0; j < kOptimChain; ++j) {
            const int i = j * kOptimThreads + t;
            const bool in = i < n;
            gv[j] = in ? g[i] : 0.f;
            pv[j] = in ? pm[i] : 0.f;
            mv[j] = in ? m[i] : 0.f;
            vv[j] = in ? v[i] : 0.f;
        }
#pragma unroll
        for (int j = 0; j < kOptimChain; ++j) {
            const int i = j * kOptimThreads + t;
            if (i >= n) continue;
            adamw_update(k, gv[j], pv[j], mv[j], vv[j]);
            m[i] = mv[j];
            v[i] = vv[j];
            pm[i] = pv[j];
            if constexpr (kWriteBack) pp[i] = (T)pv[j];
            if (zero) g[i] = 0.f;
        }
    }
}

// ---- host side --------------------------------------------------------------------------------------------------------------
long long chunks_of(long long numel) { return (numel + kOptimChunk - 1) / kOptimChunk; }
size_t partials_bytes(long long chunks) { return ((size_t)chunks * sizeof(float) + 255) & ~(size_t)255; }

// n, the table pointer, every numel, the chunk count: what both entry points need.  -> total chunks, or -1 with the error set
long long validate_sizes(const char* what, const tp_optim_tensor* t, int n) {
    if (n < 0) { set_error("%s: n = %d is negative", what, n); return -1; }
    if (n > 0 && !t) { set_error("%s: NULL table with n = %d", what, n); return -1; }
    long long chunks = 0;
    for (int i = 0; i < n; ++i) {
        if (t[i].numel <= 0) { set_error("%s: entry #%d: numel = %lld must be positive", what, i, (long long)t[i].numel); return -1; }
        chunks += chunks_of(t[i].numel);
        if (chunks > 0x7fffffffll) { set_error("%s: entry #%d: more than 2^31 chunks of %d elements in one call", what, i, kOptimChunk); return -1; }
    }
    return chunks;
}

bool finite_nonneg(float x) { return x >= 0.f && x <= 3.402823466e+38f; }

bool check_hyper(const char* what, const tp_optim_hyper* h) {
    if (!h) { set_error("%s: NULL hyper-parameters", what); return false; }
    if (!(h->beta1 >= 0.f && h->beta1 < 1.f)) { set_error("%s: beta1 = %g outside [0, 1)", what, (double)h->beta1); return false; }
    if (!(h->beta2 >= 0.f && h->beta2 < 1.f)) { set_error("%s: beta2 = %g outside [0, 1)", what, (double)h->beta2); return false; }
    if (!finite_nonneg(h->eps)) { set_error("%s: eps = %g must be finite and >= 0", what, (double)h->eps); return false; }
    if (h->max_grad_norm != h->max_grad_norm) { set_error("%s: max_grad_norm is NaN (<= 0 or +inf: no clipping)", what); return false; }
    if (h->dtype != TP_BF16 && h->dtype != TP_F16 && h->dtype != TP_F32) {
        set_error("%s: dtype %d unsupported (the parameters are bf16 / fp16, or fp32 and their own masters)", what, h->dtype);
        return false;
    }
    if (h->flags & ~(uint32_t)TP_OPTIM_ZERO_GRAD) { set_error("%s: unknown flags 0x%x", what, h->flags); return false; }
    return true;
}

// Every pointer of the table: NULL, alignment, the same address twice; lr / weight_decay.  `grad_only` (tp_optim_sumsq): only
// `grad` is looked at, as only `grad` is read.
bool check_table(const char* what, const tp_optim_tensor* t, int n, bool own_master, bool grad_only) {
    std::vector<std::pair<uintptr_t, int>> seen;
    seen.reserve((size_t)n * 5);
    for (int i = 0; i < n; ++i) {
        const void* ptr[5] = {t[i].param, t[i].master, t[i].grad, t[i].exp_avg, t[i].exp_avg_sq};
        static const char* const name[5] = {"param", "master", "grad", "exp_avg", "exp_avg_sq"};
        if (!grad_only && own_master && ptr[0]) {
            set_error("%s: entry #%d: param must be NULL with dtype TP_F32 (master is the parameter)", what, i);
            return false;
        }
        for (int k = grad_only ? 2 : own_master ? 1 : 0; k < (grad_only ? 3 : 5); ++k) {
            if (!ptr[k]) { set_error("%s: entry #%d: %s is NULL", what, i, name[k]); return false; }
            if ((uintptr_t)ptr[k] & (k == 0 ? 1 : 3)) {
                set_error("%s: entry #%d: %s is not aligned to its %d-byte elements", what, i, name[k], k == 0 ? 2 : 4);
                return false;
            }
            seen.emplace_back((uintptr_t)ptr[k], i);
        }
        if (grad_only) continue;
        if (!finite_nonneg(t[i].lr)) { set_error("%s: entry #%d: lr = %g must be finite and >= 0", what, i, (double)t[i].lr); return false; }
        if (!finite_nonneg(t[i].weight_decay)) {
            set_error("%s: entry #%d: weight_decay = %g must be finite and >= 0", what, i, (double)t[i].weight_decay);
            return false;
        }
    }
    std::sort(seen.begin(), seen.end());
    for (size_t k = 1; k < seen.size(); ++k)
        if (seen[k].first == seen[k - 1].first) {
            set_error("%s: entry #%d: address %p appears twice in the table (entry #%d has it too)", what, seen[k].second,
                      (void*)seen[k].first, seen[k - 1].second);
            return false;
        }
    return true;
}

bool check_scales(const char* what, const float* inv_scale, float grad_scale) {
    if (inv_scale && ((uintptr_t)inv_scale & 3)) { set_error("%s: inv_scale is not 4-byte aligned", what); return false; }
    if (!(grad_scale > 0.f && grad_scale <= 3.402823466e+38f)) {
        set_error("%s: grad_scale = %g must be finite and > 0 (1 / world size, or 1)", what, (double)grad_scale);
        return false;
    }
    return true;
}

bool check_workspace(const char* what, const void* workspace, size_t workspace_bytes, size_t need) {
    if (need && (!workspace || ((uintptr_t)workspace & 15) || workspace_bytes < need)) {
        set_error("%s: workspace %zu B < %zu B (or NULL / not 16-byte aligned)", what, workspace ? workspace_bytes : (size_t)0, need);
        return false;
    }
    return true;
}

// One pass over the table, kOptimTable entries per launch.  pass 0: the sums of squares -> partials; pass 1: the update.
int launch_pass(int pass, const tp_optim_tensor* t, int n, const tp_optim_hyper* h, const float* inv_scale, float grad_scale,
                const tp_optim_state* st, float* partials, hipStream_t stream) {
    int first_chunk = 0;
    for (int i0 = 0; i0 < n; i0 += kOptimTable) {
        OptimTable tab;
        tab.count = n - i0 < kOptimTable ? n - i0 : kOptimTable;
        tab.chunk_base = first_chunk;
        for (int k = 0; k < tab.count; ++k) {
            const tp_optim_tensor& s = t[i0 + k];
            tab.e[k] = OptimEntry{s.param, s.master, s.grad, s.exp_avg, s.exp_avg_sq, (long long)s.numel, s.lr, s.weight_decay, first_chunk, 0};
            first_chunk += (int)chunks_of(s.numel);
        }
        for (int k = tab.count; k < kOptimTable; ++k) tab.e[k] = OptimEntry{};
        const dim3 grid((unsigned)(first_chunk - tab.chunk_base)), block(kOptimThreads);
        if (pass == 0) {
            hipLaunchKernelGGL(optim_sumsq_kernel, grid, block, 0, stream, tab, inv_scale, grad_scale, partials);
            if (int rc = check_launch("optim_sumsq_kernel")) return rc;
        } else if (h->dtype == TP_BF16) {
            hipLaunchKernelGGL(optim_adamw_kernel<bf16_t>, grid, block, 0, stream, tab, inv_scale, grad_scale, st, h->beta1, h->beta2,
                               h->eps, (unsigned)h->flags);
            if (int rc = check_launch("optim_adamw_kernel")) return rc;
        } else if (h->dtype == TP_F32) {
            hipLaunchKernelGGL(optim_adamw_kernel<float>, grid, block, 0, stream, tab, inv_scale, grad_scale, st, h->beta1, h->beta2,
                               h->eps, (unsigned)h->flags);
            if (int rc = check_launch("optim_adamw_kernel")) return rc;
        } else {
            hipLaunchKernelGGL(optim_adamw_kernel<f16_t>, grid, block, 0, stream, tab, inv_scale, grad_scale, st, h->beta1, h->beta2,
                               h->eps, (unsigned)h->flags);
            if (int rc = check_launch("optim_adamw_kernel")) return rc;
        }
    }
    return TP_OK;
}

}  // namespace

extern "C" {

size_t tp_optim_workspace_bytes(const tp_optim_tensor* t, int n) {
    const long long chunks = validate_sizes("tp_optim_workspace_bytes", t, n);
    if (chunks < 0) return 0;
    return partials_bytes(chunks) + TP_OPTIM_STATE_BYTES;
}

int tp_optim_step(const tp_optim_tensor* t, int n, const tp_optim_hyper* h, const float* inv_scale, void* state, void* workspace,
                  size_t workspace_bytes, void* stream_) {
    const char* what = "tp_optim_step";
    const long long chunks = validate_sizes(what, t, n);
    if (chunks < 0) return TP_ERR_INVALID_ARG;
    if (n == 0) return TP_OK;
    if (!check_hyper(what, h) || !check_table(what, t, n, h->dtype == TP_F32, false)) return TP_ERR_INVALID_ARG;
    if (!state || ((uintptr_t)state & 15)) { set_error("%s: state must be a 16-byte aligned block of %d bytes", what, TP_OPTIM_STATE_BYTES); return TP_ERR_INVALID_ARG; }
    if (!check_scales(what, inv_scale, 1.0f)) return TP_ERR_INVALID_ARG;
    if (!check_workspace(what, workspace, workspace_bytes, partials_bytes(chunks) + TP_OPTIM_STATE_BYTES)) return TP_ERR_INVALID_ARG;

    hipStream_t stream = (hipStream_t)stream_;
    float* partials = (float*)workspace;
    tp_optim_state* st = (tp_optim_state*)state;
    // the sums of squares; then the state block; then the update
    if (int rc = launch_pass(0, t, n, h, inv_scale, 1.0f, st, partials, stream)) return rc;
    hipLaunchKernelGGL(optim_prepare_kernel, dim3(1), dim3(kOptimThreads), 0, stream, (const float*)partials, (int)chunks, h->beta1,
                       h->beta2, h->max_grad_norm, st);
    if (int rc = check_launch("optim_prepare_kernel")) return rc;
    return launch_pass(1, t, n, h, inv_scale, 1.0f, st, partials, stream);
}

int tp_optim_sumsq(const tp_optim_tensor* t, int n, const float* inv_scale, float grad_scale, double* sumsq_out, void* workspace,
                   size_t workspace_bytes, void* stream_) {
    const char* what = "tp_optim_sumsq";
    const long long chunks = validate_sizes(what, t, n);
    if (chunks < 0) return TP_ERR_INVALID_ARG;
    if (!check_table(what, t, n, false, true) || !check_scales(what, inv_scale, grad_scale)) return TP_ERR_INVALID_ARG;
    if (!sumsq_out || ((uintptr_t)sumsq_out & 7)) { set_error("%s: sumsq_out must be an 8-byte aligned device double", what); return TP_ERR_INVALID_ARG; }
    if (!check_workspace(what, workspace, workspace_bytes, chunks ? partials_bytes(chunks) : 0)) return TP_ERR_INVALID_ARG;

    hipStream_t stream = (hipStream_t)stream_;
    float* partials = (float*)workspace;                          // (n == 0: may be NULL; the reduction of no partials reads nothing)
    if (int rc = launch_pass(0, t, n, nullptr, inv_scale, grad_scale, nullptr, partials, stream)) return rc;
    hipLaunchKernelGGL(optim_reduce_kernel, dim3(1), dim3(kOptimThreads), 0, stream, (const float*)partials, (int)chunks, sumsq_out);
    return check_launch("optim_reduce_kernel");
}

int tp_optim_apply(const tp_optim_tensor* t, int n, const tp_optim_hyper* h, const float* inv_scale, float grad_scale,
                   const double* sums, int nsums, void* state, void* stream_) {
    const char* what = "tp_optim_apply";
    const long long chunks = validate_sizes(what, t, n);
    if (chunks < 0) return TP_ERR_INVALID_ARG;
    if (!check_hyper(what, h) || !check_table(what, t, n, h->dtype == TP_F32, false)) return TP_ERR_INVALID_ARG;
    if (!state || ((uintptr_t)state & 15)) { set_error("%s: state must be a 16-byte aligned block of %d bytes", what, TP_OPTIM_STATE_BYTES); return TP_ERR_INVALID_ARG; }
    if (!check_scales(what, inv_scale, grad_scale)) return TP_ERR_INVALID_ARG;
    if (nsums < 1) { set_error("%s: nsums = %d: at least one sum of squares (one per rank)", what, nsums); return TP_ERR_INVALID_ARG; }
    if (!sums || ((uintptr_t)sums & 7)) { set_error("%s: sums must be %d 8-byte aligned device doubles", what, nsums); return TP_ERR_INVALID_ARG; }

    hipStream_t stream = (hipStream_t)stream_;
    tp_optim_state* st = (tp_optim_state*)state;
    hipLaunchKernelGGL(optim_prepare_sums_kernel, dim3(1), dim3(64), 0, stream, sums, nsums, h->beta1, h->beta2, h->max_grad_norm, st);
    if (int rc = check_launch("optim_prepare_sums_kernel")) return rc;
    return launch_pass(1, t, n, h, inv_scale, grad_scale, st, nullptr, stream);       // (n == 0: the counters advanced, nothing to update)
}

}  // extern "C"
