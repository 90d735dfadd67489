// tp_test_hooks.hip — the test hooks of include/tokenpacker_test.h.  Linked into libtokenpacker_exp.so only (Makefile target `exp`);
// the product library does not export them.  Stateless: each reads nothing but its arguments and the device.
#include "tp_internal.h"
#include "../../include/tokenpacker_test.h"
#include <string.h>

using namespace tp;
#define TP_TRY(expr) do { int rc_ = (expr); if (rc_ != TP_OK) return rc_; } while (0)
// Host-side refusal of a mistaken test call: the launchers below trust their callers (tp_train.hip), the hooks do not.
#define TP_REQUIRE(cond, ...) do { if (!(cond)) { set_error(__VA_ARGS__); return TP_ERR_INVALID_ARG; } } while (0)

static bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
static bool half_dtype(int dt) { return dt == TP_BF16 || dt == TP_F16; }
static bool any_dtype(int dt) { return dt == TP_BF16 || dt == TP_F16 || dt == TP_F32; }

extern "C" {

int tp_test_occupy_cus(int workgroups, int microseconds, void* scratch_int, void* stream) {
    if (workgroups <= 0 || microseconds <= 0 || !scratch_int) { set_error("tp_test_occupy_cus: bad argument"); return TP_ERR_INVALID_ARG; }
    return occupy_cus_launch(workgroups, microseconds, (int*)scratch_int, (hipStream_t)stream);
}


int tp_test_pair_occupancy(void) { return gemm_pair_occupancy(); }
int tp_test_gemm_route(int M, int N, int K, int flags, int groups) {
    if (M <= 0 || N <= 0 || K <= 0 || N % 128 != 0 || K % 64 != 0) { set_error("tp_test_gemm_route: bad shape"); return -1; }
    GemmArgs a = plain_gemm(nullptr, K, nullptr, nullptr, N, M, N, K, nullptr, flags);
    a.groups = groups > 0 ? groups : 1;
    return gemm_route_of(TP_F16, TP_F16, a);
}

size_t tp_test_pack_qr_scratch_bytes(void) { return pack_qr_scratch_bytes(1); }

int tp_test_pack_qr(const void* w2_f16, const float* b2, void* r_f16, float* c_tilde, float* wbar, void* scratch, void* stream) {
    if (!w2_f16 || !r_f16 || !c_tilde || !wbar || !scratch) { set_error("tp_test_pack_qr: NULL argument"); return TP_ERR_INVALID_ARG; }
    hipStream_t st = (hipStream_t)stream;
    TP_TRY(pack_qr_center_launch(w2_f16, b2, scratch, 0, wbar, st));
    TP_TRY(pack_qr_factor_launch(scratch, 1, st));
    return pack_qr_extract_launch(scratch, 0, r_f16, c_tilde, st, nullptr);
}

// Where tp_pack_weights puts a tensor of the image (host logic only): `name` is a PackedLayout field (tp_internal.h), "total" included.
int tp_test_packed_layout(int hidden_size, const char* name, size_t* offset, size_t* bytes) {
    TP_REQUIRE(name && offset && bytes, "tp_test_packed_layout: NULL argument");
    TP_REQUIRE(hidden_size > 0 && hidden_size % 128 == 0, "tp_test_packed_layout: hidden_size %d is not a positive multiple of 128", hidden_size);
    struct Field { const char* name; size_t PackedLayout::* member; };
#define TP_FIELD(f) {#f, &PackedLayout::f}
    static const Field fields[] = {                                   // in declaration order
        TP_FIELD(w_kv0), TP_FIELD(b_kv0), TP_FIELD(w_kv2), TP_FIELD(b_kv2), TP_FIELD(w_q1),
        TP_FIELD(w_in_kv), TP_FIELD(c_in_kv), TP_FIELD(b_in_kv), TP_FIELD(w_in_q), TP_FIELD(c_in_q), TP_FIELD(b_in_q),
        TP_FIELD(w_qt), TP_FIELD(w_qt_c), TP_FIELD(w_c_kv), TP_FIELD(d_in_kv), TP_FIELD(w_c_q),
        TP_FIELD(w_cc_kv), TP_FIELD(d_cc_kv), TP_FIELD(w_cc_q), TP_FIELD(w_qt_cc), TP_FIELD(w_cc_v3),
        TP_FIELD(w_r_kv), TP_FIELD(c_r_kv), TP_FIELD(w_r_q), TP_FIELD(wbar), TP_FIELD(scratch_qr),
        TP_FIELD(w_out), TP_FIELD(b_out), TP_FIELD(w_m0), TP_FIELD(b_m0), TP_FIELD(w_m2), TP_FIELD(b_m2), TP_FIELD(w_om), TP_FIELD(b_om),
        TP_FIELD(scratch_t), TP_FIELD(scratch_p), TP_FIELD(status), TP_FIELD(total)};
#undef TP_FIELD
    static_assert(sizeof(fields) / sizeof(fields[0]) * sizeof(size_t) == sizeof(PackedLayout), "a PackedLayout field is missing from the table");
    PackedLayout reserved{};
    const PackedLayout L = packed_layout(hidden_size, &reserved);
    for (const Field& f : fields)
        if (strcmp(name, f.name) == 0) { *offset = L.*(f.member); *bytes = reserved.*(f.member); return TP_OK; }
    set_error("tp_test_packed_layout: no PackedLayout field named '%s'", name);
    return TP_ERR_INVALID_ARG;
}

// ---- the forward's two attention kernels (tp_internal.h: region_attention_launch, region_attention_absorbed_launch) --------------

static int attention_geometry(const char* who, int B, int grid, int s, const float* mask, int mask_mode) {
    if (!(B > 0 && grid > 0 && s > 0 && grid % s == 0 && grid <= 1024)) { set_error("%s: need B > 0 and s dividing grid <= 1024", who); return TP_ERR_INVALID_ARG; }
    if (!(mask_mode >= 0 && mask_mode <= 2)) { set_error("%s: mask_mode 0 / 1 / 2", who); return TP_ERR_INVALID_ARG; }
    if ((mask_mode == 0) != (mask == nullptr)) { set_error("%s: mask_mode 0 takes no mask, mask_mode 1 / 2 needs one", who); return TP_ERR_INVALID_ARG; }
    if ((uintptr_t)mask & 3) { set_error("%s: the mask must be 4-byte aligned", who); return TP_ERR_INVALID_ARG; }
    return TP_OK;
}

int tp_test_region_attention(const void* q, const void* k, const void* v, void* o, int B, int grid, int s, const float* mask,
                             int mask_mode, int region_major, void* stream) {
    TP_REQUIRE(q && k && v && o, "tp_test_region_attention: NULL argument");
    TP_REQUIRE(al16(q) && al16(k) && al16(v) && al16(o), "tp_test_region_attention: q / k / v / o must be 16-byte aligned");
    TP_TRY(attention_geometry("tp_test_region_attention", B, grid, s, mask, mask_mode));
    TP_REQUIRE(region_major == 0 || region_major == 1, "tp_test_region_attention: region_major 0 / 1");
    return region_attention_launch(q, k, v, o, B, grid, s, (hipStream_t)stream, mask, mask_mode, region_major);
}

int tp_test_region_attention_absorbed(const void* qt, const void* h2k, const void* h2v, const float* mr_k, const float* mr_v, void* u,
                                      int B, int grid, int s, const float* mask, int mask_mode, void* stream) {
    TP_REQUIRE(qt && h2k && h2v && mr_k && mr_v && u, "tp_test_region_attention_absorbed: NULL argument");
    TP_REQUIRE(al16(qt) && al16(h2k) && al16(h2v) && al16(u), "tp_test_region_attention_absorbed: qt / h2k / h2v / u must be 16-byte aligned");
    TP_REQUIRE(((uintptr_t)mr_k & 7) == 0 && ((uintptr_t)mr_v & 7) == 0, "tp_test_region_attention_absorbed: mr_k / mr_v must be 8-byte aligned");
    TP_TRY(attention_geometry("tp_test_region_attention_absorbed", B, grid, s, mask, mask_mode));
    return region_attention_absorbed_launch(qt, h2k, h2v, mr_k, mr_v, u, B, grid, s, (hipStream_t)stream, mask, mask_mode);   // (refuses s*s > 64)
}

// ---- the backward's kernels, one launcher each (tp_internal.h: bw_*_launch, point_queries_bwd_launch, gemm_launch) -------------

int tp_test_bw_transpose(int src_dtype, int dst_dtype, const void* src, int64_t ld, int rows_per_batch, int64_t batch_stride,
                         int R, int C, void* dst, int64_t ldd, int Rpad, const float* mean_rstd, const float* gamma,
                         const float* beta, float* colsum_part, size_t colsum_floats, void* stream) {
    TP_REQUIRE(src && dst, "tp_test_bw_transpose: NULL argument");
    TP_REQUIRE(half_dtype(src_dtype) && half_dtype(dst_dtype), "tp_test_bw_transpose: dtypes must be TP_BF16 / TP_F16");
    TP_REQUIRE(al16(src) && al16(dst), "tp_test_bw_transpose: src / dst must be 16-byte aligned");
    TP_REQUIRE(R > 0 && C > 0 && Rpad >= R && (C & 7) == 0 && (Rpad & 7) == 0, "tp_test_bw_transpose: need 0 < R <= Rpad, C and Rpad multiples of 8");
    TP_REQUIRE(ld >= C && (ld & 7) == 0 && ldd >= Rpad && (ldd & 7) == 0, "tp_test_bw_transpose: ld >= C, ldd >= Rpad, both multiples of 8");
    if (rows_per_batch > 0 && rows_per_batch < R)
        TP_REQUIRE((batch_stride & 7) == 0 && batch_stride >= (int64_t)rows_per_batch * ld,
                   "tp_test_bw_transpose: batch stride must be a multiple of 8 and cover rows_per_batch rows");
    TP_REQUIRE(!mean_rstd || (gamma && beta), "tp_test_bw_transpose: the LayerNorm needs gamma and beta");
    TP_REQUIRE(!colsum_part || colsum_floats >= (size_t)((Rpad + 63) / 64) * (size_t)C,
               "tp_test_bw_transpose: colsum_part needs ceil(Rpad / 64) * C floats");
    return bw_transpose_launch(src_dtype, dst_dtype, src, ld, rows_per_batch, batch_stride, R, C, dst, ldd, Rpad, mean_rstd, gamma,
                               beta, colsum_part, (hipStream_t)stream);
}

int tp_test_bw_transpose_batch(int src_dtype, int dst_dtype, int count, const void* const* src, const int64_t* ld, const int* R,
                               const int* C, void* const* dst, const int* Rpad, void* stream) {
    TP_REQUIRE(src && ld && R && C && dst && Rpad, "tp_test_bw_transpose_batch: NULL argument");
    TP_REQUIRE(count >= 1 && count <= kTransposeBatch, "tp_test_bw_transpose_batch: 1 .. %d matrices", kTransposeBatch);
    TP_REQUIRE(half_dtype(src_dtype) && half_dtype(dst_dtype), "tp_test_bw_transpose_batch: dtypes must be TP_BF16 / TP_F16");
    TransposeBatch tb{};
    for (int i = 0; i < count; ++i) {
        TP_REQUIRE(src[i] && dst[i] && R[i] > 0 && C[i] > 0 && Rpad[i] >= R[i] && ld[i] >= C[i],
                   "tp_test_bw_transpose_batch: matrix %d: NULL pointer or bad shape", i);
        tb.add(src[i], ld[i], R[i], C[i], dst[i], Rpad[i]);
    }
    return bw_transpose_batch_launch(src_dtype, dst_dtype, tb, (hipStream_t)stream);      // (checks the 8-element / 16-byte alignment)
}

int tp_test_bw_colsum_rows(int dtype, const void* src, int64_t ld, int64_t R, int C, float* part, size_t part_floats,
                           float* amax_part, size_t amax_floats, int* amax_count, void* stream) {
    TP_REQUIRE(src && part, "tp_test_bw_colsum_rows: NULL argument");
    TP_REQUIRE(half_dtype(dtype), "tp_test_bw_colsum_rows: dtype must be TP_BF16 / TP_F16");
    TP_REQUIRE(al16(src) && al16(part), "tp_test_bw_colsum_rows: src / part must be 16-byte aligned");
    TP_REQUIRE(R > 0 && C > 0 && (C & 7) == 0 && ld >= C && (ld & 7) == 0, "tp_test_bw_colsum_rows: need R > 0, C %% 8 == 0, ld >= C, ld %% 8 == 0");
    // (an upper bound of the launcher's slice count that does not repeat its formula)
    const int64_t max_slices = std::min<int64_t>(kColsumMaxSlices, std::max<int64_t>(1, R / 64));
    TP_REQUIRE(part_floats >= (size_t)max_slices * (size_t)C, "tp_test_bw_colsum_rows: part needs min(%d, max(1, R / 64)) * C floats", kColsumMaxSlices);
    TP_REQUIRE(!amax_part || (amax_count && amax_floats >= (size_t)kColsumAmaxParts),
               "tp_test_bw_colsum_rows: amax_part needs amax_count and %d floats", kColsumAmaxParts);
    return bw_colsum_rows_launch(dtype, src, ld, R, C, part, (hipStream_t)stream, amax_part, amax_part ? amax_count : nullptr);
}

int tp_test_bw_reduce_parts(int dst_dtype, const float* part, int64_t part_stride, int nparts, int64_t n, void* out,
                            const float* out_scale, void* stream) {
    TP_REQUIRE(part && out, "tp_test_bw_reduce_parts: NULL argument");
    TP_REQUIRE(any_dtype(dst_dtype), "tp_test_bw_reduce_parts: bad output dtype");
    TP_REQUIRE(al16(part) && al16(out), "tp_test_bw_reduce_parts: part / out must be 16-byte aligned");
    TP_REQUIRE(nparts > 0 && n > 0 && (nparts == 1 || part_stride >= n), "tp_test_bw_reduce_parts: need nparts > 0, n > 0, part_stride >= n");
    return bw_reduce_parts_launch(dst_dtype, part, part_stride, nparts, n, out, (hipStream_t)stream, out_scale);
}

int tp_test_bw_reduce_many_parts(int dst_dtype, const float* part, int64_t part_stride, int nparts, int n, void* out, float* scratch,
                                 size_t scratch_floats, const float* out_scale, int n_out, void* stream) {
    TP_REQUIRE(part && out && scratch, "tp_test_bw_reduce_many_parts: NULL argument");
    TP_REQUIRE(any_dtype(dst_dtype), "tp_test_bw_reduce_many_parts: bad output dtype");
    TP_REQUIRE(al16(part) && al16(out) && al16(scratch), "tp_test_bw_reduce_many_parts: part / out / scratch must be 16-byte aligned");
    TP_REQUIRE(nparts > 0 && n > 0 && (n & 3) == 0 && (part_stride & 3) == 0 && part_stride >= n && n_out >= -1 && n_out <= n,
               "tp_test_bw_reduce_many_parts: need nparts > 0, n and part_stride multiples of 4, part_stride >= n, -1 <= n_out <= n");
    TP_REQUIRE(scratch_floats >= (size_t)kReduceSlices * (size_t)n, "tp_test_bw_reduce_many_parts: scratch needs %d * n floats", kReduceSlices);
    return bw_reduce_many_parts_launch(dst_dtype, part, part_stride, nparts, n, out, scratch, (hipStream_t)stream, out_scale, n_out);
}

int tp_test_bw_dynamic_scale(const float* amax_part, int nparts, float* scale, void* stream) {
    TP_REQUIRE(amax_part && scale && nparts > 0, "tp_test_bw_dynamic_scale: NULL argument or nparts <= 0");
    return bw_scale_from_partials_launch(amax_part, nparts, scale, (hipStream_t)stream);
}

int tp_test_bw_scale_cast(int src_dtype, const void* src, int64_t n, const float* scale, void* dst_f16, int* sat_flag, void* stream) {
    TP_REQUIRE(src && scale && dst_f16, "tp_test_bw_scale_cast: NULL argument");
    TP_REQUIRE(half_dtype(src_dtype), "tp_test_bw_scale_cast: dtype must be TP_BF16 / TP_F16");
    TP_REQUIRE(n > 0, "tp_test_bw_scale_cast: n must be positive");
    return bw_scale_cast_launch(src_dtype, src, n, scale, dst_f16, (hipStream_t)stream, sat_flag);   // (checks n %% 8 and the alignment)
}

int tp_test_bw_ln_backward(int gdtype, const void* dy, const void* x_f16, const float* mean_rstd, const float* gamma, void* dx,
                           float* part, size_t part_floats, int nblocks, int64_t rows, const float* beta, void* xn, int* sat_flag,
                           void* stream) {
    TP_REQUIRE(dy && x_f16 && mean_rstd && gamma && dx && part, "tp_test_bw_ln_backward: NULL argument");
    TP_REQUIRE(half_dtype(gdtype), "tp_test_bw_ln_backward: gradient dtype must be TP_BF16 / TP_F16");
    TP_REQUIRE(al16(dy) && al16(x_f16) && al16(dx) && al16(xn) && al16(part), "tp_test_bw_ln_backward: dy / x / dx / xn / part must be 16-byte aligned");
    TP_REQUIRE(rows > 0 && nblocks > 0 && nblocks <= 65535, "tp_test_bw_ln_backward: need rows > 0 and 1 <= nblocks <= 65535");
    TP_REQUIRE(part_floats >= (size_t)nblocks * 3 * kEmbed, "tp_test_bw_ln_backward: part needs nblocks * 3 * %d floats", kEmbed);
    return bw_ln_backward_launch(gdtype, dy, x_f16, mean_rstd, gamma, dx, part, nblocks, rows, (hipStream_t)stream, beta, xn, sat_flag);
}

int tp_test_bw_region_attention(int gdtype, const void* q, const void* k, const void* v, const void* dout, void* dq, void* dk,
                                void* dv, int B, int grid, int s, const float* mask, int mask_mode, float* dmask,
                                const float* inv_scale, float* part, size_t part_bytes, float* redscratch, size_t redscratch_floats,
                                int* sat_flag, void* stream) {
    TP_REQUIRE(q && k && v && dout && dq && dk && dv, "tp_test_bw_region_attention: NULL argument");
    TP_REQUIRE(half_dtype(gdtype), "tp_test_bw_region_attention: gradient dtype must be TP_BF16 / TP_F16");
    TP_REQUIRE(al16(q) && al16(k) && al16(v) && al16(dout) && al16(dq) && al16(dk) && al16(dv),
               "tp_test_bw_region_attention: the seven tensors must be 16-byte aligned");
    TP_REQUIRE(B > 0 && grid > 0 && s > 0 && grid % s == 0 && grid <= 1024, "tp_test_bw_region_attention: need B > 0 and s dividing grid");
    TP_REQUIRE(mask_mode >= 0 && mask_mode <= 2, "tp_test_bw_region_attention: mask_mode 0 / 1 / 2");
    if (mask_mode == 0) {
        TP_REQUIRE(!mask && !dmask, "tp_test_bw_region_attention: mask_mode 0 takes no mask and no dmask");
        return bw_region_attention_launch(gdtype, q, k, v, dout, dq, dk, dv, B, grid, s, (hipStream_t)stream, sat_flag);
    }
    TP_REQUIRE(mask, "tp_test_bw_region_attention: mask_mode %d needs a mask", mask_mode);
    if (dmask && mask_mode == 1) {
        const int G = grid / s, S2p = (s * s + 3) & ~3;
        TP_REQUIRE(part && redscratch && al16(part) && al16(redscratch) && al16(dmask),
                   "tp_test_bw_region_attention: a mode-1 dmask needs 16-byte aligned part and redscratch");
        TP_REQUIRE(part_bytes >= (size_t)B * G * G * S2p * 4 && redscratch_floats >= (size_t)kReduceSlices * S2p,
                   "tp_test_bw_region_attention: part needs B*M*ceil4(s*s) floats, redscratch %d*ceil4(s*s)", kReduceSlices);
    }
    return bw_region_attention_masked_launch(gdtype, q, k, v, dout, dq, dk, dv, B, grid, s, (hipStream_t)stream, sat_flag, mask,
                                             mask_mode, dmask, inv_scale, part, part_bytes, redscratch);
}

int tp_test_point_queries_bwd(int dtype, const float* dq0, const float* inv_scale, void* dx, int B, int grid, int s, void* stream) {
    TP_REQUIRE(dq0 && dx, "tp_test_point_queries_bwd: NULL argument");
    TP_REQUIRE(half_dtype(dtype), "tp_test_point_queries_bwd: dtype must be TP_BF16 / TP_F16");
    TP_REQUIRE(al16(dq0) && al16(dx), "tp_test_point_queries_bwd: dq0 / dx must be 16-byte aligned");
    TP_REQUIRE(B > 0 && grid > 0 && s > 0 && grid % s == 0, "tp_test_point_queries_bwd: need B > 0 and s dividing grid");
    return point_queries_bwd_launch(dtype, dq0, inv_scale, dx, B, grid, s, (hipStream_t)stream);
}

int tp_test_linear_bwd(int M, int N, int K, int dtype, int out_dtype, int flags, const void* A, int64_t lda, const void* W, void* C,
                       int64_t ldc, const void* Z, int64_t ldz, const float* out_scale, int tile, void* stream) {
    TP_REQUIRE(A && W && C, "tp_test_linear_bwd: NULL argument");
    TP_REQUIRE(half_dtype(dtype) && any_dtype(out_dtype), "tp_test_linear_bwd: bad dtype");
    TP_REQUIRE((flags & ~TP_LINEAR_GELU_BWD) == 0, "tp_test_linear_bwd: flags 0 or TP_LINEAR_GELU_BWD");
    TP_REQUIRE(al16(A) && al16(W) && al16(C) && al16(Z), "tp_test_linear_bwd: A / W / C / Z must be 16-byte aligned");
    TP_REQUIRE(M > 0 && N > 0 && K > 0 && lda >= K && (lda & 7) == 0 && ldc >= N && (ldc & 7) == 0,
               "tp_test_linear_bwd: need lda >= K, ldc >= N, both multiples of 8 elements");
    TP_REQUIRE(tile == 0 || tile == 128 || tile == 256, "tp_test_linear_bwd: tile 0 / 128 / 256");
    if (flags & TP_LINEAR_GELU_BWD) TP_REQUIRE(Z && ldz >= N && (ldz & 7) == 0, "tp_test_linear_bwd: TP_LINEAR_GELU_BWD needs Z with ldz >= N, ldz %% 8 == 0");
    else TP_REQUIRE(!Z, "tp_test_linear_bwd: Z without TP_LINEAR_GELU_BWD");
    GemmArgs g = plain_gemm(A, lda, W, C, ldc, M, N, K, nullptr, flags);       // (as tp_linear / tp_backward's dgrad build theirs)
    g.Z = (const char*)Z; g.ldz = ldz; g.out_scale = out_scale; g.tile = tile;
    return gemm_launch(dtype, out_dtype, g, (hipStream_t)stream);
}

// ---- the weight-gradient contraction dW = dY^T · X (tp_internal.h: wgrad_tt_launch, wgrad_tn_launch, wgrad_plan) ------------------

int tp_test_wgrad_plan(int64_t rows, int n_out, int k_in, int transposed, int64_t rpad, int* splits, long long* rows_per_split) {
    TP_REQUIRE(splits && rows_per_split, "tp_test_wgrad_plan: NULL argument");
    TP_REQUIRE(transposed == 0 || transposed == 1, "tp_test_wgrad_plan: transposed 0 / 1");
    TP_REQUIRE(rows > 0 && n_out > 0 && k_in > 0 && n_out % 8 == 0 && k_in % 256 == 0,
               "tp_test_wgrad_plan: need rows > 0, n_out %% 8 == 0, k_in %% 256 == 0");
    if (transposed) TP_REQUIRE(rpad % 1024 == 0 && rpad >= rows, "tp_test_wgrad_plan: the transposed form needs rpad %% 1024 == 0, rpad >= rows");
    wgrad_plan(rows, n_out, k_in, transposed != 0, rpad, splits, rows_per_split);
    return TP_OK;
}

int tp_test_wgrad(const void* dy, int64_t ldy, const void* x, int64_t ldx, int rows_per_batch, int64_t batch_stride,
                  const void* x_part0, const void* x_part1, const void* x_part2, const void* x_part3, int n_part,
                  int64_t rows, int n_out, int k_in, int dtype, int out_dtype, void* grad_out, void* grad_out_hi, int split_row,
                  const float* out_scale, int accumulate, int* counters, size_t counter_ints, void* part, size_t part_bytes,
                  int transposed, void* stream) {
    const void* parts[4] = {x_part0, x_part1, x_part2, x_part3};
    const bool any_part = x_part0 || x_part1 || x_part2 || x_part3 || n_part != 0;
    TP_REQUIRE(transposed == 0 || transposed == 1, "tp_test_wgrad: transposed 0 / 1");
    TP_REQUIRE(half_dtype(dtype) && any_dtype(out_dtype), "tp_test_wgrad: dtype must be TP_BF16 / TP_F16, out_dtype one of the three");
    TP_REQUIRE(accumulate == 0 || accumulate == 1, "tp_test_wgrad: accumulate 0 / 1");
    TP_REQUIRE(!accumulate || out_dtype == TP_F32, "tp_test_wgrad: accumulate needs an fp32 output (out_dtype %d)", out_dtype);
    TP_REQUIRE(!(transposed && any_part), "tp_test_wgrad: the transposed form takes one X^T, not four parts");
    TP_REQUIRE(!(transposed && split_row != 0), "tp_test_wgrad: the transposed form has no split_row / grad_out_hi");
    TP_REQUIRE(!(transposed && grad_out_hi), "tp_test_wgrad: the transposed form has no split_row / grad_out_hi");
    TP_REQUIRE(!(transposed && (rows_per_batch != 0 || batch_stride != 0)), "tp_test_wgrad: the transposed form has no batch stride");
    TP_REQUIRE(dy && part, "tp_test_wgrad: NULL argument (dy / part)");
    if (any_part) {
        TP_REQUIRE(x_part0 && x_part1 && x_part2 && x_part3 && !x, "tp_test_wgrad: NULL argument (parts: all four, and x NULL)");
        TP_REQUIRE(n_part > 0, "tp_test_wgrad: parts need n_part > 0");
        TP_REQUIRE(al16(x_part0) && al16(x_part1) && al16(x_part2) && al16(x_part3), "tp_test_wgrad: the x parts must be 16-byte aligned");
    } else {
        TP_REQUIRE(x, "tp_test_wgrad: NULL argument (x)");
    }
    TP_REQUIRE(rows > 0 && n_out > 0 && k_in > 0, "tp_test_wgrad: need rows, n_out, k_in > 0");
    TP_REQUIRE(split_row >= 0 && split_row < n_out, "tp_test_wgrad: split_row must lie in [0, n_out)");
    if (split_row > 0) TP_REQUIRE(grad_out || grad_out_hi, "tp_test_wgrad: NULL argument (grad_out and grad_out_hi)");
    else TP_REQUIRE(grad_out && !grad_out_hi, "tp_test_wgrad: NULL argument (grad_out), or grad_out_hi without a split_row");
    TP_REQUIRE(al16(dy) && al16(x) && al16(grad_out) && al16(grad_out_hi), "tp_test_wgrad: dy / x / grad_out / grad_out_hi must be 16-byte aligned");
    TP_REQUIRE(((uintptr_t)part & 255) == 0, "tp_test_wgrad: part must be 256-byte aligned");
    TP_REQUIRE(((uintptr_t)out_scale & 3) == 0 && ((uintptr_t)counters & 3) == 0, "tp_test_wgrad: out_scale / counters must be 4-byte aligned");
    TP_REQUIRE(!counters || counter_ints >= 32, "tp_test_wgrad: a counters slot is 32 zeroed ints ([4 groups][8 XCDs])");
    TP_REQUIRE(ldy >= n_out, "tp_test_wgrad: ldy < n_out");
    if (transposed) {
        TP_REQUIRE(ldx >= rows, "tp_test_wgrad: the transposed form needs ldx (= rpad) >= rows");
        return wgrad_tn_launch(dtype, dy, ldy, x, ldx, rows, n_out, k_in, (float*)part, part_bytes, out_dtype, grad_out, counters,
                               (hipStream_t)stream, out_scale, accumulate != 0);
    }
    TP_REQUIRE(ldx >= (any_part ? n_part : k_in), "tp_test_wgrad: ldx is shorter than a row of x");
    if (rows_per_batch > 0 && rows_per_batch < rows)
        TP_REQUIRE(batch_stride >= (int64_t)rows_per_batch * ldx, "tp_test_wgrad: batch_stride must cover rows_per_batch rows");
    const WgradX X{any_part ? x_part0 : x, ldx, rows_per_batch, batch_stride, any_part ? parts : nullptr, any_part ? n_part : 0};
    return wgrad_tt_launch(dtype, dy, ldy, X, rows, n_out, k_in, (float*)part, part_bytes, out_dtype, grad_out, counters,
                           (hipStream_t)stream, grad_out_hi, split_row, out_scale, accumulate != 0);
}

}  // extern "C"
