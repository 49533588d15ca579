// The backward's own tile steps, shared by the attention backward kernels (attention_bwd.hip: the LDS kernel, dense and packed;
// attention_bwd_stream.hip: the query-owned and the key-owned streaming kernel), head dim 64.  The LDS images, the lane ownership and the
// MFMA operand forms are attention_tile.h's: Q, K and dO are read by rows AND transposed (Img64<true>), V only by rows (Img64<false>).
// tests/attention_bwd_ref.backward_emulated states the same arithmetic on the CPU.  The head-dim-80 forms of the steps
// (attention_bwd80.hip) stand at the end of the file.
// Rounding points: P and dS to bf16 only as MFMA operands (tile_pack), fp32 accumulators, dq / dk / dv to bf16 at the store (tile_store);
// everything else fp32, P = exp2(fma(s, log2e, -m log2e)) * (1 / l) wherever it comes from saved row statistics: bwd_p in the streaming
// kernels; phase 2 of the LDS kernel spells the same expression out, for the measured reason given there, and phase 1 has its own softmax.
#pragma once
#include "attention_tile.h"

namespace kemr {

// The score pair of one 16-row tile of the other side (row = the tile's row lrow): s += rows(img1) . b1 and dp += rows(img2) . b2 over
// the two k-steps of d = 64, b1 / b2 the own tile's fragments.  img1 is an Img64<true>; TRL2 is the swizzle of img2.
template <bool TRL2>
__device__ __forceinline__ void bwd_scores(const char* img1, const char* img2, int row, int lq, const bf16x8 (&b1)[2],
                                           const bf16x8 (&b2)[2], f32x4& s, f32x4& dp) {
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
        s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(tile_row<Img64<true>>(img1, row, kk * 4 + lq), b1[kk], s, 0, 0, 0);
        dp = __builtin_amdgcn_mfma_f32_16x16x32_bf16(tile_row<Img64<TRL2>>(img2, row, kk * 4 + lq), b2[kk], dp, 0, 0, 0);
    }
}

// P from the saved row statistics m = max * log2e and inv = 1 / sum; the caller's dS = P * (dP - D) follows it
__device__ __forceinline__ float bwd_p(float s, float m, float inv, bool ok) {
    return ok ? __builtin_amdgcn_exp2f(__builtin_fmaf(s, LOG2E, -m)) * inv : 0.f;
}

// acc += M^T . x over the 32 other rows of block u of the Img64<true> image M, x0 / x1 = the tiles 2 u and 2 u + 1 of P or dS.  a holds the
// A fragments and belongs to the caller: the two products of one block (dK and dV) go through ONE array, which keeps the second
// product's reads behind the first product's MFMAs -- with an array each, the LDS kernel compiles to 200 VGPRs at 64 rows where it has 140.
__device__ __forceinline__ void bwd_accum(const char* img, int u, int lrow, int lq, const f32x4& x0, const f32x4& x1, bf16x8 (&a)[4],
                                          f32x4 (&acc)[4]) {
    tile_tr<Img64<true>>(img, u, lrow, lq, a);
    const bf16x8 xf = tile_pack(x0, x1);
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) acc[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[dt], xf, acc[dt], 0, 0, 0);
}

// The refusals the three entry points share, in their order, on the host before any HIP call; each op's grid check follows them where
// its launch geometry is.  row_start points at the packed op's row_start argument, which is tested, and is nullptr for an op that has
// none; t_name is how the op words its length argument ("t" / "max_t"); the non-causal op passes causal = 0.
inline int bwd_refuse(const char* op, const void* qkv, const void* dout, const void* dqkv, const int* const* row_start, const char* t_name,
                      int t, int t_max, int width, int causal, int batch) {
    if (!qkv) KEMR_FAIL(KEMR_ERR_INVALID, "%s: qkv is NULL", op);
    if (!dout) KEMR_FAIL(KEMR_ERR_INVALID, "%s: dout is NULL", op);
    if (!dqkv) KEMR_FAIL(KEMR_ERR_INVALID, "%s: dqkv is NULL", op);
    if (row_start && !*row_start) KEMR_FAIL(KEMR_ERR_INVALID, "%s: row_start is NULL", op);
    if (t < 1 || t > t_max) KEMR_FAIL(KEMR_ERR_INVALID, "%s: %s = %d is outside 1..%d", op, t_name, t, t_max);
    if (width <= 0 || width % 64 != 0) KEMR_FAIL(KEMR_ERR_INVALID, "%s: width = %d is not a positive multiple of 64 (heads of 64)", op, width);
    if (causal != 0 && causal != 1) KEMR_FAIL(KEMR_ERR_INVALID, "%s: causal = %d is neither 0 nor 1", op, causal);
    if (batch < 0) KEMR_FAIL(KEMR_ERR_INVALID, "%s: batch = %d is negative", op, batch);
    return KEMR_OK;
}

// ---- head dim 80 (attention_bwd80.hip): additions, the head-dim-64 steps above are as they were ------------------------------------------
// Every chunk image is an Img80 (rows of 160 B, no swizzle; read by rows and transposed alike).  The contraction over 80 is
// attention80.hip's: two K = 32 steps and a third whose k slots 16..31 (the lanes lq >= 2) are zero in both operands -- the own tile's
// third fragment is cleared in registers where it is loaded (bwd_own80), the streamed side's read of those lanes goes to `zero`, one
// 16-byte chunk of zeros the kernel keeps in LDS.  Nothing beyond column 79 of a head is loaded.

// The three B fragments of the wave's own row p (80 bf16): columns 0..31, 32..63, and 64..79 in the k slots 0..15 with zeros made here in
// the slots 16..31 (the lanes lq >= 2 load the columns 64 + 8 (lq & 1) .. of their own head again and clear them).
__device__ __forceinline__ void bwd_own80(const bf16_t* p, int lq, bf16x8 (&dst)[3]) {
    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
    const unsigned keep = lq < 2 ? 0xffffffffu : 0u;
    dst[0] = *(const bf16x8*)(p + lq * 8);
    dst[1] = *(const bf16x8*)(p + 32 + lq * 8);
    u32x4 t = *(const u32x4*)(p + 64 + (lq & 1) * 8);
    t.x &= keep; t.y &= keep; t.z &= keep; t.w &= keep;
    dst[2] = __builtin_bit_cast(bf16x8, t);
}

// bwd_scores over d = 80: s += rows(img1) . b1 and dp += rows(img2) . b2, both images Img80
__device__ __forceinline__ void bwd_scores80(const char* img1, const char* img2, const char* zero, int row, int lq, const bf16x8 (&b1)[3],
                                             const bf16x8 (&b2)[3], f32x4& s, f32x4& dp) {
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
        s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(tile_row<Img80>(img1, row, kk * 4 + lq), b1[kk], s, 0, 0, 0);
        dp = __builtin_amdgcn_mfma_f32_16x16x32_bf16(tile_row<Img80>(img2, row, kk * 4 + lq), b2[kk], dp, 0, 0, 0);
    }
    const int c2 = 8 + (lq & 1);                         // the chunks 8 and 9 of the row: columns 64..79
    const bf16x8 a1 = *(const bf16x8*)(lq < 2 ? img1 + Img80::off(row, c2) : zero);
    const bf16x8 a2 = *(const bf16x8*)(lq < 2 ? img2 + Img80::off(row, c2) : zero);
    s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, b1[2], s, 0, 0, 0);
    dp = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a2, b2[2], dp, 0, 0, 0);
}

// bwd_accum with five d-tiles: acc += M^T . x over the 32 other rows of block u of the Img80 image M
__device__ __forceinline__ void bwd_accum80(const char* img, int u, int lrow, int lq, const f32x4& x0, const f32x4& x1, bf16x8 (&a)[5],
                                            f32x4 (&acc)[5]) {
    tile_tr<Img80>(img, u, lrow, lq, a);
    const bf16x8 xf = tile_pack(x0, x1);
#pragma unroll
    for (int dt = 0; dt < 5; ++dt) acc[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[dt], xf, acc[dt], 0, 0, 0);
}

// bwd_refuse for an op that takes the head dim as an argument (head_dim is one the op serves: the op tests that first).  The causal
// form exists at heads of 64 only.
inline int bwd_refuse_hd(const char* op, const void* qkv, const void* dout, const void* dqkv, int t, int t_max, int width, int head_dim,
                         int causal, int batch) {
    if (!qkv) KEMR_FAIL(KEMR_ERR_INVALID, "%s: qkv is NULL", op);
    if (!dout) KEMR_FAIL(KEMR_ERR_INVALID, "%s: dout is NULL", op);
    if (!dqkv) KEMR_FAIL(KEMR_ERR_INVALID, "%s: dqkv is NULL", op);
    if (t < 1 || t > t_max) KEMR_FAIL(KEMR_ERR_INVALID, "%s: t = %d is outside 1..%d", op, t, t_max);
    if (width <= 0 || width % head_dim != 0)
        KEMR_FAIL(KEMR_ERR_INVALID, "%s: width = %d is not a positive multiple of %d (heads of %d)", op, width, head_dim, head_dim);
    if (causal != 0 && causal != 1) KEMR_FAIL(KEMR_ERR_INVALID, "%s: causal = %d is neither 0 nor 1", op, causal);
    if (causal && head_dim != 64)
        KEMR_FAIL(KEMR_ERR_INVALID, "%s: causal = 1 is not served at head_dim = %d (no tower has causal heads of %d)", op, head_dim, head_dim);
    if (batch < 0) KEMR_FAIL(KEMR_ERR_INVALID, "%s: batch = %d is negative", op, batch);
    return KEMR_OK;
}

}  // namespace kemr
