// The tile arithmetic the attention backward kernels share (attention_bwd.hip: the LDS kernel, dense and packed; attention_bwd_stream.hip:
// the query-owned and the key-owned streaming kernel), head dim 64: the one statement of the LDS layout, of the MFMA operand forms and
// of the rounding points.  tests/attention_bwd_ref.backward_emulated states the same arithmetic on the CPU.
//
// LDS images: rows of 128 B = 64 bf16 = eight 16-byte chunks.  An image that is read by rows AND transposed (Q, K, dO) carries the
// forward's V swizzle (TRL: 32-byte chunk ^= (row >> 1) & 3: transposed reads conflict-free, row reads 2-way); an image that is only
// read by rows (V) carries the K swizzle (16-byte chunk ^= (row >> 1) & 7: conflict-free).  An image that starts at a multiple of 8 rows
// has the swizzle of its local rows.
// Lane ownership, lrow = lane & 15, lq = lane >> 4: a wave owns the 16 rows of one side (queries or keys) and meets 16-row tiles t of
// the other side; s[t][r] / dp[t][r] belong to (own row lrow of the wave's tile, other row 16 t + 4 lq + r), so a lane holds 4
// consecutive other rows of ONE own row and a sum over the other side is a register sum and two shuffles (xor 16, 32).
// Rounding points: P and dS to bf16 only as MFMA operands (bwd_pack), fp32 accumulators, dq / dk / dv to bf16 at the store (bwd_store);
// everything else fp32, P = exp2(fma(s, log2e, -m log2e)) * (1 / l) wherever it comes from saved row statistics: bwd_p in the streaming
// kernels; phase 2 of the LDS kernel spells the same expression out, for the measured reason given there, and phase 1 has its own softmax.
#pragma once
#include "common.h"

namespace kemr {

constexpr float LOG2E = 1.4426950408889634f;

template <bool TRL>
__device__ __forceinline__ int bwd_off(int row, int c) {
    return row * 128 + ((TRL ? (c ^ (((row >> 1) & 3) << 1)) : (c ^ ((row >> 1) & 7))) << 4);
}
template <bool TRL>
__device__ __forceinline__ bf16x8 bwd_row(const char* img, int row, int c) { return *(const bf16x8*)(img + bwd_off<TRL>(row, c)); }

// one 16-byte piece of a row into its image, zeroed when the row is a pad row
template <bool TRL>
__device__ __forceinline__ void bwd_put(char* img, int row, int c, uint4 a, bool valid) {
    const unsigned keep = valid ? 0xffffffffu : 0u;
    a.x &= keep; a.y &= keep; a.z &= keep; a.w &= keep;
    *(uint4*)(img + bwd_off<TRL>(row, c)) = a;
}

// the A fragments (4 d-tiles) of M^T for the 32 rows of block u of the TRL image M (forward's load_v): k slot 8 lq + j <-> row
// 32 u + 16 (j >> 2) + 4 lq + (j & 3), the rows bwd_pack gives the same slots.  ds_read_b64_tr_b16 gathers across lanes: EXEC must be
// full, so whatever skips a block is wave-uniform and no lane leaves before the last transposed read.
__device__ __forceinline__ void bwd_tr(const char* img, int u, int lrow, int lq, bf16x8 (&dst)[4]) {
    const int ra = u * 32 + lq * 4 + (lrow >> 2), rb = ra + 16;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
        const int c = dt * 2 + ((lrow & 3) >> 1);
        const bf16x4 va = lds_read_tr16(img + bwd_off<true>(ra, c) + (lrow & 1) * 8);
        const bf16x4 vb = lds_read_tr16(img + bwd_off<true>(rb, c) + (lrow & 1) * 8);
        dst[dt][0] = va[0]; dst[dt][1] = va[1]; dst[dt][2] = va[2]; dst[dt][3] = va[3];
        dst[dt][4] = vb[0]; dst[dt][5] = vb[1]; dst[dt][6] = vb[2]; dst[dt][7] = vb[3];
    }
}
// the B fragment of the tiles 2 u (a) and 2 u + 1 (b) of P or dS, rounded to bf16
__device__ __forceinline__ bf16x8 bwd_pack(const f32x4& a, const f32x4& b) {
    union { bf16x8 v; uint32_t w[4]; } f;
    f.w[0] = pack_bf16x2(a[0], a[1]); f.w[1] = pack_bf16x2(a[2], a[3]);
    f.w[2] = pack_bf16x2(b[0], b[1]); f.w[3] = pack_bf16x2(b[2], b[3]);
    return f.v;
}
// acc[dt][r] = d(own row lrow)[d = 16 dt + 4 lq + r]; dst points at d = 4 lq of that row
__device__ __forceinline__ void bwd_store(bf16_t* dst, const f32x4 (&acc)[4]) {
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
        uint2 pk;
        pk.x = pack_bf16x2(acc[dt][0], acc[dt][1]);
        pk.y = pack_bf16x2(acc[dt][2], acc[dt][3]);
        *(uint2*)(dst + dt * 16) = pk;
    }
}

// The score pair of one 16-row tile of the other side (row = the tile's row lrow): s += rows(img1) . b1 and dp += rows(img2) . b2 over
// the two k-steps of d = 64, b1 / b2 the own tile's fragments.  img1 is a TRL image; TRL2 is the swizzle of img2.
template <bool TRL2>
__device__ __forceinline__ void bwd_scores(const char* img1, const char* img2, int row, int lq, const bf16x8 (&b1)[2],
                                           const bf16x8 (&b2)[2], f32x4& s, f32x4& dp) {
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
        s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bwd_row<true>(img1, row, kk * 4 + lq), b1[kk], s, 0, 0, 0);
        dp = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bwd_row<TRL2>(img2, row, kk * 4 + lq), b2[kk], dp, 0, 0, 0);
    }
}

// P from the saved row statistics m = max * log2e and inv = 1 / sum; the caller's dS = P * (dP - D) follows it
__device__ __forceinline__ float bwd_p(float s, float m, float inv, bool ok) {
    return ok ? __builtin_amdgcn_exp2f(__builtin_fmaf(s, LOG2E, -m)) * inv : 0.f;
}

// acc += M^T . x over the 32 other rows of block u of the TRL image M, x0 / x1 = the tiles 2 u and 2 u + 1 of P or dS.  a holds the
// A fragments and belongs to the caller: the two products of one block (dK and dV) go through ONE array, which keeps the second
// product's reads behind the first product's MFMAs -- with an array each, the LDS kernel compiles to 200 VGPRs at 64 rows where it has 140.
__device__ __forceinline__ void bwd_accum(const char* img, int u, int lrow, int lq, const f32x4& x0, const f32x4& x1, bf16x8 (&a)[4],
                                          f32x4 (&acc)[4]) {
    bwd_tr(img, u, lrow, lq, a);
    const bf16x8 xf = bwd_pack(x0, x1);
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

}  // namespace kemr
