// The one statement of what the attention kernels share, forward and backward, head dims 64 and 80 (attention.hip, attention_stream.hip,
// attention80.hip, fp32x3.hip, attention_bwd.hip, attention_bwd_stream.hip; attention_bwd_tile.h adds the backward's own steps): the LDS
// images, the MFMA operand forms and the forward's rounding points.
//
// Lane ownership, lrow = lane & 15, lq = lane >> 4: a wave owns 16 rows of one side (the forward: queries) and meets 16-row tiles t of
// the other side (keys); s[t][r] belongs to (own row lrow, other row 16 t + 4 lq + r), so a lane holds 4 consecutive other rows of ONE
// own row and a reduction over the other side is a register reduction and two shuffles (row_max / row_sum).
// The k-slot order of the second product (O^T = V^T . P^T and its backward kin) is permuted, slot 8 lq + j <-> other row
// 32 u + 16 (j >> 2) + 4 lq + (j & 3), identically for both operands (tile_tr and tile_pack): the score registers feed the MFMA with no
// lane movement.
// The forward's rounding points: P goes to bf16 only as an MFMA operand (tile_pack), the row sum is taken in fp32 BEFORE that rounding
// (tile_exp; the pooled-row kernels of attention.hip and attention80.hip do the same over an LDS row), and the fp32 accumulators meet
// one division by it, at the store (tile_store).
#pragma once
#include "common.h"

namespace kemr {

constexpr float LOG2E = 1.4426950408889634f;

// ds_read_b64_tr_b16: the transposed read that makes a V^T MFMA fragment out of the row-major V image
__device__ __forceinline__ bf16x4 lds_read_tr16(const char* p) {
    typedef __attribute__((ext_vector_type(4))) short s4;
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s4*)p);
}
// LDS stores of all lanes of a wave before any lane's loads (a wave working on its own: no workgroup barrier)
__device__ __forceinline__ void wave_lds_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// Which (head, image) a workgroup computes.  xbatch == 0: blockIdx.x = head, blockIdx.y = image.  xbatch = the batch size: the
// grid is (heads, batch rounded up to 8) and the workgroups -- dealt to the eight XCDs round-robin by their linear id -- are
// renumbered so that XCD x computes the images = x (mod 8), all heads of an image next to each other in time: the 128-byte
// slices the sixteen heads take out of one token's 6 KB q|k|v row then come through ONE L2 at about the same time instead of
// through eight (round 3: 155 -> 150 us at B = 255 x 16 heads, bit-identical results; the default, debug switch attn_xcd).
__device__ __forceinline__ bool attn_item(int xbatch, int& h, int& b) {
    h = blockIdx.x; b = blockIdx.y;
    if (xbatch == 0) return true;
    const int id = blockIdx.y * gridDim.x + blockIdx.x, j = id >> 3;
    b = (j / (int)gridDim.x) * 8 + (id & 7);
    h = j % (int)gridDim.x;
    return b < xbatch;
}

// ---- the LDS images: row-major, ROWB bytes per row, off(row, c) = the byte offset of 16-byte chunk c of a row ---------------------
// Head dim 64: rows of 128 B = 64 bf16 = eight chunks, XOR-swizzled.  An image that starts at a multiple of 8 rows has the swizzle of
// its local rows.
//   TRL = false, the K type: an image that is only read by rows (the forward's K, the backward's V).  chunk ^= (row >> 1) & 7:
//     ds_read_b128 of 16 consecutive rows at one chunk is conflict-free.
//   TRL = true, the V type: an image that is read transposed (the forward's V), or by rows AND transposed (the backward's Q, K, dO).
//     32-byte chunk ^= (row >> 1) & 3: the transposed reads are conflict-free, row reads 2-way.
template <bool TRL>
struct Img64 {
    static constexpr int ROWB = 128, ND = 4;            // ND: 16-column d-tiles of a row
    static __device__ __forceinline__ int swz(int row, int c) {       // byte offset of chunk c inside its row
        return (TRL ? (c ^ (((row >> 1) & 3) << 1)) : (c ^ ((row >> 1) & 7))) << 4;
    }
    static __device__ __forceinline__ int off(int row, int c) { return row * 128 + swz(row, c); }
};
// Head dim 80: rows of exactly 160 B (80 bf16 = ten chunks, no pad columns), NO swizzle -- ten is no power of two, and the pitch itself
// spreads the banks: 160 B = 10 slots of 16 B = 40 banks, and 5 r mod 8 is a bijection of r mod 8, so
//   * ds_read_b128 (K fragments; a lane group of 16 = rows {0-3, 12-15} at chunk c and rows 4-11 at chunk c + 1, or the mirror):
//     slot (10 r + c) mod 16 = 2 (5 r mod 8) + c takes the 8 even values over 8 rows that differ mod 8, chunk c + 1 the odd ones:
//     16 lanes on 16 different slots, conflict-free;
//   * ds_read_b64_tr_b16 (V^T fragments; a 32-lane half = 8 consecutive rows 8 n .. 8 n + 7, 32 B = 8 banks of each at the same
//     column offset): bank (40 r + 8 dt) mod 64 = 8 (5 r + dt mod 8) is a different multiple of 8 for each of the 8 rows: 8 x 8
//     banks = all 64, conflict-free.
// The contraction over 80 columns is two K = 32 steps and a third whose k slots 16..31 (the lanes lq >= 2) are zero in both operands:
// their K read goes to ONE 16-byte chunk of zeros (broadcast) that the kernel keeps ZERO bytes behind the V image.
struct Img80 {
    static constexpr int ROWB = 160, ND = 5, ZERO = 16;
    static __device__ __forceinline__ int swz(int, int c) { return c * 16; }
    static __device__ __forceinline__ int off(int row, int c) { return row * 160 + c * 16; }
};

template <class L>
__device__ __forceinline__ bf16x8 tile_row(const char* img, int row, int c) { return *(const bf16x8*)(img + L::off(row, c)); }

// one 16-byte piece of a row into its image, zeroed when the row is a pad row (component-wise: a struct select went to scratch)
template <class L>
__device__ __forceinline__ void tile_put(char* img, int row, int c, uint4 a, bool valid) {
    const unsigned keep = valid ? 0xffffffffu : 0u;
    a.x &= keep; a.y &= keep; a.z &= keep; a.w &= keep;
    *(uint4*)(img + L::off(row, c)) = a;
}

// ---- the MFMA operand forms of the second product ---------------------------------------------------------------------------------
// The A fragments (L::ND d-tiles) of M^T for the 32 rows of block u of the image M: rows 32 u + 4 lq .. + 3 in the first half of the
// lane's k slots, rows 32 u + 16 + 4 lq .. + 3 in the second.  ds_read_b64_tr_b16 gathers across lanes: EXEC must be full, so
// whatever skips a block is wave-uniform and no lane leaves before the last transposed read.
template <class L>
__device__ __forceinline__ void tile_tr(const char* img, int u, int lrow, int lq, bf16x8 (&dst)[L::ND]) {
    const int ra = u * 32 + lq * 4 + (lrow >> 2), rb = ra + 16;
#pragma unroll
    for (int dt = 0; dt < L::ND; ++dt) {
        const int c = dt * 2 + ((lrow & 3) >> 1);       // columns 16 dt + 4 (lrow & 3) .. + 3 of the row
        const bf16x4 va = lds_read_tr16(img + L::off(ra, c) + (lrow & 1) * 8);
        const bf16x4 vb = lds_read_tr16(img + L::off(rb, c) + (lrow & 1) * 8);
        dst[dt][0] = va[0]; dst[dt][1] = va[1]; dst[dt][2] = va[2]; dst[dt][3] = va[3];
        dst[dt][4] = vb[0]; dst[dt][5] = vb[1]; dst[dt][6] = vb[2]; dst[dt][7] = vb[3];
    }
}
// the B fragment of the tiles 2 u (a) and 2 u + 1 (b) of P (backward: or dS), rounded to bf16 here and nowhere else
__device__ __forceinline__ bf16x8 tile_pack(const f32x4& a, const f32x4& b) {
    union { bf16x8 v; uint32_t w[4]; } f;
    f.w[0] = pack_bf16x2(a[0], a[1]); f.w[1] = pack_bf16x2(a[2], a[3]);
    f.w[2] = pack_bf16x2(b[0], b[1]); f.w[3] = pack_bf16x2(b[2], b[3]);
    return f.v;
}
// acc[dt][r] = (own row lrow)[d = 16 dt + 4 lq + r], times inv (the forward's 1 / row sum; the backward stores unscaled), to bf16;
// dst points at d = 4 lq of that row
template <int ND>
__device__ __forceinline__ void tile_store(bf16_t* dst, const f32x4 (&acc)[ND], float inv = 1.0f) {
#pragma unroll
    for (int dt = 0; dt < ND; ++dt) {
        uint2 pk;
        pk.x = pack_bf16x2(acc[dt][0] * inv, acc[dt][1] * inv);
        pk.y = pack_bf16x2(acc[dt][2] * inv, acc[dt][3] * inv);
        *(uint2*)(dst + dt * 16) = pk;
    }
}

// ---- the forward's softmax steps --------------------------------------------------------------------------------------------------
// the row exchange: the lanes lq = 0..3 of one own row
__device__ __forceinline__ float row_max(float v) {
    v = fmaxf(v, __shfl_xor(v, 16));
    return fmaxf(v, __shfl_xor(v, 32));
}
__device__ __forceinline__ float row_sum(float v) {
    v += __shfl_xor(v, 16);
    return v + __shfl_xor(v, 32);
}
// s = exp(s - max) = exp2(s * log2e - max * log2e) for one tile, l2 = {LOG2E, LOG2E}, nm = {-max log2e, ..}; masked keys (-inf) -> 0.
// The multiply-add and the row sum run two elements per instruction (v_pk_fma_f32 / v_pk_add_f32): the softmax is issue-bound, the
// MFMAs hide behind it.  sum2 takes the unrounded P.
__device__ __forceinline__ void tile_exp(f32x4& s, f32x2_t l2, f32x2_t nm, f32x2_t& sum2) {
    f32x2_t a = f32x2_t{s[0], s[1]} * l2 + nm, c = f32x2_t{s[2], s[3]} * l2 + nm;
    a.x = __builtin_amdgcn_exp2f(a.x); a.y = __builtin_amdgcn_exp2f(a.y);
    c.x = __builtin_amdgcn_exp2f(c.x); c.y = __builtin_amdgcn_exp2f(c.y);
    s[0] = a.x; s[1] = a.y; s[2] = c.x; s[3] = c.y;
    sum2 += a;
    sum2 += c;
}

}  // namespace kemr
