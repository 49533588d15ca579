// Non-causal multi-head attention for long vision sequences: 289 <= T <= KEMR_MAX_VISION_TOKENS (ViT-L/14@336px: T = 577).
// Head dim 64, the q | k | v rows of attention.hip ([B*T, 3W] bf16, q pre-scaled by 1/8), output [B*T, W] bf16.
//
// attention.hip keeps a head's whole K and V in LDS and the full score row in registers; at 608 padded keys that would take
// 152 KB of LDS and about 152 fp32 VGPRs per lane for the scores alone.  This kernel is the flash form of the same tile code:
//   * one workgroup of 4 waves per (image, head, block of QB = 128 queries); a wave owns two 16-query tiles (rows
//     128 qb + 16 w + 64 i, i = 0, 1), so every K / V fragment it reads from LDS feeds two MFMAs;
//   * K and V stream through LDS in chunks of KC = 64 keys, double-buffered: the global loads of chunk c + 1 are in flight in
//     registers while chunk c is computed, then written to the other LDS buffer -- one barrier per chunk;
//   * per query a running max m and row sum l in fp32: for every chunk m' = max(m, chunk max), O and l are scaled by
//     exp(m - m') (exactly 1 when the max did not move), P = exp(S - m');
//   * the MFMA forms and LDS images are attention.hip's: S^T = K . Q^T puts four keys of one query in a lane (row max and
//     sum: two shuffles), V^T comes through ds_read_b64_tr_b16 from the row-major V image, and the permuted k-slot order lets
//     the bf16 P registers feed the PV MFMA with no lane movement.  K rows 128 B with chunk ^= (row >> 1) & 7, V rows with
//     32-byte chunk ^= (row >> 1) & 3: conflict-free (a chunk starts at a multiple of 64 rows, so the swizzle is unchanged).
// Rounding as in the tile kernels: P is rounded to bf16 for the PV product, the row sum is accumulated in fp32 from the
// unrounded P, and the output is divided by it once at the end.  No atomics, a fixed order of every sum: bit-identical run to run.
// Pad keys (the ragged last chunk: 577 = 9 * 64 + 1) are zero-filled in LDS and masked to -inf; key tiles made only of pad keys
// are skipped (wave-uniform).  Pad queries read the last valid row and are not stored.
// Compile-time A/B switches (tools/ab_build_flag.sh; the defaults are the product): KEMR_ATTN_LONG_QT query tiles per wave,
// KEMR_ATTN_LONG_KC keys per chunk, KEMR_ATTN_LONG_OCC waves per SIMD asked of the register allocator.  At T = 577, B = 85,
// width 1024 (tools/bench_attention_long.py): QT 2 / KC 64 / 2 waves (180 VGPRs) 314-326 us; QT 1 / KC 64 / 4 waves (126 VGPRs)
// 325 us; QT 1 / KC 128, 3 or 4 waves, 415 us.  Occupancy is not what holds it back: the counters put it at 2.35 x the VALU
// instructions per MFMA of the 257-token kernel (softmax and per-chunk bookkeeping; DESIGN.md, "Long sequences").
#include "common.h"

namespace kemr {

namespace {

#ifndef KEMR_ATTN_LONG_QT
#define KEMR_ATTN_LONG_QT 2
#endif
#ifndef KEMR_ATTN_LONG_OCC
#define KEMR_ATTN_LONG_OCC 2
#endif
constexpr int LA_NW = 4;                  // waves per workgroup
constexpr int LA_QT = KEMR_ATTN_LONG_QT;  // 16-query tiles per wave
constexpr int LA_QB = LA_NW * LA_QT * 16; // queries per workgroup
#ifndef KEMR_ATTN_LONG_KC
#define KEMR_ATTN_LONG_KC 64
#endif
constexpr int LA_KC = KEMR_ATTN_LONG_KC;  // keys per LDS chunk
constexpr int LA_NT16 = LA_KC / 16;       // 16-key S^T tiles per chunk
constexpr int LA_NU = LA_KC / 32;         // 32-key PV blocks per chunk
constexpr int LA_STAGE = LA_KC * 128 * 2; // bytes of one K + V chunk image
constexpr int LA_NCH = LA_KC * 8 / (LA_NW * 64);   // 16-byte pieces of K (and of V) per thread and chunk

__device__ __forceinline__ bf16x4 lds_read_tr16_l(const char* p) {
    typedef __attribute__((ext_vector_type(4))) short s4;
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s4*)p);
}

}  // namespace

// Work items (query block fastest, then head, then image) are numbered so that the workgroups dealt to one XCD (the dispatcher
// deals linear ids round-robin over the eight XCDs) take a contiguous range: the query blocks of one (image, head) read the same
// K / V rows through the same L2.  Only a locality heuristic; every item is computed exactly once whatever the placement.
__global__ __launch_bounds__(LA_NW * 64, KEMR_ATTN_LONG_OCC) void attention_long_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ out,
                                                                     int T, int width, int nqb, int items) {
    constexpr float LOG2E = 1.4426950408889634f;
    __shared__ __attribute__((aligned(16))) char smem[2 * LA_STAGE];

    const int heads = width >> 6;
    const int per_xcd = (int)(gridDim.x >> 3);
    const int id = (int)blockIdx.x;
    const int item = (id & 7) * per_xcd + (id >> 3);
    if (item >= items) return;                         // whole workgroup: before any barrier
    const int qb = item % nqb, hb = item / nqb;
    const int h = hb % heads, b = hb / heads;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ld = 3 * width;
    const bf16_t* base = qkv + (size_t)b * T * ld + h * 64;
    const int lrow = lane & 15, lq = lane >> 4;
    const int nch = (T + LA_KC - 1) / LA_KC;

    // query fragments of the wave's two tiles (B operand of S^T = K . Q^T): rows clamped to the last valid one
    bf16x8 qf[LA_QT][2];
#pragma unroll
    for (int i = 0; i < LA_QT; ++i) {
        const int q = qb * LA_QB + i * (LA_NW * 16) + wid * 16 + lrow;
        const int qc = q < T ? q : T - 1;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) qf[i][kk] = *(const bf16x8*)(base + (size_t)qc * ld + kk * 32 + lq * 8);
    }

    // chunk staging: LA_NCH pieces of K and of V per thread, loaded into registers, written swizzled.  Plain (temporal) loads: unlike
    // attention.hip, where one workgroup reads a head's K / V, the nqb query-block workgroups of a head read the same rows (through one
    // L2, see the numbering above).  Same time as non-temporal loads at T = 577 (368.5 vs 374.6 us).
    uint4 kv[LA_NCH], vv[LA_NCH];
    auto load_chunk = [&](int c) {
#pragma unroll
        for (int i = 0; i < LA_NCH; ++i) {
            const int idx = tid + i * (LA_NW * 64);
            const int row = c * LA_KC + (idx >> 3), ch = idx & 7;
            const int rc = row < T ? row : T - 1;
            kv[i] = *(const uint4*)(base + (size_t)rc * ld + width + ch * 8);
            vv[i] = *(const uint4*)(base + (size_t)rc * ld + 2 * width + ch * 8);
        }
    };
    auto store_chunk = [&](int c, char* stage) {
        char* sK = stage;
        char* sV = stage + LA_KC * 128;
#pragma unroll
        for (int i = 0; i < LA_NCH; ++i) {
            const int idx = tid + i * (LA_NW * 64);
            const int row = idx >> 3, ch = idx & 7;
            const unsigned keep = c * LA_KC + row < T ? 0xffffffffu : 0u;
            uint4 a = kv[i], v = vv[i];
            a.x &= keep; a.y &= keep; a.z &= keep; a.w &= keep;
            v.x &= keep; v.y &= keep; v.z &= keep; v.w &= keep;
            *(uint4*)(sK + row * 128 + ((ch ^ ((row >> 1) & 7)) << 4)) = a;
            *(uint4*)(sV + row * 128 + ((ch ^ (((row >> 1) & 3) << 1)) << 4)) = v;
        }
    };

    load_chunk(0);
    store_chunk(0, smem);
    __syncthreads();

    f32x4 o[LA_QT][4];
    float ml[LA_QT], l[LA_QT];                         // running max (times log2 e) and the lane's partial row sum
#pragma unroll
    for (int i = 0; i < LA_QT; ++i) {
        ml[i] = -INFINITY;
        l[i] = 0.f;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) o[i][dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    }

    for (int c = 0; c < nch; ++c) {
        const bool more = c + 1 < nch;
        if (more) load_chunk(c + 1);                   // in flight while this chunk is computed
        const char* sK = smem + (c & 1) * LA_STAGE;
        const char* sV = sK + LA_KC * 128;
        const int k0 = c * LA_KC;
        const bool tail = k0 + LA_KC > T;              // the ragged last chunk: masks, dead tiles skipped (uniform)

        // S^T tiles: s[i][t][r] = S[query of tile i, lrow][key k0 + 16 t + 4 lq + r]
        f32x4 s[LA_QT][LA_NT16];
        bf16x8 kf[LA_NT16][2];
#pragma unroll
        for (int t = 0; t < LA_NT16; ++t)
#pragma unroll
            for (int kk = 0; kk < 2; ++kk)
                kf[t][kk] = *(const bf16x8*)(sK + (t * 16 + lrow) * 128 + (((kk * 4 + lq) ^ (lrow >> 1)) << 4));
#pragma unroll
        for (int t = 0; t < LA_NT16; ++t)
#pragma unroll
            for (int i = 0; i < LA_QT; ++i) {
                s[i][t] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (!tail || k0 + t * 16 < T) {
                    s[i][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[t][0], qf[i][0], s[i][t], 0, 0, 0);
                    s[i][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[t][1], qf[i][1], s[i][t], 0, 0, 0);
                }
            }

        // V^T fragments of the chunk's two 32-key blocks, issued before the softmax so that their latency hides behind it
        bf16x8 vf[LA_NU][4];
#pragma unroll
        for (int u = 0; u < LA_NU; ++u) {
            const int ra = u * 32 + lq * 4 + (lrow >> 2);
            const int rb = ra + 16;
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) {
                const int cc = dt * 2 + ((lrow & 3) >> 1);
                const bf16x4 va = lds_read_tr16_l(sV + ra * 128 + ((cc ^ (((ra >> 1) & 3) << 1)) << 4) + (lrow & 1) * 8);
                const bf16x4 vb = lds_read_tr16_l(sV + rb * 128 + ((cc ^ (((rb >> 1) & 3) << 1)) << 4) + (lrow & 1) * 8);
                vf[u][dt][0] = va[0]; vf[u][dt][1] = va[1]; vf[u][dt][2] = va[2]; vf[u][dt][3] = va[3];
                vf[u][dt][4] = vb[0]; vf[u][dt][5] = vb[1]; vf[u][dt][6] = vb[2]; vf[u][dt][7] = vb[3];
            }
        }

        // online softmax per query tile
#pragma unroll
        for (int i = 0; i < LA_QT; ++i) {
            if (tail) {
#pragma unroll
                for (int t = 0; t < LA_NT16; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        s[i][t][r] = k0 + t * 16 + lq * 4 + r < T ? s[i][t][r] : -INFINITY;
            }
            float mx = -INFINITY;
#pragma unroll
            for (int t = 0; t < LA_NT16; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) mx = fmaxf(mx, s[i][t][r]);
            mx = fmaxf(mx, __shfl_xor(mx, 16));
            mx = fmaxf(mx, __shfl_xor(mx, 32));
            const float mnew = fmaxf(ml[i], mx * LOG2E);
            const float alpha = __builtin_amdgcn_exp2f(ml[i] - mnew);     // 0 on the first chunk (-inf), 1 when the max stays
            ml[i] = mnew;
            f32x2_t sum2 = {0.f, 0.f};
            const f32x2_t l2 = {LOG2E, LOG2E}, nm = {-mnew, -mnew};
#pragma unroll
            for (int t = 0; t < LA_NT16; ++t) {
                f32x2_t a = f32x2_t{s[i][t][0], s[i][t][1]} * l2 + nm, e = f32x2_t{s[i][t][2], s[i][t][3]} * l2 + nm;
                a.x = __builtin_amdgcn_exp2f(a.x); a.y = __builtin_amdgcn_exp2f(a.y);
                e.x = __builtin_amdgcn_exp2f(e.x); e.y = __builtin_amdgcn_exp2f(e.y);
                s[i][t][0] = a.x; s[i][t][1] = a.y; s[i][t][2] = e.x; s[i][t][3] = e.y;
                sum2 += a;
                sum2 += e;
            }
            l[i] = l[i] * alpha + (sum2.x + sum2.y);
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) o[i][dt] *= alpha;
        }

        // O^T += V^T . P^T per 32-key block (a block of pad keys only has P = 0 and is skipped)
#pragma unroll
        for (int u = 0; u < LA_NU; ++u) {
            if (tail && k0 + u * 32 >= T) continue;
#pragma unroll
            for (int i = 0; i < LA_QT; ++i) {
                union { bf16x8 v; uint32_t w[4]; } pf;
                pf.w[0] = pack_bf16x2(s[i][2 * u][0], s[i][2 * u][1]);
                pf.w[1] = pack_bf16x2(s[i][2 * u][2], s[i][2 * u][3]);
                pf.w[2] = pack_bf16x2(s[i][2 * u + 1][0], s[i][2 * u + 1][1]);
                pf.w[3] = pack_bf16x2(s[i][2 * u + 1][2], s[i][2 * u + 1][3]);
#pragma unroll
                for (int dt = 0; dt < 4; ++dt)
                    o[i][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf[u][dt], pf.v, o[i][dt], 0, 0, 0);
            }
        }

        if (more) store_chunk(c + 1, smem + ((c + 1) & 1) * LA_STAGE);   // that buffer was last read before the previous barrier
        __syncthreads();
    }

    // o[i][dt][r] = O[query lrow of tile i][d = 16 dt + 4 lq + r]
#pragma unroll
    for (int i = 0; i < LA_QT; ++i) {
        float sum = l[i];
        sum += __shfl_xor(sum, 16);
        sum += __shfl_xor(sum, 32);
        const int q = qb * LA_QB + i * (LA_NW * 16) + wid * 16 + lrow;
        if (q < T) {
            const float inv = 1.0f / sum;
            bf16_t* dst = out + ((size_t)b * T + q) * width + h * 64 + lq * 4;
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) {
                uint2 pk;
                pk.x = pack_bf16x2(o[i][dt][0] * inv, o[i][dt][1] * inv);
                pk.y = pack_bf16x2(o[i][dt][2] * inv, o[i][dt][3] * inv);
                *(uint2*)(dst + dt * 16) = pk;
            }
        }
    }
}

int launch_attention_long(const bf16_t* qkv, bf16_t* out, int batch, int t, int width, hipStream_t stream) {
    if (batch <= 0) return KEMR_OK;
    if (width % 64 != 0 || t <= 0 || t > KEMR_MAX_VISION_TOKENS)
        KEMR_FAIL(KEMR_ERR_INVALID, "attention: sequence length %d not in 1..%d (non-causal)", t, KEMR_MAX_VISION_TOKENS);
    const int nqb = (t + LA_QB - 1) / LA_QB;
    const long long items = (long long)batch * (width / 64) * nqb;
    if (items > 0x7ffffff0LL) KEMR_FAIL(KEMR_ERR_INVALID, "attention: batch %d too large", batch);
    const long long blocks = (items + 7) / 8 * 8;
    ProfScope prof(PROF_ATTENTION, stream);
    hipLaunchKernelGGL(attention_long_kernel, dim3((unsigned)blocks), dim3(LA_NW * 64), 0, stream, qkv, out, t, width, nqb, (int)items);
    KEMR_CHECK_LAUNCH("attention_long_kernel");
    return KEMR_OK;
}

}  // namespace kemr
