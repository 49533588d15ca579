// Backward of the non-causal multi-head self-attention at head dim 80 (the vision tower of ViT-H-14: width 1280 = 16 heads of 80, 257
// tokens), any 1 <= t <= KEMR_MAX_VISION_TOKENS: kemr_op_attention_backward_hd.  The head-dim-80 form of attention_bwd_stream.hip, whose
// header states the mathematics, the ownership and the rounding points; that file, attention_bwd.hip and attention80.hip are not
// touched and their kernels keep their code and bits (attention80.hip records what a shared <HD> template cost).
//
//   qkv   bf16 [batch * t, 3 width]  q | k | v as kemr_op_attention_hd reads them (q already scaled by 1/sqrt(80))
//   dout  bf16 [batch * t, width]    gradient of the forward's output
//   dqkv  bf16 [batch * t, 3 width]  gradient with respect to the three planes AS GIVEN (the caller owns the 1/sqrt(80) of q)
//   stats fp32 [batch * heads * t, 3] the workspace: max * log2e, 1 / sum and D of every query row of every head, heads = width / 80
//
// Why streaming and nothing else: the whole-head-in-LDS kernel of attention_bwd.hip would need four images of TP x 160 B, 184 320 B at
// the 257 tokens (TP = 288) of the one model this is for -- more than the 160 KiB of a CU.  One route, two kernels, for every t:
//   QUERY-OWNED (attention_bwd80_q_kernel): a wave owns 16 queries (Q and dO fragments in registers); K and V stream through LDS in
//     64-row chunks, twice.  Sweep 1 keeps the online maximum, the row sum and a = sum e dP in fp32; sweep 2 takes P from the final
//     statistics, dS = P o (dP - D) and dQ^T += K^T . dS^T.  It writes dq and the three statistics of its rows.
//   KEY-OWNED (attention_bwd80_kv_kernel): a wave owns 16 keys; Q, dO and the chunk's statistics stream once; dV^T += dO^T . P and
//     dK^T += Q^T . dS.
// No atomics: every element of dqkv and of the workspace has one owner and one fixed summation order (chunks ascending, the MFMA's own
// order inside), so two launches give the same bits.  The forward saves nothing.
// Images: every chunk image is an Img80 (attention_tile.h): rows of exactly 160 B, no swizzle -- its comment shows that the row reads
// and the transposed reads are both conflict-free at that pitch.  K (query-owned), Q and dO (key-owned) are read by rows AND
// transposed, V by rows only.  The contraction over 80 is attention80.hip's: two K = 32 steps and a third whose k slots 16..31 are zero
// in both operands (own tile: cleared in registers, bwd_own80; streamed side: the lanes lq >= 2 read ONE 16-byte chunk of zeros kept
// behind the stages).  Nothing beyond column 79 of a head is ever loaded: columns 80..95 are the next head, the next plane, or memory
// past the allocation.  The second products have 5 d-tiles.
// Staging: a 64-row chunk of one image is 640 16-byte pieces = 2.5 per thread, so the third round belongs to the waves 0 and 1 only
// (idx < 640: wave-uniform).  Pad rows clamp their load to the item's last row and are zeroed at the LDS write, tiles made only of pad
// rows are skipped with wave-uniform tests (EXEC is full at every transposed read), rows >= t are never stored: exactly batch * t rows of
// dqkv and batch * heads * t rows of the workspace are written.
// LDS: 2 x (2 x 10 240) + 16 = 40 976 B (query-owned), 2 x (2 x 10 240 + 768) + 16 = 42 512 B (key-owned): room for three workgroups per
// CU; the registers (OCC, below) hold two.
// Registers, LDS, waves per SIMD and the measured times: DESIGN.md "Head-dim-80 attention backward".
#include "attention_bwd_tile.h"

namespace kemr {

namespace {

constexpr int HD = 80;                      // head dim
constexpr int RCH = HD / 8;                 // 16-byte pieces of a row
constexpr int NW = 4;                       // waves per workgroup
constexpr int OCC = 2;                      // waves per SIMD asked of the register allocator: 186 / 190 VGPRs, no scratch (at 3 the
                                            // 168-VGPR budget spilled 12 / 20 bytes per lane to scratch, which this op may not use)
constexpr int RB = NW * 16;                 // rows a workgroup owns
constexpr int RC = 64;                      // rows per LDS chunk
constexpr int IMG = RC * Img80::ROWB;       // bytes of one chunk image
constexpr int NP = RC * RCH;                // 16-byte pieces of one chunk image: 640
constexpr int NCH = (NP + NW * 64 - 1) / (NW * 64);     // staging rounds: 3, the last one for idx < NP only
constexpr int STAGE_Q = 2 * IMG;            // query-owned: K | V
constexpr int STAGE_KV = 2 * IMG + RC * 3 * 4;      // key-owned: Q | dO | the chunk's statistics [3][64]

}  // namespace

// Work item = blockIdx.x: row block fastest, then head, then item.
__global__ __launch_bounds__(NW * 64, OCC) void attention_bwd80_q_kernel(const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ dout,
                                                                    bf16_t* __restrict__ dqkv, float* __restrict__ stats, int T,
                                                                    int width, int heads, int nrb) {
    __shared__ __attribute__((aligned(16))) char smem[2 * STAGE_Q + Img80::ZERO];
    const char* sZ = smem + 2 * STAGE_Q;                // 16 bytes of zeros: the streamed operand of the k slots 16..31 of the third step
    const int id = (int)blockIdx.x;
    const int qb = id % nrb, bh = id / nrb;
    const int h = bh % heads, b = bh / heads;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lrow = lane & 15, lq = lane >> 4;
    const size_t ld = 3 * (size_t)width, row0 = (size_t)b * T;
    const bf16_t* base = qkv + row0 * ld + h * HD;
    const bf16_t* gbase = dout + row0 * width + h * HD;
    const int nch = (T + RC - 1) / RC;

    // the wave's query tile (B operands of S^T = K . Q^T and dP^T = V . dO^T): rows clamped to the item's last one
    const int q = qb * RB + wid * 16 + lrow;
    const int qc = q < T ? q : T - 1;
    bf16x8 qf[3], gf[3];
    bwd_own80(base + (size_t)qc * ld, lq, qf);
    bwd_own80(gbase + (size_t)qc * width, lq, gf);
    if (tid == 0) *(uint4*)(smem + 2 * STAGE_Q) = make_uint4(0u, 0u, 0u, 0u);

    uint4 kv[NCH], vv[NCH];
    auto load_chunk = [&](int c) {
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
            const int idx = tid + i * (NW * 64);
            if (idx < NP) {                             // (the third round: waves 0 and 1)
                const int lr = idx / RCH, ch = idx - lr * RCH;
                const int row = c * RC + lr;
                const int rc = row < T ? row : T - 1;
                kv[i] = *(const uint4*)(base + (size_t)rc * ld + width + ch * 8);
                vv[i] = *(const uint4*)(base + (size_t)rc * ld + 2 * width + ch * 8);
            }
        }
    };
    auto store_chunk = [&](int c, char* stage) {
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
            const int idx = tid + i * (NW * 64);
            if (idx < NP) {
                const int row = idx / RCH, ch = idx - row * RCH;
                const bool valid = c * RC + row < T;
                tile_put<Img80>(stage, row, ch, kv[i], valid);
                tile_put<Img80>(stage + IMG, row, ch, vv[i], valid);
            }
        }
    };

    load_chunk(0);
    store_chunk(0, smem);
    __syncthreads();

    float ml = -INFINITY, l = 0.f, a = 0.f;             // running max * log2e; the lane's partial row sum and sum of e dP
    float inv = 0.f, dd = 0.f;                          // after sweep 1: 1 / l and D
    f32x4 dq[5];
#pragma unroll
    for (int dt = 0; dt < 5; ++dt) dq[dt] = f32x4{0.f, 0.f, 0.f, 0.f};

    // 2 nch steps: the chunks 0 .. nch - 1 for sweep 1, then again for sweep 2
    for (int cc = 0; cc < 2 * nch; ++cc) {
        const bool more = cc + 1 < 2 * nch;
        const int c = cc < nch ? cc : cc - nch;
        const int cn = cc + 1 < nch ? cc + 1 : cc + 1 - nch;
        if (more) load_chunk(cn);                       // in flight while this chunk is computed
        const char* sK = smem + (cc & 1) * STAGE_Q;
        const char* sV = sK + IMG;
        const int k0 = c * RC;

        if (cc == nch) {                                // between the sweeps (uniform): the row's sum and D
            l += __shfl_xor(l, 16);
            l += __shfl_xor(l, 32);
            a += __shfl_xor(a, 16);
            a += __shfl_xor(a, 32);
            inv = 1.0f / l;
            dd = a * inv;
            if (lq == 0 && q < T) {
                float* st = stats + ((size_t)bh * T + q) * 3;
                st[0] = ml; st[1] = inv; st[2] = dd;
            }
        }

        // s[t][r] / dp[t][r] belong to (query lrow of the tile, key k0 + 16 t + 4 lq + r); a tile of pad keys only is skipped (uniform)
        f32x4 s[4], dp[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            s[t] = f32x4{0.f, 0.f, 0.f, 0.f};
            dp[t] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (k0 + t * 16 < T) bwd_scores80(sK, sV, sZ, t * 16 + lrow, lq, qf, gf, s[t], dp[t]);
        }

        if (cc < nch) {
            // sweep 1.  Key k0 is a key of the item (k0 < T), so the chunk's maximum is finite; pad keys have dP = 0 (V rows zeroed)
            float mx = -INFINITY;
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    s[t][r] = k0 + t * 16 + lq * 4 + r < T ? s[t][r] : -INFINITY;
                    mx = fmaxf(mx, s[t][r]);
                }
            mx = fmaxf(mx, __shfl_xor(mx, 16));
            mx = fmaxf(mx, __shfl_xor(mx, 32));
            const float mnew = fmaxf(ml, mx * LOG2E);
            const float alpha = __builtin_amdgcn_exp2f(ml - mnew);      // 0 on the first chunk (-inf), 1 when the max stays
            ml = mnew;
            float sum = 0.f, acc = 0.f;
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float e = __builtin_amdgcn_exp2f(__builtin_fmaf(s[t][r], LOG2E, -mnew));      // masked: exp2(-inf) = 0
                    sum += e;
                    acc = __builtin_fmaf(e, dp[t][r], acc);
                }
            l = __builtin_fmaf(l, alpha, sum);
            a = __builtin_fmaf(a, alpha, acc);
        } else {
            // sweep 2: P from the final statistics, dS = P o (dP - D) in place of dP, dQ^T += K^T . dS^T
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float p = bwd_p(s[t][r], ml, inv, k0 + t * 16 + lq * 4 + r < T);
                    dp[t][r] = p * (dp[t][r] - dd);
                }
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                if (k0 + u * 32 >= T) continue;         // a block of pad keys only has dS = 0 (uniform)
                bf16x8 af[5];
                bwd_accum80(sK, u, lrow, lq, dp[2 * u], dp[2 * u + 1], af, dq);
            }
        }

        if (more) store_chunk(cn, smem + ((cc + 1) & 1) * STAGE_Q);     // that buffer was last read before the previous barrier
        __syncthreads();
    }

    // dq[dt][r] = dQ[query lrow of the tile][d = 16 dt + 4 lq + r]
    if (q < T) tile_store(dqkv + (row0 + q) * ld + h * HD + lq * 4, dq);
}

__global__ __launch_bounds__(NW * 64, OCC) void attention_bwd80_kv_kernel(const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ dout,
                                                                     bf16_t* __restrict__ dqkv, const float* __restrict__ stats, int T,
                                                                     int width, int heads, int nrb) {
    __shared__ __attribute__((aligned(16))) char smem[2 * STAGE_KV + Img80::ZERO];
    const char* sZ = smem + 2 * STAGE_KV;
    const int id = (int)blockIdx.x;
    const int kb = id % nrb, bh = id / nrb;
    const int h = bh % heads, b = bh / heads;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lrow = lane & 15, lq = lane >> 4;
    const size_t ld = 3 * (size_t)width, row0 = (size_t)b * T;
    const bf16_t* base = qkv + row0 * ld + h * HD;
    const bf16_t* gbase = dout + row0 * width + h * HD;
    const float* sbase = stats + (size_t)bh * T * 3;
    const int nch = (T + RC - 1) / RC;

    // the wave's key tile (B operands of S = Q . K^T and dP = dO . V^T): rows clamped to the item's last one
    const int k = kb * RB + wid * 16 + lrow;
    const int kc = k < T ? k : T - 1;
    bf16x8 kf[3], vf[3];
    bwd_own80(base + (size_t)kc * ld + width, lq, kf);
    bwd_own80(base + (size_t)kc * ld + 2 * width, lq, vf);
    if (tid == 0) *(uint4*)(smem + 2 * STAGE_KV) = make_uint4(0u, 0u, 0u, 0u);

    // chunk staging: Q and dO pieces, and for the first 192 threads one of the chunk's 64 x 3 statistics (rows clamped as well: a pad
    // query gets the last query's finite values and P = 0 by the mask)
    uint4 qv[NCH], gv[NCH];
    float sv = 0.f;
    const int srow = tid / 3, scomp = tid - srow * 3;
    auto load_chunk = [&](int c) {
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
            const int idx = tid + i * (NW * 64);
            if (idx < NP) {                             // (the third round: waves 0 and 1)
                const int lr = idx / RCH, ch = idx - lr * RCH;
                const int row = c * RC + lr;
                const int rc = row < T ? row : T - 1;
                qv[i] = *(const uint4*)(base + (size_t)rc * ld + ch * 8);
                gv[i] = *(const uint4*)(gbase + (size_t)rc * width + ch * 8);
            }
        }
        if (tid < RC * 3) {
            const int row = c * RC + srow;
            const int rc = row < T ? row : T - 1;
            sv = sbase[(size_t)rc * 3 + scomp];
        }
    };
    auto store_chunk = [&](int c, char* stage) {
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
            const int idx = tid + i * (NW * 64);
            if (idx < NP) {
                const int row = idx / RCH, ch = idx - row * RCH;
                const bool valid = c * RC + row < T;
                tile_put<Img80>(stage, row, ch, qv[i], valid);
                tile_put<Img80>(stage + IMG, row, ch, gv[i], valid);
            }
        }
        if (tid < RC * 3) ((float*)(stage + 2 * IMG))[scomp * RC + srow] = sv;
    };

    load_chunk(0);
    store_chunk(0, smem);
    __syncthreads();

    f32x4 dk[5], dv[5];
#pragma unroll
    for (int dt = 0; dt < 5; ++dt) { dk[dt] = f32x4{0.f, 0.f, 0.f, 0.f}; dv[dt] = f32x4{0.f, 0.f, 0.f, 0.f}; }

    for (int c = 0; c < nch; ++c) {
        const bool more = c + 1 < nch;
        if (more) load_chunk(c + 1);                    // in flight while this chunk is computed
        const char* sQ = smem + (c & 1) * STAGE_KV;
        const char* sG = sQ + IMG;
        const float* sS = (const float*)(sQ + 2 * IMG);
        const int q0 = c * RC;

        // s[t][r] / dp[t][r] belong to (key lrow of the tile, query q0 + 16 t + 4 lq + r); a tile of pad queries only is skipped (uniform)
        f32x4 s[4], dp[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            s[t] = f32x4{0.f, 0.f, 0.f, 0.f};
            dp[t] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (q0 + t * 16 < T) {
                bwd_scores80(sQ, sG, sZ, t * 16 + lrow, lq, kf, vf, s[t], dp[t]);
                const float4 m4 = *(const float4*)(sS + t * 16 + lq * 4);
                const float4 i4 = *(const float4*)(sS + RC + t * 16 + lq * 4);
                const float4 d4 = *(const float4*)(sS + 2 * RC + t * 16 + lq * 4);
                const float mm[4] = {m4.x, m4.y, m4.z, m4.w}, ii[4] = {i4.x, i4.y, i4.z, i4.w}, d[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float p = bwd_p(s[t][r], mm[r], ii[r], q0 + t * 16 + lq * 4 + r < T);
                    s[t][r] = p;
                    dp[t][r] = p * (dp[t][r] - d[r]);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            if (q0 + u * 32 >= T) continue;             // a block of pad queries only has P = dS = 0 (uniform)
            bf16x8 af[5];
            bwd_accum80(sQ, u, lrow, lq, dp[2 * u], dp[2 * u + 1], af, dk);   // Q^T . dS
            bwd_accum80(sG, u, lrow, lq, s[2 * u], s[2 * u + 1], af, dv);     // dO^T . P
        }

        if (more) store_chunk(c + 1, smem + ((c + 1) & 1) * STAGE_KV);      // that buffer was last read before the previous barrier
        __syncthreads();
    }

    // dk[dt][r] / dv[dt][r] = d(key lrow of the tile)[d = 16 dt + 4 lq + r]
    if (k < T) {
        bf16_t* p = dqkv + (row0 + k) * ld + h * HD + lq * 4;
        tile_store(p + width, dk);
        tile_store(p + 2 * width, dv);
    }
}

}  // namespace kemr

using namespace kemr;

// head dim 64: what engine.attention_backward routes to -- no workspace up to KEMR_MAX_TEXT_CTX rows (and the causal op has none at
// all: the size cannot know causal, and a caller of the causal form may pass any workspace, it is ignored), the long op's above
extern "C" size_t kemr_attention_backward_hd_workspace_bytes(int batch, int t, int width, int head_dim) {
    if (head_dim == 64) return t <= KEMR_MAX_TEXT_CTX ? 0 : kemr_attention_backward_long_workspace_bytes(batch, t, width);
    if (head_dim != HD || batch <= 0 || t < 1 || t > KEMR_MAX_VISION_TOKENS || width <= 0 || width % HD != 0) return 0;
    return (size_t)batch * (size_t)(width / HD) * (size_t)t * 3 * sizeof(float);
}

extern "C" int kemr_op_attention_backward_hd(const void* qkv_dev, const void* dout_dev, void* dqkv_dev, int batch, int t, int width,
                                             int head_dim, int causal, void* workspace_dev, size_t workspace_bytes, void* stream) {
    // everything is refused here, on the host, before any HIP call
    if (head_dim != 64 && head_dim != HD)
        KEMR_FAIL(KEMR_ERR_INVALID, "op_attention_backward_hd: head_dim = %d is neither 64 nor 80", head_dim);
    if (head_dim == 64) {                               // the two ops of heads of 64, with their bits, refusals and messages
        if (causal || t <= KEMR_MAX_TEXT_CTX) return kemr_op_attention_backward(qkv_dev, dout_dev, dqkv_dev, batch, t, width, causal, stream);
        return kemr_op_attention_backward_long(qkv_dev, dout_dev, dqkv_dev, batch, t, width, workspace_dev, workspace_bytes, stream);
    }
    KEMR_TRY(bwd_refuse_hd("op_attention_backward_hd", qkv_dev, dout_dev, dqkv_dev, t, KEMR_MAX_VISION_TOKENS, width, HD, causal, batch));
    const int heads = width / HD, nrb = (t + RB - 1) / RB;
    const long long blocks = (long long)batch * heads * nrb;
    if (blocks > 0x7fffffffLL)
        KEMR_FAIL(KEMR_ERR_INVALID, "op_attention_backward_hd: batch = %d x %d heads x %d row blocks exceeds the grid (2^31 - 1 workgroups)",
                  batch, heads, nrb);
    const size_t need = kemr_attention_backward_hd_workspace_bytes(batch, t, width, HD);
    if (need && !workspace_dev) KEMR_FAIL(KEMR_ERR_INVALID, "op_attention_backward_hd: workspace is NULL");
    if (workspace_bytes < need)
        KEMR_FAIL(KEMR_ERR_INVALID, "op_attention_backward_hd: workspace_bytes = %zu, %zu needed (kemr_attention_backward_hd_workspace_bytes)",
                  workspace_bytes, need);
    if ((uintptr_t)workspace_dev & 3) KEMR_FAIL(KEMR_ERR_INVALID, "op_attention_backward_hd: workspace must be 4-byte aligned");
    if (batch == 0) return KEMR_OK;
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(PROF_ATTENTION, s);
    hipLaunchKernelGGL(attention_bwd80_q_kernel, dim3((unsigned)blocks), dim3(NW * 64), 0, s, (const bf16_t*)qkv_dev, (const bf16_t*)dout_dev,
                       (bf16_t*)dqkv_dev, (float*)workspace_dev, t, width, heads, nrb);
    KEMR_CHECK_LAUNCH("attention_bwd80_q_kernel");
    hipLaunchKernelGGL(attention_bwd80_kv_kernel, dim3((unsigned)blocks), dim3(NW * 64), 0, s, (const bf16_t*)qkv_dev, (const bf16_t*)dout_dev,
                       (bf16_t*)dqkv_dev, (const float*)workspace_dev, t, width, heads, nrb);
    KEMR_CHECK_LAUNCH("attention_bwd80_kv_kernel");
    return KEMR_OK;
}
