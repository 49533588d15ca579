// Streaming backward of the non-causal multi-head self-attention (head dim 64), any t <= KEMR_MAX_VISION_TOKENS:
// kemr_op_attention_backward_long.  attention_bwd.hip keeps a head's Q, K, V and dO in LDS for the whole kernel (147 KB at 288 rows)
// and ends there; here nothing but 64-row chunks is ever in LDS, so the sequence length is bounded by nothing in the kernels.
//
//   qkv   bf16 [batch * t, 3 width]  q | k | v as the forward reads them (q already scaled by 1/8)
//   dout  bf16 [batch * t, width]    gradient of the forward's output
//   dqkv  bf16 [batch * t, 3 width]  gradient with respect to the three planes AS GIVEN (the caller owns the 1/8 of q)
//   stats fp32 [batch * heads * t, 3] the workspace: max * log2e, 1 / sum and D of every query row of every head
//
// The forward saves nothing.  The mathematics is attention_bwd.hip's: S = q k^T, P = softmax(S), dP = dO v^T, D_i = sum_j P_ij dP_ij,
// dS = P o (dP - D), dq = dS k, dk = dS^T q, dv = P^T dO.  Two kernels on the caller's stream, each a workgroup of four waves per
// (item, head, block of 64 rows), each wave owning one 16-row tile whose fragments stay in registers while the other side streams
// through LDS in 64-row chunks, double-buffered with one barrier per chunk as in attention_stream.hip:
//   QUERY-OWNED (attention_bwd_q_kernel): a wave owns 16 queries (Q and dO fragments in registers); K and V stream, twice.
//     sweep 1: S^T = K . Q^T and dP^T = V . dO^T per chunk (a lane holds 4 consecutive keys of ONE query), the online maximum m, the
//       row sum l and the unnormalised a = sum_j e^(s_j - m) dP_j in fp32; for every chunk m' = max(m, chunk max) and l, a are scaled
//       by exp(m - m') (exactly 1 when the maximum did not move), as the forward scales l and O.  Then 1 / l and D = a / l.
//     sweep 2: S^T and dP^T again, P from the FINAL m and 1 / l, dS = P o (dP - D), dQ^T += K^T . dS^T (K^T by ds_read_b64_tr_b16, the
//       dS registers rounded to bf16 in place).  It writes dq and the three statistics of its rows.
//   KEY-OWNED (attention_bwd_kv_kernel): a wave owns 16 keys (K and V fragments in registers); Q and dO stream once, each chunk with
//     the 64 x 3 statistics of its queries.  S = Q . K^T and dP = dO . V^T (a lane holds 4 consecutive queries of ONE key), P from the
//     saved statistics by the same expression as in sweep 2, dV^T += dO^T . P and dK^T += Q^T . dS (both by transposed reads).
// 9 score-sized products (S and dP three times each, then dQ, dK, dV) against the 7 of the LDS kernel and the minimum of 5: the
// price of saving nothing in the forward and owning every output.  No atomics: every element of dqkv and of the workspace has one
// owner and one fixed summation order (chunks in ascending order, the MFMA's own order inside), so two launches give the same bits.
// The LDS layout and the MFMA operand forms are attention_tile.h's, the backward's tile steps and rounding points attention_bwd_tile.h's,
// shared with attention_bwd.hip; D comes from the unrounded fp32 P.
// Memory: staging loads and fragment loads clamp their row to the item's last one, pad rows are zeroed at the LDS write and masked (pad
// keys to -inf in sweep 1, P = 0 elsewhere), tiles made only of pad rows are skipped (wave-uniform, never a barrier: EXEC is full at
// every transposed read), rows >= t are not stored: exactly batch * t rows of dqkv and batch * heads * t rows of the workspace are
// written, and nothing outside an item's rows of qkv and dout can reach its rows of dqkv.  The key-owned kernel reads only workspace
// rows the query-owned kernel of the same call wrote.
// LDS images: K (query-owned), Q and dO (key-owned) are read by rows AND transposed (Img64<true>), V is only read by rows; a chunk is
// addressed by its local rows.  32 KB (query-owned) / 33.5 KB (key-owned) of LDS per workgroup.
// Measured on an MI355X (the op alone, width 1024, medians of alternating windows; DESIGN.md "Streaming attention backward"): one tile
// per wave at 3 waves per SIMD, as here, 0.437 ms at batch 32 x 577 tokens and 1.177 ms at 32 x 1025; at 2 waves per SIMD 0.441 / 1.237;
// two tiles per wave (128-row blocks, half the chunk traffic, 198 VGPRs) 0.534 / 1.622, so blocks of 64 rows it is.  The three
// variants gave the same bits.
#include "attention_bwd_tile.h"

namespace kemr {

namespace {

constexpr int NW = 4;                       // waves per workgroup
constexpr int OCC = 3;                      // waves per SIMD asked of the register allocator (150 / 146 VGPRs, no scratch)
constexpr int RB = NW * 16;                 // rows a workgroup owns
constexpr int RC = 64;                      // rows per LDS chunk
constexpr int IMG = RC * 128;               // bytes of one chunk image
constexpr int NCH = RC * 8 / (NW * 64);     // 16-byte pieces of one image per thread and chunk
constexpr int STAGE_Q = 2 * IMG;            // query-owned: K | V
constexpr int STAGE_KV = 2 * IMG + RC * 3 * 4;      // key-owned: Q | dO | the chunk's statistics [3][64]

}  // namespace

// Work item = blockIdx.x: row block fastest, then head, then item.
__global__ __launch_bounds__(NW * 64, OCC) void attention_bwd_q_kernel(const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ dout,
                                                                  bf16_t* __restrict__ dqkv, float* __restrict__ stats, int T, int width,
                                                                  int heads, int nrb) {
    __shared__ __attribute__((aligned(16))) char smem[2 * STAGE_Q];
    const int id = (int)blockIdx.x;
    const int qb = id % nrb, bh = id / nrb;
    const int h = bh % heads, b = bh / heads;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lrow = lane & 15, lq = lane >> 4;
    const size_t ld = 3 * (size_t)width, row0 = (size_t)b * T;
    const bf16_t* base = qkv + row0 * ld + h * 64;
    const bf16_t* gbase = dout + row0 * width + h * 64;
    const int nch = (T + RC - 1) / RC;

    // the wave's query tile (B operands of S^T = K . Q^T and dP^T = V . dO^T): rows clamped to the item's last one
    const int q = qb * RB + wid * 16 + lrow;
    const int qc = q < T ? q : T - 1;
    bf16x8 qf[2], gf[2];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
        qf[kk] = *(const bf16x8*)(base + (size_t)qc * ld + kk * 32 + lq * 8);
        gf[kk] = *(const bf16x8*)(gbase + (size_t)qc * width + kk * 32 + lq * 8);
    }

    uint4 kv[NCH], vv[NCH];
    auto load_chunk = [&](int c) {
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
            const int idx = tid + i * (NW * 64);
            const int row = c * RC + (idx >> 3), ch = idx & 7;
            const int rc = row < T ? row : T - 1;
            kv[i] = *(const uint4*)(base + (size_t)rc * ld + width + ch * 8);
            vv[i] = *(const uint4*)(base + (size_t)rc * ld + 2 * width + ch * 8);
        }
    };
    auto store_chunk = [&](int c, char* stage) {
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
            const int idx = tid + i * (NW * 64);
            const int row = idx >> 3, ch = idx & 7;
            const bool valid = c * RC + row < T;
            tile_put<Img64<true>>(stage, row, ch, kv[i], valid);
            tile_put<Img64<false>>(stage + IMG, row, ch, vv[i], valid);
        }
    };

    load_chunk(0);
    store_chunk(0, smem);
    __syncthreads();

    float ml = -INFINITY, l = 0.f, a = 0.f;             // running max * log2e; the lane's partial row sum and sum of e dP
    float inv = 0.f, dd = 0.f;                          // after sweep 1: 1 / l and D
    f32x4 dq[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) dq[dt] = f32x4{0.f, 0.f, 0.f, 0.f};

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
            if (k0 + t * 16 < T) bwd_scores<false>(sK, sV, t * 16 + lrow, lq, qf, gf, s[t], dp[t]);
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
                bf16x8 af[4];
                bwd_accum(sK, u, lrow, lq, dp[2 * u], dp[2 * u + 1], af, dq);
            }
        }

        if (more) store_chunk(cn, smem + ((cc + 1) & 1) * STAGE_Q);     // that buffer was last read before the previous barrier
        __syncthreads();
    }

    // dq[dt][r] = dQ[query lrow of the tile][d = 16 dt + 4 lq + r]
    if (q < T) tile_store(dqkv + (row0 + q) * ld + h * 64 + lq * 4, dq);
}

__global__ __launch_bounds__(NW * 64, OCC) void attention_bwd_kv_kernel(const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ dout,
                                                                   bf16_t* __restrict__ dqkv, const float* __restrict__ stats, int T,
                                                                   int width, int heads, int nrb) {
    __shared__ __attribute__((aligned(16))) char smem[2 * STAGE_KV];
    const int id = (int)blockIdx.x;
    const int kb = id % nrb, bh = id / nrb;
    const int h = bh % heads, b = bh / heads;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lrow = lane & 15, lq = lane >> 4;
    const size_t ld = 3 * (size_t)width, row0 = (size_t)b * T;
    const bf16_t* base = qkv + row0 * ld + h * 64;
    const bf16_t* gbase = dout + row0 * width + h * 64;
    const float* sbase = stats + (size_t)bh * T * 3;
    const int nch = (T + RC - 1) / RC;

    // the wave's key tile (B operands of S = Q . K^T and dP = dO . V^T): rows clamped to the item's last one
    const int k = kb * RB + wid * 16 + lrow;
    const int kc = k < T ? k : T - 1;
    bf16x8 kf[2], vf[2];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
        kf[kk] = *(const bf16x8*)(base + (size_t)kc * ld + width + kk * 32 + lq * 8);
        vf[kk] = *(const bf16x8*)(base + (size_t)kc * ld + 2 * width + kk * 32 + lq * 8);
    }

    // chunk staging: Q and dO pieces, and for the first 192 threads one of the chunk's 64 x 3 statistics (rows clamped as well: a pad
    // query gets the last query's finite values and P = 0 by the mask)
    uint4 qv[NCH], gv[NCH];
    float sv = 0.f;
    const int srow = tid / 3, scomp = tid - srow * 3;
    auto load_chunk = [&](int c) {
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
            const int idx = tid + i * (NW * 64);
            const int row = c * RC + (idx >> 3), ch = idx & 7;
            const int rc = row < T ? row : T - 1;
            qv[i] = *(const uint4*)(base + (size_t)rc * ld + ch * 8);
            gv[i] = *(const uint4*)(gbase + (size_t)rc * width + ch * 8);
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
            const int row = idx >> 3, ch = idx & 7;
            const bool valid = c * RC + row < T;
            tile_put<Img64<true>>(stage, row, ch, qv[i], valid);
            tile_put<Img64<true>>(stage + IMG, row, ch, gv[i], valid);
        }
        if (tid < RC * 3) ((float*)(stage + 2 * IMG))[scomp * RC + srow] = sv;
    };

    load_chunk(0);
    store_chunk(0, smem);
    __syncthreads();

    f32x4 dk[4], dv[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) { dk[dt] = f32x4{0.f, 0.f, 0.f, 0.f}; dv[dt] = f32x4{0.f, 0.f, 0.f, 0.f}; }

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
                bwd_scores<true>(sQ, sG, t * 16 + lrow, lq, kf, vf, s[t], dp[t]);
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
            bf16x8 af[4];
            bwd_accum(sQ, u, lrow, lq, dp[2 * u], dp[2 * u + 1], af, dk);   // Q^T . dS
            bwd_accum(sG, u, lrow, lq, s[2 * u], s[2 * u + 1], af, dv);     // dO^T . P
        }

        if (more) store_chunk(c + 1, smem + ((c + 1) & 1) * STAGE_KV);      // that buffer was last read before the previous barrier
        __syncthreads();
    }

    // dk[dt][r] / dv[dt][r] = d(key lrow of the tile)[d = 16 dt + 4 lq + r]
    if (k < T) {
        bf16_t* p = dqkv + (row0 + k) * ld + h * 64 + lq * 4;
        tile_store(p + width, dk);
        tile_store(p + 2 * width, dv);
    }
}

}  // namespace kemr

using namespace kemr;

extern "C" size_t kemr_attention_backward_long_workspace_bytes(int batch, int t, int width) {
    if (batch <= 0 || t < 1 || t > KEMR_MAX_VISION_TOKENS || width <= 0 || width % 64 != 0) return 0;
    return (size_t)batch * (size_t)(width / 64) * (size_t)t * 3 * sizeof(float);
}

extern "C" int kemr_op_attention_backward_long(const void* qkv_dev, const void* dout_dev, void* dqkv_dev, int batch, int t, int width,
                                               void* workspace_dev, size_t workspace_bytes, void* stream) {
    // everything is refused here, on the host, before any HIP call (non-causal: causal = 0)
    KEMR_TRY(bwd_refuse("op_attention_backward_long", qkv_dev, dout_dev, dqkv_dev, nullptr, "t", t, KEMR_MAX_VISION_TOKENS, width, 0, batch));
    const int heads = width / 64, nrb = (t + RB - 1) / RB;
    const long long blocks = (long long)batch * heads * nrb;
    if (blocks > 0x7fffffffLL)
        KEMR_FAIL(KEMR_ERR_INVALID, "op_attention_backward_long: batch = %d x %d heads x %d row blocks exceeds the grid (2^31 - 1 workgroups)",
                  batch, heads, nrb);
    const size_t need = kemr_attention_backward_long_workspace_bytes(batch, t, width);
    if (need && !workspace_dev) KEMR_FAIL(KEMR_ERR_INVALID, "op_attention_backward_long: workspace is NULL");
    if (workspace_bytes < need)
        KEMR_FAIL(KEMR_ERR_INVALID, "op_attention_backward_long: workspace_bytes = %zu, %zu needed (kemr_attention_backward_long_workspace_bytes)",
                  workspace_bytes, need);
    if ((uintptr_t)workspace_dev & 3) KEMR_FAIL(KEMR_ERR_INVALID, "op_attention_backward_long: workspace must be 4-byte aligned");
    if (batch == 0) return KEMR_OK;
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(PROF_ATTENTION, s);
    hipLaunchKernelGGL(attention_bwd_q_kernel, dim3((unsigned)blocks), dim3(NW * 64), 0, s, (const bf16_t*)qkv_dev, (const bf16_t*)dout_dev,
                       (bf16_t*)dqkv_dev, (float*)workspace_dev, t, width, heads, nrb);
    KEMR_CHECK_LAUNCH("attention_bwd_q_kernel");
    hipLaunchKernelGGL(attention_bwd_kv_kernel, dim3((unsigned)blocks), dim3(NW * 64), 0, s, (const bf16_t*)qkv_dev, (const bf16_t*)dout_dev,
                       (bf16_t*)dqkv_dev, (const float*)workspace_dev, t, width, heads, nrb);
    KEMR_CHECK_LAUNCH("attention_bwd_kv_kernel");
    return KEMR_OK;
}
