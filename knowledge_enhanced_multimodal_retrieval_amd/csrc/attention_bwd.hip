// Backward of the multi-head self-attention of attention.hip (head dim 64, t <= 288, causal or not): kemr_op_attention_backward, and
// kemr_op_attention_backward_packed, the same kernel over items of different lengths packed one behind the other (PACKED, below).
//
//   qkv  bf16 [batch * t, 3 width]  q | k | v as the forward reads them (q already scaled by 1/8)
//   dout bf16 [batch * t, width]    gradient of the forward's output
//   dqkv bf16 [batch * t, 3 width]  gradient with respect to the three planes AS GIVEN (the caller owns the 1/8 of q)
//
// The forward saves nothing, so everything is recomputed from qkv in fp32: S = q k^T, the row maximum and sum, P = softmax(S),
// dP = dO v^T, D_i = sum_j P_ij dP_ij (which equals dO_i . O_i, so no `out` argument is needed and the op is consistent with the P
// it uses), dS = P o (dP - D), then dq = dS k, dk = dS^T q, dv = P^T dO.
//
// One workgroup of four waves per (item, head).  The Q, K, V and dO tiles of the head (t padded to TP = a multiple of 32 rows, pad
// rows zero) sit in LDS for the whole kernel: 4 x TP x 128 B, 147 456 B at TP = 288, plus three fp32 per row (below).  Two phases,
// every element of dqkv owned by one wave and summed in one fixed order -- no atomics, the same bits on every launch:
//   phase 1, a wave owns 16-QUERY tiles: S^T = K . Q^T and dP^T = V . dO^T over all key tiles (A = K / V rows, B = the tile's Q / dO
//     rows; a lane holds 4 consecutive keys of ONE query, so row max, row sum and D are register sums and two shuffles), then
//     dQ^T = K^T . dS^T (A = K^T by ds_read_b64_tr_b16, B = the dS registers rounded to bf16 in place: the forward's PV product
//     with K for V and dS for P).  It leaves max * log2e, 1 / sum and D of its rows in LDS.
//   phase 2, a wave owns 16-KEY tiles: the same two products with the roles swapped, S = Q . K^T and dP = dO . V^T over all query
//     tiles (a lane holds 4 consecutive queries of ONE key), P from the saved row statistics by the same expression as in phase 1,
//     then dV^T = dO^T . P and dK^T = Q^T . dS (A = dO^T / Q^T by transposed reads, B = the P / dS registers).
// Both phases are one function (bwd_own_tile) with the operands exchanged.  S and dP are computed twice (7 products instead of 5):
// the price of owning every output without a workspace.  Causal: tiles wholly behind the diagonal are skipped in both phases.
// The LDS images and the MFMA operand forms are attention_tile.h's, the backward's tile steps and rounding points attention_bwd_tile.h's,
// shared with attention_bwd_stream.hip: Q, K and dO are read by rows AND transposed (Img64<true>), V is only read by rows.
#include "attention_bwd_tile.h"

#include <type_traits>

namespace kemr {

// PHASE 1: own = the 16 queries of tile ot, other = keys; PHASE 2: own = the 16 keys of tile ot, other = queries.
// Lane ownership of s[t][r] / dp[t][r] as attention_tile.h states it; every skip below is wave-uniform, so EXEC stays full.
template <int NT32, bool CAUSAL, int PHASE>
__device__ __forceinline__ void bwd_own_tile(const char* sQ, const char* sK, const char* sV, const char* sG, float* sM, float* sI,
                                             float* sD, int ot, int T, int lane, bf16_t* dst, size_t ld, int width) {
    constexpr int NT16 = NT32 * 2;
    const int lrow = lane & 15, lq = lane >> 4;
    const char* own1 = PHASE == 1 ? sQ : sK;
    const char* own2 = PHASE == 1 ? sG : sV;
    const char* oth1 = PHASE == 1 ? sK : sQ;
    const char* oth2 = PHASE == 1 ? sV : sG;
    const int o = ot * 16 + lrow;
    bf16x8 b1[2], b2[2];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
        b1[kk] = tile_row<Img64<true>>(own1, o, kk * 4 + lq);
        b2[kk] = tile_row<Img64<PHASE == 1>>(own2, o, kk * 4 + lq);
    }
    f32x4 s[NT16], dp[NT16];
#pragma unroll
    for (int t = 0; t < NT16; ++t) {
        s[t] = f32x4{0.f, 0.f, 0.f, 0.f};
        dp[t] = f32x4{0.f, 0.f, 0.f, 0.f};
        // tiles made only of pad rows, or (causal) wholly behind the diagonal, are skipped (uniform); the masks below cover them
        if (t * 16 < T && (!CAUSAL || (PHASE == 1 ? t <= ot : t >= ot)))
            bwd_scores<PHASE == 2>(oth1, oth2, t * 16 + lrow, lq, b1, b2, s[t], dp[t]);
    }
    if constexpr (PHASE == 1) {
        float mx = -INFINITY;
#pragma unroll
        for (int t = 0; t < NT16; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int x = t * 16 + lq * 4 + r;
                const bool ok = x < T && (!CAUSAL || x <= o);       // key 0 is always in: the maximum is finite
                s[t][r] = ok ? s[t][r] : -INFINITY;
                mx = fmaxf(mx, s[t][r]);
            }
        mx = fmaxf(mx, __shfl_xor(mx, 16));
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        const float m2 = mx * LOG2E;
        float sum = 0.f;
#pragma unroll
        for (int t = 0; t < NT16; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                s[t][r] = __builtin_amdgcn_exp2f(__builtin_fmaf(s[t][r], LOG2E, -m2));      // masked: exp2(-inf) = 0
                sum += s[t][r];
            }
        sum += __shfl_xor(sum, 16);
        sum += __shfl_xor(sum, 32);
        const float inv = 1.0f / sum;
        float dd = 0.f;
#pragma unroll
        for (int t = 0; t < NT16; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                s[t][r] *= inv;
                dd = __builtin_fmaf(s[t][r], dp[t][r], dd);
            }
        dd += __shfl_xor(dd, 16);
        dd += __shfl_xor(dd, 32);
#pragma unroll
        for (int t = 0; t < NT16; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) dp[t][r] = s[t][r] * (dp[t][r] - dd);
        if (lq == 0) { sM[o] = m2; sI[o] = inv; sD[o] = dd; }
    } else {
#pragma unroll
        for (int t = 0; t < NT16; ++t) {
            if (t * 16 < T && (!CAUSAL || t >= ot)) {
                const float4 m4 = *(const float4*)(sM + t * 16 + lq * 4);
                const float4 i4 = *(const float4*)(sI + t * 16 + lq * 4);
                const float4 d4 = *(const float4*)(sD + t * 16 + lq * 4);
                const float mm[4] = {m4.x, m4.y, m4.z, m4.w}, ii[4] = {i4.x, i4.y, i4.z, i4.w}, dd[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int x = t * 16 + lq * 4 + r;
                    const bool ok = x < T && (!CAUSAL || o <= x);
                    // bwd_p's expression, spelled out.  Through the call this kernel compiles differently (148 VGPRs at 64 rows for 140,
                    // 312 at 288 for 264) and measured 0.5 % slower than the previous commit's at 512 x 77 x 768 causal, outside the
                    // 0.02 % between two copies of that one; spelled out it is within it (profiles/attention_backward_refactor_ab.json)
                    const float p = ok ? __builtin_amdgcn_exp2f(__builtin_fmaf(s[t][r], LOG2E, -mm[r])) * ii[r] : 0.f;
                    s[t][r] = p;
                    dp[t][r] = p * (dp[t][r] - dd[r]);
                }
            }
        }
    }
    f32x4 acc1[4], acc2[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) { acc1[dt] = f32x4{0.f, 0.f, 0.f, 0.f}; acc2[dt] = f32x4{0.f, 0.f, 0.f, 0.f}; }
#pragma unroll
    for (int u = 0; u < NT32; ++u) {
        // a block of 32 other rows that is all pad, or (causal) all behind the diagonal, has P = dS = 0 and is skipped (uniform)
        if (!(u * 32 < T && (!CAUSAL || (PHASE == 1 ? u * 32 <= ot * 16 + 15 : u * 32 + 31 >= ot * 16)))) continue;
        bf16x8 a[4];
        bwd_accum(oth1, u, lrow, lq, dp[2 * u], dp[2 * u + 1], a, acc1);                            // K^T . dS^T (phase 1) / Q^T . dS (phase 2)
        if constexpr (PHASE == 2) bwd_accum(oth2, u, lrow, lq, s[2 * u], s[2 * u + 1], a, acc2);    // dO^T . P
    }
    // acc[dt][r] = d(own row lrow)[d = dt * 16 + lq * 4 + r]
    if (o < T) {
        bf16_t* p = dst + (size_t)o * ld + lq * 4;
        if constexpr (PHASE == 1) tile_store(p, acc1);                   // dq
        else { tile_store(p + width, acc1); tile_store(p + 2 * width, acc2); }    // dk, dv
    }
}

// PACKED: item b = rows row_start[b] .. row_start[b + 1] - 1 of the three buffers, cut at its first T (= max_t) rows; an empty item's
// workgroup leaves before any load.  NT32 comes from max_t, so an item shorter than NT32 * 32 rows runs in a larger instantiation than
// the dense op would give it: the tiles beyond its own padded length are skipped by the same wave-uniform tests that skip the pad tiles
// of the dense op (they add -inf to the maximum, exp2(-inf) = 0 to the sums, and no MFMA), and the order of the sums over the live
// tiles does not depend on NT32 -- an item has the bits of the dense op at batch = 1, t = its length.
template <int NT32, bool CAUSAL, bool PACKED>
__global__ __launch_bounds__(256) void attention_bwd_kernel(const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ dout,
                                                            bf16_t* __restrict__ dqkv, const int* __restrict__ row_start, int T, int width,
                                                            int heads) {
    constexpr int TP = NT32 * 32;
    constexpr int NTH = 256, NW = 4;
    constexpr int NCH = (TP * 8 + NTH - 1) / NTH;       // 16-byte chunks of one matrix per thread
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* sQ = smem;
    char* sK = smem + TP * 128;
    char* sV = smem + 2 * TP * 128;
    char* sG = smem + 3 * TP * 128;
    float* sM = (float*)(smem + 4 * TP * 128);
    float* sI = sM + TP;
    float* sD = sI + TP;

    const int b = blockIdx.x / heads, h = blockIdx.x - b * heads;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    size_t row0 = (size_t)b * T;
    if constexpr (PACKED) {
        const int first = row_start[b], len = row_start[b + 1] - first;
        T = len < T ? len : T;
        if (T <= 0) return;                             // an empty item: no load (the pad rows below clamp to row T - 1), no store
        row0 = (size_t)first;
    }
    const size_t ld = 3 * (size_t)width;
    const bf16_t* qbase = qkv + row0 * ld + h * 64;
    const bf16_t* gbase = dout + row0 * width + h * 64;

    // stage Q, K, V and dO: pad rows load the last valid row (branch-free) and are zeroed at the LDS write
#pragma unroll
    for (int mtx = 0; mtx < 4; ++mtx) {
        const bf16_t* src = mtx < 3 ? qbase + mtx * width : gbase;
        const size_t sld = mtx < 3 ? ld : (size_t)width;
        char* img = smem + mtx * TP * 128;
        auto put = [&](int idx, uint4 a) {              // piece idx of the matrix: chunk idx & 7 of row idx >> 3
            const int row = idx >> 3, c = idx & 7;
            if (mtx == 2) tile_put<Img64<false>>(img, row, c, a, row < T);
            else tile_put<Img64<true>>(img, row, c, a, row < T);
        };
        if constexpr (PACKED) {
            // the item's own padded length (a multiple of 32 rows, at most TP): no row beyond it is ever read.  32 rows are one chunk
            // per thread, so a thread stages ceil(T / 32) chunks: groups of four in flight, then the one to three that are left
            // (uniform counts, every load of a group issued before its first LDS write, no load that is not stored)
            const int nblk = (T + 31) >> 5;
            auto stage = [&](auto depth, int blk) {
                constexpr int M = decltype(depth)::value;
                uint4 v[M];
#pragma unroll
                for (int i = 0; i < M; ++i) {
                    const int idx = (blk + i) * NTH + tid;
                    const int row = idx >> 3, c = idx & 7;
                    const int rc = row < T ? row : T - 1;
                    v[i] = *(const uint4*)(src + (size_t)rc * sld + c * 8);
                }
#pragma unroll
                for (int i = 0; i < M; ++i) put((blk + i) * NTH + tid, v[i]);
            };
            int blk = 0;
            for (; blk + 4 <= nblk; blk += 4) stage(std::integral_constant<int, 4>{}, blk);
            switch (nblk - blk) {
                case 3: stage(std::integral_constant<int, 3>{}, blk); break;
                case 2: stage(std::integral_constant<int, 2>{}, blk); break;
                case 1: stage(std::integral_constant<int, 1>{}, blk); break;
            }
            continue;
        }
        uint4 v[NCH];
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
            const int idx = tid + i * NTH;
            const int row = idx >> 3, c = idx & 7;
            const int rc = row < T ? row : T - 1;
            v[i] = *(const uint4*)(src + (size_t)rc * sld + c * 8);
        }
#pragma unroll
        for (int i = 0; i < NCH; ++i)
            if (tid + i * NTH < TP * 8) put(tid + i * NTH, v[i]);
    }
    __syncthreads();
    const int nt = (T + 15) >> 4;
    bf16_t* dst = dqkv + row0 * ld + h * 64;
    for (int ot = wid; ot < nt; ot += NW)               // wave-uniform trip counts
        bwd_own_tile<NT32, CAUSAL, 1>(sQ, sK, sV, sG, sM, sI, sD, ot, T, lane, dst, ld, width);
    __syncthreads();                                    // the row statistics of every query tile
    for (int ot = wid; ot < nt; ot += NW)
        bwd_own_tile<NT32, CAUSAL, 2>(sQ, sK, sV, sG, sM, sI, sD, ot, T, lane, dst, ld, width);
}

// row_start == nullptr: the dense op (items of t rows one behind the other); otherwise the packed op, t = max_t
template <int NT32>
static int launch_bwd_nt(const bf16_t* qkv, const bf16_t* dout, bf16_t* dqkv, const int* row_start, int batch, int t, int width,
                         int causal, hipStream_t stream) {
    constexpr int smem = NT32 * 32 * (4 * 128 + 3 * 4);
    static_assert(smem <= 160 * 1024, "the head's four tiles and row statistics must fit the LDS of one CU");
    void (*kern)(const bf16_t*, const bf16_t*, bf16_t*, const int*, int, int, int) =
        row_start ? (causal ? attention_bwd_kernel<NT32, true, true> : attention_bwd_kernel<NT32, false, true>)
                  : (causal ? attention_bwd_kernel<NT32, true, false> : attention_bwd_kernel<NT32, false, false>);
    ProfScope prof(PROF_ATTENTION, stream);
    KEMR_CHECK_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, smem));
    const int heads = width / 64;
    hipLaunchKernelGGL(kern, dim3((unsigned)((long long)batch * heads)), dim3(256), smem, stream, qkv, dout, dqkv, row_start, t, width,
                       heads);
    KEMR_CHECK_LAUNCH("attention_bwd_kernel");
    return KEMR_OK;
}

static int launch_bwd(const bf16_t* qkv, const bf16_t* dout, bf16_t* dqkv, const int* row_start, int batch, int t, int width, int causal,
                      hipStream_t stream, const char* who) {
    if ((long long)batch * (width / 64) > 0x7fffffffLL)         // on the host, before any HIP call, as every refusal
        KEMR_FAIL(KEMR_ERR_INVALID, "%s: batch = %d x %d heads exceeds the grid (2^31 - 1 workgroups)", who, batch, width / 64);
    switch ((t + 31) / 32) {
        case 1: return launch_bwd_nt<1>(qkv, dout, dqkv, row_start, batch, t, width, causal, stream);
        case 2: return launch_bwd_nt<2>(qkv, dout, dqkv, row_start, batch, t, width, causal, stream);
        case 3: return launch_bwd_nt<3>(qkv, dout, dqkv, row_start, batch, t, width, causal, stream);
        case 4: return launch_bwd_nt<4>(qkv, dout, dqkv, row_start, batch, t, width, causal, stream);
        case 5: return launch_bwd_nt<5>(qkv, dout, dqkv, row_start, batch, t, width, causal, stream);
        case 6: return launch_bwd_nt<6>(qkv, dout, dqkv, row_start, batch, t, width, causal, stream);
        case 7: return launch_bwd_nt<7>(qkv, dout, dqkv, row_start, batch, t, width, causal, stream);
        case 8: return launch_bwd_nt<8>(qkv, dout, dqkv, row_start, batch, t, width, causal, stream);
        case 9: return launch_bwd_nt<9>(qkv, dout, dqkv, row_start, batch, t, width, causal, stream);
    }
    KEMR_FAIL(KEMR_ERR_INVALID, "%s: %s = %d is outside 1..%d", who, row_start ? "max_t" : "t", t, KEMR_MAX_TEXT_CTX);
}

// arguments checked by the caller (kemr_op_attention_backward): 1 <= t <= KEMR_MAX_TEXT_CTX, width % 64 == 0, batch >= 1
int launch_attention_backward(const bf16_t* qkv, const bf16_t* dout, bf16_t* dqkv, int batch, int t, int width, int causal, hipStream_t stream) {
    return launch_bwd(qkv, dout, dqkv, nullptr, batch, t, width, causal, stream, "op_attention_backward");
}

}  // namespace kemr

using namespace kemr;

extern "C" int kemr_op_attention_backward(const void* qkv_dev, const void* dout_dev, void* dqkv_dev, int batch, int t, int width,
                                          int causal, void* stream) {
    KEMR_TRY(bwd_refuse("op_attention_backward", qkv_dev, dout_dev, dqkv_dev, nullptr, "t", t, KEMR_MAX_TEXT_CTX, width, causal, batch));
    if (batch == 0) return KEMR_OK;                     // (the grid of an empty batch cannot be too large)
    return launch_attention_backward((const bf16_t*)qkv_dev, (const bf16_t*)dout_dev, (bf16_t*)dqkv_dev, batch, t, width, causal,
                                     (hipStream_t)stream);
}

// The packed form: item b = rows row_start[b] .. row_start[b + 1] - 1 (device array of batch + 1 ints), one workgroup per (item, head)
// in the instantiation of max_t.  See kemr.h.
extern "C" int kemr_op_attention_backward_packed(const void* qkv_dev, const void* dout_dev, void* dqkv_dev, const int* row_start_dev,
                                                 int batch, int max_t, int width, int causal, void* stream) {
    KEMR_TRY(bwd_refuse("op_attention_backward_packed", qkv_dev, dout_dev, dqkv_dev, &row_start_dev, "max_t", max_t, KEMR_MAX_TEXT_CTX, width,
                        causal, batch));
    if (batch == 0) return KEMR_OK;
    return launch_bwd((const bf16_t*)qkv_dev, (const bf16_t*)dout_dev, (bf16_t*)dqkv_dev, row_start_dev, batch, max_t, width, causal,
                      (hipStream_t)stream, "op_attention_backward_packed");
}
