// Retrieve-then-rerank: the learned "cross_attention" fusion head scored on LISTED (query, candidate) pairs only -- the deep
// shortlists of kemr_sim_topk_deep -- instead of on the whole [N, M] grid (rank.hip, cross_attn_pair_kernel).
//
// Per pair the arithmetic is that of the dense route: 8 + 8 per-head dot products Q.K_x (the dense route takes them from the
// similarity kernel's score planes; here they are fp32 FMA chains over the gathered key rows), 2-way softmax per head,
// hidden1 = relu(c0 + sum_h w_i P_i + w_t P_t) in the dense kernel's FMA order, the hid1 -> hid2 layer, hid2 -> 1, 0.5 * tanh.
//
// The work is gather-bound: a pair reads two key rows (2 * dim * 4 B) and two P rows (2 * 8 * hid1 * 4 B), 22 KB at dim 768 /
// hid1 256, for ~21 kFLOP.  Layout:
//   * one 512-thread workgroup = one query and a run of 32 list slots, so a single query at depth 200 is 7 workgroups;
//   * what the slots share is staged in LDS once -- the query row, c0, b2, w3 and W2^T (row stride 80 floats: the four k rows
//     an MFMA step reads then fall into different banks) -- the gathered rows are not: every row is read once, by one wave,
//     16 bytes per lane, fully coalesced, straight into registers (P rows are requested before the dot products are reduced);
//   * a wave owns 4 slots; its hidden1 rows go to LDS (row stride hid1 + 2: conflict-free A-operand reads);
//   * the hid1 -> hid2 layer of the 32 slots is a [32 x hid1] x [hid1 x 64] product: 2 x 4 tiles of v_mfma_f32_16x16x4_f32,
//     one tile per wave, ONE accumulator chain per tile in ascending k -- bit for bit the fmaf chain of the dense kernel
//     (exact fp32, no reduced-precision path), at the matrix pipe's rate instead of 64 LDS-fed VALU FMAs per hidden unit;
//   * 32 threads finish one slot each (bias, ReLU, the hid2 -> 1 chain in ascending k, 0.5 * tanh) and write it.
// Every output element has exactly one owner, nothing is accumulated across workgroups: the result is a pure function of the
// input.  Tails (a run of fewer than 32 slots, padded ids) are wave-uniform branches.
#include "common.h"

namespace kemr {

constexpr int RR_THREADS = 512;
constexpr int RR_SLOTS = 32;             // list slots per workgroup: two 16-row MFMA tiles
constexpr int RR_SLOTS_PER_WAVE = 4;
constexpr int RR_W2_LD = 80;             // LDS row stride of W2^T: 64 columns + 16 (k rows 4s .. 4s+3 in distinct banks)
constexpr int RR_Z_LD = 65;              // LDS row stride of the hid2-wide pre-activations
constexpr int RR_SLOT_OUTSIDE = -2;      // slot at or beyond `depth`: not written
constexpr int RR_SLOT_PAD = -1;          // padded id: -inf

typedef float rr_f32x4 __attribute__((ext_vector_type(4)));

static inline size_t rerank_lds_bytes(int dim, int hid1) {
    const size_t hid1p = (size_t)(hid1 + 3) / 4 * 4;
    return (hid1p * RR_W2_LD + (size_t)RR_SLOTS * (hid1p + 2) + (size_t)RR_SLOTS * RR_Z_LD + (size_t)(dim + 3) / 4 * 4 + hid1p + 64 + 64 +
            RR_SLOTS) * 4;
}

// V = floats per lane and load of a key row: 4 where dim and the head dim are multiples of 4 (dim % 32 == 0), else 1
template <int H, int V>
__global__ __launch_bounds__(RR_THREADS) void cross_attn_rerank_kernel(
    const float* __restrict__ q, const float* __restrict__ k_i, const float* __restrict__ k_t, const float* __restrict__ p_i,
    const float* __restrict__ p_t, const float* __restrict__ c0, const float* __restrict__ w2t, const float* __restrict__ b2,
    const float* __restrict__ w3, float b3, int ng, int dim, int hid1, int hid2, const int32_t* __restrict__ cand, int depth,
    long long ld, int runs, float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int hid1p = (hid1 + 3) & ~3, h1_ld = hid1p + 2;
    float* sW2 = (float*)smem;                       // [hid1p][RR_W2_LD], zero outside [hid1][hid2]
    float* sH1 = sW2 + hid1p * RR_W2_LD;             // [RR_SLOTS][h1_ld], zero where nothing is computed
    float* sZ = sH1 + RR_SLOTS * h1_ld;              // [RR_SLOTS][RR_Z_LD]
    float* sQ = sZ + RR_SLOTS * RR_Z_LD;             // [ceil4(dim)]
    float* sC0 = sQ + ((dim + 3) & ~3);              // [hid1p]
    float* sB2 = sC0 + hid1p;                        // [64]
    float* sW3 = sB2 + 64;                           // [64]
    int* sState = (int*)(sW3 + 64);                  // [RR_SLOTS] candidate id, RR_SLOT_PAD or RR_SLOT_OUTSIDE
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int qrow = blockIdx.x / runs, slot0 = (blockIdx.x % runs) * RR_SLOTS;
    const int nslots = min(RR_SLOTS, depth - slot0);
    const int hd = dim / H;

    for (int i = tid; i < hid1p * RR_W2_LD; i += RR_THREADS) {
        const int r = i / RR_W2_LD, c = i - r * RR_W2_LD;
        sW2[i] = (r < hid1 && c < hid2) ? w2t[(size_t)r * hid2 + c] : 0.f;
    }
    for (int i = tid; i < RR_SLOTS * h1_ld; i += RR_THREADS) sH1[i] = 0.f;
    for (int i = tid; i < dim; i += RR_THREADS) sQ[i] = q[(size_t)qrow * dim + i];
    for (int i = tid; i < hid1p; i += RR_THREADS) sC0[i] = i < hid1 ? c0[i] : 0.f;
    if (tid < 64) {
        sB2[tid] = tid < hid2 ? b2[tid] : 0.f;
        sW3[tid] = tid < hid2 ? w3[tid] : 0.f;
    }
    __syncthreads();

    // ---- gather stage: a wave per slot, 4 slots one after the other
    for (int s = 0; s < RR_SLOTS_PER_WAVE; ++s) {
        const int slot = wave * RR_SLOTS_PER_WAVE + s;
        int c = RR_SLOT_OUTSIDE;
        if (slot < nslots) {
            c = cand[(size_t)qrow * ld + slot0 + slot];
            if (c < 0 || c >= ng) c = RR_SLOT_PAD;               // an id outside the gallery is never dereferenced
        }
        c = __builtin_amdgcn_readfirstlane(c);
        if (lane == 0) sState[slot] = c;
        if (c < 0) continue;
        // the first 4 * 64 hidden units' P rows: requested now, used after the dot products
        const float* pi_row = p_i + (size_t)c * H * hid1;
        const float* pt_row = p_t + (size_t)c * H * hid1;
        float4 pi0[H], pt0[H];
        const bool first = lane * 4 < hid1;
#pragma unroll
        for (int h = 0; h < H; ++h) {
            pi0[h] = first ? *(const float4*)(pi_row + h * hid1 + lane * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
            pt0[h] = first ? *(const float4*)(pt_row + h * hid1 + lane * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        const float* ki_row = k_i + (size_t)c * dim;
        const float* kt_row = k_t + (size_t)c * dim;
        float ai[H], at[H];
#pragma unroll
        for (int h = 0; h < H; ++h) ai[h] = at[h] = 0.f;
        for (int e0 = lane * V; e0 < dim; e0 += 64 * V) {
            float pa = 0.f, pb = 0.f;
            if constexpr (V == 4) {
                const float4 qv = *(const float4*)(sQ + e0);
                const float4 a = *(const float4*)(ki_row + e0), b = *(const float4*)(kt_row + e0);
                pa = fmaf(qv.w, a.w, fmaf(qv.z, a.z, fmaf(qv.y, a.y, qv.x * a.x)));
                pb = fmaf(qv.w, b.w, fmaf(qv.z, b.z, fmaf(qv.y, b.y, qv.x * b.x)));
            } else {
                pa = sQ[e0] * ki_row[e0];
                pb = sQ[e0] * kt_row[e0];
            }
            const int head = e0 / hd;                            // hd % V == 0: the V elements lie in one head
#pragma unroll
            for (int h = 0; h < H; ++h) {
                ai[h] += h == head ? pa : 0.f;
                at[h] += h == head ? pb : 0.f;
            }
        }
        float wi[H], wt[H];
#pragma unroll
        for (int h = 0; h < H; ++h) {
            const float a = wave_sum(ai[h]), b = wave_sum(at[h]);
            const float mx = fmaxf(a, b);
            const float ea = __expf(a - mx), eb = __expf(b - mx);
            const float inv = 1.0f / (ea + eb);
            wi[h] = ea * inv;
            wt[h] = eb * inv;
        }
        float* h1 = sH1 + slot * h1_ld;
        for (int j0 = lane * 4; j0 < hid1; j0 += 256) {
            float4 hs = *(const float4*)(sC0 + j0);
#pragma unroll
            for (int h = 0; h < H; ++h) {
                float4 a, b;
                if (j0 < 256) {
                    a = pi0[h];
                    b = pt0[h];
                } else {
                    a = *(const float4*)(pi_row + h * hid1 + j0);
                    b = *(const float4*)(pt_row + h * hid1 + j0);
                }
                hs.x = fmaf(wi[h], a.x, fmaf(wt[h], b.x, hs.x));
                hs.y = fmaf(wi[h], a.y, fmaf(wt[h], b.y, hs.y));
                hs.z = fmaf(wi[h], a.z, fmaf(wt[h], b.z, hs.z));
                hs.w = fmaf(wi[h], a.w, fmaf(wt[h], b.w, hs.w));
            }
            h1[j0] = fmaxf(hs.x, 0.f);
            h1[j0 + 1] = fmaxf(hs.y, 0.f);
            h1[j0 + 2] = fmaxf(hs.z, 0.f);
            h1[j0 + 3] = fmaxf(hs.w, 0.f);
        }
    }
    __syncthreads();

    // ---- hid1 -> hid2 for the run: wave (mt, nt) owns rows mt * 16 .. + 15, columns nt * 16 .. + 15
    {
        const int mt = wave >> 2, nt = wave & 3;
        if (mt * 16 < nslots && nt * 16 < hid2) {
            const float* a_ptr = sH1 + (mt * 16 + (lane & 15)) * h1_ld + (lane >> 4);       // A[row = lane & 15][k = lane >> 4]
            const float* b_ptr = sW2 + (lane >> 4) * RR_W2_LD + nt * 16 + (lane & 15);      // B[k = lane >> 4][col = lane & 15]
            rr_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            for (int k0 = 0; k0 < hid1p; k0 += 4)
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a_ptr[k0], b_ptr[k0 * RR_W2_LD], acc, 0, 0, 0);
#pragma unroll
            for (int r = 0; r < 4; ++r)                                                     // D[row = (lane >> 4) * 4 + r][col = lane & 15]
                sZ[(mt * 16 + (lane >> 4) * 4 + r) * RR_Z_LD + nt * 16 + (lane & 15)] = acc[r];
        }
    }
    __syncthreads();

    if (tid < nslots) {
        const int state = sState[tid];
        float res = -INFINITY;
        if (state >= 0) {
            float o = b3;
            for (int k = 0; k < hid2; ++k) o = fmaf(fmaxf(sZ[tid * RR_Z_LD + k] + sB2[k], 0.f), sW3[k], o);
            res = 0.5f * tanhf(o);
        }
        out[(size_t)qrow * ld + slot0 + tid] = res;
    }
}

}  // namespace kemr

using namespace kemr;

extern "C" int kemr_cross_attention_rerank(const float* q_dev, const float* k_i_dev, const float* k_t_dev, const float* p_i_dev,
                                           const float* p_t_dev, const float* c0_dev, const float* w2t_dev, const float* b2_dev,
                                           const float* w3_dev, float b3, int heads, int nq, int ng, int dim, int hid1, int hid2,
                                           const int32_t* cand_idx_dev, int depth, int64_t ld, float* out_scores_dev, void* stream) {
    if (nq == 0 || depth == 0) return KEMR_OK;
#define RR_NONNULL(p) if (!(p)) KEMR_FAIL(KEMR_ERR_INVALID, "cross_attention_rerank: " #p " is null")
    RR_NONNULL(q_dev);
    RR_NONNULL(k_i_dev);
    RR_NONNULL(k_t_dev);
    RR_NONNULL(p_i_dev);
    RR_NONNULL(p_t_dev);
    RR_NONNULL(c0_dev);
    RR_NONNULL(w2t_dev);
    RR_NONNULL(b2_dev);
    RR_NONNULL(w3_dev);
    RR_NONNULL(cand_idx_dev);
    RR_NONNULL(out_scores_dev);
#undef RR_NONNULL
    if (heads != 8) KEMR_FAIL(KEMR_ERR_INVALID, "cross_attention_rerank: the reference head has 8 attention heads (got heads=%d)", heads);
    if (dim < heads || dim % heads != 0) KEMR_FAIL(KEMR_ERR_INVALID, "cross_attention_rerank: dim=%d is not a multiple of heads=%d", dim, heads);
    if (hid2 < 1 || hid2 > 64) KEMR_FAIL(KEMR_ERR_INVALID, "cross_attention_rerank: hid2=%d not in 1..64", hid2);
    if (hid1 < 4 || hid1 % 4 != 0) KEMR_FAIL(KEMR_ERR_INVALID, "cross_attention_rerank: hid1=%d is not a positive multiple of 4", hid1);
    if (depth < 1 || depth > KEMR_MAX_DEEP_K) KEMR_FAIL(KEMR_ERR_INVALID, "cross_attention_rerank: depth=%d not in 1..%d", depth, KEMR_MAX_DEEP_K);
    if (ld < depth) KEMR_FAIL(KEMR_ERR_INVALID, "cross_attention_rerank: ld=%lld is shorter than depth=%d", (long long)ld, depth);
    if (nq < 0 || ng < 0) KEMR_FAIL(KEMR_ERR_INVALID, "cross_attention_rerank: negative size (nq=%d, ng=%d)", nq, ng);
    const size_t smem = rerank_lds_bytes(dim, hid1);
    if (smem > 160 * 1024)
        KEMR_FAIL(KEMR_ERR_INVALID, "cross_attention_rerank: dim=%d, hid1=%d need %zu bytes of LDS (limit 163840)", dim, hid1, smem);
    const int runs = (depth + RR_SLOTS - 1) / RR_SLOTS;
    if ((long long)nq * runs > 0x7fffffffLL) KEMR_FAIL(KEMR_ERR_INVALID, "cross_attention_rerank: nq=%d lists of depth=%d exceed one launch", nq, depth);
    auto kern = dim % 32 == 0 ? cross_attn_rerank_kernel<8, 4> : cross_attn_rerank_kernel<8, 1>;
    KEMR_CHECK_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
    hipLaunchKernelGGL(kern, dim3((unsigned)((long long)nq * runs)), dim3(RR_THREADS), smem, (hipStream_t)stream, q_dev, k_i_dev, k_t_dev,
                       p_i_dev, p_t_dev, c0_dev, w2t_dev, b2_dev, w3_dev, b3, ng, dim, hid1, hid2, cand_idx_dev, depth, (long long)ld,
                       runs, out_scores_dev);
    KEMR_CHECK_LAUNCH("cross_attn_rerank_kernel");
    return KEMR_OK;
}
