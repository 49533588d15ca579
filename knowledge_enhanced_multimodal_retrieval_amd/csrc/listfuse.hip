// Knowledge-fused rerank, last stage: the SPARQL bonus on a learned head's LISTED scores, and the ground truth's place in the fused
// list -- head_weight * head + bonus on the deep shortlists that kemr_cross_attention_rerank / kemr_linear_head have scored.
//
// Per slot (q, j), j < depth, with id c = list_idx[q, j]:
//   c < 0 (the deep lists' padding): out = -inf;
//   otherwise f = score_scale * s as ONE fp32 multiply (skipped at score_scale == 1: the input's own bits), then every entry of bonus
//   row q whose column is c added one after the other in list order, each as ONE fp32 add (bonus_run_add, rank_order.h: what
//   kemr_sim_topk_deep_fused's deep_bonus_kernel calls too), so the dense route and this one give a pair the same bits.
// The bonus row is a run of the CSR with ascending columns: a lower-bound binary search finds the first entry of column c, the
// entries of that column follow it.  Rows of at most LF_STAGE entries are copied to LDS first (every slot of the list searches the
// same row); longer rows -- a query with thousands of hits -- are searched where they lie.  The arithmetic is the same either way.
//
// Ground truth (optional): found = the row lists gt_idx[q]; gt_score = that slot's fused score (-inf where absent); ahead = the
// slots with id >= 0 and id != gt whose (fused score, id) ranks before (gt_score, gt) by order_key (rank_order.h: score descending,
// -0.0 == +0.0, NaN behind -inf, then lower id) -- where the ground truth is absent every slot with id >= 0.  So where found, ahead + 1
// is the ground truth's position in kemr_select_topk(out, idx, k = depth).
//
// Layout: one 256-thread workgroup per query row, slot j belongs to thread j % 256 (at most 4 slots per thread at depth 1024, kept
// in registers between the fuse and the count), one block reduction (wave shuffles + 4 LDS words) for `ahead`, a second of the same
// kind that names the ground truth's slot.  Every output element has one owner, nothing is accumulated in memory, no atomics: the
// result is a pure function of the input.  out may alias list_scores (a slot is read and written by the same thread).
#include "common.h"
#include "rank_order.h"

namespace kemr {

constexpr int LF_THREADS = 256;
constexpr int LF_SLOTS = KEMR_MAX_DEEP_K / LF_THREADS;      // slots per thread at the deepest list
constexpr int LF_STAGE = 2048;                              // bonus entries staged in LDS: 16 KiB
static_assert(LF_SLOTS * LF_THREADS == KEMR_MAX_DEEP_K, "a thread owns depth / 256 slots, rounded up");

// f + the entries of column c in cols[0 .. len), ascending columns (bonus_run_add's arithmetic)
__device__ __forceinline__ float list_fuse_add(float f, int c, const int32_t* cols, const float* vals, int len) {
    int lo = 0, hi = len;
    while (lo < hi) {                                             // first entry with column >= c
        const int mid = (lo + hi) >> 1;
        if (cols[mid] < c) lo = mid + 1; else hi = mid;
    }
    return bonus_run_add(f, c, cols, vals, lo, len);
}

__device__ __forceinline__ int lf_block_reduce(int v, bool take_min, int* s_red, int tid) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int w = __shfl_xor(v, o);
        v = take_min ? min(v, w) : v + w;
    }
    if ((tid & 63) == 0) s_red[tid >> 6] = v;
    __syncthreads();
    int r = s_red[0];
#pragma unroll
    for (int w = 1; w < LF_THREADS / 64; ++w) r = take_min ? min(r, s_red[w]) : r + s_red[w];
    __syncthreads();                                              // s_red is free again
    return r;
}

// list_scores and out may be the same buffer: neither is __restrict__
__global__ __launch_bounds__(LF_THREADS) void list_fuse_kernel(const float* list_scores, const int32_t* __restrict__ list_idx, int depth,
                                                               long long ld, float scale, const int32_t* __restrict__ brow,
                                                               const int32_t* __restrict__ bcol, const float* __restrict__ bval,
                                                               const int32_t* __restrict__ gt_idx, int32_t* __restrict__ ahead,
                                                               int32_t* __restrict__ found, float* __restrict__ gt_score, float* out) {
    __shared__ int32_t s_col[LF_STAGE];
    __shared__ float s_val[LF_STAGE];
    __shared__ int s_red[LF_THREADS / 64];
    __shared__ float s_gt;
    const int tid = threadIdx.x;
    const long long q = blockIdx.x;
    const float* row_s = list_scores + q * ld;
    const int32_t* row_i = list_idx + q * ld;
    float* row_o = out + q * ld;

    // ---- the query's bonus row
    const int32_t* cols = nullptr;
    const float* vals = nullptr;
    int blen = 0;
    if (brow) {
        const int b0 = brow[q], b1 = brow[q + 1];
        blen = b1 > b0 ? b1 - b0 : 0;
        cols = bcol + b0;
        vals = bval + b0;
        if (blen > 0 && blen <= LF_STAGE) {                       // block-uniform
            for (int i = tid; i < blen; i += LF_THREADS) {
                s_col[i] = cols[i];
                s_val[i] = vals[i];
            }
            cols = s_col;
            vals = s_val;
            __syncthreads();
        }
    }

    // ---- fuse: slot tid + s * 256
    float f[LF_SLOTS];
    int id[LF_SLOTS];
#pragma unroll
    for (int s = 0; s < LF_SLOTS; ++s) {
        const int j = tid + s * LF_THREADS;
        id[s] = -1;
        f[s] = -INFINITY;
        if (j < depth) {
            const int c = row_i[j];
            if (c >= 0) {
                const float v = row_s[j];
                float x = scale == 1.0f ? v : __fmul_rn(scale, v);
                if (blen > 0) x = list_fuse_add(x, c, cols, vals, blen);
                id[s] = c;
                f[s] = x;
            }
            row_o[j] = f[s];
        }
    }
    if (!gt_idx) return;                                          // block-uniform

    // ---- the ground truth's slot (the first, should a caller repeat an id), its fused score, the slots ranked before it
    const int gt = gt_idx[q];
    int mine = INT_MAX;
#pragma unroll
    for (int s = LF_SLOTS - 1; s >= 0; --s)
        if (gt >= 0 && id[s] == gt) mine = tid + s * LF_THREADS;
    const int at = lf_block_reduce(mine, true, s_red, tid);
    const bool here = at != INT_MAX;
    if (here && (at % LF_THREADS) == tid) {
        float g = 0.f;
#pragma unroll
        for (int s = 0; s < LF_SLOTS; ++s)
            if (s == at / LF_THREADS) g = f[s];
        s_gt = g;
    }
    __syncthreads();
    const float g = here ? s_gt : -INFINITY;
    const u64 gkey = order_key(g, gt);
    int cnt = 0;
#pragma unroll
    for (int s = 0; s < LF_SLOTS; ++s)
        if (id[s] >= 0 && id[s] != gt) cnt += (!here || order_key(f[s], id[s]) > gkey) ? 1 : 0;
    const int total = lf_block_reduce(cnt, false, s_red, tid);
    if (tid == 0) {
        ahead[q] = total;
        found[q] = here ? 1 : 0;
        gt_score[q] = g;
    }
}

}  // namespace kemr

using namespace kemr;

extern "C" int kemr_list_fuse(const float* list_scores_dev, const int32_t* list_idx_dev, int nq, int depth, int64_t ld, float score_scale,
                              const int32_t* bonus_rowptr_dev, const int32_t* bonus_col_dev, const float* bonus_val_dev,
                              const int32_t* gt_idx_dev, int32_t* ahead_dev, int32_t* found_dev, float* gt_score_dev,
                              float* out_scores_dev, void* stream) {
    if (nq == 0) return KEMR_OK;
    if (!list_scores_dev || !list_idx_dev || !out_scores_dev)
        KEMR_FAIL(KEMR_ERR_INVALID, "list_fuse: list_scores, list_idx and out_scores are required");
    if ((bonus_rowptr_dev != nullptr) != (bonus_col_dev != nullptr) || (bonus_rowptr_dev != nullptr) != (bonus_val_dev != nullptr))
        KEMR_FAIL(KEMR_ERR_INVALID, "list_fuse: bonus CSR arrays must be given together");
    const int ngt = (gt_idx_dev != nullptr) + (ahead_dev != nullptr) + (found_dev != nullptr) + (gt_score_dev != nullptr);
    if (ngt != 0 && ngt != 4)
        KEMR_FAIL(KEMR_ERR_INVALID, "list_fuse: gt_idx, ahead, found and gt_score must be given together");
    if (nq < 0) KEMR_FAIL(KEMR_ERR_INVALID, "list_fuse: negative size (nq=%d)", nq);
    if (depth < 1 || depth > KEMR_MAX_DEEP_K) KEMR_FAIL(KEMR_ERR_INVALID, "list_fuse: depth=%d not in 1..%d", depth, KEMR_MAX_DEEP_K);
    if (ld < depth) KEMR_FAIL(KEMR_ERR_INVALID, "list_fuse: ld=%lld is shorter than depth=%d", (long long)ld, depth);
    hipLaunchKernelGGL(list_fuse_kernel, dim3((unsigned)nq), dim3(LF_THREADS), 0, (hipStream_t)stream, list_scores_dev, list_idx_dev, depth,
                       (long long)ld, score_scale, bonus_rowptr_dev, bonus_col_dev, bonus_val_dev, gt_idx_dev, ahead_dev, found_dev,
                       gt_score_dev, out_scores_dev);
    KEMR_CHECK_LAUNCH("list_fuse_kernel");
    return KEMR_OK;
}
