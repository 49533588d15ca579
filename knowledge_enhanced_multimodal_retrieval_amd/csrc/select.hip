// Deep top-k of materialised score rows: the k <= KEMR_MAX_DEEP_K best (score, id) of a row of n fp32 scores, sorted by the
// project's order rule (score descending, then lower id).  Serves kemr_select_topk and the second stage of kemr_sim_topk_deep
// (sim.hip), where the register-resident lists of sim.hip / rank.hip (O(k) per insert, k registers per lane) end at k = 32.
//
// One 1024-thread workgroup per row.  Every entry becomes its 64-bit order_key (rank_order.h: sign-flip mapping of the fp32 bits,
// -0.0 as +0.0, NaN below -inf, then 0x7fffffff - id), so with distinct ids all keys are distinct and "the k largest keys" IS the
// order rule: ties at the k-th score need no special case.
//   1. radix select, 12 key bits per pass from the top: an integer LDS histogram of the entries that share the prefix found so
//      far, a suffix scan over its 4 096 bins, the bin that holds the k-th largest key extends the prefix.  Integer sums do not
//      depend on the order the atomics arrive in.  The passes stop as soon as the entries above the boundary bin plus the bin
//      itself fit SEL_CAP LDS slots (standard-normal or cosine scores at n = 43 000: two passes; an all-equal row: the 32 score
//      bits and the upper id bits are one bin each, five passes), at the latest when all 64 bits are fixed and the bin holds one key.
//   2. one gather pass: every entry with key >= the boundary bin's smallest key goes to LDS with its column, in arrival order;
//   3. a bitonic sort of those <= SEL_CAP (key, column) pairs makes the output a pure function of the input; the first k leave
//      with the score and id re-read from their column (the input's own bits: a -0.0 or a NaN payload comes back as it went in).
// The row is streamed from L2 / Infinity Cache (its producer has just written it) once per pass: 16-byte loads where the row is
// aligned, scalar loads for the head, the tail and unaligned id rows; nothing is read at or beyond column n.
// Ids must be distinct within a row (they are candidate ids).  Repeated (score, id) pairs stay memory-safe -- the gather stops
// at SEL_CAP entries -- but which of the copies is returned is then unspecified.
#include "common.h"
#include "rank_order.h"

namespace kemr {

constexpr int SEL_THREADS = 1024;
constexpr int SEL_DIGIT = 12;
constexpr int SEL_BINS = 1 << SEL_DIGIT;       // 4 per thread
constexpr int SEL_CAP = 4096;                  // gathered entries: < KEMR_MAX_DEEP_K above the boundary bin + the bin itself
static_assert(SEL_BINS == 4 * SEL_THREADS, "the suffix scan gives every thread four bins");
static_assert(SEL_CAP >= 2 * KEMR_MAX_DEEP_K && (SEL_CAP & (SEL_CAP - 1)) == 0, "SEL_CAP: a power of two with room for k winners");

// f(key, column) for every valid entry of the row (id >= 0), each column < n exactly once, spread over the workgroup: the head /
// 16-byte vectors / tail walk of row_for_each (rank_order.h) SPELLED OUT, with the ids read 16 bytes at a time next to the scores.
// Built on row_for_each the kernels ran new instructions (same registers, LDS and occupancy) and kemr_sim_topk_deep_fused at
// 1 024 x 43 000, k = 100 took +0.9 % where two copies of the previous library differed by 0.05 %
// (profiles/rank_order_refactor_ab.json); this form compiles to the previous instructions.
template <class F>
__device__ __forceinline__ void select_for_each(const float* __restrict__ row, const int32_t* __restrict__ ids, int n,
                                                long long id_offset, int tid, F&& f) {
    auto one = [&](int c, float s) {
        const int id = ids ? ids[c] : (int)(id_offset + c);
        if (id >= 0) f(order_key(s, id), c);
    };
    int head = (int)((4u - (uint32_t)(((uintptr_t)row >> 2) & 3u)) & 3u);          // columns in front of the first 16-byte boundary
    head = head < n ? head : n;
    const int nvec = (n - head) >> 2;
    const int tail = head + nvec * 4;
    if (tid < head) one(tid, row[tid]);
    const float4* row4 = (const float4*)(row + head);
    const bool ids16 = ids && (((uintptr_t)(ids + head)) & 15u) == 0;
    for (int v = tid; v < nvec; v += SEL_THREADS) {
        const float4 s4 = row4[v];
        const int c = head + v * 4;
        if (ids16) {
            const int4 i4 = *(const int4*)(ids + c);
            if (i4.x >= 0) f(order_key(s4.x, i4.x), c);
            if (i4.y >= 0) f(order_key(s4.y, i4.y), c + 1);
            if (i4.z >= 0) f(order_key(s4.z, i4.z), c + 2);
            if (i4.w >= 0) f(order_key(s4.w, i4.w), c + 3);
        } else {
            one(c, s4.x); one(c + 1, s4.y); one(c + 2, s4.z); one(c + 3, s4.w);
        }
    }
    if (tid < n - tail) one(tail + tid, row[tail + tid]);
}

// COUNT (kemr_sim_topk_deep_fused with a ground truth; ids are id_offset + column): the first sweep -- the one pass that sees every
// entry of the row -- also counts the entries that rank before (gt_score[row], gt_idx[row]) and adds the sum to ahead[row].  On the
// keys that is `key > key(gt_score, gt_idx)`: the key order IS ranks_before except for a NaN gt_score, before which ranks_before
// puts nothing (rank_order.h: where the two forms differ): no count then.
// The entry with the ground truth's own id is left out whatever its score.  Integer sums: wave shuffles, one LDS atomic per wave.
template <bool COUNT>
__global__ __launch_bounds__(SEL_THREADS) void select_topk_kernel(const float* __restrict__ S, const int32_t* __restrict__ I, int n,
                                                                  long long ld, long long id_offset, int k,
                                                                  float* __restrict__ top_s, int32_t* __restrict__ top_i,
                                                                  const int32_t* __restrict__ gt_idx, const float* __restrict__ gt_score,
                                                                  int32_t* __restrict__ ahead) {
    __shared__ u64 s_key[SEL_CAP];                    // 32 KiB
    __shared__ int s_hist[SEL_BINS];                  // 16 KiB; the gathered columns once the last histogram is read
    __shared__ int s_wave[SEL_THREADS / 64];
    __shared__ int s_pick[3];                         // boundary bin, entries in the bins above it, entries in it
    __shared__ int s_total, s_fill, s_ahead;
    int* s_col = s_hist;
    static_assert(SEL_CAP <= SEL_BINS, "the gathered columns alias the histogram");

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* row = S + (size_t)blockIdx.x * ld;
    const int32_t* ids = I ? I + (size_t)blockIdx.x * ld : nullptr;
    float* out_s = top_s + (size_t)blockIdx.x * k;
    int32_t* out_i = top_i + (size_t)blockIdx.x * k;

    u64 prefix = 0;           // the upper `bits` bits of the k-th largest key
    int bits = 0;
    int need = k;             // keys still to take out of the entries that share the prefix
    int above = 0;            // entries known to rank before all of those
    int gathered = 0;
    u64 gt_key = ~0ull;       // COUNT: the ground truth's key; all ones (above every key) = count nothing
    if constexpr (COUNT) {
        const float sg = gt_score[blockIdx.x];
        if (sg == sg) gt_key = order_key(sg, gt_idx[blockIdx.x]);
        if (tid == 0) s_ahead = 0;
    }
    for (;;) {
        const int dbits = 64 - bits < SEL_DIGIT ? 64 - bits : SEL_DIGIT;
        const int shift = 64 - bits - dbits;
        for (int b = tid; b < SEL_BINS; b += SEL_THREADS) s_hist[b] = 0;
        __syncthreads();
        if (COUNT && bits == 0) {
            int cnt = 0;
            select_for_each(row, ids, n, id_offset, tid, [&](u64 key, int) {
                atomicAdd(&s_hist[(int)(key >> shift)], 1);
                cnt += (key > gt_key && (uint32_t)key != (uint32_t)gt_key) ? 1 : 0;
            });
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
            if (lane == 0 && cnt) atomicAdd(&s_ahead, cnt);
        } else {
            select_for_each(row, ids, n, id_offset, tid, [&](u64 key, int) {
                if (bits == 0 || (key >> (64 - bits)) == prefix) atomicAdd(&s_hist[(int)((key >> shift) & (u64)((1 << dbits) - 1))], 1);
            });
        }
        __syncthreads();
        // inclusive suffix sums over the threads' groups of four bins
        const int h0 = s_hist[4 * tid], h1 = s_hist[4 * tid + 1], h2 = s_hist[4 * tid + 2], h3 = s_hist[4 * tid + 3];
        const int mine = h0 + h1 + h2 + h3;
        int suf = mine;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_down(suf, o);
            if (lane + o < 64) suf += t;
        }
        if (lane == 0) s_wave[wave] = suf;
        __syncthreads();
        for (int w = wave + 1; w < SEL_THREADS / 64; ++w) suf += s_wave[w];
        if (tid == 0) s_total = suf;
        __syncthreads();
        const int total = s_total;                   // entries that share the prefix (first pass: the row's valid entries)
        if (bits == 0) {
            if (need > total) need = total;          // fewer than k entries: all of them, the rest of the list is padding
            if (total <= SEL_CAP) { gathered = total; break; }      // everything fits: prefix stays empty, the sort does the rest
        }
        const int hi = suf - mine;                   // entries in the bins above this thread's
        if (suf >= need && hi < need) {              // exactly one thread: its bins hold the need-th largest
            const int h[4] = {h0, h1, h2, h3};
            int acc = hi;
#pragma unroll
            for (int b = 3; b >= 0; --b) {
                if (acc < need && acc + h[b] >= need) { s_pick[0] = 4 * tid + b; s_pick[1] = acc; s_pick[2] = h[b]; }
                acc += h[b];
            }
        }
        __syncthreads();
        const int bin = s_pick[0], over = s_pick[1], cnt = s_pick[2];
        prefix = (prefix << dbits) | (u64)bin;
        bits += dbits;
        above += over;
        need -= over;
        gathered = above + cnt;
        if (gathered <= SEL_CAP || bits == 64) break;
    }
    const int kout = above + need;                   // min(k, valid entries)
    if (kout > 0) {
        const u64 lo_key = bits == 0 ? 0ull : prefix << (64 - bits);         // the boundary bin's smallest key
        if (tid == 0) s_fill = 0;
        __syncthreads();                                                     // also: every thread has read the histogram
        select_for_each(row, ids, n, id_offset, tid, [&](u64 key, int c) {
            if (key >= lo_key) {
                const int slot = atomicAdd(&s_fill, 1);
                if (slot < SEL_CAP) { s_key[slot] = key; s_col[slot] = c; }
            }
        });
        gathered = gathered < SEL_CAP ? gathered : SEL_CAP;
        int m = 2;
        while (m < gathered) m <<= 1;
        __syncthreads();
        for (int j = gathered + tid; j < m; j += SEL_THREADS) { s_key[j] = 0ull; s_col[j] = -1; }
        __syncthreads();
        // bitonic sort, descending by (key, column): a padding slot (column -1) goes behind a valid entry whose key is 0
        for (int size = 2; size <= m; size <<= 1) {
            for (int stride = size >> 1; stride > 0; stride >>= 1) {
                for (int t = tid; t < (m >> 1); t += SEL_THREADS) {
                    const int l = 2 * t - (t & (stride - 1)), r = l + stride;
                    const u64 kl = s_key[l], kr = s_key[r];
                    const int cl = s_col[l], cr = s_col[r];
                    const bool l_first = kl > kr || (kl == kr && cl > cr);
                    const bool descending = (l & size) == 0;
                    if (l_first != descending) { s_key[l] = kr; s_key[r] = kl; s_col[l] = cr; s_col[r] = cl; }
                }
                __syncthreads();
            }
        }
    }
    for (int j = tid; j < k; j += SEL_THREADS) {
        const int c = j < kout ? s_col[j] : -1;
        out_s[j] = c >= 0 ? row[c] : -INFINITY;
        out_i[j] = c >= 0 ? (ids ? ids[c] : (int)(id_offset + c)) : -1;
    }
    if constexpr (COUNT) {
        if (tid == 0 && s_ahead) ahead[blockIdx.x] += s_ahead;       // one workgroup per row: a plain add, shards follow on the stream
    }
}

int launch_select_topk(const float* scores, const int32_t* idx, int nq, int n, long long ld, long long id_offset, int k,
                       float* top_scores, int32_t* top_idx, hipStream_t stream, const int32_t* gt_idx, const float* gt_score,
                       int32_t* ahead) {
    if (gt_idx) {
        if (idx || !gt_score || !ahead) KEMR_FAIL(KEMR_ERR_INVALID, "select_topk: the rank count takes id_offset ids and gt_idx, gt_score, ahead together");
        hipLaunchKernelGGL(select_topk_kernel<true>, dim3(nq), dim3(SEL_THREADS), 0, stream, scores, idx, n, ld, id_offset, k, top_scores,
                           top_idx, gt_idx, gt_score, ahead);
    } else {
        hipLaunchKernelGGL(select_topk_kernel<false>, dim3(nq), dim3(SEL_THREADS), 0, stream, scores, idx, n, ld, id_offset, k, top_scores,
                           top_idx, nullptr, nullptr, nullptr);
    }
    KEMR_CHECK_LAUNCH("select_topk_kernel");
    return KEMR_OK;
}

}  // namespace kemr

using namespace kemr;

extern "C" int kemr_select_topk(const float* scores_dev, const int32_t* idx_dev, int nq, int n, int64_t ld, int64_t id_offset,
                                int k, float* top_scores_dev, int32_t* top_idx_dev, void* stream) {
    if (k < 1 || k > KEMR_MAX_DEEP_K) KEMR_FAIL(KEMR_ERR_INVALID, "select_topk: k=%d not in 1..%d", k, KEMR_MAX_DEEP_K);
    if (!scores_dev || !top_scores_dev || !top_idx_dev) KEMR_FAIL(KEMR_ERR_INVALID, "select_topk: null pointer");
    if (nq < 0 || n < 1) KEMR_FAIL(KEMR_ERR_INVALID, "select_topk: bad shape (nq=%d n=%d)", nq, n);
    if (ld < n) KEMR_FAIL(KEMR_ERR_INVALID, "select_topk: ld=%lld < n=%d", (long long)ld, n);
    if (!idx_dev && (id_offset < 0 || id_offset + n > 0x7fffffffLL)) KEMR_FAIL(KEMR_ERR_INVALID, "select_topk: candidate ids exceed int32");
    if (nq == 0) return KEMR_OK;
    return launch_select_topk(scores_dev, idx_dev, nq, n, ld, id_offset, k, top_scores_dev, top_idx_dev, (hipStream_t)stream);
}
