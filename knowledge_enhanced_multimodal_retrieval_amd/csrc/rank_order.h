// The one statement of the order of candidates (include/kemr.h: "score descending, then lower id") and of the steps every producer of
// a ranked list or an `ahead` count shares: sim.hip, rank.hip, select.hip, listfuse.hip.  Device code only.
//
// The rule has two forms.
//   predicate  ranks_before(sa, ia, sb, ib) = sa > sb || (sa == sb && ia < ib)      fp32 compares, the k <= 32 routes: the register
//              lists and their merges (sim.hip, rank.hip), every `ahead` count of those routes;
//   key        order_key(s, id) = ordered_u32(s) << 32 | (0x7fffffff - id), larger key = earlier      integer compares, the deep routes:
//              the radix selection and its count (select.hip), the place of the ground truth in a fused list (listfuse.hip).
// They AGREE -- a ranks before b exactly when key(a) > key(b) -- on finite scores and +-inf, -0.0 equal to +0.0, ids >= 0: there both
// are the same strict total order, and distinct ids give distinct keys.
// They DIFFER on NaN:
//   a NaN entry      the predicate puts it before nothing and nothing before it; the key puts it behind -inf, NaNs among themselves by
//                    lower id.  So no route counts a NaN entry as ahead of a non-NaN ground truth, and only the key lists one.
//   a NaN ground truth   the predicate puts nothing before it (ahead = 0); by the key every non-NaN entry is before it.  select.hip's
//                    count follows the predicate there (it counts nothing: it continues sim.hip's count), listfuse.hip follows the key.
// -inf is ordered alike by both forms; what differs is what the lists ADMIT: a register list (topk_insert) takes an entry only above
// its last score and is padded with -inf, so it never holds -inf or NaN, while the key-based lists hold every entry with an id >= 0,
// -inf behind the finite ones and NaN behind -inf.  Padding is told by the id (< 0), never by the score.
//
// One place restates the rule instead of including it: the SIM scan of gemm256u.hip compares a lane's 16 accumulators with ONE
// threshold per lane (the ground truth's score, or the next float below it, by which side of the ground truth's id the lane's ids lie
// on) inside the GEMM's hot loop, where a call per candidate with its id would cost the loop its schedule.
// Four spots SPELL a helper OUT under a comment that names it (sim_kernel's bonus cursor, the rounds of simk_select_kernel and
// topk_merge_block_kernel, select_for_each's row walk): called there the kernel left the timing margin between two copies of the
// previous library, spelled out it compiles to the previous instructions (profiles/rank_order_refactor_ab.json).  They use
// ranks_before / order_key from here; change a helper and its spelled-out twin together.
#pragma once
#include "common.h"

namespace kemr {

typedef unsigned long long u64;

__device__ __forceinline__ bool ranks_before(float sa, int ia, float sb, int ib) {
    return sa > sb || (sa == sb && ia < ib);
}

__device__ __forceinline__ u64 order_key(float s, int id) {
    uint32_t u = __float_as_uint(s);
    uint32_t o;
    if ((u & 0x7fffffffu) > 0x7f800000u) {
        o = 0u;                                                   // NaN: behind -inf (0x007fffff)
    } else {
        if (u == 0x80000000u) u = 0u;                             // -0.0 ties with +0.0
        o = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    }
    return ((u64)o << 32) | (uint32_t)(0x7fffffff - id);
}

// (v, idx) into a list sorted by descending score, pad (-inf, -1).  The caller tests v > s[KMAX - 1] first and hands a thread ids
// that only increase, so the strict '>' keeps "lower id first" among equal scores.
template <int KMAX>
__device__ __forceinline__ void topk_insert(float (&s)[KMAX], int (&id)[KMAX], float v, int idx) {
#pragma unroll
    for (int i = KMAX - 1; i > 0; --i) {
        const bool shift = v > s[i - 1];
        const bool here = !shift && v > s[i];
        s[i] = shift ? s[i - 1] : (here ? v : s[i]);
        id[i] = shift ? id[i - 1] : (here ? idx : id[i]);
    }
    if (v > s[0]) { s[0] = v; id[0] = idx; }
}

// ---- selection: k rounds of "the best entry after the previous pick", so a list is a pure function of the SET of entries it is
// picked from -- how they were dealt to lanes, lists or shards does not matter.  (bs, bi) is the best so far, bi < 0 = none yet.
// An entry of this round: it comes after the previous pick (ps, pi) -- in the first round every entry does -- and before my best
__device__ __forceinline__ void pick_entry(bool first, float ps, int pi, float es, int ei, float& bs, int& bi) {
    const bool after_prev = first || ranks_before(ps, pi, es, ei);
    if (after_prev && (bi < 0 || ranks_before(es, ei, bs, bi))) { bs = es; bi = ei; }
}
// Another lane's or wave's best (oi < 0: it has none) against mine
__device__ __forceinline__ void pick_merge(float os, int oi, float& bs, int& bi) {
    if (oi >= 0 && (bi < 0 || ranks_before(os, oi, bs, bi))) { bs = os; bi = oi; }
}
// The best of the 64 lanes' bests, in every lane
__device__ __forceinline__ void wave_pick(float& bs, int& bi) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float os = __shfl_xor(bs, off);
        const int oi = __shfl_xor(bi, off);
        pick_merge(os, oi, bs, bi);
    }
}
// Round o's pick into row q of the [nq, k] lists, by thread t == 0 of the nt that hold it.  No pick (bi < 0): the entries are
// exhausted, the nt threads pad slots o + 1 .. k - 1 with (-inf, -1) and the rounds end.
__device__ __forceinline__ void write_pick(float* __restrict__ out_s, int32_t* __restrict__ out_i, int q, int k, int o, float bs, int bi,
                                           int t) {
    if (t == 0) { out_s[(size_t)q * k + o] = bi >= 0 ? bs : -INFINITY; out_i[(size_t)q * k + o] = bi; }
}
__device__ __forceinline__ void pad_picks(float* __restrict__ out_s, int32_t* __restrict__ out_i, int q, int k, int o, int t, int nt) {
    for (int r = o + 1 + t; r < k; r += nt) { out_s[(size_t)q * k + r] = -INFINITY; out_i[(size_t)q * k + r] = -1; }
}
// One wave picks row q's k best of n entries; fetch(e, es, ei) reads entry e and returns false for padding
template <class Fetch>
__device__ __forceinline__ void wave_select(int lane, int n, int q, int k, float* __restrict__ out_s, int32_t* __restrict__ out_i,
                                            Fetch&& fetch) {
    float ps = INFINITY;
    int pi = -1;
    for (int o = 0; o < k; ++o) {
        float bs = -INFINITY;
        int bi = -1;
        for (int e = lane; e < n; e += 64) {
            float es;
            int ei;
            if (!fetch(e, es, ei)) continue;
            pick_entry(o == 0, ps, pi, es, ei, bs, bi);
        }
        wave_pick(bs, bi);
        write_pick(out_s, out_i, q, k, o, bs, bi, lane);
        if (bi < 0) { pad_picks(out_s, out_i, q, k, o, lane, 64); break; }
        ps = bs;
        pi = bi;
    }
}

// ---- the SPARQL bonus of candidate c: f plus the run of entries e .. with cols[e] == c (columns ascend within a CSR row, so the run
// is contiguous), one fp32 add per entry in list order and never an FMA: every route gives a pair the same bits.  e is left behind
// the run.
__device__ __forceinline__ float bonus_run_add(float f, int c, const int32_t* cols, const float* vals, int& e, int end) {
    for (; e < end && cols[e] == c; ++e) f = __fadd_rn(f, vals[e]);
    return f;
}

// ---- a row of n fp32 read by nt threads: the columns in front of the first 16-byte boundary (at most 3), 16-byte vectors
// f4(float4, first column), the columns behind the last whole vector (at most 3).  Every column < n exactly once, nothing at or
// beyond column n is read, rows need no alignment; a thread's columns only increase.
template <class F1, class F4>
__device__ __forceinline__ void row_for_each(const float* __restrict__ row, int n, int tid, int nt, F1&& f1, F4&& f4) {
    int head = (int)((4u - (uint32_t)(((uintptr_t)row >> 2) & 3u)) & 3u);
    head = head < n ? head : n;
    const int nvec = (n - head) >> 2;
    const int tail = head + nvec * 4;
    if (tid < head) f1(row[tid], tid);
    const float4* row4 = (const float4*)(row + head);
    for (int v = tid; v < nvec; v += nt) {
        const float4 x = row4[v];                                 // ONE 16-byte load: f4 takes the value, not a reference into the row
        f4(x, head + v * 4);
    }
    if (tid < n - tail) f1(row[tail + tid], tail + tid);
}
template <class F1>
__device__ __forceinline__ void row_for_each(const float* __restrict__ row, int n, int tid, int nt, F1&& f1) {
    row_for_each(row, n, tid, nt, f1, [&](float4 v, int c) { f1(v.x, c); f1(v.y, c + 1); f1(v.z, c + 2); f1(v.w, c + 3); });
}

}  // namespace kemr
