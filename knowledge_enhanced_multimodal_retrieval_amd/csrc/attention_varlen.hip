// Non-causal multi-head attention over PACKED items of different lengths (the BERT sentence encoders, model family 2): item b owns the
// rows row_start[b] .. row_start[b + 1] - 1 of the q | k | v buffer of attention.hip ([rows, 3W] bf16, head dim 64, q pre-scaled by
// 1/8), 1 .. KEMR_MAX_BERT_CTX of them; output [rows, W] bf16.  A padding mask is a length: there are no pad positions to mask, and
// an item's keys are its own rows only.
//
// The tile code is attention_long.hip's, with the sequence length and the first row read per item instead of passed per launch:
//   * one workgroup of 4 waves per (item, head, block of QB = 128 queries); the grid is sized for the longest length the launch
//     admits (max_t) and a workgroup whose query block starts at or behind its item's length returns before the first barrier
//     (the whole workgroup: the test is on values every thread of the workgroup shares);
//   * a wave owns the two 16-query tiles at rows 128 qb + 16 w + 64 i; a tile with no valid query (short items: most of them) is
//     skipped by its wave -- MFMAs, softmax and store, never a barrier or a staging load, so the barriers stay workgroup-uniform;
//   * K and V stream through LDS in chunks of 64 keys, double-buffered, one barrier per chunk; S^T = K . Q^T on
//     v_mfma_f32_16x16x32_bf16, V^T through ds_read_b64_tr_b16 from the row-major V image, the swizzled LDS images, the online
//     softmax with the fp32 row sum taken from the unrounded P and P rounded to bf16 for PV, one division at the end.
// Per item the arithmetic and its order are exactly attention_long.hip's at T = the item's length (oracle/rounding.py
// attention_long_emulation states the rounding).  No atomics, a fixed order of every sum: bit-identical run to run, and an item's
// output does not depend on what is packed around it.
// Memory: the staging loads clamp their row to the item's last one, so no row outside row_start[b] .. row_start[b + 1] - 1 is read for
// item b (not as a key, not as a query); pad keys of the last chunk are zero-filled in LDS and masked to -inf; exactly the item's rows
// of `out` are written.  Lengths beyond max_t are clamped to it (the rows behind are then left unwritten; the encoder's row_start comes
// from row_starts_kernel, which clamps the lengths to ctx itself).
//
// BIAS (model family 3, MPNet): scores = q . k^T + bias[h][key - query], a learned relative position bias.  The instantiation takes a
// device table bias_by_distance fp32 [heads, VA_ND = 1023], entry [h][d + 511] for d = key - query in -511 .. 511 (model.hip expands
// the checkpoint's 32 buckets once at finalize).  The head's 4 KB row is staged into LDS behind the two chunk images before the first
// barrier; lane (lrow, lq) of S^T tile (i, t) holds the keys k0 + 16 t + 4 lq + r, r = 0..3, of ONE query, so its four biases are four
// consecutive entries, read as the START VALUE of the tile's first MFMA accumulator instead of zero (no add instruction; q carries the
// 1/8, the bias enters unscaled).  Clamped query rows index with their clamped position and pad keys reach at most key 511, so every
// index stays in 0 .. 1022; the pad-key mask to -inf comes after, as before.  The table is read-only and per head: the fixed order of
// every sum, the isolation of an item and the memory contract above hold unchanged.  The instantiation without BIAS is the kernel as it
// was: every bias statement is under `if constexpr`.
//
// CAUSAL (model family 0, the CLIP text towers of 129 .. KEMR_MAX_TEXT_CTX positions, Long-CLIP's 248 among them; packed items of up to
// 128 rows keep attention.hip's tile kernels): query q of an item sees its keys 0 .. q.  The instantiation changes three things, each
// under `if constexpr`, so the non-causal instantiations are the kernels they were:
//   * a workgroup's chunk loop ends at the last chunk that holds a key <= its block's last valid query instead of at the item's last;
//   * a wave skips the MFMAs, the softmax and the update of a chunk that lies wholly behind one of its 16-query tiles (chunk start >
//     the tile's last query) -- wave-uniform, and never a barrier or a staging load, exactly as for a dead tile; inside a processed
//     chunk the 16-key score tiles and 32-key PV blocks wholly behind the tile are skipped too (their P is 0);
//   * in a chunk that reaches behind the tile's first query, the keys behind the lane's query go to -inf where the pad keys do.
// No row ever meets a processed chunk without a valid key: tiles start at multiples of 16 and chunks at multiples of 64, so "chunk
// start 64 c <= the tile's last query q0 + 15" is "64 c <= q0", and every row q0 + j of the tile has key 64 c <= its own position;
// 64 c <= the block's last valid query < T, so that key is no pad key either.  The running maximum of a row is therefore finite
// from its first processed chunk on (always chunk 0) and exp2(-inf - (-inf)) cannot occur.  Rows of a live tile behind the item's last
// row compute on the clamped query against the keys 0 .. T - 1 and are not stored.  The order of every sum is the non-causal one with
// the skipped terms left out: an item's bits depend on its own rows alone, run to run.  oracle/rounding.py _attention_chunked with the
// lower-triangular key mask states the arithmetic.
#include "common.h"

namespace kemr {

namespace {

#ifndef KEMR_ATTN_VARLEN_QT
#define KEMR_ATTN_VARLEN_QT 2
#endif
#ifndef KEMR_ATTN_VARLEN_OCC
#define KEMR_ATTN_VARLEN_OCC 2
#endif
constexpr int VA_NW = 4;                  // waves per workgroup
constexpr int VA_QT = KEMR_ATTN_VARLEN_QT;  // 16-query tiles per wave
constexpr int VA_QB = VA_NW * VA_QT * 16; // queries per workgroup
#ifndef KEMR_ATTN_VARLEN_KC
#define KEMR_ATTN_VARLEN_KC 64
#endif
constexpr int VA_KC = KEMR_ATTN_VARLEN_KC;  // keys per LDS chunk
constexpr int VA_NT16 = VA_KC / 16;       // 16-key S^T tiles per chunk
constexpr int VA_NU = VA_KC / 32;         // 32-key PV blocks per chunk
constexpr int VA_STAGE = VA_KC * 128 * 2; // bytes of one K + V chunk image
constexpr int VA_NCH = VA_KC * 8 / (VA_NW * 64);   // 16-byte pieces of K (and of V) per thread and chunk
constexpr int VA_ND = 2 * KEMR_MAX_BERT_CTX - 1;   // distances key - query of the bias table: -511 .. 511
constexpr int VA_NDP = 2 * KEMR_MAX_BERT_CTX;      // floats of its LDS image
static_assert(VA_NDP <= VA_NW * 64 * 4, "the bias row is staged in one pass of four floats per thread");

__device__ __forceinline__ bf16x4 lds_read_tr16_v(const char* p) {
    typedef __attribute__((ext_vector_type(4))) short s4;
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s4*)p);
}

}  // namespace

// Work items (query block fastest, then head, then item) are numbered so that the workgroups dealt to one XCD (the dispatcher
// deals linear ids round-robin over the eight XCDs) take a contiguous range: the query blocks of one (item, head) read the same
// K / V rows through the same L2.  Only a locality heuristic; every work item is computed exactly once whatever the placement.
template <bool BIAS, bool CAUSAL>
__global__ __launch_bounds__(VA_NW * 64, KEMR_ATTN_VARLEN_OCC) void attention_varlen_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ out,
                                                                       const int* __restrict__ row_start, int max_t, int width, int nqb, int items,
                                                                       const float* __restrict__ bias_by_distance) {
    constexpr float LOG2E = 1.4426950408889634f;
    __shared__ __attribute__((aligned(16))) char smem[2 * VA_STAGE + (BIAS ? VA_NDP * 4 : 0)];

    const int heads = width >> 6;
    const int per_xcd = (int)(gridDim.x >> 3);
    const int id = (int)blockIdx.x;
    const int item = (id & 7) * per_xcd + (id >> 3);
    if (item >= items) return;                         // whole workgroup: before any barrier
    const int qb = item % nqb, hb = item / nqb;
    const int h = hb % heads, b = hb / heads;
    const int r0 = row_start[b];
    int T = row_start[b + 1] - r0;
    T = T < max_t ? T : max_t;
    if (qb * VA_QB >= T) return;                       // a query block behind the item's last row (T <= 0 included): whole workgroup

    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ld = 3 * width;
    const bf16_t* base = qkv + (size_t)r0 * ld + h * 64;
    const int lrow = lane & 15, lq = lane >> 4;
    // CAUSAL: up to the chunk of the block's last valid query (< T: no more chunks than the item has)
    const int nch = CAUSAL ? ((qb + 1) * VA_QB <= T ? (qb + 1) * VA_QB - 1 : T - 1) / VA_KC + 1 : (T + VA_KC - 1) / VA_KC;

    // query fragments of the wave's two tiles (B operand of S^T = K . Q^T): rows clamped to the last valid one
    bf16x8 qf[VA_QT][2];
    bool live[VA_QT];                                  // wave-uniform: the tile holds at least one query of the item
    int boff[VA_QT];                                   // BIAS: the table index of the lane's query against key 4 lq
    int tq0[VA_QT];                                    // CAUSAL: the tile's first query (wave-uniform, a multiple of 16)
#pragma unroll
    for (int i = 0; i < VA_QT; ++i) {
        live[i] = qb * VA_QB + i * (VA_NW * 16) + wid * 16 < T;
        if constexpr (CAUSAL) tq0[i] = qb * VA_QB + i * (VA_NW * 16) + wid * 16;
        const int q = qb * VA_QB + i * (VA_NW * 16) + wid * 16 + lrow;
        const int qc = q < T ? q : T - 1;
        boff[i] = (KEMR_MAX_BERT_CTX - 1) - qc + lq * 4;            // 0 <= qc <= 511: with a key in 0 .. 508 + r the index is in 0 .. 1022
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) qf[i][kk] = *(const bf16x8*)(base + (size_t)qc * ld + kk * 32 + lq * 8);
    }

    // chunk staging: VA_NCH pieces of K and of V per thread, loaded into registers, written swizzled.  Plain (temporal) loads: the
    // query-block workgroups of an (item, head) read the same rows (through one L2, see the numbering above).  Rows clamped to the
    // item's last one: the neighbouring item's rows are never read.
    uint4 kv[VA_NCH], vv[VA_NCH];
    auto load_chunk = [&](int c) {
#pragma unroll
        for (int i = 0; i < VA_NCH; ++i) {
            const int idx = tid + i * (VA_NW * 64);
            const int row = c * VA_KC + (idx >> 3), ch = idx & 7;
            const int rc = row < T ? row : T - 1;
            kv[i] = *(const uint4*)(base + (size_t)rc * ld + width + ch * 8);
            vv[i] = *(const uint4*)(base + (size_t)rc * ld + 2 * width + ch * 8);
        }
    };
    auto store_chunk = [&](int c, char* stage) {
        char* sK = stage;
        char* sV = stage + VA_KC * 128;
#pragma unroll
        for (int i = 0; i < VA_NCH; ++i) {
            const int idx = tid + i * (VA_NW * 64);
            const int row = idx >> 3, ch = idx & 7;
            const unsigned keep = c * VA_KC + row < T ? 0xffffffffu : 0u;
            uint4 a = kv[i], v = vv[i];
            a.x &= keep; a.y &= keep; a.z &= keep; a.w &= keep;
            v.x &= keep; v.y &= keep; v.z &= keep; v.w &= keep;
            *(uint4*)(sK + row * 128 + ((ch ^ ((row >> 1) & 7)) << 4)) = a;
            *(uint4*)(sV + row * 128 + ((ch ^ (((row >> 1) & 3) << 1)) << 4)) = v;
        }
    };

    load_chunk(0);
    const float* sB = (const float*)(smem + 2 * VA_STAGE);
    if constexpr (BIAS) {                              // the head's row of the table: visible behind the first barrier, read-only from then on
        const float* src = bias_by_distance + (size_t)h * VA_ND;
        float* dstb = (float*)(smem + 2 * VA_STAGE);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int e = tid * 4 + j;
            if (e < VA_NDP) dstb[e] = e < VA_ND ? src[e] : 0.f;
        }
    }
    store_chunk(0, smem);
    __syncthreads();

    f32x4 o[VA_QT][4];
    float ml[VA_QT], l[VA_QT];                         // running max (times log2 e) and the lane's partial row sum
#pragma unroll
    for (int i = 0; i < VA_QT; ++i) {
        ml[i] = -INFINITY;
        l[i] = 0.f;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) o[i][dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    }

    for (int c = 0; c < nch; ++c) {
        const bool more = c + 1 < nch;
        if (more) load_chunk(c + 1);                   // in flight while this chunk is computed
        const char* sK = smem + (c & 1) * VA_STAGE;
        const char* sV = sK + VA_KC * 128;
        const int k0 = c * VA_KC;
        const bool tail = k0 + VA_KC > T;              // the ragged last chunk: masks, dead tiles skipped (uniform)
        // wave-uniform: the tile takes part in this chunk (CAUSAL: the chunk is not wholly behind the tile); keys from `key` on are in reach
        auto act = [&](int i) { if constexpr (CAUSAL) return live[i] && k0 <= tq0[i] + 15; else return live[i]; };
        auto reach = [&](int i, int key) { if constexpr (CAUSAL) return key <= tq0[i] + 15; else return true; };

        // S^T tiles: s[i][t][r] = S[query of tile i, lrow][key k0 + 16 t + 4 lq + r]
        f32x4 s[VA_QT][VA_NT16];
        bf16x8 kf[VA_NT16][2];
#pragma unroll
        for (int t = 0; t < VA_NT16; ++t)
#pragma unroll
            for (int kk = 0; kk < 2; ++kk)
                kf[t][kk] = *(const bf16x8*)(sK + (t * 16 + lrow) * 128 + (((kk * 4 + lq) ^ (lrow >> 1)) << 4));
#pragma unroll
        for (int t = 0; t < VA_NT16; ++t)
#pragma unroll
            for (int i = 0; i < VA_QT; ++i) {
                s[i][t] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (act(i) && (!tail || k0 + t * 16 < T) && reach(i, k0 + t * 16)) {       // (a score tile out of reach is masked below)
                    if constexpr (BIAS) {              // the accumulator starts at bias[key - query]: keys k0 + 16 t + 4 lq + r
                        const float* bp = sB + boff[i] + k0 + t * 16;
                        s[i][t] = f32x4{bp[0], bp[1], bp[2], bp[3]};
                    }
                    s[i][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[t][0], qf[i][0], s[i][t], 0, 0, 0);
                    s[i][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[t][1], qf[i][1], s[i][t], 0, 0, 0);
                }
            }

        // V^T fragments of the chunk's two 32-key blocks, issued before the softmax so that their latency hides behind it
        bf16x8 vf[VA_NU][4];
#pragma unroll
        for (int u = 0; u < VA_NU; ++u) {
            const int ra = u * 32 + lq * 4 + (lrow >> 2);
            const int rb = ra + 16;
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) {
                const int cc = dt * 2 + ((lrow & 3) >> 1);
                const bf16x4 va = lds_read_tr16_v(sV + ra * 128 + ((cc ^ (((ra >> 1) & 3) << 1)) << 4) + (lrow & 1) * 8);
                const bf16x4 vb = lds_read_tr16_v(sV + rb * 128 + ((cc ^ (((rb >> 1) & 3) << 1)) << 4) + (lrow & 1) * 8);
                vf[u][dt][0] = va[0]; vf[u][dt][1] = va[1]; vf[u][dt][2] = va[2]; vf[u][dt][3] = va[3];
                vf[u][dt][4] = vb[0]; vf[u][dt][5] = vb[1]; vf[u][dt][6] = vb[2]; vf[u][dt][7] = vb[3];
            }
        }

        // online softmax per query tile
#pragma unroll
        for (int i = 0; i < VA_QT; ++i) {
            if (!act(i)) continue;
            if (tail) {
#pragma unroll
                for (int t = 0; t < VA_NT16; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        s[i][t][r] = k0 + t * 16 + lq * 4 + r < T ? s[i][t][r] : -INFINITY;
            }
            if constexpr (CAUSAL) {
                if (k0 + VA_KC - 1 > tq0[i]) {         // the chunk reaches behind the tile's first query: keys behind the lane's query
                    const int q = tq0[i] + lrow;
#pragma unroll
                    for (int t = 0; t < VA_NT16; ++t)
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            s[i][t][r] = k0 + t * 16 + lq * 4 + r <= q ? s[i][t][r] : -INFINITY;
                }
            }
            float mx = -INFINITY;
#pragma unroll
            for (int t = 0; t < VA_NT16; ++t)
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
            for (int t = 0; t < VA_NT16; ++t) {
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
        for (int u = 0; u < VA_NU; ++u) {
            if (tail && k0 + u * 32 >= T) continue;
#pragma unroll
            for (int i = 0; i < VA_QT; ++i) {
                if (!act(i) || !reach(i, k0 + u * 32)) continue;   // (out of reach: every key of the block is behind the tile, P = 0)
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

        if (more) store_chunk(c + 1, smem + ((c + 1) & 1) * VA_STAGE);   // that buffer was last read before the previous barrier
        __syncthreads();
    }

    // o[i][dt][r] = O[query lrow of tile i][d = 16 dt + 4 lq + r]
#pragma unroll
    for (int i = 0; i < VA_QT; ++i) {
        float sum = l[i];
        sum += __shfl_xor(sum, 16);
        sum += __shfl_xor(sum, 32);
        const int q = qb * VA_QB + i * (VA_NW * 16) + wid * 16 + lrow;
        if (q < T) {
            const float inv = 1.0f / sum;
            bf16_t* dst = out + ((size_t)r0 + q) * width + h * 64 + lq * 4;
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

int launch_attention_varlen(const bf16_t* qkv, bf16_t* out, const int* row_start, int batch, int max_t, int width, hipStream_t stream,
                            const float* bias_by_distance) {
    if (batch <= 0) return KEMR_OK;
    if (!row_start) KEMR_FAIL(KEMR_ERR_INVALID, "attention_varlen: null row_start");
    if (width <= 0 || width % 64 != 0) KEMR_FAIL(KEMR_ERR_INVALID, "attention_varlen: width %d is not a multiple of the head dim 64", width);
    if (max_t <= 0 || max_t > KEMR_MAX_BERT_CTX)
        KEMR_FAIL(KEMR_ERR_INVALID, "attention_varlen: longest item %d not in 1..%d", max_t, KEMR_MAX_BERT_CTX);
    const int nqb = (max_t + VA_QB - 1) / VA_QB;
    const long long items = (long long)batch * (width / 64) * nqb;
    if (items > 0x7ffffff0LL) KEMR_FAIL(KEMR_ERR_INVALID, "attention_varlen: batch %d too large", batch);
    const long long blocks = (items + 7) / 8 * 8;
    ProfScope prof(PROF_ATTENTION, stream);
    if (bias_by_distance)
        hipLaunchKernelGGL((attention_varlen_kernel<true, false>), dim3((unsigned)blocks), dim3(VA_NW * 64), 0, stream, qkv, out, row_start, max_t, width, nqb, (int)items, bias_by_distance);
    else
        hipLaunchKernelGGL((attention_varlen_kernel<false, false>), dim3((unsigned)blocks), dim3(VA_NW * 64), 0, stream, qkv, out, row_start, max_t, width, nqb, (int)items, bias_by_distance);
    KEMR_CHECK_LAUNCH("attention_varlen_kernel");
    return KEMR_OK;
}

// The causal instantiation: launch_attention_packed's route for items of 129 .. KEMR_MAX_TEXT_CTX rows (it has checked batch, row_start
// and the width).
int launch_attention_varlen_causal(const bf16_t* qkv, bf16_t* out, const int* row_start, int batch, int max_t, int width, hipStream_t stream) {
    if (max_t <= 0 || max_t > KEMR_MAX_TEXT_CTX)
        KEMR_FAIL(KEMR_ERR_INVALID, "attention: packed rows support lengths up to %d, got %d", KEMR_MAX_TEXT_CTX, max_t);
    const int nqb = (max_t + VA_QB - 1) / VA_QB;
    const long long items = (long long)batch * (width / 64) * nqb;
    const long long blocks = (items + 7) / 8 * 8;
    ProfScope prof(PROF_ATTENTION, stream);
    hipLaunchKernelGGL((attention_varlen_kernel<false, true>), dim3((unsigned)blocks), dim3(VA_NW * 64), 0, stream, qkv, out, row_start, max_t, width, nqb, (int)items, nullptr);
    KEMR_CHECK_LAUNCH("attention_varlen_kernel (causal)");
    return KEMR_OK;
}

}  // namespace kemr
