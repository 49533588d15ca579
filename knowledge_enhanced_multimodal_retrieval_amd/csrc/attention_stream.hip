// Streaming multi-head attention, head dim 64: K and V go through LDS in chunks with an online softmax, so the sequence length is
// bounded by nothing in the kernel.  ONE kernel template serves every sequence attention.hip's tile kernels (whole K / V in LDS,
// the full score row in registers: at 608 padded keys 152 KB of LDS and about 152 fp32 VGPRs per lane) cannot hold:
//   <PACKED, BIAS, CAUSAL>
//   <false, false, false>   launch_attention_long: the long vision towers, 289 <= T <= KEMR_MAX_VISION_TOKENS (ViT-L/14@336px: 577)
//   <true,  false, false>   launch_attention_varlen: the BERT sentence encoders (model family 2), items of 1 .. KEMR_MAX_BERT_CTX rows
//   <true,  true,  false>   the same with MPNet's relative position bias (model family 3)
//   <true,  false, true >   launch_attention_varlen_causal: CLIP text towers of 129 .. KEMR_MAX_TEXT_CTX positions (Long-CLIP's 248)
// Operands as in attention.hip: the q | k | v rows [rows, 3W] bf16 with q pre-scaled by 1/8, output [rows, W] bf16.
//
// The design, common to all four:
//   * one workgroup of 4 waves per (item, head, block of QB = 128 queries); a wave owns two 16-query tiles (rows 128 qb + 16 w + 64 i,
//     i = 0, 1), so every K / V fragment it reads from LDS feeds two MFMAs;
//   * K and V stream through LDS in chunks of KC = 64 keys, double-buffered: the global loads of chunk c + 1 are in flight in
//     registers while chunk c is computed, then written to the other LDS buffer -- one barrier per chunk;
//   * per query a running max m and row sum l in fp32: for every chunk m' = max(m, chunk max), O and l are scaled by
//     exp(m - m') (exactly 1 when the max did not move), P = exp(S - m');
//   * the MFMA forms, the lane ownership and the LDS images (K: Img64<false>, V: Img64<true>) are attention_tile.h's, as in
//     attention.hip; a chunk starts at a multiple of 64 rows, so it has the swizzle of its local rows.
// Rounding at attention_tile.h's three points, as in the tile kernels (oracle/rounding.py attention_long_emulation states it, for every
// instantiation per item at T = the item's length).  No atomics, a fixed order of every sum: bit-identical run to run.
// Pad keys (the ragged last chunk: 577 = 9 * 64 + 1) are zero-filled in LDS and masked to -inf; key tiles made only of pad keys
// are skipped (wave-uniform).  Pad queries read the last valid row and are not stored.
// Every difference between the instantiations is under `if constexpr`: each is the kernel it would be if written alone.
//
// PACKED: item b owns the rows row_start[b] .. row_start[b + 1] - 1 (device ints), 1 .. max_t of them, instead of the rows b T ..
// b T + T - 1 of a launch-wide T.  A padding mask is a length: there are no pad positions to mask, and an item's keys are its own rows.
//   * the grid is sized for the longest length the launch admits (max_t) and a workgroup whose query block starts at or behind its
//     item's length returns before the first barrier (the whole workgroup: the test is on values every thread of it shares);
//   * a tile with no valid query (short items: most of them) is skipped by its wave -- MFMAs, softmax and store, never a barrier
//     or a staging load, so the barriers stay workgroup-uniform.  (The fixed-length instantiation computes the dead tiles of its
//     last query block: their rows are clamped and not stored.)
//   * memory: the staging loads clamp their row to the item's last one, so no row outside row_start[b] .. row_start[b + 1] - 1 is
//     read for item b (not as a key, not as a query), and exactly the item's rows of `out` are written: an item's output does not
//     depend on what is packed around it.  Lengths beyond max_t are clamped to it (the rows behind are then left unwritten; the
//     encoder's row_start comes from row_starts_kernel, which clamps the lengths to ctx itself).
//
// BIAS (MPNet): scores = q . k^T + bias[h][key - query], a learned relative position bias.  The instantiation takes a device table
// bias_by_distance fp32 [heads, ND = 1023], entry [h][d + 511] for d = key - query in -511 .. 511 (model.hip expands the
// checkpoint's 32 buckets once at finalize).  The head's 4 KB row is staged into LDS behind the two chunk images before the first
// barrier; lane (lrow, lq) of S^T tile (i, t) holds the keys k0 + 16 t + 4 lq + r, r = 0..3, of ONE query, so its four biases are four
// consecutive entries, read as the START VALUE of the tile's first MFMA accumulator instead of zero (no add instruction; q carries the
// 1/8, the bias enters unscaled).  Clamped query rows index with their clamped position and pad keys reach at most key 511, so every
// index stays in 0 .. 1022; the pad-key mask to -inf comes after.  The table is read-only and per head: the fixed order of every
// sum, the isolation of an item and the memory contract above hold unchanged.
//
// CAUSAL (packed items of up to 128 rows keep attention.hip's tile kernels): query q of an item sees its keys 0 .. q.  Three changes:
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
//
// Compile-time A/B switches (tools/ab_build_flag.sh; the defaults are the product): KEMR_ATTN_STREAM_QT query tiles per wave,
// KEMR_ATTN_STREAM_KC keys per chunk, KEMR_ATTN_STREAM_OCC waves per SIMD asked of the register allocator.  Fixed length, T = 577,
// B = 85, width 1024 (tools/bench_attention_long.py): QT 2 / KC 64 / 2 waves (180 VGPRs) 314-326 us; QT 1 / KC 64 / 4 waves (126
// VGPRs) 325 us; QT 1 / KC 128, 3 or 4 waves, 415 us.  Occupancy is not what holds it back: the counters put it at 2.35 x the VALU
// instructions per MFMA of the 257-token kernel (softmax and per-chunk bookkeeping; DESIGN.md, "Long sequences").
#include "attention_tile.h"

namespace kemr {

namespace {

#ifndef KEMR_ATTN_STREAM_QT
#define KEMR_ATTN_STREAM_QT 2
#endif
#ifndef KEMR_ATTN_STREAM_OCC
#define KEMR_ATTN_STREAM_OCC 2
#endif
#ifndef KEMR_ATTN_STREAM_KC
#define KEMR_ATTN_STREAM_KC 64
#endif
constexpr int NW = 4;                     // waves per workgroup
constexpr int QT = KEMR_ATTN_STREAM_QT;   // 16-query tiles per wave
constexpr int QB = NW * QT * 16;          // queries per workgroup
constexpr int KC = KEMR_ATTN_STREAM_KC;   // keys per LDS chunk
constexpr int NT16 = KC / 16;             // 16-key S^T tiles per chunk
constexpr int NU = KC / 32;               // 32-key PV blocks per chunk
constexpr int STAGE = KC * 128 * 2;       // bytes of one K + V chunk image
constexpr int NCH = KC * 8 / (NW * 64);   // 16-byte pieces of K (and of V) per thread and chunk
constexpr int ND = 2 * KEMR_MAX_BERT_CTX - 1;      // BIAS: distances key - query of the table: -511 .. 511
constexpr int NDP = 2 * KEMR_MAX_BERT_CTX;         // floats of its LDS image
static_assert(NDP <= NW * 64 * 4, "the bias row is staged in one pass of four floats per thread");

}  // namespace

// Work items (query block fastest, then head, then item) are numbered so that the workgroups dealt to one XCD (the dispatcher
// deals linear ids round-robin over the eight XCDs) take a contiguous range: the query blocks of one (item, head) read the same
// K / V rows through the same L2.  Only a locality heuristic; every work item is computed exactly once whatever the placement.
// !PACKED: T = max_t for every item, row_start is not read.  !BIAS: bias_by_distance is not read.
// Where the kernel spells attention_tile.h's arithmetic out: with every step a call the bits were equal and the non-causal instantiations
// 0.6 - 0.7 % faster, but <true, false, true> measured +0.02 % and +0.09 % at the 248-position packed mix in two of three runs where two
// copies of the previous library differed by 0.03 % and 0.02 % (profiles/attention_tile_refactor_ab.json).  The spots were not timed one by
// one: row_max, tile_exp and tile_pack stay calls and the V gather takes the header's swizzle, which leave the device code as it was; the
// staging write, the K read, row_sum and the store change it and are spelled out.  All four instantiations compile to the previous
// commit's instructions.
template <bool PACKED, bool BIAS, bool CAUSAL>
__global__ __launch_bounds__(NW * 64, KEMR_ATTN_STREAM_OCC) void attention_stream_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ out,
                                                                       const int* __restrict__ row_start, int max_t, int width, int nqb, int items,
                                                                       const float* __restrict__ bias_by_distance) {
    __shared__ __attribute__((aligned(16))) char smem[2 * STAGE + (BIAS ? NDP * 4 : 0)];

    const int heads = width >> 6;
    const int per_xcd = (int)(gridDim.x >> 3);
    const int id = (int)blockIdx.x;
    const int item = (id & 7) * per_xcd + (id >> 3);
    if (item >= items) return;                         // whole workgroup: before any barrier
    const int qb = item % nqb, hb = item / nqb;
    const int h = hb % heads, b = hb / heads;
    int T = max_t;
    size_t row0;                                       // the item's first row
    if constexpr (PACKED) {
        const int r0 = row_start[b];
        T = row_start[b + 1] - r0;
        T = T < max_t ? T : max_t;
        if (qb * QB >= T) return;                      // a query block behind the item's last row (T <= 0 included): whole workgroup
        row0 = (size_t)r0;
    } else {
        row0 = (size_t)b * T;
    }

    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ld = 3 * width;
    const bf16_t* base = qkv + row0 * ld + h * 64;
    const int lrow = lane & 15, lq = lane >> 4;
    // CAUSAL: up to the chunk of the block's last valid query (< T: no more chunks than the item has)
    const int nch = CAUSAL ? ((qb + 1) * QB <= T ? (qb + 1) * QB - 1 : T - 1) / KC + 1 : (T + KC - 1) / KC;

    // query fragments of the wave's two tiles (B operand of S^T = K . Q^T): rows clamped to the last valid one
    bf16x8 qf[QT][2];
    bool live[QT];                                     // wave-uniform: the tile holds at least one query of the item (!PACKED: always)
    int boff[QT];                                      // BIAS: the table index of the lane's query against key 4 lq
    int tq0[QT];                                       // CAUSAL: the tile's first query (wave-uniform, a multiple of 16)
#pragma unroll
    for (int i = 0; i < QT; ++i) {
        live[i] = !PACKED || qb * QB + i * (NW * 16) + wid * 16 < T;
        if constexpr (CAUSAL) tq0[i] = qb * QB + i * (NW * 16) + wid * 16;
        const int q = qb * QB + i * (NW * 16) + wid * 16 + lrow;
        const int qc = q < T ? q : T - 1;
        boff[i] = (KEMR_MAX_BERT_CTX - 1) - qc + lq * 4;            // 0 <= qc <= 511: with a key in 0 .. 508 + r the index is in 0 .. 1022
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) qf[i][kk] = *(const bf16x8*)(base + (size_t)qc * ld + kk * 32 + lq * 8);
    }

    // chunk staging: NCH pieces of K and of V per thread, loaded into registers, written swizzled.  Plain (temporal) loads: unlike
    // attention.hip, where one workgroup reads a head's K / V, the query-block workgroups of an (item, head) read the same rows
    // (through one L2, see the numbering above).  Same time as non-temporal loads at T = 577 (368.5 vs 374.6 us).  Rows
    // clamped to the item's last one: the neighbouring item's rows are never read.
    uint4 kv[NCH], vv[NCH];
    auto load_chunk = [&](int c) {
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
            const int idx = tid + i * (NW * 64);
            const int row = c * KC + (idx >> 3), ch = idx & 7;
            const int rc = row < T ? row : T - 1;
            kv[i] = *(const uint4*)(base + (size_t)rc * ld + width + ch * 8);
            vv[i] = *(const uint4*)(base + (size_t)rc * ld + 2 * width + ch * 8);
        }
    };
    auto store_chunk = [&](int c, char* stage) {
        char* sK = stage;
        char* sV = stage + KC * 128;
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
            const int idx = tid + i * (NW * 64);
            const int row = idx >> 3, ch = idx & 7;
            const unsigned keep = c * KC + row < T ? 0xffffffffu : 0u;      // two tile_put, spelled out (see the note at the kernel)
            uint4 a = kv[i], v = vv[i];
            a.x &= keep; a.y &= keep; a.z &= keep; a.w &= keep;
            v.x &= keep; v.y &= keep; v.z &= keep; v.w &= keep;
            *(uint4*)(sK + row * 128 + ((ch ^ ((row >> 1) & 7)) << 4)) = a;
            *(uint4*)(sV + row * 128 + ((ch ^ (((row >> 1) & 3) << 1)) << 4)) = v;
        }
    };

    load_chunk(0);
    const float* sB = (const float*)(smem + 2 * STAGE);
    if constexpr (BIAS) {                              // the head's row of the table: visible behind the first barrier, read-only from then on
        const float* src = bias_by_distance + (size_t)h * ND;
        float* dstb = (float*)(smem + 2 * STAGE);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int e = tid * 4 + j;
            if (e < NDP) dstb[e] = e < ND ? src[e] : 0.f;
        }
    }
    store_chunk(0, smem);
    __syncthreads();

    f32x4 o[QT][4];
    float ml[QT], l[QT];                               // running max (times log2 e) and the lane's partial row sum
#pragma unroll
    for (int i = 0; i < QT; ++i) {
        ml[i] = -INFINITY;
        l[i] = 0.f;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) o[i][dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    }

    for (int c = 0; c < nch; ++c) {
        const bool more = c + 1 < nch;
        if (more) load_chunk(c + 1);                   // in flight while this chunk is computed
        const char* sK = smem + (c & 1) * STAGE;
        const char* sV = sK + KC * 128;
        const int k0 = c * KC;
        const bool tail = k0 + KC > T;                 // the ragged last chunk: masks, dead tiles skipped (uniform)
        // wave-uniform: the tile takes part in this chunk (CAUSAL: the chunk is not wholly behind the tile); keys from `key` on are in reach
        auto act = [&](int i) { if constexpr (CAUSAL) return live[i] && k0 <= tq0[i] + 15; else return live[i]; };
        auto reach = [&](int i, int key) { if constexpr (CAUSAL) return key <= tq0[i] + 15; else return true; };

        // S^T tiles: s[i][t][r] = S[query of tile i, lrow][key k0 + 16 t + 4 lq + r]
        f32x4 s[QT][NT16];
        bf16x8 kf[NT16][2];
#pragma unroll
        for (int t = 0; t < NT16; ++t)
#pragma unroll
            for (int kk = 0; kk < 2; ++kk)
                kf[t][kk] = *(const bf16x8*)(sK + (t * 16 + lrow) * 128 + (((kk * 4 + lq) ^ (lrow >> 1)) << 4));   // tile_row<Img64<false>>, spelled out
#pragma unroll
        for (int t = 0; t < NT16; ++t)
#pragma unroll
            for (int i = 0; i < QT; ++i) {
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
        bf16x8 vf[NU][4];
#pragma unroll
        for (int u = 0; u < NU; ++u) {                 // tile_tr<Img64<true>>, spelled out on the header's swizzle
            const int ra = u * 32 + lq * 4 + (lrow >> 2);
            const int rb = ra + 16;
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) {
                const int cc = dt * 2 + ((lrow & 3) >> 1);
                const bf16x4 va = lds_read_tr16(sV + ra * 128 + Img64<true>::swz(ra, cc) + (lrow & 1) * 8);
                const bf16x4 vb = lds_read_tr16(sV + rb * 128 + Img64<true>::swz(rb, cc) + (lrow & 1) * 8);
                vf[u][dt][0] = va[0]; vf[u][dt][1] = va[1]; vf[u][dt][2] = va[2]; vf[u][dt][3] = va[3];
                vf[u][dt][4] = vb[0]; vf[u][dt][5] = vb[1]; vf[u][dt][6] = vb[2]; vf[u][dt][7] = vb[3];
            }
        }

        // online softmax per query tile
#pragma unroll
        for (int i = 0; i < QT; ++i) {
            if (!act(i)) continue;
            if (tail) {
#pragma unroll
                for (int t = 0; t < NT16; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        s[i][t][r] = k0 + t * 16 + lq * 4 + r < T ? s[i][t][r] : -INFINITY;
            }
            if constexpr (CAUSAL) {
                if (k0 + KC - 1 > tq0[i]) {            // the chunk reaches behind the tile's first query: keys behind the lane's query
                    const int q = tq0[i] + lrow;
#pragma unroll
                    for (int t = 0; t < NT16; ++t)
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            s[i][t][r] = k0 + t * 16 + lq * 4 + r <= q ? s[i][t][r] : -INFINITY;
                }
            }
            float mx = -INFINITY;
#pragma unroll
            for (int t = 0; t < NT16; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) mx = fmaxf(mx, s[i][t][r]);
            const float mnew = fmaxf(ml[i], row_max(mx) * LOG2E);
            const float alpha = __builtin_amdgcn_exp2f(ml[i] - mnew);     // 0 on the first chunk (-inf), 1 when the max stays
            ml[i] = mnew;
            f32x2_t sum2 = {0.f, 0.f};
            const f32x2_t l2 = {LOG2E, LOG2E}, nm = {-mnew, -mnew};
#pragma unroll
            for (int t = 0; t < NT16; ++t) tile_exp(s[i][t], l2, nm, sum2);
            l[i] = l[i] * alpha + (sum2.x + sum2.y);
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) o[i][dt] *= alpha;
        }

        // O^T += V^T . P^T per 32-key block (a block of pad keys only has P = 0 and is skipped)
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            if (tail && k0 + u * 32 >= T) continue;
#pragma unroll
            for (int i = 0; i < QT; ++i) {
                if (!act(i) || !reach(i, k0 + u * 32)) continue;   // (out of reach: every key of the block is behind the tile, P = 0)
                const bf16x8 pf = tile_pack(s[i][2 * u], s[i][2 * u + 1]);
#pragma unroll
                for (int dt = 0; dt < 4; ++dt)
                    o[i][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf[u][dt], pf, o[i][dt], 0, 0, 0);
            }
        }

        if (more) store_chunk(c + 1, smem + ((c + 1) & 1) * STAGE);   // that buffer was last read before the previous barrier
        __syncthreads();
    }

    // o[i][dt][r] = O[query lrow of tile i][d = 16 dt + 4 lq + r]
#pragma unroll
    for (int i = 0; i < QT; ++i) {
        float sum = l[i];                              // row_sum and tile_store, spelled out
        sum += __shfl_xor(sum, 16);
        sum += __shfl_xor(sum, 32);
        const int q = qb * QB + i * (NW * 16) + wid * 16 + lrow;
        if (q < T) {
            const float inv = 1.0f / sum;
            bf16_t* dst = out + (row0 + q) * width + h * 64 + lq * 4;
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

namespace {

// The launchers below have checked their arguments; `who` names the caller in the one refusal left.
template <bool PACKED, bool BIAS, bool CAUSAL>
int launch_stream(const char* who, const bf16_t* qkv, bf16_t* out, const int* row_start, int batch, int max_t, int width,
                  const float* bias_by_distance, hipStream_t stream) {
    const int nqb = (max_t + QB - 1) / QB;
    const long long items = (long long)batch * (width / 64) * nqb;
    if (items > 0x7ffffff0LL) KEMR_FAIL(KEMR_ERR_INVALID, "%s: batch %d too large", who, batch);
    const long long blocks = (items + 7) / 8 * 8;
    ProfScope prof(PROF_ATTENTION, stream);
    hipLaunchKernelGGL((attention_stream_kernel<PACKED, BIAS, CAUSAL>), dim3((unsigned)blocks), dim3(NW * 64), 0, stream, qkv, out, row_start, max_t,
                       width, nqb, (int)items, bias_by_distance);
    KEMR_CHECK_LAUNCH("attention_stream_kernel");
    return KEMR_OK;
}

}  // namespace

int launch_attention_long(const bf16_t* qkv, bf16_t* out, int batch, int t, int width, hipStream_t stream) {
    if (batch <= 0) return KEMR_OK;
    if (width % 64 != 0 || t <= 0 || t > KEMR_MAX_VISION_TOKENS)
        KEMR_FAIL(KEMR_ERR_INVALID, "attention: sequence length %d not in 1..%d (non-causal)", t, KEMR_MAX_VISION_TOKENS);
    return launch_stream<false, false, false>("attention", qkv, out, nullptr, batch, t, width, nullptr, stream);
}

int launch_attention_varlen(const bf16_t* qkv, bf16_t* out, const int* row_start, int batch, int max_t, int width, hipStream_t stream,
                            const float* bias_by_distance) {
    if (batch <= 0) return KEMR_OK;
    if (!row_start) KEMR_FAIL(KEMR_ERR_INVALID, "attention_varlen: null row_start");
    if (width <= 0 || width % 64 != 0) KEMR_FAIL(KEMR_ERR_INVALID, "attention_varlen: width %d is not a multiple of the head dim 64", width);
    if (max_t <= 0 || max_t > KEMR_MAX_BERT_CTX)
        KEMR_FAIL(KEMR_ERR_INVALID, "attention_varlen: longest item %d not in 1..%d", max_t, KEMR_MAX_BERT_CTX);
    if (bias_by_distance) return launch_stream<true, true, false>("attention_varlen", qkv, out, row_start, batch, max_t, width, bias_by_distance, stream);
    return launch_stream<true, false, false>("attention_varlen", qkv, out, row_start, batch, max_t, width, nullptr, stream);
}

// The causal instantiation: launch_attention_packed's route for items of 129 .. KEMR_MAX_TEXT_CTX rows (it has checked batch, row_start
// and the width).
int launch_attention_varlen_causal(const bf16_t* qkv, bf16_t* out, const int* row_start, int batch, int max_t, int width, hipStream_t stream) {
    if (max_t <= 0 || max_t > KEMR_MAX_TEXT_CTX)
        KEMR_FAIL(KEMR_ERR_INVALID, "attention: packed rows support lengths up to %d, got %d", KEMR_MAX_TEXT_CTX, max_t);
    return launch_stream<true, false, true>("attention", qkv, out, row_start, batch, max_t, width, nullptr, stream);
}

}  // namespace kemr
