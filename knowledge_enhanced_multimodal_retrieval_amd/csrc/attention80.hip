// Head-dim-80 attention: the vision tower of ViT-H-14 (width 1280 = 16 heads of 80, 257 tokens).  Three kernels, the head-dim-80
// forms of attention_kernel / attention_pooled_kernel (attention.hip) and attention_x3_kernel (fp32x3.hip); the head-dim-64
// kernels are not touched.  Non-causal only: no text tower has heads of 80.
//
// attention80_kernel -- the design of attention_kernel: one workgroup per (image, head), the whole K and V of that head in LDS
// (T <= 288 keys), a wave owns 16-query tiles and keeps the full score row in registers, plain softmax, v_mfma_f32_16x16x32_bf16
// throughout; lane ownership, k-slot order, the LDS image (Img80: rows of 160 B, no swizzle) and the rounding points are
// attention_tile.h's.
//   S^T tile = K_tile . Q^T: the contraction over 80 is two K = 32 steps (columns 0..63) and a THIRD K = 32 step whose k slots
//              0..15 are columns 64..79 and whose slots 16..31 are zero in BOTH operands.  Slot 8 * lq + j belongs to lane group
//              lq = lane >> 4, so the zero slots are the lanes lq >= 2: their Q registers are cleared in the kernel and their K
//              read goes to the chunk of zeros the kernel writes behind the V image.  Nothing beyond column 79 of a head is
//              ever loaded -- columns 80..95 would be the next head, the next plane of the row, or (V of the last row) memory past
//              the allocation.
//   O^T      = V^T . P^T: 5 d-tiles of 16 instead of 4.
// LDS per workgroup: 288 keys x 160 B x 2 + 16 = 92 176 B, so ONE workgroup per CU (two would need 184 KB of the CU's 160 KiB; a
// 257-key image cannot go below 272 rows = 87 KB either), not the two of the head-dim-64 kernel.  The occupancy is restored inside
// the workgroup: EIGHT waves (two per SIMD, 17 query tiles = 3 / 2 / 2 / 2 / 2 / 2 / 2 / 2) share one K / V image, <= 256 VGPRs
// each.  Four waves (one per SIMD, 5 / 4 / 4 / 4) are kept as debug switch attn80_waves = 4 for the comparison; the measured
// launch times of both are in DESIGN.md section "Head dim 80".  T == 257 is a compile-time specialisation as in attention_kernel
// (every pad-key mask and tile-skip test folds away); other lengths keep T a run-time value and run with four waves, whose 512-VGPR
// budget holds the uniform conditions of the unrolled tiles (up to 166 SGPRs spilled to VGPR lanes, no scratch).
//
// attention80_pooled_kernel -- attention_pooled_kernel for 80 columns: sixteen lanes per key row (ten of them hold a 16-byte
// chunk), four keys per pass; out[d] with lane = (4 columns of d, key parity), the two parities added by one shuffle.
//
// attention80_x3_kernel -- attention_x3_kernel (streaming, hi / lo operand pairs, three products) with d padded to 96 in the K
// image (zeros written once by the kernel), the Q pad slots cleared in registers, 80 V^T rows and 5 output d-tiles.  A kernel of its
// own: as the HD = 80 instantiation of one attention_x3_kernel<HD> template it had the same bits but measured 0.9 % and 1.2 % slower
// at 64 x 257 x 1280, where two copies of the previous library differed by 0.02 % and 0.07 % (profiles/attention_tile_refactor_ab.json).
#include "attention_tile.h"

namespace kemr {

int g_attn80_waves = 0;    // tools: 0 = the default (8 waves per workgroup), 4 = one wave per SIMD (T = 257 only)

namespace {

constexpr int HD = 80;             // head dim
constexpr int ROWB = Img80::ROWB;  // bytes per K / V row in LDS
constexpr int RCH = HD / 8;        // 16-byte chunks per row

typedef unsigned u32x4_ __attribute__((ext_vector_type(4)));

template <int NT32, int TC, int NW>        // keys padded to NT32 * 32; TC > 0: compile-time sequence length; NW waves per workgroup
__global__ __launch_bounds__(NW * 64) void attention80_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ out, int T_rt,
                                                              int width, int xbatch) {
    constexpr int TP = NT32 * 32;
    constexpr int NT16 = NT32 * 2;
    constexpr int NTH = NW * 64;
    constexpr int NCH = (TP * RCH + NTH - 1) / NTH;     // 16-byte chunks of K (and of V) per thread
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* sK = smem;
    char* sV = smem + TP * ROWB;
    char* sZ = smem + 2 * TP * ROWB;                    // 16 bytes of zeros: the K operand of the k slots 16..31 of the third step

    int h, b;
    __builtin_assume(xbatch != 0);                      // xbatch = batch >= 1: this kernel always deals the images to the XCDs
    if (!attn_item(xbatch, h, b)) return;               // (the whole workgroup)
    const int T = TC > 0 ? TC : T_rt;
    const size_t row0 = (size_t)b * T;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ld = 3 * width;
    const bf16_t* base = qkv + row0 * ld + h * HD;
    const int lrow = lane & 15, lq = lane >> 4;
    const int nqt = (T + 15) >> 4;
    const unsigned qkeep = lq < 2 ? 0xffffffffu : 0u;

    // a query tile's three B fragments: columns 0..31, 32..63, and 64..79 in the k slots 0..15 (lanes lq < 2) with zeros made here in
    // the slots 16..31 (the lanes lq >= 2 load the columns 64 + 8 (lq & 1) .. of their own head again and clear them)
    auto load_q = [&](int qrow, bf16x8 (&dst)[3]) {
        const int qc = qrow < T ? qrow : T - 1;
        const bf16_t* p = base + (size_t)qc * ld;
        dst[0] = *(const bf16x8*)(p + lq * 8);
        dst[1] = *(const bf16x8*)(p + 32 + lq * 8);
        u32x4_ t = *(const u32x4_*)(p + 64 + (lq & 1) * 8);
        t.x &= qkeep; t.y &= qkeep; t.z &= qkeep; t.w &= qkeep;
        dst[2] = __builtin_bit_cast(bf16x8, t);
    };
    bf16x8 qn[3];
    load_q(wid * 16 + lrow, qn);                        // first query tile: its loads overlap the K / V staging
    if (tid == 0) *(uint4*)sZ = make_uint4(0u, 0u, 0u, 0u);
    {
        uint4 kv[NCH], vv[NCH];
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
            const int idx = tid + i * NTH;
            const int row = idx / RCH, c = idx - row * RCH;
            const int rc = row < T ? row : T - 1;       // pad rows (and the threads beyond the image) load the last valid row; zeroed / skipped below
            const u32x4_ a_ = __builtin_nontemporal_load((const u32x4_*)(base + (size_t)rc * ld + width + c * 8));
            const u32x4_ b_ = __builtin_nontemporal_load((const u32x4_*)(base + (size_t)rc * ld + 2 * width + c * 8));
            kv[i] = make_uint4(a_.x, a_.y, a_.z, a_.w);
            vv[i] = make_uint4(b_.x, b_.y, b_.z, b_.w);
        }
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
            const int idx = tid + i * NTH;
            const int row = idx / RCH, c = idx - row * RCH;
            if (idx < TP * RCH) {
                tile_put<Img80>(sK, row, c, kv[i], row < T);
                tile_put<Img80>(sV, row, c, vv[i], row < T);
            }
        }
    }
    __syncthreads();

    for (int qt = wid; qt < nqt; qt += NW) {           // wave-uniform trip count: EXEC stays full for the tr reads
        const int q = qt * 16 + lrow;
        bf16x8 qf[3] = {qn[0], qn[1], qn[2]};
        if (qt + NW < nqt) load_q(q + NW * 16, qn);    // prefetch the next query tile of this wave

        constexpr int G = (NT16 % 3 == 0) ? 3 : 2;
        constexpr int NG = NT16 / G;
        f32x4 s[NT16];
        bf16x8 kfr[2][G][3];
        auto load_group = [&](int g, bf16x8 (&dst)[G][3]) {
#pragma unroll
            for (int j = 0; j < G; ++j) {
                const int row = (g * G + j) * 16 + lrow;
                dst[j][0] = tile_row<Img80>(sK, row, lq);
                dst[j][1] = tile_row<Img80>(sK, row, 4 + lq);
                dst[j][2] = *(const bf16x8*)(lq < 2 ? sK + Img80::off(row, 8 + lq) : sZ);
            }
        };
        load_group(0, kfr[0]);
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            if (g + 1 < NG && (g + 1) * G * 16 < T) load_group(g + 1, kfr[(g + 1) & 1]);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int j = 0; j < G; ++j) {
                const int t = g * G + j;
                s[t] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (t * 16 < T) {                       // tiles made only of pad keys are skipped (uniform); the mask below covers them
                    s[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kfr[g & 1][j][0], qf[0], s[t], 0, 0, 0);
                    s[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kfr[g & 1][j][1], qf[1], s[t], 0, 0, 0);
                    s[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kfr[g & 1][j][2], qf[2], s[t], 0, 0, 0);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        // s[t][r] = S[query lrow][key t*16 + lq*4 + r]
        float mx = -INFINITY;
#pragma unroll
        for (int t = 0; t < NT16; ++t) {
            const bool partial = (t + 1) * 16 > T;      // only the boundary tiles need a mask
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (partial) {
                    const int key = t * 16 + lq * 4 + r;
                    s[t][r] = key < T ? s[t][r] : -INFINITY;
                }
                mx = fmaxf(mx, s[t][r]);
            }
        }
        const float mxl = row_max(mx) * LOG2E;
        f32x2_t sum2 = {0.f, 0.f};
        const f32x2_t l2 = {LOG2E, LOG2E}, nm = {-mxl, -mxl};
#pragma unroll
        for (int t = 0; t < NT16; ++t) tile_exp(s[t], l2, nm, sum2);

        f32x4 o[5];
#pragma unroll
        for (int dt = 0; dt < 5; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
        // O^T += V^T . P^T per 32-key block, V fragments double-buffered
        bf16x8 vfr[2][5];
        tile_tr<Img80>(sV, 0, lrow, lq, vfr[0]);
#pragma unroll
        for (int u = 0; u < NT32; ++u) {
            if (u * 32 >= T) continue;                  // a block that is all pad keys has P = 0 (uniform); the live blocks are a prefix
            if (u + 1 < NT32 && (u + 1) * 32 < T) tile_tr<Img80>(sV, u + 1, lrow, lq, vfr[(u + 1) & 1]);
            __builtin_amdgcn_sched_barrier(0);
            const bf16x8 pf = tile_pack(s[2 * u], s[2 * u + 1]);
#pragma unroll
            for (int dt = 0; dt < 5; ++dt)
                o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vfr[u & 1][dt], pf, o[dt], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
        const float sum = row_sum(sum2.x + sum2.y);
        // o[dt][r] = O[query lrow][d = dt*16 + lq*4 + r]
        if (q < T) tile_store(out + (row0 + q) * width + h * HD + lq * 4, o, 1.0f / sum);
    }
}

template <int NT32>
int launch80_nt(const bf16_t* qkv, bf16_t* out, int batch, int t, int width, hipStream_t stream) {
    constexpr int smem = NT32 * 32 * ROWB * 2 + Img80::ZERO;
    const dim3 grid(width / HD, (batch + 7) / 8 * 8);
    ProfScope prof(PROF_ATTENTION, stream);
    // run-time T (tests, other image sizes): four waves, whose 512-VGPR budget holds the uniform conditions of the unrolled tiles that
    // a run-time T leaves in registers
    void (*kern)(const bf16_t*, bf16_t*, int, int, int) = attention80_kernel<NT32, 0, 4>;
    int threads = 256;
    if constexpr (NT32 == 9) {
        if (t == 257 && g_attn80_waves == 4) kern = attention80_kernel<9, 257, 4>;
        else if (t == 257) { kern = attention80_kernel<9, 257, 8>; threads = 512; }
    }
    KEMR_CHECK_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, smem));
    hipLaunchKernelGGL(kern, grid, dim3(threads), smem, stream, qkv, out, t, width, batch);
    KEMR_CHECK_LAUNCH("attention80_kernel");
    return KEMR_OK;
}

// ---- the attention of the pooled row alone (last block of the vision tower), 80 columns per head --------------------------------
// attention_pooled_kernel's arithmetic: the scores of the one query against the item's keys (a lane's eight bf16 products summed in
// fp32 by fma, then the lanes of the key by shuffles), softmax in fp32 with P rounded to bf16 and the row sum taken before the
// rounding, out[d] = sum_j p_j v_j[d] over the keys of a parity in order, the two parities added, one division.

constexpr int PMAXK = 320;         // keys per item the LDS row holds (towers of head dim 80 have at most 288 tokens)

__global__ __launch_bounds__(256) void attention80_pooled_kernel(const bf16_t* __restrict__ q, const bf16_t* __restrict__ qkv,
                                                                 bf16_t* __restrict__ out, int items, int tokens, int width) {
    __shared__ float sp[4][PMAXK];
    const int heads = width / HD, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int item = blockIdx.x * 4 + wv;
    if (item >= items * heads) return;                  // (no barrier below: a wave works on its own)
    const int b = item / heads, h = item - b * heads;
    const int r0 = b * tokens;
    const int nk = tokens < 1 ? 1 : (tokens > PMAXK ? PMAXK : tokens);
    const size_t ld = 3 * (size_t)width;
    // scores: sixteen lanes share a key row, the first ten hold one 16-byte chunk each (the other six add zeros made here); four
    // keys per pass
    const int ck = lane & 15, kq = lane >> 4;
    const bool live = ck < RCH;
    const int cc = live ? ck : RCH - 1;                 // the idle lanes load a chunk of their own head and drop it
    float qf[8];
    {
        const uint4 v = ((const uint4*)(q + (size_t)b * width + h * HD))[cc];
        const uint32_t w4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            qf[2 * k] = bf16_to_f32((bf16_t)(w4[k] & 0xffff));
            qf[2 * k + 1] = bf16_to_f32((bf16_t)(w4[k] >> 16));
        }
    }
    const bf16_t* kbase = qkv + (size_t)r0 * ld + width + h * HD + cc * 8;
    const int npass = (nk + 3) >> 2;
    for (int pss = 0; pss < npass; ++pss) {
        const int j = pss * 4 + kq;
        const int jc = j < nk ? j : nk - 1;
        const uint4 v = *(const uint4*)(kbase + (size_t)jc * ld);
        const uint32_t w4[4] = {v.x, v.y, v.z, v.w};
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            s = fmaf(qf[2 * k], bf16_to_f32((bf16_t)(w4[k] & 0xffff)), s);
            s = fmaf(qf[2 * k + 1], bf16_to_f32((bf16_t)(w4[k] >> 16)), s);
        }
        s = live ? s : 0.f;
        s += __shfl_xor(s, 1);
        s += __shfl_xor(s, 2);
        s += __shfl_xor(s, 4);
        s += __shfl_xor(s, 8);
        if (ck == 0 && j < nk) sp[wv][j] = s;
    }
    // the softmax of attention_pooled_kernel, line for line (the wave's LDS row is written and read by this wave only).  As a shared
    // pooled_softmax<MAXK> in attention_tile.h it gave the same bits, but the 64-column op measured +0.06 % at 255 x 257 x 1024 and this one
    // +0.01 % over the slower of two copies of the previous library at 64 x 257 x 1280 in one of four runs, so both kernels keep theirs
    wave_lds_fence();
    float sc[PMAXK / 64];
    float mx = -INFINITY;
#pragma unroll
    for (int pss = 0; pss < PMAXK / 64; ++pss) {
        const int j = pss * 64 + lane;
        sc[pss] = j < nk ? sp[wv][j] : -INFINITY;
        mx = fmaxf(mx, sc[pss]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    float sum = 0.f;
#pragma unroll
    for (int pss = 0; pss < PMAXK / 64; ++pss) {
        const int j = pss * 64 + lane;
        const float p = __builtin_amdgcn_exp2f((sc[pss] - mx) * LOG2E);         // -inf -> 0 beyond the keys
        sum += p;
        sp[wv][j] = bf16_to_f32(f32_to_bf16(p));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    wave_lds_fence();                                  // the bf16-rounded P row: stores of all lanes before any lane's loads
    // lane = (dq: columns 4 dq .. 4 dq + 3, key parity): lanes 0..19 the even keys, 20..39 the odd ones, 40..63 idle
    const int par = lane / 20, dq = lane - par * 20;
    float a[4] = {0.f, 0.f, 0.f, 0.f};
    if (par < 2) {
        const bf16_t* vp = qkv + (size_t)r0 * ld + 2 * width + h * HD + dq * 4;
#pragma unroll 4
        for (int j = par; j < nk; j += 2) {
            const uint2 v = *(const uint2*)(vp + (size_t)j * ld);
            const float p = sp[wv][j];
            a[0] = fmaf(p, bf16_to_f32((bf16_t)(v.x & 0xffff)), a[0]);
            a[1] = fmaf(p, bf16_to_f32((bf16_t)(v.x >> 16)), a[1]);
            a[2] = fmaf(p, bf16_to_f32((bf16_t)(v.y & 0xffff)), a[2]);
            a[3] = fmaf(p, bf16_to_f32((bf16_t)(v.y >> 16)), a[3]);
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) a[k] += __shfl_down(a[k], 20);
    if (par == 0) {
        const float inv = 1.0f / sum;
        uint2 pk;
        pk.x = pack_bf16x2(a[0] * inv, a[1] * inv);
        pk.y = pack_bf16x2(a[2] * inv, a[3] * inv);
        *(uint2*)(out + (size_t)b * width + h * HD + dq * 4) = pk;
    }
}

// ---- KEMR_PREC_FP32X3 ------------------------------------------------------------------------------------------------------------
constexpr int AQ = 64;     // queries per workgroup
constexpr int AK = 32;     // keys per chunk
constexpr int KLD = 104;   // bf16 per K row in LDS: 80 + 16 zeros + 8 (208 B = 13 slots of 16 B: ds_read_b128 of 16 consecutive rows spread over the banks)
constexpr int VLD = 40;    // bf16 per V^T row: 32 slots + 8 (80 B)

__global__ __launch_bounds__(256) void attention80_x3_kernel(const float* __restrict__ qkv, bf16_t* __restrict__ out, int T, int width) {
    __shared__ __attribute__((aligned(16))) bf16_t sKh[AK * KLD];
    __shared__ __attribute__((aligned(16))) bf16_t sKl[AK * KLD];
    __shared__ __attribute__((aligned(16))) bf16_t sVh[HD * VLD];
    __shared__ __attribute__((aligned(16))) bf16_t sVl[HD * VLD];

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int lq = lane & 15, g = lane >> 4;
    const int h = blockIdx.y, b = blockIdx.z;
    const int r0 = b * T, len = T;
    const int q0 = blockIdx.x * AQ;
    if (q0 >= len) return;                                  // the whole workgroup
    const int ld = 3 * width;
    const float* base = qkv + (size_t)r0 * ld + h * HD;
    const int qi = q0 + wid * 16 + lq;                      // this lane's query
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);

    // Q: columns 0..31, 32..63, and 64..79 in the k slots 0..15 (g < 2) of a third step whose slots 16..31 are zeros made here
    bf16x8 qh[3], ql[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float4 a = z4, bb = z4;
        if (qi < len && (c < 2 || g < 2)) {
            const float* src = base + (size_t)qi * ld + c * 32 + g * 8;
            a = *(const float4*)src;
            bb = *(const float4*)(src + 4);
        }
        split8(a, bb, qh[c], ql[c]);
    }
    // the K image's pad columns 80..95, zeroed once (the staging below never writes them; the loop's first barrier orders this)
    if (tid < AK * 2) {
        const int key = tid >> 1, half = tid & 1;
        *(uint4*)(sKh + key * KLD + HD + half * 8) = make_uint4(0u, 0u, 0u, 0u);
        *(uint4*)(sKl + key * KLD + HD + half * 8) = make_uint4(0u, 0u, 0u, 0u);
    }

    const float NEG_INF = -__builtin_inff();
    float m = NEG_INF, lsum = 0.f;
    f32x4 acc[5];
#pragma unroll
    for (int dt = 0; dt < 5; ++dt) acc[dt] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int k0 = 0; k0 < len; k0 += AK) {
        __syncthreads();                                    // the previous chunk has been read
#pragma unroll
        for (int i = 0; i < 3; ++i) {                       // 32 keys x 20 groups of 4 columns = 640 items over 256 threads
            const int idx = tid + i * 256;
            if (idx < AK * (HD / 4)) {
                const int key = idx / (HD / 4), d4 = (idx - key * (HD / 4)) * 4;
                const int kk = k0 + key;
                float4 kv = z4, vv = z4;
                if (kk < len) {
                    const float* src = base + (size_t)kk * ld + d4;
                    kv = *(const float4*)(src + width);
                    vv = *(const float4*)(src + 2 * width);
                }
                uint2 hi, lo;
                split_bf16x2(kv.x, kv.y, hi.x, lo.x);
                split_bf16x2(kv.z, kv.w, hi.y, lo.y);
                *(uint2*)(sKh + key * KLD + d4) = hi;
                *(uint2*)(sKl + key * KLD + d4) = lo;
                split_bf16x2(vv.x, vv.y, hi.x, lo.x);
                split_bf16x2(vv.z, vv.w, hi.y, lo.y);
                const int slot = ((key & 15) >> 2) * 8 + (key >> 4) * 4 + (key & 3);
                sVh[(d4 + 0) * VLD + slot] = (bf16_t)(hi.x & 0xffff);
                sVh[(d4 + 1) * VLD + slot] = (bf16_t)(hi.x >> 16);
                sVh[(d4 + 2) * VLD + slot] = (bf16_t)(hi.y & 0xffff);
                sVh[(d4 + 3) * VLD + slot] = (bf16_t)(hi.y >> 16);
                sVl[(d4 + 0) * VLD + slot] = (bf16_t)(lo.x & 0xffff);
                sVl[(d4 + 1) * VLD + slot] = (bf16_t)(lo.x >> 16);
                sVl[(d4 + 2) * VLD + slot] = (bf16_t)(lo.y & 0xffff);
                sVl[(d4 + 3) * VLD + slot] = (bf16_t)(lo.y >> 16);
            }
        }
        __syncthreads();

        f32x4 st[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            st[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int off = (t * 16 + lq) * KLD + c * 32 + g * 8;       // c == 2, g >= 2: the zero columns 80..95
                const bf16x8 kh = *(const bf16x8*)(sKh + off);
                const bf16x8 kl = *(const bf16x8*)(sKl + off);
                st[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kh, qh[c], st[t], 0, 0, 0);
                st[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kh, ql[c], st[t], 0, 0, 0);
                st[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kl, qh[c], st[t], 0, 0, 0);
            }
        }
        float s[8];
        float cmax = NEG_INF;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int kk = k0 + (j >> 2) * 16 + g * 4 + (j & 3);
            s[j] = kk < len ? st[j >> 2][j & 3] : NEG_INF;
            cmax = fmaxf(cmax, s[j]);
        }
        // attention_tile.h's row_max (and row_sum at the end), spelled out: the kernel is kept at the previous commit's code
        cmax = fmaxf(cmax, __shfl_xor(cmax, 16));
        cmax = fmaxf(cmax, __shfl_xor(cmax, 32));
        const float m_new = fmaxf(m, cmax);
        const float m_use = m_new == NEG_INF ? 0.f : m_new;
        const float alpha = __builtin_amdgcn_exp2f((m - m_use) * LOG2E);
        m = m_new;
        float p[8];
        float psum = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            p[j] = __builtin_amdgcn_exp2f((s[j] - m_use) * LOG2E);
            psum += p[j];
        }
        lsum = lsum * alpha + psum;
        bf16x8 ph, pl;
        split8(make_float4(p[0], p[1], p[2], p[3]), make_float4(p[4], p[5], p[6], p[7]), ph, pl);
#pragma unroll
        for (int dt = 0; dt < 5; ++dt) {
            const int off = (dt * 16 + lq) * VLD + g * 8;
            const bf16x8 vh = *(const bf16x8*)(sVh + off);
            const bf16x8 vl = *(const bf16x8*)(sVl + off);
            f32x4 a = acc[dt];
            a[0] *= alpha; a[1] *= alpha; a[2] *= alpha; a[3] *= alpha;
            a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vh, ph, a, 0, 0, 0);
            a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vh, pl, a, 0, 0, 0);
            a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vl, ph, a, 0, 0, 0);
            acc[dt] = a;
        }
    }

    lsum += __shfl_xor(lsum, 16);
    lsum += __shfl_xor(lsum, 32);
    if (qi >= len) return;
    bf16_t* dst = out + (size_t)(r0 + qi) * ld + h * HD + g * 4;
#pragma unroll
    for (int dt = 0; dt < 5; ++dt) {
        uint2 hi, lo;
        split_bf16x2(acc[dt][0] / lsum, acc[dt][1] / lsum, hi.x, lo.x);
        split_bf16x2(acc[dt][2] / lsum, acc[dt][3] / lsum, hi.y, lo.y);
        *(uint2*)(dst + dt * 16) = hi;
        *(uint2*)(dst + dt * 16 + width) = lo;
        *(uint2*)(dst + dt * 16 + 2 * width) = hi;
    }
}

}  // namespace

int launch_attention80(const bf16_t* qkv, bf16_t* out, int batch, int t, int width, int causal, hipStream_t stream) {
    if (batch <= 0) return KEMR_OK;
    if (width <= 0 || width % HD != 0 || t <= 0) KEMR_FAIL(KEMR_ERR_INVALID, "attention (head dim 80): bad shape t=%d width=%d (width must be a multiple of 80)", t, width);
    if (causal) KEMR_FAIL(KEMR_ERR_INVALID, "attention (head dim 80): the causal form is not served (no text tower has heads of 80)");
    if (t > 288) KEMR_FAIL(KEMR_ERR_INVALID, "attention (head dim 80): sequence length %d > 288 not supported (the streaming kernel serves head dim 64 only)", t);
    if (batch > 65528) KEMR_FAIL(KEMR_ERR_INVALID, "attention (head dim 80): batch %d > 65528 (grid.y, rounded up to a multiple of 8)", batch);
    switch ((t + 31) / 32) {
        case 1: return launch80_nt<1>(qkv, out, batch, t, width, stream);
        case 2: return launch80_nt<2>(qkv, out, batch, t, width, stream);
        case 3: return launch80_nt<3>(qkv, out, batch, t, width, stream);
        case 4: return launch80_nt<4>(qkv, out, batch, t, width, stream);
        case 5: return launch80_nt<5>(qkv, out, batch, t, width, stream);
        case 6: return launch80_nt<6>(qkv, out, batch, t, width, stream);
        case 7: return launch80_nt<7>(qkv, out, batch, t, width, stream);
        case 8: return launch80_nt<8>(qkv, out, batch, t, width, stream);
        default: return launch80_nt<9>(qkv, out, batch, t, width, stream);
    }
}

int launch_attention80_pooled(const bf16_t* q, const bf16_t* qkv, bf16_t* out, int items, int tokens, int width, int causal,
                              hipStream_t stream) {
    if (items <= 0) return KEMR_OK;
    if (width <= 0 || width % HD != 0 || tokens <= 0) KEMR_FAIL(KEMR_ERR_INVALID, "attention (pooled row, head dim 80): bad shape t=%d width=%d (width must be a multiple of 80)", tokens, width);
    if (causal) KEMR_FAIL(KEMR_ERR_INVALID, "attention (pooled row, head dim 80): the causal form is not served (no text tower has heads of 80)");
    if (tokens > 288) KEMR_FAIL(KEMR_ERR_INVALID, "attention (pooled row, head dim 80): %d tokens > 288 not supported", tokens);
    ProfScope prof(PROF_ATTENTION, stream);
    const long waves = (long)items * (width / HD);
    hipLaunchKernelGGL(attention80_pooled_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, stream, q, qkv, out, items, tokens, width);
    KEMR_CHECK_LAUNCH("attention80_pooled_kernel");
    return KEMR_OK;
}

int launch_attention80_x3(const float* qkv, bf16_t* out_panel, int batch, int t, int width, int causal, hipStream_t stream) {
    if (batch <= 0 || t <= 0) return KEMR_OK;
    if (width <= 0 || width % HD) KEMR_FAIL(KEMR_ERR_INVALID, "attention_x3 (head dim 80): width %d is not a multiple of the head size 80", width);
    if (causal) KEMR_FAIL(KEMR_ERR_INVALID, "attention_x3 (head dim 80): the causal form is not served (no text tower has heads of 80)");
    if (t > 288) KEMR_FAIL(KEMR_ERR_INVALID, "attention_x3 (head dim 80): %d tokens > 288 not supported", t);
    if (batch > 65535) KEMR_FAIL(KEMR_ERR_INVALID, "attention_x3 (head dim 80): batch %d too large", batch);
    ProfScope prof(PROF_ATTENTION, stream);
    hipLaunchKernelGGL(attention80_x3_kernel, dim3((t + AQ - 1) / AQ, width / HD, batch), dim3(256), 0, stream, qkv, out_panel, t, width);
    KEMR_CHECK_LAUNCH("attention80_x3_kernel");
    return KEMR_OK;
}

}  // namespace kemr
