// The logit-tile machinery the fused contrastive kernels share (infonce.hip, pairhead.hip): the bf16-pair panels' K loop with its three
// virtual segments, the 128 x 128 fp32 tile per 256-thread workgroup, the per-row online (max, sum) scan of a tile in LDS, and the host
// launchers of the panel, merge and loss kernels that infonce.hip defines.
#pragma once
#include "common.h"
#include <cmath>

// z = fl(s / tau) is ONE rounded value everywhere it is used (infonce.hip): nothing below may be contracted into an fma.
#pragma clang fp contract(off)

namespace kemr {

constexpr int NBK = 64;
constexpr int NT = 128;           // tile edge
constexpr int NLD = 132;          // LDS row stride of the logit tile in floats (sim.hip SLD)
constexpr int NCE_TILE_BYTES = NT * NBK * 2;                  // 16 KiB: one operand tile of one K step
constexpr int NCE_A_BYTES = NT * NLD * 4;                     // 67 584: logit tile, aliases the two operand stages (65 536)
constexpr int NCE_P_BYTES = 4 * NCE_TILE_BYTES;               // dL/dz tile as [hi k0 | hi k1 | lo k0 | lo k1]
constexpr int NCE_MAX_CHUNKS = 16;
constexpr int NCE_MAX_NS = 2;         // 3 (192 accumulator VGPRs) spills 36 registers next to the logit tile's 64
constexpr float NCE_LOG2E = 1.4426950408889634f;

__device__ __forceinline__ void nce_glds16(const void* gsrc, void* lds_wave_base) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)gsrc,
                                     (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0, 0);
}

// ------------------------------------------------------------------------------------------------ logit tile
// acc[ci][qi][r] = S[x row wq*64 + qi*16 + lrow][y row wcn*64 + ci*16 + lq*4 + r] over hi.hi + (lo.hi, hi.lo | swap: hi.lo, lo.hi).
// Ends behind a workgroup barrier: every wave is done with the stages, the caller may overwrite them.
__device__ __forceinline__ void nce_logit_tile(const bf16_t* __restrict__ gX, const bf16_t* __restrict__ gY, int dpad, int swap, char* smem,
                                               f32x4 (&acc)[4][4], int wid, int lane) {
    constexpr int STAGE_BYTES = 2 * NCE_TILE_BYTES;
    const int ld = 2 * dpad;
    const int srow = lane >> 3, schunk = lane & 7;
    const int lrow = lane & 15, lq = lane >> 4;
    const int swz = lrow >> 1;
    const int wq = wid >> 1, wcn = wid & 1;
    const int per = dpad / NBK, nt = 3 * per;
    auto stage = [&](int buf, int kt) {
        char* sA = smem + buf * STAGE_BYTES;         // Y tile
        char* sB = sA + NCE_TILE_BYTES;              // X tile
        const int term = kt / per, k0 = (kt - term * per) * NBK;
        const int xseg = swap ? (term == 2) : (term == 1);
        const int yseg = swap ? (term == 1) : (term == 2);
        const int xo = xseg * dpad + k0, yo = yseg * dpad + k0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int piece = wid * 4 + j;
            const int r = piece * 8 + srow;
            const int c = schunk ^ ((r >> 1) & 7);
            nce_glds16(gY + (size_t)r * ld + yo + c * 8, sA + piece * 1024);
            nce_glds16(gX + (size_t)r * ld + xo + c * 8, sB + piece * 1024);
        }
    };
#pragma unroll
    for (int ci = 0; ci < 4; ++ci)
#pragma unroll
        for (int qi = 0; qi < 4; ++qi) acc[ci][qi] = f32x4{0.f, 0.f, 0.f, 0.f};
    stage(0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (int kt = 0; kt < nt; ++kt) {
        const int cur = kt & 1;
        if (kt + 1 < nt) stage(cur ^ 1, kt + 1);
        const char* sA = smem + cur * STAGE_BYTES + (wcn * 64 + lrow) * 128;
        const char* sB = smem + cur * STAGE_BYTES + NCE_TILE_BYTES + (wq * 64 + lrow) * 128;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            const int coff = ((kk * 4 + lq) ^ swz) << 4;
            bf16x8 yf[4], xf[4];
#pragma unroll
            for (int ci = 0; ci < 4; ++ci) yf[ci] = *(const bf16x8*)(sA + ci * 16 * 128 + coff);
#pragma unroll
            for (int qi = 0; qi < 4; ++qi) xf[qi] = *(const bf16x8*)(sB + qi * 16 * 128 + coff);
#pragma unroll
            for (int ci = 0; ci < 4; ++ci)
#pragma unroll
                for (int qi = 0; qi < 4; ++qi)
                    acc[ci][qi] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(yf[ci], xf[qi], acc[ci][qi], 0, 0, 0);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
}

__device__ __forceinline__ void nce_dump_tile(const f32x4 (&acc)[4][4], float* sS, int wid, int lane) {
    const int lrow = lane & 15, lq = lane >> 4;
    const int wq = wid >> 1, wcn = wid & 1;
#pragma unroll
    for (int ci = 0; ci < 4; ++ci)
#pragma unroll
        for (int qi = 0; qi < 4; ++qi) {
            const f32x4 v = acc[ci][qi];
            *(float4*)(sS + (wq * 64 + qi * 16 + lrow) * NLD + wcn * 64 + ci * 16 + lq * 4) = make_float4(v[0], v[1], v[2], v[3]);
        }
}

// One tile's share of a row's statistics: thread (q_local, half) folds its 64 logits of the tile in sS (pad columns masked) into the
// running (m, s) pair and, where the tile holds it, writes the row's diagonal logit.  z = fl(score * inv_t).
__device__ __forceinline__ void nce_scan_tile(const float* sS, int q_local, int half, int qrow, bool q_valid, int gtile, int n, float inv_t,
                                              float& m, float& s, float* __restrict__ diag) {
    const int c0 = gtile * NT + half * 64;
    const int nvalid = min(64, n - c0);              // pad columns (logit 0) are not data
    if (q_valid && nvalid > 0) {
        const float* rowp = sS + q_local * NLD + half * 64;
        float tm = -INFINITY;
#pragma unroll 4
        for (int j4 = 0; j4 < 16; ++j4) {
            const float4 v4 = *(const float4*)(rowp + j4 * 4);
            const float ve[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (j4 * 4 + e < nvalid) tm = fmaxf(tm, ve[e] * inv_t);
        }
        if (tm > m) {                                  // exp2(-inf) = 0 on the first tile
            s *= __builtin_amdgcn_exp2f((m - tm) * NCE_LOG2E);
            m = tm;
        }
        float ts = 0.f;
#pragma unroll 4
        for (int j4 = 0; j4 < 16; ++j4) {
            const float4 v4 = *(const float4*)(rowp + j4 * 4);
            const float ve[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (j4 * 4 + e < nvalid) ts += __builtin_amdgcn_exp2f((ve[e] * inv_t - m) * NCE_LOG2E);
        }
        s += ts;
        const int dj = qrow - c0;
        if (dj >= 0 && dj < 64) diag[qrow] = rowp[dj] * inv_t;        // one owner per row
    }
}

// The two scanner threads of a row merge their pairs through xs (LDS, 512 floats) and thread half 0 stores the (row, chunk) pair.
__device__ __forceinline__ void nce_store_part(float* xs, int q_local, int half, int qrow, bool q_valid, float m, float s, int nchunks, int chunk,
                                               float* __restrict__ part) {
    xs[(q_local * 2 + half) * 2] = m;
    xs[(q_local * 2 + half) * 2 + 1] = s;
    __syncthreads();
    if (q_valid && half == 0) {
        const float m0 = xs[q_local * 4], s0 = xs[q_local * 4 + 1], m1 = xs[q_local * 4 + 2], s1 = xs[q_local * 4 + 3];
        const float mm = fmaxf(m0, m1);
        float ss = 0.f;
        if (m0 > -INFINITY) ss += s0 * __builtin_amdgcn_exp2f((m0 - mm) * NCE_LOG2E);
        if (m1 > -INFINITY) ss += s1 * __builtin_amdgcn_exp2f((m1 - mm) * NCE_LOG2E);
        float* dst = part + ((size_t)qrow * nchunks + chunk) * 2;
        dst[0] = mm;
        dst[1] = ss;
    }
}

// ---- host launchers of infonce.hip's kernels (asynchronous on s)
// panel [n256, 2 dpad] = [hi | lo] of src [n, d]; pad rows and columns +0
int nce_launch_panel(const float* src, int n, int d, int dpad, int n256, bf16_t* out, hipStream_t s);
// lse[row] = log of the chunks' sums merged in chunk order; term[row] = lse - diag[row]
int nce_launch_merge(const float* part, const float* diag, int n, int nchunks, float* lse, float* term, hipStream_t s);
// loss[1] = mean term[0 .. n), loss[2] = mean term[n .. 2 n), loss[0] = their mean: fp64, fixed tree
int nce_launch_loss(const float* term, int n, float* loss, hipStream_t s);

template <typename K>
static int nce_lds_attr(K kern, int bytes, int* attr_dev) {
    int dev = 0;
    KEMR_CHECK_HIP(hipGetDevice(&dev));
    if (*attr_dev != dev) {
        KEMR_CHECK_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
        *attr_dev = dev;
    }
    return KEMR_OK;
}

}  // namespace kemr
