// KEMR_PREC_FP32X3: the kernels of the split-bf16 encoder mode that are not a GEMM epilogue (gemm.hip) or a LayerNorm store
// (layernorm.hip): attention on fp32 q | k | v and the im2col whose rows are A-side triples.
//
// Every fp32 operand a enters v_mfma_f32_16x16x32_bf16 as hi = rne_bf16(a), lo = rne_bf16(a - hi), and every product is
// hi.hi + lo.hi + hi.lo with fp32 accumulation (the convention of the terms == 3 similarity panels, sim.hip).
//
// attention_x3_kernel: one streaming (online-softmax) kernel for every shape of the mode -- non-causal up to KEMR_MAX_VISION_TOKENS
// tokens, causal, and the packed rows of the text tower.  A workgroup of 4 waves owns 64 queries of one (item, head), a wave 16 of
// them; the keys go by in chunks of 32.  Per chunk the workgroup splits the chunk's K and V rows once into LDS (K as [key][d],
// V transposed as [d][slot]); a wave then computes
//   S^T[key][query] = K . Q^T     2 key tiles x 2 d halves x 3 products   (lane: query = lane & 15, keys (lane >> 4) * 4 + r of a tile)
//   O^T[d][query]  += V^T . P^T   4 d tiles x 3 products                  (lane: the same query, d = tile * 16 + (lane >> 4) * 4 + r)
// so the softmax statistics of a query live in the lanes that hold its scores and its output (no transposition through LDS): the
// S^T accumulators of a lane ARE its B operand of the second product once the key slots are numbered to match -- MFMA slot
// (lane >> 4) * 8 + j holds key (lane >> 4) * 4 + j of tile 0 for j < 4 and of tile 1 for j >= 4 -- and V^T is written to LDS in
// that slot order.  Softmax in fp32 (v_exp_f32 on (s - m) log2 e; the argument's rounding, |s - m| 2^-23, is far inside the
// 3 x 2^-16 |s| that the operand split leaves in a logit), P split like every other operand, O / l at the end, stored as the
// A-side triple [hi | lo | hi] of the out-proj GEMM.  Same bits on every launch (no atomics, fixed order).
#include "attention_tile.h"

namespace kemr {

namespace {

constexpr int AQ = 64;     // queries per workgroup
constexpr int AK = 32;     // keys per chunk
constexpr int KLD = 72;    // bf16 per K row in LDS: 64 + 8 (144 B: ds_read_b128 of 16 consecutive rows spread over the banks)
constexpr int VLD = 40;    // bf16 per V^T row: 32 slots + 8 (80 B)

__global__ __launch_bounds__(256) void attention_x3_kernel(const float* __restrict__ qkv, bf16_t* __restrict__ out,
                                                           const int* __restrict__ row_start, int T, int width, int causal) {
    __shared__ __attribute__((aligned(16))) bf16_t sKh[AK * KLD];
    __shared__ __attribute__((aligned(16))) bf16_t sKl[AK * KLD];
    __shared__ __attribute__((aligned(16))) bf16_t sVh[64 * VLD];
    __shared__ __attribute__((aligned(16))) bf16_t sVl[64 * VLD];

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int lq = lane & 15, g = lane >> 4;
    const int h = blockIdx.y, b = blockIdx.z;
    int r0 = b * T, len = T;
    if (row_start) {
        r0 = row_start[b];
        len = row_start[b + 1] - r0;
        len = len < 0 ? 0 : (len > T ? T : len);
    }
    const int q0 = blockIdx.x * AQ;
    if (q0 >= len) return;                                  // the whole workgroup
    const int ld = 3 * width;
    const float* base = qkv + (size_t)r0 * ld + h * 64;
    const int qi = q0 + wid * 16 + lq;                      // this lane's query
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);

    bf16x8 qh[2], ql[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        float4 a = z4, bb = z4;
        if (qi < len) {
            const float* src = base + (size_t)qi * ld + c * 32 + g * 8;
            a = *(const float4*)src;
            bb = *(const float4*)(src + 4);
        }
        split8(a, bb, qh[c], ql[c]);
    }

    const float NEG_INF = -__builtin_inff();
    float m = NEG_INF, lsum = 0.f;
    f32x4 acc[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) acc[dt] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int kend = causal ? (len < q0 + AQ ? len : q0 + AQ) : len;
    for (int k0 = 0; k0 < kend; k0 += AK) {
        __syncthreads();                                    // the previous chunk has been read
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int idx = tid + i * 256;
            const int key = idx >> 4, d4 = (idx & 15) * 4;
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
        __syncthreads();

        f32x4 st[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            st[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const int off = (t * 16 + lq) * KLD + c * 32 + g * 8;
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
            const bool ok = kk < len && (!causal || kk <= qi);
            s[j] = ok ? st[j >> 2][j & 3] : NEG_INF;
            cmax = fmaxf(cmax, s[j]);
        }
        // attention_tile.h's row_max (and row_sum at the end), spelled out: the kernel is kept at the previous commit's code
        cmax = fmaxf(cmax, __shfl_xor(cmax, 16));
        cmax = fmaxf(cmax, __shfl_xor(cmax, 32));
        const float m_new = fmaxf(m, cmax);
        const float m_use = m_new == NEG_INF ? 0.f : m_new;          // a query with no key yet: every p is exp2(-inf) = 0
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
        for (int dt = 0; dt < 4; ++dt) {
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
    bf16_t* dst = out + (size_t)(r0 + qi) * ld + h * 64 + g * 4;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
        uint2 hi, lo;
        split_bf16x2(acc[dt][0] / lsum, acc[dt][1] / lsum, hi.x, lo.x);
        split_bf16x2(acc[dt][2] / lsum, acc[dt][3] / lsum, hi.y, lo.y);
        *(uint2*)(dst + dt * 16) = hi;
        *(uint2*)(dst + dt * 16 + width) = lo;
        *(uint2*)(dst + dt * 16 + 2 * width) = hi;
    }
}

__global__ __launch_bounds__(256) void im2col_x3_kernel(const float* __restrict__ px, bf16_t* __restrict__ out, int image_size,
                                                        int patch, int grid, int kpad, int kvalid, long long total_pairs) {
    // embed.hip's im2col_kernel with the split store: one thread per pair of adjacent k
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    if (gid >= total_pairs) return;
    const int kp2 = kpad >> 1;
    const long long row = gid / kp2;
    const int k = (int)(gid - row * kp2) * 2;
    const int P = grid * grid;
    const int b = (int)(row / P), pi = (int)(row - (long long)b * P);
    const int py = pi / grid, pxi = pi - py * grid;
    float v[2];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const int kk = k + e;
        if (kk < kvalid) {
            const int c = kk / (patch * patch), rem = kk - c * patch * patch;
            const int dy = rem / patch, dx = rem - dy * patch;
            v[e] = px[(((size_t)b * 3 + c) * image_size + (py * patch + dy)) * image_size + pxi * patch + dx];
        } else {
            v[e] = 0.f;
        }
    }
    uint32_t hi, lo;
    split_bf16x2(v[0], v[1], hi, lo);
    bf16_t* dst = out + (size_t)row * 3 * kpad + k;
    *(uint32_t*)dst = hi;
    *(uint32_t*)(dst + kpad) = lo;
    *(uint32_t*)(dst + 2 * kpad) = hi;
}

}  // namespace

int launch_attention_x3(const float* qkv, bf16_t* out_panel, const int* row_start, int batch, int t, int width, int causal,
                        hipStream_t stream) {
    if (batch <= 0 || t <= 0) return KEMR_OK;
    if (width <= 0 || width % 64) KEMR_FAIL(KEMR_ERR_INVALID, "attention_x3: width %d is not a multiple of the head size 64", width);
    if (t > KEMR_MAX_VISION_TOKENS || (causal && t > KEMR_MAX_TEXT_CTX))
        KEMR_FAIL(KEMR_ERR_INVALID, "attention_x3: %d tokens (%s) not supported", t, causal ? "causal" : "non-causal");
    if (row_start && !causal) KEMR_FAIL(KEMR_ERR_INVALID, "attention_x3: packed rows are causal");
    if (batch > 65535) KEMR_FAIL(KEMR_ERR_INVALID, "attention_x3: batch %d too large", batch);
    ProfScope prof(PROF_ATTENTION, stream);
    hipLaunchKernelGGL(attention_x3_kernel, dim3((t + AQ - 1) / AQ, width / 64, batch), dim3(256), 0, stream, qkv, out_panel,
                       row_start, t, width, causal);
    KEMR_CHECK_LAUNCH("attention_x3_kernel");
    return KEMR_OK;
}

int launch_im2col_x3(const float* pixels, bf16_t* patches, int batch, int image_size, int patch, int kpad, hipStream_t stream) {
    const int grid = image_size / patch;
    const long long pairs = (long long)batch * grid * grid * (kpad / 2);
    if (pairs <= 0) return KEMR_OK;
    const long long blocks = (pairs + 255) / 256;
    if (blocks > 0x7fffffffLL) KEMR_FAIL(KEMR_ERR_INVALID, "im2col_x3: batch too large");
    ProfScope prof(PROF_OTHER, stream);
    hipLaunchKernelGGL(im2col_x3_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, pixels, patches, image_size, patch, grid, kpad,
                       3 * patch * patch, pairs);
    KEMR_CHECK_LAUNCH("im2col_x3_kernel");
    return KEMR_OK;
}

}  // namespace kemr
