// Fused pair-score contrastive loss: symmetric InfoNCE over S = head(q, img, tgt), forward and backward; the n x n scores never leave
// the CU.  It is infonce.hip with a fusion head between the logits and the softmax (nce_tile.h holds what the two share).
//
//   t2i = q img^T, t2t = q tgt^T (fp32 grade: bf16 pairs, hi.hi + lo.hi + hi.lo), s_ij = head(t2i_ij, t2t_ij; query i), z = s / tau
//   GATED   s = g_i t2i + (1 - g_i) t2t                                   g fp32 [n]: the head's gate, computed by the caller
//   LINEAR  s = b1 + sum_k w1_k max(0, w0_k0 t2i + w0_k1 t2t + b0_k)      rank.hip's linear_head_kernel, fma for fma
//   loss = (mean_i (lse_j z_ij - z_ii) + mean_j (lse_i z_ij - z_jj)) / 2,   G = dL/ds = ((P + Q) / (2 n) - I / n) / tau
//
// Forward, pairhead_stats_kernel<MODE>: a workgroup owns 128 rows and walks a chunk of 128-item tiles.  Per tile it runs the K loop twice
// (two logit tiles, 2 x 64 accumulator VGPRs a lane), forms the score in registers, dumps it to LDS and scans it exactly as
// infonce_stats_kernel does; merge and loss are infonce.hip's kernels.  The column statistics are the same kernel with img / tgt as the
// row operands, q as the other and the mixed segments swapped: both passes see the same bits of every t2i_ij and t2t_ij, hence of z_ij
// (the gate then indexes the tile's columns).
//
// Backward, pairhead_bwd_kernel<MODE>: one pass over the pairs on the forward's (row tile, chunk) grid; it recomputes the scores and forms
// G in registers from the saved lse values.
//   GATED   dL/dg_i = sum_j G_ij (t2i_ij - t2t_ij): each lane sums its 16 pairs of a row over the chunk's tiles, the 8 lanes of a row are
//           added in a fixed order through LDS, the (row, chunk) partials in chunk order by pairhead_gate_merge_kernel.
//   LINEAR  4 hidden + 1 sums over all n^2 pairs.  The outer loop is over hidden units: a lane adds its 64 pairs' four contributions, a
//           butterfly over the wave's 64 lanes adds those, and lane k mod 64 keeps unit k's four accumulators (16 VGPRs for 256 units).
//           Per workgroup the four waves are added in wave order, the partials go to the workspace and pairhead_param_reduce_kernel adds
//           them over the workgroups in index order in fp64.
// Every output has one owner and one summation order: no atomics; the same inputs give the same bits.
#include "nce_tile.h"

#pragma clang fp contract(off)

namespace kemr {

constexpr int PH_GATED = KEMR_PAIRHEAD_GATED, PH_LINEAR = KEMR_PAIRHEAD_LINEAR;
constexpr int PH_MAX_HIDDEN = 256;
constexpr int PH_HW_BYTES = PH_MAX_HIDDEN * 16;              // per unit (w0_k0, w0_k1, b0_k, w1_k)
constexpr int PH_SMEM = NCE_A_BYTES + PH_HW_BYTES;

struct PhArgs {
    const bf16_t* X1;       // row operand of the t2i tile
    const bf16_t* X2;       // row operand of the t2t tile
    const bf16_t* Y1;       // the other operand of the t2i tile
    const bf16_t* Y2;
    int n, dpad, swap;      // swap: rows are gallery items, columns queries
    float inv_t;
    const float* gate;      // GATED [n], per query
    const float* w0;        // LINEAR [hidden, 2]
    const float* b0;        // [hidden]
    const float* w1;        // [hidden]
    const float* b1;        // [1]
    int hidden;
    int nchunks, tiles_per_chunk, g_tiles;
    float* part;            // forward [n, nchunks, 2]
    float* diag;            // forward [n]
    const float* lse_x;     // backward: lse over the columns, per row
    const float* lse_y;     // backward: lse over the rows, per column
    float* bpart;           // backward: GATED [n, nchunks]; LINEAR [workgroups, 4 hidden + 1]
};

__device__ __forceinline__ void ph_load_units(const PhArgs& p, float4* hw, int tid) {
    for (int k = tid; k < p.hidden; k += 256) hw[k] = make_float4(p.w0[2 * k], p.w0[2 * k + 1], p.b0[k], p.w1[k]);
}

// sc = head(ti, tt) on the lane's 64 pairs: element [ci][qi][r] is row row0 + qi*16, column col0 + ci*16 + r
template <int MODE>
__device__ __forceinline__ void ph_score(const f32x4 (&ti)[4][4], const f32x4 (&tt)[4][4], const PhArgs& p, const float4* hw, int row0, int col0,
                                         f32x4 (&sc)[4][4]) {
    if (MODE == PH_GATED) {
        if (!p.swap) {
#pragma unroll
            for (int qi = 0; qi < 4; ++qi) {
                const int row = row0 + qi * 16;
                const float g = row < p.n ? p.gate[row] : 0.f;
                const float h = 1.f - g;
#pragma unroll
                for (int ci = 0; ci < 4; ++ci)
#pragma unroll
                    for (int r = 0; r < 4; ++r) sc[ci][qi][r] = g * ti[ci][qi][r] + h * tt[ci][qi][r];
            }
        } else {
#pragma unroll
            for (int ci = 0; ci < 4; ++ci)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int col = col0 + ci * 16 + r;
                    const float g = col < p.n ? p.gate[col] : 0.f;
                    const float h = 1.f - g;
#pragma unroll
                    for (int qi = 0; qi < 4; ++qi) sc[ci][qi][r] = g * ti[ci][qi][r] + h * tt[ci][qi][r];
                }
        }
    } else {
        const float b1 = p.b1[0];
#pragma unroll
        for (int ci = 0; ci < 4; ++ci)
#pragma unroll
            for (int qi = 0; qi < 4; ++qi) sc[ci][qi] = f32x4{b1, b1, b1, b1};
        for (int k = 0; k < p.hidden; ++k) {
            const float4 w = hw[k];
#pragma unroll
            for (int ci = 0; ci < 4; ++ci)
#pragma unroll
                for (int qi = 0; qi < 4; ++qi)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        sc[ci][qi][r] = fmaf(w.w, fmaxf(fmaf(w.x, ti[ci][qi][r], fmaf(w.y, tt[ci][qi][r], w.z)), 0.f), sc[ci][qi][r]);
        }
    }
}

// ------------------------------------------------------------------------------------------------ forward
template <int MODE>
__global__ __launch_bounds__(256) void pairhead_stats_kernel(const PhArgs p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* sS = (float*)smem;
    float4* hw = (float4*)(smem + NCE_A_BYTES);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wq = wid >> 1, wcn = wid & 1;
    const int lrow = lane & 15, lq = lane >> 4;
    const int qt = blockIdx.x / p.nchunks, chunk = blockIdx.x % p.nchunks;
    const int tile_begin = chunk * p.tiles_per_chunk;
    const int tile_end = min(tile_begin + p.tiles_per_chunk, p.g_tiles);
    const size_t ld = 2 * (size_t)p.dpad;
    const bf16_t* gX1 = p.X1 + (size_t)qt * NT * ld;
    const bf16_t* gX2 = p.X2 + (size_t)qt * NT * ld;
    const int q_local = tid & 127, half = tid >> 7;
    const int qrow = qt * NT + q_local;
    const bool q_valid = qrow < p.n;
    float m = -INFINITY, s = 0.f;
    if (MODE == PH_LINEAR) ph_load_units(p, hw, tid);         // visible behind the K loop's barriers

    for (int gtile = tile_begin; gtile < tile_end; ++gtile) {
        {
            f32x4 ti[4][4], tt[4][4], sc[4][4];
            nce_logit_tile(gX1, p.Y1 + (size_t)gtile * NT * ld, p.dpad, p.swap, smem, ti, wid, lane);
            nce_logit_tile(gX2, p.Y2 + (size_t)gtile * NT * ld, p.dpad, p.swap, smem, tt, wid, lane);
            ph_score<MODE>(ti, tt, p, hw, qt * NT + wq * 64 + lrow, gtile * NT + wcn * 64 + lq * 4, sc);
            nce_dump_tile(sc, sS, wid, lane);
        }
        __syncthreads();
        nce_scan_tile(sS, q_local, half, qrow, q_valid, gtile, p.n, p.inv_t, m, s, p.diag);
        __syncthreads();          // the scan is done with sS before the next tile's operands are staged over it
    }
    nce_store_part(sS, q_local, half, qrow, q_valid, m, s, p.nchunks, chunk, p.part);
}

// ------------------------------------------------------------------------------------------------ backward
__device__ __forceinline__ float ph_wave_sum(float v) {       // butterfly: every lane ends with the same sum, in one fixed order
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

template <int MODE>
__global__ __launch_bounds__(256) void pairhead_bwd_kernel(const PhArgs p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* sS = (float*)smem;
    float4* hw = (float4*)(smem + NCE_A_BYTES);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wq = wid >> 1, wcn = wid & 1;
    const int lrow = lane & 15, lq = lane >> 4;
    const int qt = blockIdx.x / p.nchunks, chunk = blockIdx.x % p.nchunks;
    const int tile_begin = chunk * p.tiles_per_chunk;
    const int tile_end = min(tile_begin + p.tiles_per_chunk, p.g_tiles);
    const size_t ld = 2 * (size_t)p.dpad;
    const bf16_t* gX1 = p.X1 + (size_t)qt * NT * ld;
    const bf16_t* gX2 = p.X2 + (size_t)qt * NT * ld;
    const int row0 = qt * NT + wq * 64 + lrow;
    const float inv_n = 1.0f / (float)p.n, half_inv_n = 0.5f / (float)p.n;
    if (MODE == PH_LINEAR) ph_load_units(p, hw, tid);
    float lse_r[4];
#pragma unroll
    for (int qi = 0; qi < 4; ++qi) lse_r[qi] = row0 + qi * 16 < p.n ? p.lse_x[row0 + qi * 16] : 0.f;

    float dg[4] = {0.f, 0.f, 0.f, 0.f};           // GATED: this lane's share of dL/dg of its four rows
    float uacc[4][4];                             // LINEAR: unit kb*64 + lane: sum of gp t2i, gp t2t, gp, G h  (gp = G where the unit is active)
    float b1acc = 0.f;
#pragma unroll
    for (int kb = 0; kb < 4; ++kb)
#pragma unroll
        for (int c = 0; c < 4; ++c) uacc[kb][c] = 0.f;

    for (int gtile = tile_begin; gtile < tile_end; ++gtile) {
        f32x4 ti[4][4], tt[4][4], G[4][4];
        nce_logit_tile(gX1, p.Y1 + (size_t)gtile * NT * ld, p.dpad, 0, smem, ti, wid, lane);
        nce_logit_tile(gX2, p.Y2 + (size_t)gtile * NT * ld, p.dpad, 0, smem, tt, wid, lane);
        const int col0 = gtile * NT + wcn * 64 + lq * 4;
        ph_score<MODE>(ti, tt, p, hw, row0, col0, G);
        // G = dL/ds * tau of the lane's pairs, 0 on pad rows and columns
#pragma unroll
        for (int ci = 0; ci < 4; ++ci)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int col = col0 + ci * 16 + r;
                const bool c_valid = col < p.n;
                const float lse_c = c_valid ? p.lse_y[col] : 0.f;
#pragma unroll
                for (int qi = 0; qi < 4; ++qi) {
                    const int row = row0 + qi * 16;
                    float v = 0.f;
                    if (c_valid && row < p.n) {
                        const float z = G[ci][qi][r] * p.inv_t;
                        v = (__builtin_amdgcn_exp2f((z - lse_r[qi]) * NCE_LOG2E) + __builtin_amdgcn_exp2f((z - lse_c) * NCE_LOG2E)) * half_inv_n;
                        if (col == row) v -= inv_n;
                    }
                    G[ci][qi][r] = v;
                }
            }
        if (MODE == PH_GATED) {
#pragma unroll
            for (int qi = 0; qi < 4; ++qi) {
                float a = 0.f;
#pragma unroll
                for (int ci = 0; ci < 4; ++ci)
#pragma unroll
                    for (int r = 0; r < 4; ++r) a += G[ci][qi][r] * (ti[ci][qi][r] - tt[ci][qi][r]);
                dg[qi] += a;
            }
        } else {
            float gs = 0.f;
#pragma unroll
            for (int ci = 0; ci < 4; ++ci)
#pragma unroll
                for (int qi = 0; qi < 4; ++qi)
#pragma unroll
                    for (int r = 0; r < 4; ++r) gs += G[ci][qi][r];
            b1acc += ph_wave_sum(gs);
#pragma unroll
            for (int kb = 0; kb < 4; ++kb) {
                const int kend = min(64, p.hidden - kb * 64);         // uniform
                for (int kk = 0; kk < kend; ++kk) {
                    const float4 w = hw[kb * 64 + kk];
                    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll
                    for (int ci = 0; ci < 4; ++ci)
#pragma unroll
                        for (int qi = 0; qi < 4; ++qi)
#pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                const float a = ti[ci][qi][r], b = tt[ci][qi][r], g = G[ci][qi][r];
                                const float pre = fmaf(w.x, a, fmaf(w.y, b, w.z));
                                const float gp = pre > 0.f ? g : 0.f;
                                a0 += gp * a;
                                a1 += gp * b;
                                a2 += gp;
                                a3 += g * fmaxf(pre, 0.f);
                            }
                    a0 = ph_wave_sum(a0);
                    a1 = ph_wave_sum(a1);
                    a2 = ph_wave_sum(a2);
                    a3 = ph_wave_sum(a3);
                    if (lane == kk) { uacc[kb][0] += a0; uacc[kb][1] += a1; uacc[kb][2] += a2; uacc[kb][3] += a3; }
                }
            }
        }
    }
    // the K loop's last barrier is behind every wave: the LDS is free
    if (MODE == PH_GATED) {
#pragma unroll
        for (int qi = 0; qi < 4; ++qi) sS[(wq * 64 + qi * 16 + lrow) * 8 + wcn * 4 + lq] = dg[qi];
        __syncthreads();
        const int row = qt * NT + tid;
        if (tid < NT && row < p.n) {
            float a = 0.f;
#pragma unroll
            for (int e = 0; e < 8; ++e) a += sS[tid * 8 + e];
            p.bpart[(size_t)row * p.nchunks + chunk] = a;
        }
    } else {
        const int stride = 4 * p.hidden + 1;
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) {
            const int k = kb * 64 + lane;
            if (k < p.hidden)
#pragma unroll
                for (int c = 0; c < 4; ++c) sS[wid * stride + k * 4 + c] = uacc[kb][c];
        }
        if (lane == 0) sS[wid * stride + 4 * p.hidden] = b1acc;
        __syncthreads();
        float* dst = p.bpart + (size_t)blockIdx.x * stride;
        for (int e = tid; e < stride; e += 256) dst[e] = ((sS[e] + sS[stride + e]) + sS[2 * stride + e]) + sS[3 * stride + e];
    }
}

// dL/dg[row] = the row's chunk partials in chunk order, / tau
__global__ __launch_bounds__(256) void pairhead_gate_merge_kernel(const float* __restrict__ bpart, int n, int nchunks, float inv_t,
                                                                  float* __restrict__ grad) {
    const int row = blockIdx.x * 256 + threadIdx.x;
    if (row >= n) return;
    float a = 0.f;
    for (int c = 0; c < nchunks; ++c) a += bpart[(size_t)row * nchunks + c];
    grad[row] = a * inv_t;
}

// grad = [dw0 (2 hidden) | db0 (hidden) | dw1 (hidden) | db1]: the workgroups' partials in index order, fp64, one thread per sum
__global__ __launch_bounds__(256) void pairhead_param_reduce_kernel(const float* __restrict__ bpart, int groups, int hidden,
                                                                    const float* __restrict__ w1, float inv_t, float* __restrict__ grad) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    const int stride = 4 * hidden + 1;
    if (e >= stride) return;
    double a = 0.0;
    for (int g = 0; g < groups; ++g) a += (double)bpart[(size_t)g * stride + e];
    a *= (double)inv_t;
    if (e == 4 * hidden) { grad[4 * hidden] = (float)a; return; }
    const int k = e >> 2, c = e & 3;
    if (c == 3) grad[3 * hidden + k] = (float)a;
    else {
        const float v = (float)(a * (double)w1[k]);
        if (c == 2) grad[2 * hidden + k] = v;
        else grad[2 * k + c] = v;
    }
}

// ------------------------------------------------------------------------------------------------ host side
struct PhLayout {
    int n256, dpad, g_tiles, nchunks, tpc, groups;
    size_t off_q, off_i, off_t, off_part, off_diag, off_term, off_bpart, bytes;
};

static PhLayout ph_layout(int mode, int n, int d, int hidden) {
    PhLayout L;
    L.n256 = (int)round_up(n, 256);
    L.dpad = (int)round_up(d, 64);
    L.g_tiles = (n + NT - 1) / NT;
    const int want = L.g_tiles < NCE_MAX_CHUNKS ? L.g_tiles : NCE_MAX_CHUNKS;
    L.tpc = (L.g_tiles + want - 1) / want;
    L.nchunks = (L.g_tiles + L.tpc - 1) / L.tpc;
    L.groups = L.g_tiles * L.nchunks;
    size_t at = 0;
    auto take = [&](size_t b) { const size_t o = at; at += (size_t)round_up((int64_t)b, 256); return o; };
    const size_t panel = (size_t)L.n256 * 2 * L.dpad * 2;
    L.off_q = take(panel);
    L.off_i = take(panel);
    L.off_t = take(panel);
    L.off_part = take((size_t)2 * n * NCE_MAX_CHUNKS * 2 * 4);
    L.off_diag = take((size_t)2 * n * 4);
    L.off_term = take((size_t)2 * n * 4);
    L.off_bpart = take(mode == PH_LINEAR ? (size_t)L.groups * (4 * hidden + 1) * 4 : (size_t)n * NCE_MAX_CHUNKS * 4);
    L.bytes = at;
    return L;
}

static bool ph_shape_ok(int mode, int n, int d, int hidden) {
    if (mode != PH_GATED && mode != PH_LINEAR) return false;
    if (n < 1 || n > 65536 || d < 4 || d > 1280 || d % 4) return false;
    return mode == PH_GATED || (hidden >= 1 && hidden <= PH_MAX_HIDDEN);
}

struct PhCall {
    int mode;
    const float *q, *img, *tgt;
    int n, d;
    float inv_t;
    const float *gate, *w0, *b0, *w1, *b1;
    int hidden;
    void* ws;
    size_t ws_bytes;
};

static int ph_check(const char* fn, const PhCall& c) {
    if (c.mode != PH_GATED && c.mode != PH_LINEAR) KEMR_FAIL(KEMR_ERR_INVALID, "%s: mode=%d is neither KEMR_PAIRHEAD_GATED nor KEMR_PAIRHEAD_LINEAR", fn, c.mode);
    if (c.n < 1 || c.n > 65536) KEMR_FAIL(KEMR_ERR_INVALID, "%s: n=%d not in 1..65536", fn, c.n);
    if (c.d < 4 || c.d > 1280 || c.d % 4) KEMR_FAIL(KEMR_ERR_INVALID, "%s: d=%d must be a multiple of 4 in 4..1280", fn, c.d);
    if (!(c.inv_t > 0.f) || !std::isfinite(c.inv_t)) KEMR_FAIL(KEMR_ERR_INVALID, "%s: inv_temperature=%g must be positive and finite", fn, (double)c.inv_t);
    if (!c.q) KEMR_FAIL(KEMR_ERR_INVALID, "%s: q_dev is null", fn);
    if (!c.img) KEMR_FAIL(KEMR_ERR_INVALID, "%s: img_dev is null", fn);
    if (!c.tgt) KEMR_FAIL(KEMR_ERR_INVALID, "%s: tgt_dev is null", fn);
    if (c.mode == PH_GATED) {
        if (!c.gate) KEMR_FAIL(KEMR_ERR_INVALID, "%s: gate_dev is null", fn);
    } else {
        if (c.hidden < 1 || c.hidden > PH_MAX_HIDDEN) KEMR_FAIL(KEMR_ERR_INVALID, "%s: hidden=%d not in 1..%d", fn, c.hidden, PH_MAX_HIDDEN);
        if (!c.w0) KEMR_FAIL(KEMR_ERR_INVALID, "%s: w0_dev is null", fn);
        if (!c.b0) KEMR_FAIL(KEMR_ERR_INVALID, "%s: b0_dev is null", fn);
        if (!c.w1) KEMR_FAIL(KEMR_ERR_INVALID, "%s: w1_dev is null", fn);
        if (!c.b1) KEMR_FAIL(KEMR_ERR_INVALID, "%s: b1_dev is null", fn);
    }
    const size_t need = ph_layout(c.mode, c.n, c.d, c.hidden).bytes;
    if (!c.ws || c.ws_bytes < need) KEMR_FAIL(KEMR_ERR_WORKSPACE, "%s: workspace %zu < %zu bytes", fn, c.ws ? c.ws_bytes : (size_t)0, need);
    if ((uintptr_t)c.ws % 256) KEMR_FAIL(KEMR_ERR_WORKSPACE, "%s: workspace must be 256-byte aligned", fn);
    return KEMR_OK;
}

static PhArgs ph_args(const PhCall& c, const PhLayout& L, int pass) {
    char* ws = (char*)c.ws;
    const bf16_t* pq = (const bf16_t*)(ws + L.off_q);
    const bf16_t* pi = (const bf16_t*)(ws + L.off_i);
    const bf16_t* pt = (const bf16_t*)(ws + L.off_t);
    PhArgs p{};
    p.X1 = pass ? pi : pq; p.X2 = pass ? pt : pq;
    p.Y1 = pass ? pq : pi; p.Y2 = pass ? pq : pt;
    p.n = c.n; p.dpad = L.dpad; p.swap = pass; p.inv_t = c.inv_t;
    p.gate = c.gate; p.w0 = c.w0; p.b0 = c.b0; p.w1 = c.w1; p.b1 = c.b1; p.hidden = c.mode == PH_LINEAR ? c.hidden : 0;
    p.nchunks = L.nchunks; p.tiles_per_chunk = L.tpc; p.g_tiles = L.g_tiles;
    return p;
}

static int ph_build_panels(const PhCall& c, const PhLayout& L, hipStream_t s) {
    char* ws = (char*)c.ws;
    KEMR_TRY(nce_launch_panel(c.q, c.n, c.d, L.dpad, L.n256, (bf16_t*)(ws + L.off_q), s));
    KEMR_TRY(nce_launch_panel(c.img, c.n, c.d, L.dpad, L.n256, (bf16_t*)(ws + L.off_i), s));
    KEMR_TRY(nce_launch_panel(c.tgt, c.n, c.d, L.dpad, L.n256, (bf16_t*)(ws + L.off_t), s));
    return KEMR_OK;
}

template <int MODE>
static int ph_launch_stats(const PhArgs& p, int groups, hipStream_t s) {
    static int attr_dev = -1;
    KEMR_TRY(nce_lds_attr(pairhead_stats_kernel<MODE>, PH_SMEM, &attr_dev));
    hipLaunchKernelGGL(pairhead_stats_kernel<MODE>, dim3(groups), dim3(256), PH_SMEM, s, p);
    KEMR_CHECK_LAUNCH("pairhead_stats_kernel");
    return KEMR_OK;
}

template <int MODE>
static int ph_launch_bwd(const PhArgs& p, int groups, hipStream_t s) {
    static int attr_dev = -1;
    KEMR_TRY(nce_lds_attr(pairhead_bwd_kernel<MODE>, PH_SMEM, &attr_dev));
    hipLaunchKernelGGL(pairhead_bwd_kernel<MODE>, dim3(groups), dim3(256), PH_SMEM, s, p);
    KEMR_CHECK_LAUNCH("pairhead_bwd_kernel");
    return KEMR_OK;
}

}  // namespace kemr

// ================================================================================================ C ABI
using namespace kemr;

extern "C" size_t kemr_pairhead_workspace_bytes(int mode, int n, int d, int hidden) {
    if (!ph_shape_ok(mode, n, d, hidden)) return 0;
    return ph_layout(mode, n, d, hidden).bytes;
}

extern "C" int kemr_pairhead_forward(int mode, const float* q_dev, const float* img_dev, const float* tgt_dev, int n, int d,
                                     float inv_temperature, const float* gate_dev, const float* w0_dev, const float* b0_dev,
                                     const float* w1_dev, const float* b1_dev, int hidden, float* loss_dev, float* lse_dev,
                                     void* workspace_dev, size_t workspace_bytes, void* stream) {
    const PhCall c{mode, q_dev, img_dev, tgt_dev, n, d, inv_temperature, gate_dev, w0_dev, b0_dev, w1_dev, b1_dev, hidden, workspace_dev, workspace_bytes};
    KEMR_TRY(ph_check("pairhead_forward", c));
    if (!loss_dev) KEMR_FAIL(KEMR_ERR_INVALID, "pairhead_forward: loss_dev is null");
    if (!lse_dev) KEMR_FAIL(KEMR_ERR_INVALID, "pairhead_forward: lse_dev is null");
    const PhLayout L = ph_layout(mode, n, d, hidden);
    char* ws = (char*)workspace_dev;
    hipStream_t s = (hipStream_t)stream;
    KEMR_TRY(ph_build_panels(c, L, s));
    float* term = (float*)(ws + L.off_term);
    for (int pass = 0; pass < 2; ++pass) {            // 0: rows of z (queries against the gallery), 1: columns (same products, same order)
        PhArgs p = ph_args(c, L, pass);
        p.part = (float*)(ws + L.off_part) + (size_t)pass * n * NCE_MAX_CHUNKS * 2;
        p.diag = (float*)(ws + L.off_diag) + (size_t)pass * n;
        if (mode == PH_GATED) KEMR_TRY(ph_launch_stats<PH_GATED>(p, L.groups, s));
        else KEMR_TRY(ph_launch_stats<PH_LINEAR>(p, L.groups, s));
        KEMR_TRY(nce_launch_merge(p.part, p.diag, n, L.nchunks, lse_dev + (size_t)pass * n, term + (size_t)pass * n, s));
    }
    KEMR_TRY(nce_launch_loss(term, n, loss_dev, s));
    return KEMR_OK;
}

extern "C" int kemr_pairhead_backward(int mode, const float* q_dev, const float* img_dev, const float* tgt_dev, const float* lse_dev, int n,
                                      int d, float inv_temperature, const float* gate_dev, const float* w0_dev, const float* b0_dev,
                                      const float* w1_dev, const float* b1_dev, int hidden, float* grad_dev, void* workspace_dev,
                                      size_t workspace_bytes, void* stream) {
    const PhCall c{mode, q_dev, img_dev, tgt_dev, n, d, inv_temperature, gate_dev, w0_dev, b0_dev, w1_dev, b1_dev, hidden, workspace_dev, workspace_bytes};
    KEMR_TRY(ph_check("pairhead_backward", c));
    if (!lse_dev) KEMR_FAIL(KEMR_ERR_INVALID, "pairhead_backward: lse_dev is null");
    if (!grad_dev) KEMR_FAIL(KEMR_ERR_INVALID, "pairhead_backward: grad_dev is null");
    const PhLayout L = ph_layout(mode, n, d, hidden);
    char* ws = (char*)workspace_dev;
    hipStream_t s = (hipStream_t)stream;
    KEMR_TRY(ph_build_panels(c, L, s));
    PhArgs p = ph_args(c, L, 0);
    p.lse_x = lse_dev;
    p.lse_y = lse_dev + n;
    p.bpart = (float*)(ws + L.off_bpart);
    if (mode == PH_GATED) {
        KEMR_TRY(ph_launch_bwd<PH_GATED>(p, L.groups, s));
        hipLaunchKernelGGL(pairhead_gate_merge_kernel, dim3((n + 255) / 256), dim3(256), 0, s, (const float*)p.bpart, n, L.nchunks, inv_temperature,
                           grad_dev);
        KEMR_CHECK_LAUNCH("pairhead_gate_merge_kernel");
    } else {
        KEMR_TRY(ph_launch_bwd<PH_LINEAR>(p, L.groups, s));
        hipLaunchKernelGGL(pairhead_param_reduce_kernel, dim3((4 * hidden + 1 + 255) / 256), dim3(256), 0, s, (const float*)p.bpart, L.groups, hidden,
                           w1_dev, inv_temperature, grad_dev);
        KEMR_CHECK_LAUNCH("pairhead_param_reduce_kernel");
    }
    return KEMR_OK;
}
