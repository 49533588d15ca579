// Fused InfoNCE (symmetric contrastive loss), forward and backward; the n x n logits never leave the CU.
//
//   z = a b^T / tau,  loss_a2b = mean_i (lse_j z_ij - z_ii),  loss_b2a = mean_j (lse_i z_ij - z_jj),  loss = their mean
//   dL/dz = (softmax_rows(z) + softmax_cols(z)) / (2 n) - I / n,  dL/da = dL/dz b / tau,  dL/db = dL/dz^T a / tau
//
// Operands are bf16 pair panels [ceil256(n), 2 dpad] = [hi | lo] (hi = rne(v), lo = rne(v - hi): the split of kemr_panel_build's terms == 3),
// and the K loop walks three virtual segments hi.hi + lo.hi + hi.lo over them, so one panel per operand serves both roles (sim.hip's
// panels store the third segment; here it would double the workspace).  The K loop itself is sim_kernel's: LDS-DMA staging, chunk-XOR
// swizzle, v_mfma_f32_16x16x32_bf16, a 128 x 128 fp32 tile per 256-thread workgroup.
// The logit tile, its dump, the per-row scan and the chunk merge live in nce_tile.h: pairhead.hip (the same loss over a fusion head's scores)
// shares them, and launches this file's panel, merge and loss kernels through nce_launch_*.
//
// Forward, infonce_stats_kernel: a workgroup owns 128 rows of X and walks a chunk of Y's 128-row tiles; two scanner threads per row
// keep an online (max, sum) pair over their 64 logits of every tile (pad columns masked) and the row's diagonal logit.  Per (row, chunk)
// pairs go to the workspace, infonce_merge_kernel combines them in chunk order, infonce_loss_kernel sums the n terms in fp64 in a fixed
// tree.  The column statistics are the same kernel on swapped operands with the two mixed segments swapped as well, so that z^T_ji
// accumulates the very products of z_ij in the very order: both passes see the same bits of every logit.
//
// Backward, infonce_bwd_kernel<NS>: a workgroup owns 128 rows of X and 128 NS output columns.  Per tile of Y it recomputes the logits,
// forms the dL/dz tile from the saved lse values in fp32, splits it into a bf16 pair in LDS and contracts it with Y^T (a transposed pair
// panel [2 dpadT, ceil256(n)], k = the tile's 128 items contiguous) in three products again.  The fp32 accumulators of 128 rows x 768
// columns would be 384 VGPRs a lane; NS <= 2 keeps them at 128 and splits wider outputs over workgroups, each recomputing the logits.
// dL/db is the same kernel on swapped operands.  Every output element has one owner and one summation order: no atomics.
#include "nce_tile.h"

// z = fl(s / tau) is ONE rounded value everywhere it is used: contracted into z - max or z - lse as an fma, the forward's maximum, its
// sum and the backward's recomputation would each see a different z (one item: lse != z, a loss and a gradient that are not 0).
#pragma clang fp contract(off)

namespace kemr {

// ------------------------------------------------------------------------------------------------ panels
// [n256, 2 dpad]: hi | lo; columns d .. dpad and rows n .. n256 are +0
__global__ __launch_bounds__(256) void infonce_panel_kernel(const float* __restrict__ src, int n, int d, int dpad, bf16_t* __restrict__ out,
                                                            long long total) {
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    if (gid >= total) return;
    const int half = dpad >> 1;
    const int i = (int)(gid % half) * 2;
    const long long row = gid / half;
    float v0 = 0.f, v1 = 0.f;
    if (row < n) {
        const float* s = src + (size_t)row * d;
        if (i < d) v0 = s[i];
        if (i + 1 < d) v1 = s[i + 1];
    }
    uint32_t hi, lo;
    split_bf16x2(v0, v1, hi, lo);
    bf16_t* dst = out + (size_t)row * (2 * dpad) + i;
    *(uint32_t*)dst = hi;
    *(uint32_t*)(dst + dpad) = lo;
}

// transposed: [2 dpadT, n256], row c = column c of src as hi, row dpadT + c as lo; rows d .. dpadT and columns n .. n256 are +0
__global__ __launch_bounds__(256) void infonce_panel_t_kernel(const float* __restrict__ src, int n, int d, int dpadT, int n256,
                                                              bf16_t* __restrict__ out, long long total) {
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    if (gid >= total) return;
    const int half = n256 >> 1;
    const int j = (int)(gid % half) * 2;
    const int c = (int)(gid / half);
    float v0 = 0.f, v1 = 0.f;
    if (c < d) {
        if (j < n) v0 = src[(size_t)j * d + c];
        if (j + 1 < n) v1 = src[(size_t)(j + 1) * d + c];
    }
    uint32_t hi, lo;
    split_bf16x2(v0, v1, hi, lo);
    *(uint32_t*)(out + (size_t)c * n256 + j) = hi;
    *(uint32_t*)(out + (size_t)(dpadT + c) * n256 + j) = lo;
}

// ------------------------------------------------------------------------------------------------ forward
struct NceStats {
    const bf16_t* X;
    const bf16_t* Y;
    int n, dpad, swap;
    float inv_t;
    float* part;        // [n, nchunks, 2]: running maximum, sum of exp(z - maximum)
    float* diag;        // [n]: z_ii
    int nchunks, tiles_per_chunk, g_tiles;
};

__global__ __launch_bounds__(256) void infonce_stats_kernel(const NceStats p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* sS = (float*)smem;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int qt = blockIdx.x / p.nchunks, chunk = blockIdx.x % p.nchunks;
    const int tile_begin = chunk * p.tiles_per_chunk;
    const int tile_end = min(tile_begin + p.tiles_per_chunk, p.g_tiles);
    const bf16_t* gX = p.X + (size_t)qt * NT * (2 * p.dpad);
    const int q_local = tid & 127, half = tid >> 7;
    const int qrow = qt * NT + q_local;
    const bool q_valid = qrow < p.n;
    float m = -INFINITY, s = 0.f;

    for (int gtile = tile_begin; gtile < tile_end; ++gtile) {
        f32x4 acc[4][4];
        nce_logit_tile(gX, p.Y + (size_t)gtile * NT * (2 * p.dpad), p.dpad, p.swap, smem, acc, wid, lane);
        nce_dump_tile(acc, sS, wid, lane);
        __syncthreads();
        nce_scan_tile(sS, q_local, half, qrow, q_valid, gtile, p.n, p.inv_t, m, s, p.diag);
        __syncthreads();          // the scan is done with sS before the next tile's operands are staged over it
    }
    nce_store_part(sS, q_local, half, qrow, q_valid, m, s, p.nchunks, chunk, p.part);
}

// lse[row] = log sum over the chunks in chunk order; term[row] = lse - z_ii
__global__ __launch_bounds__(256) void infonce_merge_kernel(const float* __restrict__ part, const float* __restrict__ diag, int n, int nchunks,
                                                            float* __restrict__ lse, float* __restrict__ term) {
    const int row = blockIdx.x * 256 + threadIdx.x;
    if (row >= n) return;
    const float* pr = part + (size_t)row * nchunks * 2;
    float mm = -INFINITY;
    for (int c = 0; c < nchunks; ++c) mm = fmaxf(mm, pr[2 * c]);
    float ss = 0.f;
    for (int c = 0; c < nchunks; ++c)
        if (pr[2 * c] > -INFINITY) ss += pr[2 * c + 1] * __builtin_amdgcn_exp2f((pr[2 * c] - mm) * NCE_LOG2E);
    const float l = mm + logf(ss);
    lse[row] = l;
    term[row] = l - diag[row];
}

// one workgroup: loss[1] = mean term[0 .. n), loss[2] = mean term[n .. 2 n), loss[0] = their mean; fp64 sums in a fixed tree
__global__ __launch_bounds__(256) void infonce_loss_kernel(const float* __restrict__ term, int n, float* __restrict__ loss) {
    __shared__ double sh[2][256];
    const int tid = threadIdx.x;
    double s0 = 0.0, s1 = 0.0;
    for (int i = tid; i < n; i += 256) { s0 += (double)term[i]; s1 += (double)term[n + i]; }
    sh[0][tid] = s0;
    sh[1][tid] = s1;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) { sh[0][tid] += sh[0][tid + w]; sh[1][tid] += sh[1][tid + w]; }
        __syncthreads();
    }
    if (tid == 0) {
        const double a = sh[0][0] / n, b = sh[1][0] / n;
        loss[0] = (float)(0.5 * (a + b));
        loss[1] = (float)a;
        loss[2] = (float)b;
    }
}

// ------------------------------------------------------------------------------------------------ backward
struct NceBwd {
    const bf16_t* X;        // [n256, 2 dpad]: the rows this call differentiates
    const bf16_t* Y;        // [n256, 2 dpad]: the other operand
    const bf16_t* YT;       // [2 dpadT, n256]
    const float* lse_x;     // [n] lse over Y's items per row of X
    const float* lse_y;     // [n] lse over X's items per row of Y
    int n, n256, d, dpad, dpadT, swap, splits;
    float inv_t;
    float* grad;            // [n, d]
};

template <int NS>
__global__ __launch_bounds__(256) void infonce_bwd_kernel(const NceBwd p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* sS = (float*)smem;
    char* sP = smem + NCE_A_BYTES;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wq = wid >> 1, wcn = wid & 1;
    const int lrow = lane & 15, lq = lane >> 4, swz = lrow >> 1;
    const int srow = lane >> 3, schunk = lane & 7;
    const int rt = blockIdx.x / p.splits, split = blockIdx.x % p.splits;
    const int col_base = split * NS * NT;
    const bf16_t* gX = p.X + (size_t)rt * NT * (2 * p.dpad);
    const int q_local = tid & 127, half = tid >> 7;
    const int qrow = rt * NT + q_local;
    const bool q_valid = qrow < p.n;
    const float lse_r = q_valid ? p.lse_x[qrow] : 0.f;
    const float inv_n = 1.0f / (float)p.n, half_inv_n = 0.5f / (float)p.n;
    const int g_tiles = (p.n + NT - 1) / NT;

    f32x4 out[NS][4][4];
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
        for (int ci = 0; ci < 4; ++ci)
#pragma unroll
            for (int qi = 0; qi < 4; ++qi) out[s][ci][qi] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int gtile = 0; gtile < g_tiles; ++gtile) {
        {
            f32x4 acc[4][4];
            nce_logit_tile(gX, p.Y + (size_t)gtile * NT * (2 * p.dpad), p.dpad, p.swap, smem, acc, wid, lane);
            nce_dump_tile(acc, sS, wid, lane);
        }
        __syncthreads();
        // dL/dz of this thread's row and 64 columns -> bf16 pair, in the operand stages' layout (row 128 B, 16-byte chunk c at c ^ swizzle)
        {
            const float* rowp = sS + q_local * NLD + half * 64;
            char* ph = sP + half * NCE_TILE_BYTES + q_local * 128;
            char* pl = ph + 2 * NCE_TILE_BYTES;
            const int c0 = gtile * NT + half * 64;
            const int pswz = (q_local >> 1) & 7;
#pragma unroll 2
            for (int ch = 0; ch < 8; ++ch) {
                float g[8];
                const float4 va = *(const float4*)(rowp + ch * 8), vb = *(const float4*)(rowp + ch * 8 + 4);
                const float sv[8] = {va.x, va.y, va.z, va.w, vb.x, vb.y, vb.z, vb.w};
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const int j = c0 + ch * 8 + e;
                    float v = 0.f;
                    if (q_valid && j < p.n) {
                        const float z = sv[e] * p.inv_t;
                        v = (__builtin_amdgcn_exp2f((z - lse_r) * NCE_LOG2E) + __builtin_amdgcn_exp2f((z - p.lse_y[j]) * NCE_LOG2E)) * half_inv_n;
                        if (j == qrow) v -= inv_n;
                    }
                    g[e] = v;
                }
                uint32_t h[4], l[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) split_bf16x2(g[2 * e], g[2 * e + 1], h[e], l[e]);
                const int slot = (ch ^ pswz) << 4;
                *(uint4*)(ph + slot) = make_uint4(h[0], h[1], h[2], h[3]);
                *(uint4*)(pl + slot) = make_uint4(l[0], l[1], l[2], l[3]);
            }
        }
        __syncthreads();          // the pair tile is complete; the logit tile is dead, its bytes stage Y^T from here on
        // out[row][c] += sum_j P[row][j] Y[j][c]: hi.hi + lo.hi + hi.lo, two K steps of 64 items each, per slab of 128 output columns
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int c0 = col_base + s * NT;
            if (c0 < p.dpadT) {                           // uniform
                auto stage_t = [&](int buf, int st) {
                    const int seg = (st >> 1) == 2 ? 1 : 0;
                    const bf16_t* src = p.YT + (size_t)(seg * p.dpadT + c0) * p.n256 + (size_t)gtile * NT + (st & 1) * NBK;
                    char* sA = smem + buf * NCE_TILE_BYTES;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int piece = wid * 4 + j;
                        const int r = piece * 8 + srow;
                        const int c = schunk ^ ((r >> 1) & 7);
                        nce_glds16(src + (size_t)r * p.n256 + c * 8, sA + piece * 1024);
                    }
                };
                stage_t(0, 0);
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __syncthreads();
                for (int st = 0; st < 6; ++st) {
                    const int cur = st & 1;
                    if (st + 1 < 6) stage_t(cur ^ 1, st + 1);
                    const int pseg = (st >> 1) == 1 ? 1 : 0;
                    const char* sA = smem + cur * NCE_TILE_BYTES + (wcn * 64 + lrow) * 128;
                    const char* sB = sP + (pseg * 2 + (st & 1)) * NCE_TILE_BYTES + (wq * 64 + lrow) * 128;
#pragma unroll
                    for (int kk = 0; kk < 2; ++kk) {
                        const int coff = ((kk * 4 + lq) ^ swz) << 4;
                        bf16x8 yf[4], pf[4];
#pragma unroll
                        for (int ci = 0; ci < 4; ++ci) yf[ci] = *(const bf16x8*)(sA + ci * 16 * 128 + coff);
#pragma unroll
                        for (int qi = 0; qi < 4; ++qi) pf[qi] = *(const bf16x8*)(sB + qi * 16 * 128 + coff);
#pragma unroll
                        for (int ci = 0; ci < 4; ++ci)
#pragma unroll
                            for (int qi = 0; qi < 4; ++qi)
                                out[s][ci][qi] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(yf[ci], pf[qi], out[s][ci][qi], 0, 0, 0);
                    }
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                    __syncthreads();
                }
            }
        }
    }
    // out[s][ci][qi][r] = grad[row rt*128 + wq*64 + qi*16 + lrow][column col_base + s*128 + wcn*64 + ci*16 + lq*4 + r] * tau
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
        for (int ci = 0; ci < 4; ++ci)
#pragma unroll
            for (int qi = 0; qi < 4; ++qi) {
                const int row = rt * NT + wq * 64 + qi * 16 + lrow;
                const int c = col_base + s * NT + wcn * 64 + ci * 16 + lq * 4;
                if (row < p.n) {
                    float* dst = p.grad + (size_t)row * p.d + c;
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (c + r < p.d) dst[r] = out[s][ci][qi][r] * p.inv_t;
                }
            }
}

// ------------------------------------------------------------------------------------------------ host side
struct NceLayout {
    int n256, dpad, dpadT, g_tiles, nchunks, tpc;
    size_t off_pa, off_pb, off_ta, off_tb, off_part, off_diag, off_term, bytes;
};

static NceLayout nce_layout(int n, int d) {
    NceLayout L;
    L.n256 = (int)round_up(n, 256);
    L.dpad = (int)round_up(d, 64);
    L.dpadT = (int)round_up(d, 128);
    L.g_tiles = (n + NT - 1) / NT;
    const int want = L.g_tiles < NCE_MAX_CHUNKS ? L.g_tiles : NCE_MAX_CHUNKS;
    L.tpc = (L.g_tiles + want - 1) / want;
    L.nchunks = (L.g_tiles + L.tpc - 1) / L.tpc;
    size_t at = 0;
    auto take = [&](size_t b) { const size_t o = at; at += (size_t)round_up((int64_t)b, 256); return o; };
    const size_t panel = (size_t)L.n256 * 2 * L.dpad * 2, panel_t = (size_t)2 * L.dpadT * L.n256 * 2;
    L.off_pa = take(panel);
    L.off_pb = take(panel);
    L.off_ta = take(panel_t);
    L.off_tb = take(panel_t);
    L.off_part = take((size_t)2 * n * NCE_MAX_CHUNKS * 2 * 4);
    L.off_diag = take((size_t)2 * n * 4);
    L.off_term = take((size_t)2 * n * 4);
    L.bytes = at;
    return L;
}

static int nce_check(const char* fn, const void* a, const void* b, int n, int d, float inv_t, const void* ws, size_t ws_bytes) {
    if (n < 1 || n > 65536) KEMR_FAIL(KEMR_ERR_INVALID, "%s: n=%d not in 1..65536", fn, n);
    if (d < 4 || d > 1280 || d % 4) KEMR_FAIL(KEMR_ERR_INVALID, "%s: d=%d must be a multiple of 4 in 4..1280", fn, d);
    if (!(inv_t > 0.f) || !std::isfinite(inv_t)) KEMR_FAIL(KEMR_ERR_INVALID, "%s: inv_temperature=%g must be positive and finite", fn, (double)inv_t);
    if (!a) KEMR_FAIL(KEMR_ERR_INVALID, "%s: a_dev is null", fn);
    if (!b) KEMR_FAIL(KEMR_ERR_INVALID, "%s: b_dev is null", fn);
    const size_t need = nce_layout(n, d).bytes;
    if (!ws || ws_bytes < need) KEMR_FAIL(KEMR_ERR_WORKSPACE, "%s: workspace %zu < %zu bytes", fn, ws ? ws_bytes : (size_t)0, need);
    if ((uintptr_t)ws % 256) KEMR_FAIL(KEMR_ERR_WORKSPACE, "%s: workspace must be 256-byte aligned", fn);
    return KEMR_OK;
}

int nce_launch_panel(const float* src, int n, int d, int dpad, int n256, bf16_t* out, hipStream_t s) {
    const long long total = (long long)n256 * (dpad / 2);
    hipLaunchKernelGGL(infonce_panel_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, src, n, d, dpad, out, total);
    KEMR_CHECK_LAUNCH("infonce_panel_kernel");
    return KEMR_OK;
}

int nce_launch_merge(const float* part, const float* diag, int n, int nchunks, float* lse, float* term, hipStream_t s) {
    hipLaunchKernelGGL(infonce_merge_kernel, dim3((n + 255) / 256), dim3(256), 0, s, part, diag, n, nchunks, lse, term);
    KEMR_CHECK_LAUNCH("infonce_merge_kernel");
    return KEMR_OK;
}

int nce_launch_loss(const float* term, int n, float* loss, hipStream_t s) {
    hipLaunchKernelGGL(infonce_loss_kernel, dim3(1), dim3(256), 0, s, term, n, loss);
    KEMR_CHECK_LAUNCH("infonce_loss_kernel");
    return KEMR_OK;
}

static int nce_build_panels(const float* a, const float* b, int n, int d, const NceLayout& L, char* ws, bool transposed, hipStream_t s) {
    KEMR_TRY(nce_launch_panel(a, n, d, L.dpad, L.n256, (bf16_t*)(ws + L.off_pa), s));
    KEMR_TRY(nce_launch_panel(b, n, d, L.dpad, L.n256, (bf16_t*)(ws + L.off_pb), s));
    if (transposed) {
        const long long tt = (long long)L.dpadT * (L.n256 / 2);
        const unsigned gt = (unsigned)((tt + 255) / 256);
        hipLaunchKernelGGL(infonce_panel_t_kernel, dim3(gt), dim3(256), 0, s, a, n, d, L.dpadT, L.n256, (bf16_t*)(ws + L.off_ta), tt);
        hipLaunchKernelGGL(infonce_panel_t_kernel, dim3(gt), dim3(256), 0, s, b, n, d, L.dpadT, L.n256, (bf16_t*)(ws + L.off_tb), tt);
        KEMR_CHECK_LAUNCH("infonce_panel_t_kernel");
    }
    return KEMR_OK;
}

template <int NS>
static int launch_nce_bwd(const NceBwd& p, hipStream_t s) {
    static int attr_dev = -1;             // per instantiation; one process drives one device at a time
    constexpr int smem = NCE_A_BYTES + NCE_P_BYTES;
    KEMR_TRY(nce_lds_attr(infonce_bwd_kernel<NS>, smem, &attr_dev));
    const int r_tiles = (p.n + NT - 1) / NT;
    hipLaunchKernelGGL(infonce_bwd_kernel<NS>, dim3(r_tiles * p.splits), dim3(256), smem, s, p);
    KEMR_CHECK_LAUNCH("infonce_bwd_kernel");
    return KEMR_OK;
}

}  // namespace kemr

// ================================================================================================ C ABI
using namespace kemr;

extern "C" size_t kemr_infonce_workspace_bytes(int n, int d) {
    if (n < 1 || n > 65536 || d < 4 || d > 1280 || d % 4) return 0;
    return nce_layout(n, d).bytes;
}

extern "C" int kemr_infonce_forward(const float* a_dev, const float* b_dev, int n, int d, float inv_temperature, float* loss_dev,
                                    float* lse_dev, void* workspace_dev, size_t workspace_bytes, void* stream) {
    KEMR_TRY(nce_check("infonce_forward", a_dev, b_dev, n, d, inv_temperature, workspace_dev, workspace_bytes));
    if (!loss_dev) KEMR_FAIL(KEMR_ERR_INVALID, "infonce_forward: loss_dev is null");
    if (!lse_dev) KEMR_FAIL(KEMR_ERR_INVALID, "infonce_forward: lse_dev is null");
    const NceLayout L = nce_layout(n, d);
    char* ws = (char*)workspace_dev;
    hipStream_t s = (hipStream_t)stream;
    KEMR_TRY(nce_build_panels(a_dev, b_dev, n, d, L, ws, false, s));
    static int attr_dev = -1;
    KEMR_TRY(nce_lds_attr(infonce_stats_kernel, NCE_A_BYTES, &attr_dev));
    float* term = (float*)(ws + L.off_term);
    for (int pass = 0; pass < 2; ++pass) {            // 0: rows of z (a against b), 1: columns (b against a, same products, same order)
        NceStats p{};
        p.X = (const bf16_t*)(ws + (pass ? L.off_pb : L.off_pa));
        p.Y = (const bf16_t*)(ws + (pass ? L.off_pa : L.off_pb));
        p.n = n; p.dpad = L.dpad; p.swap = pass; p.inv_t = inv_temperature;
        p.part = (float*)(ws + L.off_part) + (size_t)pass * n * NCE_MAX_CHUNKS * 2;
        p.diag = (float*)(ws + L.off_diag) + (size_t)pass * n;
        p.nchunks = L.nchunks; p.tiles_per_chunk = L.tpc; p.g_tiles = L.g_tiles;
        hipLaunchKernelGGL(infonce_stats_kernel, dim3(L.g_tiles * L.nchunks), dim3(256), NCE_A_BYTES, s, p);
        KEMR_CHECK_LAUNCH("infonce_stats_kernel");
        KEMR_TRY(nce_launch_merge(p.part, p.diag, n, L.nchunks, lse_dev + (size_t)pass * n, term + (size_t)pass * n, s));
    }
    KEMR_TRY(nce_launch_loss(term, n, loss_dev, s));
    return KEMR_OK;
}

extern "C" int kemr_infonce_backward(const float* a_dev, const float* b_dev, const float* lse_dev, int n, int d, float inv_temperature,
                                     float* grad_a_dev, float* grad_b_dev, void* workspace_dev, size_t workspace_bytes, void* stream) {
    KEMR_TRY(nce_check("infonce_backward", a_dev, b_dev, n, d, inv_temperature, workspace_dev, workspace_bytes));
    if (!lse_dev) KEMR_FAIL(KEMR_ERR_INVALID, "infonce_backward: lse_dev is null");
    if (!grad_a_dev) KEMR_FAIL(KEMR_ERR_INVALID, "infonce_backward: grad_a_dev is null");
    if (!grad_b_dev) KEMR_FAIL(KEMR_ERR_INVALID, "infonce_backward: grad_b_dev is null");
    const NceLayout L = nce_layout(n, d);
    char* ws = (char*)workspace_dev;
    hipStream_t s = (hipStream_t)stream;
    KEMR_TRY(nce_build_panels(a_dev, b_dev, n, d, L, ws, true, s));
    const int slabs = L.dpadT / NT;
    const int splits = (slabs + NCE_MAX_NS - 1) / NCE_MAX_NS;
    const int ns = (slabs + splits - 1) / splits;
    for (int pass = 0; pass < 2; ++pass) {            // 0: dL/da (rows a, other b), 1: dL/db
        NceBwd p{};
        p.X = (const bf16_t*)(ws + (pass ? L.off_pb : L.off_pa));
        p.Y = (const bf16_t*)(ws + (pass ? L.off_pa : L.off_pb));
        p.YT = (const bf16_t*)(ws + (pass ? L.off_ta : L.off_tb));
        p.lse_x = lse_dev + (size_t)pass * n;
        p.lse_y = lse_dev + (size_t)(1 - pass) * n;
        p.n = n; p.n256 = L.n256; p.d = d; p.dpad = L.dpad; p.dpadT = L.dpadT; p.swap = pass; p.splits = splits;
        p.inv_t = inv_temperature;
        p.grad = pass ? grad_b_dev : grad_a_dev;
        if (ns == 1) KEMR_TRY(launch_nce_bwd<1>(p, s));
        else KEMR_TRY(launch_nce_bwd<2>(p, s));
    }
    return KEMR_OK;
}
