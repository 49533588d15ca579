// The elementwise passes of a training step (tower_train.py): the backward of kemr_op_layernorm and the MLP activation on bf16 in both
// directions.  All three are HBM-bound.  Algorithmic bytes per element (LayerNorm forward, layernorm.hip: 4 read + 2 | 4 written):
//   layernorm backward   4 (x) + 2 | 4 (dy) read, 4 (dx) written  = 10 | 12   [+ gamma once per wave, L2-resident; + G slabs of 8 width
//                        bytes written and read once, G <= 512: 4 MB at width 1024 against 168 MB of rows at 16 448 rows]
//   activation forward   2 (pre) read, 2 (out) written            = 4
//   activation backward  2 (pre) + 2 (dout) read, 2 (dpre) written = 6
// No atomics, no second stream, no device-dependent size: the same inputs give the same bits on every launch.
#include "common.h"

namespace kemr {

constexpr int LNB_MAX_GROUPS = 512;      // two workgroups of four waves per CU on 256 CUs: two rows in flight per wave keep HBM busy

// G: the grid of layernorm_bwd_kernel and the number of [2, width] slabs in the workspace -- a function of rows alone
static inline int lnb_groups(int rows) {
    const int tiles = (rows + 3) / 4;
    return tiles < LNB_MAX_GROUPS ? tiles : LNB_MAX_GROUPS;
}

__device__ __forceinline__ float4 lnb_load_dy(const float* r, int i) { return ((const float4*)r)[i]; }
__device__ __forceinline__ float4 lnb_load_dy(const bf16_t* r, int i) {
    const uint2 d = ((const uint2*)r)[i];
    return make_float4(bf16_to_f32((bf16_t)(d.x & 0xffff)), bf16_to_f32((bf16_t)(d.x >> 16)),
                       bf16_to_f32((bf16_t)(d.y & 0xffff)), bf16_to_f32((bf16_t)(d.y >> 16)));
}

// One wave per row, the row in registers (lane l holds elements 4 (64 i + l) .. + 3, i < NV, like layernorm_kernel); wave w of workgroup
// g walks rows 4 g + w, + 4 G, ... with the next row's loads issued before the current row's arithmetic.  mean and rstd are the
// forward's, operation for operation.  The lanes' dgamma / dbeta partial sums (8 NV floats) stay in registers over the walk; the four
// waves then combine through LDS as ((w0 + w1) + w2) + w3 and the workgroup stores its [2, W] slab.
template <int NV, typename DYT>
__global__ __launch_bounds__(256) void layernorm_bwd_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                            const DYT* __restrict__ dy, float* __restrict__ dx,
                                                            float* __restrict__ slabs, int rows, float eps) {
    constexpr int W = NV * 256;
    __shared__ float4 part[4][2][W / 4];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int stride = gridDim.x * 4;
    float4 g[NV], ag[NV], ab[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        g[i] = ((const float4*)gamma)[i * 64 + lane];
        ag[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        ab[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    int row = blockIdx.x * 4 + wid;                      // wave-uniform
    float4 nv[NV], nd[NV];
    if (row < rows) {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            nv[i] = ((const float4*)(x + (size_t)row * W))[i * 64 + lane];
            nd[i] = lnb_load_dy(dy + (size_t)row * W, i * 64 + lane);
        }
    }
    for (; row < rows; row += stride) {
        float4 v[NV], d[NV];
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            v[i] = nv[i];
            d[i] = nd[i];
            s += (v[i].x + v[i].y) + (v[i].z + v[i].w);
        }
        const int next = row + stride;
        if (next < rows) {                               // nothing behind row rows - 1 is read
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                nv[i] = ((const float4*)(x + (size_t)next * W))[i * 64 + lane];
                nd[i] = lnb_load_dy(dy + (size_t)next * W, i * 64 + lane);
            }
        }
        const float mean = wave_sum(s) * (1.0f / W);
        float q = 0.f;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            v[i].x -= mean; v[i].y -= mean; v[i].z -= mean; v[i].w -= mean;
            q += (v[i].x * v[i].x + v[i].y * v[i].y) + (v[i].z * v[i].z + v[i].w * v[i].w);
        }
        const float rstd = 1.0f / sqrtf(wave_sum(q) * (1.0f / W) + eps);
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            v[i].x *= rstd; v[i].y *= rstd; v[i].z *= rstd; v[i].w *= rstd;                  // x^
            ab[i].x += d[i].x; ab[i].y += d[i].y; ab[i].z += d[i].z; ab[i].w += d[i].w;
            ag[i].x = fmaf(d[i].x, v[i].x, ag[i].x); ag[i].y = fmaf(d[i].y, v[i].y, ag[i].y);
            ag[i].z = fmaf(d[i].z, v[i].z, ag[i].z); ag[i].w = fmaf(d[i].w, v[i].w, ag[i].w);
            d[i].x *= g[i].x; d[i].y *= g[i].y; d[i].z *= g[i].z; d[i].w *= g[i].w;          // g = dy gamma
            s1 += (d[i].x + d[i].y) + (d[i].z + d[i].w);
            s2 += (d[i].x * v[i].x + d[i].y * v[i].y) + (d[i].z * v[i].z + d[i].w * v[i].w);
        }
        const float m1 = wave_sum(s1) * (1.0f / W), m2 = wave_sum(s2) * (1.0f / W);
        float* dxr = dx + (size_t)row * W;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            float4 o;
            o.x = rstd * ((d[i].x - m1) - v[i].x * m2);
            o.y = rstd * ((d[i].y - m1) - v[i].y * m2);
            o.z = rstd * ((d[i].z - m1) - v[i].z * m2);
            o.w = rstd * ((d[i].w - m1) - v[i].w * m2);
            ((float4*)dxr)[i * 64 + lane] = o;
        }
    }
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        part[wid][0][i * 64 + lane] = ag[i];
        part[wid][1][i * 64 + lane] = ab[i];
    }
    __syncthreads();
    float4* slab = (float4*)(slabs + (size_t)blockIdx.x * 2 * W);
    for (int j = threadIdx.x; j < 2 * (W / 4); j += 256) {
        const int k = j < W / 4 ? 0 : 1, c = j - k * (W / 4);
        const float4 a = part[0][k][c], b = part[1][k][c], e = part[2][k][c], f = part[3][k][c];
        slab[j] = make_float4(((a.x + b.x) + e.x) + f.x, ((a.y + b.y) + e.y) + f.y, ((a.z + b.z) + e.z) + f.z, ((a.w + b.w) + e.w) + f.w);
    }
}

// dgamma | dbeta [2 W] = the column sums of the G slabs.  One workgroup per 64 columns; wave w sums slabs w, w + 4, ... in that
// order, the four waves combine as ((w0 + w1) + w2) + w3.
__global__ __launch_bounds__(256) void layernorm_bwd_reduce_kernel(const float* __restrict__ slabs, float* __restrict__ dgamma,
                                                                   float* __restrict__ dbeta, int groups, int width) {
    __shared__ float part[4][64];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int col = blockIdx.x * 64 + lane;              // < 2 width: the grid is 2 width / 64
    float s = 0.f;
    for (int gidx = wid; gidx < groups; gidx += 4) s += slabs[(size_t)gidx * 2 * width + col];
    part[wid][lane] = s;
    __syncthreads();
    if (wid == 0) {
        const float t = ((part[0][lane] + part[1][lane]) + part[2][lane]) + part[3][lane];
        if (col < width) dgamma[col] = t;
        else dbeta[col - width] = t;
    }
}

template <int NV>
static int launch_lnb_nv(const float* x, const float* gamma, const void* dy, int dy_dtype, float* dx, float* dgamma, float* dbeta,
                         int rows, float* slabs, hipStream_t s) {
    const int groups = lnb_groups(rows);
    ProfScope prof(PROF_LAYERNORM, s);
    if (dy_dtype == KEMR_BF16)
        hipLaunchKernelGGL((layernorm_bwd_kernel<NV, bf16_t>), dim3(groups), dim3(256), 0, s, x, gamma, (const bf16_t*)dy, dx, slabs, rows, 1e-5f);
    else
        hipLaunchKernelGGL((layernorm_bwd_kernel<NV, float>), dim3(groups), dim3(256), 0, s, x, gamma, (const float*)dy, dx, slabs, rows, 1e-5f);
    KEMR_CHECK_LAUNCH("layernorm_bwd_kernel");
    hipLaunchKernelGGL(layernorm_bwd_reduce_kernel, dim3(2 * NV * 4), dim3(256), 0, s, slabs, dgamma, dbeta, groups, NV * 256);
    KEMR_CHECK_LAUNCH("layernorm_bwd_reduce_kernel");
    return KEMR_OK;
}

// ---- the MLP activation on bf16: 8 elements (16 bytes) per lane ---------------------------------------------------------------
// f' of QuickGELU, s + 1.702 x s (1 - s) with s = sigmoid(1.702 x), from e = exp(-1.702 |x|) in (0, 1]: q = 1 / (1 + e) and p = e q are
// sigmoid(1.702 |x|) and its complement, both to a few ulp RELATIVE (no 1 - s cancellation, nothing overflows for any finite x), and
// (s, 1 - s) = (q, p) or (p, q) by the sign of x.  The exponent's argument is carried as a + r like gelu_erf's: a = fl(|x| c_hi), r = the
// product's exact remainder + |x| c_lo (c_hi + c_lo = -1.702 log2 e to 2^-49), and 2^(a + r) = 2^a (1 + r ln 2).
__device__ __forceinline__ float quick_gelu_grad(float v) {
    const float ax = fabsf(v);
    const float a = ax * -2.455467f;
    float r = fmaf(ax, 2.6109499e-8f, fmaf(ax, -2.455467f, -a));
    r = a > -150.0f ? r : 0.0f;                          // 2^a is 0 there; keeps an overflowed a out of the correction
    const float e0 = __builtin_amdgcn_exp2f(a);
    const float e = fmaf(e0, r * 0.6931472f, e0);
    const float q = __builtin_amdgcn_rcpf(1.0f + e);
    const float p = e * q;
    const float s = v < 0.0f ? p : q;
    return fmaf((v * p) * q, 1.702f, s);
}
// f' of the exact GELU, Phi(x) + x phi(x).  Phi = 0.5 erfc(-x / sqrt 2) exactly as gelu_erf evaluates it (relative accuracy in the
// negative tail, where the two terms cancel).  phi = exp(-x^2 / 2) / sqrt(2 pi) with x^2 carried as t + u (u = the square's exact
// remainder): exp(-(t + u) / 2) = exp(-t / 2) (1 - u / 2), expf of the device library on an exact argument.  |x| is capped at 20 for phi
// (phi(20) = 0 in fp32), so x^2 never overflows.
__device__ __forceinline__ float gelu_erf_grad(float v) {
    const float z = v * -0.70710677f;
    const float ze = fmaf(v, -1.2101617e-8f, fmaf(v, -0.70710677f, -z));
    const float c = fmaf(-2.0f * fmaxf(z, 0.0f), ze, 1.0f);
    const float cdf = 0.5f * (erfcf(z) * c);
    const float ax = fminf(fabsf(v), 20.0f);
    const float t = ax * ax;
    const float u = fmaf(ax, ax, -t);
    const float pdf = (expf(-0.5f * t) * fmaf(-0.5f, u, 1.0f)) * 0.3989423f;
    return fmaf(v, pdf, cdf);
}

__device__ __forceinline__ void unpack8(const uint4 p, float* f) {
    f[0] = __uint_as_float(p.x << 16); f[1] = __uint_as_float(p.x & 0xffff0000u);
    f[2] = __uint_as_float(p.y << 16); f[3] = __uint_as_float(p.y & 0xffff0000u);
    f[4] = __uint_as_float(p.z << 16); f[5] = __uint_as_float(p.z & 0xffff0000u);
    f[6] = __uint_as_float(p.w << 16); f[7] = __uint_as_float(p.w & 0xffff0000u);
}
__device__ __forceinline__ uint4 pack8(const float* f) {
    return make_uint4(pack_bf16x2(f[0], f[1]), pack_bf16x2(f[2], f[3]), pack_bf16x2(f[4], f[5]), pack_bf16x2(f[6], f[7]));
}

template <int KIND>
__global__ __launch_bounds__(256) void act_forward_kernel(const uint4* __restrict__ pre, uint4* __restrict__ out, long long n8) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n8) return;
    float f[8];
    unpack8(pre[i], f);
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] = KIND == 0 ? quick_gelu(f[j]) : gelu_erf(f[j]);
    out[i] = pack8(f);
}

template <int KIND>
__global__ __launch_bounds__(256) void act_backward_kernel(const uint4* __restrict__ pre, const uint4* __restrict__ dout,
                                                           uint4* __restrict__ dpre, long long n8) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n8) return;
    float f[8], d[8];
    unpack8(pre[i], f);
    unpack8(dout[i], d);
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] = d[j] * (KIND == 0 ? quick_gelu_grad(f[j]) : gelu_erf_grad(f[j]));
    dpre[i] = pack8(f);
}

static int act_check(const char* op, const void* a, const void* b, const void* c, long long n, int kind) {
    if (!a || !b || (!c)) KEMR_FAIL(KEMR_ERR_INVALID, "%s: a buffer pointer is NULL", op);
    if (kind != 0 && kind != 1) KEMR_FAIL(KEMR_ERR_INVALID, "%s: kind = %d is neither 0 (QuickGELU) nor 1 (exact GELU)", op, kind);
    if (n < 0) KEMR_FAIL(KEMR_ERR_INVALID, "%s: n = %lld is negative", op, n);
    if (n % 8 != 0) KEMR_FAIL(KEMR_ERR_INVALID, "%s: n = %lld is not a multiple of 8 (16-byte loads and stores)", op, n);
    if (n / 8 > 0x7fffffffLL * 256) KEMR_FAIL(KEMR_ERR_INVALID, "%s: n = %lld exceeds the grid (2^31 - 1 workgroups of 2048 elements)", op, n);
    if (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15) KEMR_FAIL(KEMR_ERR_INVALID, "%s: a buffer pointer is not 16-byte aligned", op);
    return KEMR_OK;
}

}  // namespace kemr

using namespace kemr;

extern "C" size_t kemr_layernorm_backward_workspace_bytes(int rows, int width) {
    if (rows <= 0 || width <= 0) return 0;
    return (size_t)lnb_groups(rows) * 2 * (size_t)width * sizeof(float);
}

extern "C" int kemr_op_layernorm_backward(const float* x_dev, const float* gamma_dev, const void* dy_dev, int dy_dtype, float* dx_dev,
                                          float* dgamma_dev, float* dbeta_dev, int rows, int width, void* workspace_dev,
                                          size_t workspace_bytes, void* stream) {
    // everything is refused here, on the host, before any HIP call
    if (!x_dev) KEMR_FAIL(KEMR_ERR_INVALID, "op_layernorm_backward: x is NULL");
    if (!gamma_dev) KEMR_FAIL(KEMR_ERR_INVALID, "op_layernorm_backward: gamma is NULL");
    if (!dy_dev) KEMR_FAIL(KEMR_ERR_INVALID, "op_layernorm_backward: dy is NULL");
    if (!dx_dev) KEMR_FAIL(KEMR_ERR_INVALID, "op_layernorm_backward: dx is NULL");
    if (!dgamma_dev) KEMR_FAIL(KEMR_ERR_INVALID, "op_layernorm_backward: dgamma is NULL");
    if (!dbeta_dev) KEMR_FAIL(KEMR_ERR_INVALID, "op_layernorm_backward: dbeta is NULL");
    if (dy_dtype != KEMR_BF16 && dy_dtype != KEMR_F32) KEMR_FAIL(KEMR_ERR_INVALID, "op_layernorm_backward: dy_dtype = %d is neither KEMR_BF16 nor KEMR_F32", dy_dtype);
    if (width != 256 && width != 512 && width != 768 && width != 1024 && width != 1280)
        KEMR_FAIL(KEMR_ERR_INVALID, "op_layernorm_backward: width %d not in {256,512,768,1024,1280}", width);
    if (rows < 0) KEMR_FAIL(KEMR_ERR_INVALID, "op_layernorm_backward: rows = %d is negative", rows);
    const size_t need = kemr_layernorm_backward_workspace_bytes(rows, width);
    if (need && !workspace_dev) KEMR_FAIL(KEMR_ERR_INVALID, "op_layernorm_backward: workspace is NULL");
    if (workspace_bytes < need)
        KEMR_FAIL(KEMR_ERR_INVALID, "op_layernorm_backward: workspace_bytes = %zu, %zu needed (kemr_layernorm_backward_workspace_bytes)", workspace_bytes, need);
    if (((uintptr_t)x_dev | (uintptr_t)gamma_dev | (uintptr_t)dy_dev | (uintptr_t)dx_dev | (uintptr_t)workspace_dev) & 15)
        KEMR_FAIL(KEMR_ERR_INVALID, "op_layernorm_backward: x, gamma, dy, dx and workspace must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    if (rows == 0) {
        KEMR_CHECK_HIP(hipMemsetAsync(dgamma_dev, 0, (size_t)width * sizeof(float), s));
        KEMR_CHECK_HIP(hipMemsetAsync(dbeta_dev, 0, (size_t)width * sizeof(float), s));
        return KEMR_OK;
    }
    float* slabs = (float*)workspace_dev;
    switch (width) {
        case 256:  return launch_lnb_nv<1>(x_dev, gamma_dev, dy_dev, dy_dtype, dx_dev, dgamma_dev, dbeta_dev, rows, slabs, s);
        case 512:  return launch_lnb_nv<2>(x_dev, gamma_dev, dy_dev, dy_dtype, dx_dev, dgamma_dev, dbeta_dev, rows, slabs, s);
        case 768:  return launch_lnb_nv<3>(x_dev, gamma_dev, dy_dev, dy_dtype, dx_dev, dgamma_dev, dbeta_dev, rows, slabs, s);
        case 1024: return launch_lnb_nv<4>(x_dev, gamma_dev, dy_dev, dy_dtype, dx_dev, dgamma_dev, dbeta_dev, rows, slabs, s);
    }
    return launch_lnb_nv<5>(x_dev, gamma_dev, dy_dev, dy_dtype, dx_dev, dgamma_dev, dbeta_dev, rows, slabs, s);
}

extern "C" int kemr_op_act_forward(const void* pre_dev, void* out_dev, long long n, int kind, void* stream) {
    KEMR_TRY(act_check("op_act_forward", pre_dev, out_dev, out_dev, n, kind));
    if (n == 0) return KEMR_OK;
    const long long n8 = n / 8;
    const dim3 grid((unsigned)((n8 + 255) / 256));
    ProfScope prof(PROF_OTHER, (hipStream_t)stream);
    if (kind == 0) hipLaunchKernelGGL(act_forward_kernel<0>, grid, dim3(256), 0, (hipStream_t)stream, (const uint4*)pre_dev, (uint4*)out_dev, n8);
    else hipLaunchKernelGGL(act_forward_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, (const uint4*)pre_dev, (uint4*)out_dev, n8);
    KEMR_CHECK_LAUNCH("act_forward_kernel");
    return KEMR_OK;
}

extern "C" int kemr_op_act_backward(const void* pre_dev, const void* dout_dev, void* dpre_dev, long long n, int kind, void* stream) {
    KEMR_TRY(act_check("op_act_backward", pre_dev, dout_dev, dpre_dev, n, kind));
    if (n == 0) return KEMR_OK;
    const long long n8 = n / 8;
    const dim3 grid((unsigned)((n8 + 255) / 256));
    ProfScope prof(PROF_OTHER, (hipStream_t)stream);
    if (kind == 0) hipLaunchKernelGGL(act_backward_kernel<0>, grid, dim3(256), 0, (hipStream_t)stream, (const uint4*)pre_dev, (const uint4*)dout_dev, (uint4*)dpre_dev, n8);
    else hipLaunchKernelGGL(act_backward_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, (const uint4*)pre_dev, (const uint4*)dout_dev, (uint4*)dpre_dev, n8);
    KEMR_CHECK_LAUNCH("act_backward_kernel");
    return KEMR_OK;
}
