// libkemr.so: the error string, the ABI version, the event profiler, the debug knobs and the per-kernel pass-throughs behind the C ABI
// (include/kemr.h, include/kemr_debug.h).  The model handle lives in model.hip, the encoder launch sequences in encode.hip.
// Host-side C++ only; every kernel lives in gemm.hip / layernorm.hip / attention.hip / embed.hip / sim.hip.
#include "common.h"
#include "../../include/kemr_debug.h"

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <vector>

namespace kemr {

static thread_local char g_err[512] = "";
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

// ---- event profiler: off by default; bench.py turns it on for a few untimed-for-throughput steps ----
struct ProfState {
    bool on = false;
    std::vector<hipEvent_t> ev;       // 2 per slot
    std::vector<int> cls;
    int used = 0;
};
static ProfState g_prof;

ProfScope::ProfScope(int c, hipStream_t s) : slot(-1), stream(s) {
    if (!g_prof.on || g_prof.used >= (int)g_prof.cls.size()) return;
    slot = g_prof.used++;
    g_prof.cls[slot] = c;
    (void)hipEventRecord(g_prof.ev[2 * slot], stream);
}
ProfScope::~ProfScope() {
    if (slot >= 0) (void)hipEventRecord(g_prof.ev[2 * slot + 1], stream);
}

}  // namespace kemr

using namespace kemr;

extern "C" const char* kemr_last_error(void) { return g_err; }
extern "C" int kemr_abi_version(void) { return KEMR_ABI_VERSION; }

// ------------------------------------------------------------------------------------------------ include/kemr_debug.h
// Process-wide experiment switches of tools/ and tests/ (not thread-safe, not part of the product ABI): one key per knob.
namespace {
#ifdef KEMR_AB_VARIANTS
int g_ab_variants = 1;
#else
int g_ab_variants = 0;
#endif
// `product`: bit v set = value v selects a kernel the PRODUCT library holds (a routing choice between kernels it needs anyway);
// every other value names an experiment kernel that exists only in a `build.py --ab-variants` library and is refused without it.
struct DebugKnob { const char* key; int* var; int lo, hi; unsigned product; };
int* sim_lists_knob();
const DebugKnob* debug_knobs(int* n) {
    static const DebugKnob knobs[] = {
        {"gemm_variant", &g_gemm_variant, 0, 9, 1u << 0 | 1u << 1 | 1u << 2 | 1u << 7 | 1u << 8},   // 0 auto, 1 = 128x128, 2 = 256x256, 7 = persistent, 8 = skinny (all product kernels, forced); 3 = staggered 256x256, 4-6, 9 = earlier generations: A/B builds
        {"gemm_flags", &g_gemm_dbg, 0, 255, 1u << 0},  // timing-experiment flags of the DBG instantiation (1 drop stores, 4 plain stores, 32 / 64 / 128 stamps): A/B builds
        {"gemm_order", &g_gemm_order, 0, 8, ~0u},     // gemm256u tile order (0 = N fastest, else log2(column-group width) + 1)
        {"gemm_grid", &g_gemm_grid, 0, 1024, ~0u},    // tools: cap on the persistent GEMM's grid (0 = one workgroup per CU); results do not depend on it
        {"gemm_conc", &g_gemm_conc, 0, 2, ~0u},       // both wave halves' epilogues in one barrier interval: 0 never, 1 always, 2 = QuickGELU / GELU only
        {"gemm_kl", &g_gemm_kl, 0, 1, 1u << 0},       // 0 = eight 256-cycle barrier intervals per K-tile (the product loop), 1 = four of 512 (round-3 experiment): A/B builds
        {"attn_v", &g_attn_v, 0, 5, 1u << 0},         // 0 = the product kernel, 1..4 = attention_ab.hip: A/B builds
        {"attn_xcd", &g_attn_xcd, 0, 1, ~0u},         // attention: images dealt to the XCDs
        {"attn80_waves", &g_attn80_waves, 0, 8, 1u << 0 | 1u << 4 | 1u << 8},   // head-dim-80 tile kernel at T = 257: 0 / 8 = eight waves per workgroup (default), 4 = four; both are in the product library
        {"attn_waves", &g_attn_waves, 0, 8, 1u << 0}, // waves per attention workgroup at T = 257 (0 = default; others: A/B builds)
        {"ln_nt", &g_ln_nt, 0, 3, 1u << 3},           // LayerNorm cache hints: 3 = deltas, residual rows and the x write-back non-temporal (the product kernel); 0 / 1 / 2 = earlier levels: A/B builds
        {"sim_lists", sim_lists_knob(), 0, 3, ~0u},   // 0 = never the candidate-list route, 1 = where it pays, 2 = wherever it fits + the fallback forced, 3 = wherever it fits
        {"ab_variants", &g_ab_variants, -1, -2, 0},   // read-only: 1 = this library was built with the A/B experiment kernels
        {"staging_slots", &g_staging_slots, -1, -2, 0},   // read-only: pinned staging slots in the ring (preprocess.hip: 8 to begin with, 64 at most)
        {"staging_grown", &g_staging_grown, -1, -2, 0},   // read-only: times a staging slot took a larger buffer and kept the outgrown one
    };
    *n = (int)(sizeof(knobs) / sizeof(knobs[0]));
    return knobs;
}
int* sim_lists_knob() { return &g_sim_lists; }
}  // namespace

extern "C" int kemr_debug_set(const char* key, int value) {
    if (!key) KEMR_FAIL(KEMR_ERR_INVALID, "debug_set: null key");
    int n = 0;
    const DebugKnob* k = debug_knobs(&n);
    for (int i = 0; i < n; ++i)
        if (!strcmp(k[i].key, key)) {
            if (k[i].lo > k[i].hi) KEMR_FAIL(KEMR_ERR_INVALID, "debug_set(%s): read-only", key);
            if (value < k[i].lo || value > k[i].hi) KEMR_FAIL(KEMR_ERR_INVALID, "debug_set(%s): %d not in %d..%d", key, value, k[i].lo, k[i].hi);
            if (!g_ab_variants && !(value < 32 && ((k[i].product >> value) & 1u)) && k[i].product != ~0u)
                KEMR_FAIL(KEMR_ERR_INVALID, "debug_set(%s): %d selects an A/B experiment kernel that is not in this library (build.py --ab-variants)", key, value);
            *k[i].var = value;
            return KEMR_OK;
        }
    KEMR_FAIL(KEMR_ERR_INVALID, "debug_set: unknown key '%s'", key);
}

extern "C" int kemr_debug_get(const char* key, int* value) {
    if (!key || !value) KEMR_FAIL(KEMR_ERR_INVALID, "debug_get: null argument");
    int n = 0;
    const DebugKnob* k = debug_knobs(&n);
    for (int i = 0; i < n; ++i)
        if (!strcmp(k[i].key, key)) { *value = *k[i].var; return KEMR_OK; }
    KEMR_FAIL(KEMR_ERR_INVALID, "debug_get: unknown key '%s'", key);
}

extern "C" int kemr_debug_gemm_stamps(unsigned* host_out, int n_words) {
    if (!host_out) KEMR_FAIL(KEMR_ERR_INVALID, "debug_gemm_stamps: null output");
    return gemm_read_stamps(host_out, n_words);
}

// the head dims the attention kernels serve, and the width they split
static int check_head_dim(const char* what, int head_dim, int width) {
    if (head_dim != 64 && head_dim != 80) KEMR_FAIL(KEMR_ERR_INVALID, "%s: head dim %d not served (64 or 80)", what, head_dim);
    if (width <= 0 || width % head_dim) KEMR_FAIL(KEMR_ERR_INVALID, "%s: width %d is not a multiple of the head dim %d", what, width, head_dim);
    return KEMR_OK;
}

// pass-throughs to the launchers of the kernels a tower reaches only inside itself (tests hold them to their rounding budgets)
extern "C" int kemr_debug_op_attention_packed(const void* qkv_dev, void* out_dev, const int* row_start_dev, int batch, int max_t, int width,
                                              void* stream) {
    if (!qkv_dev || !out_dev) KEMR_FAIL(KEMR_ERR_INVALID, "debug_op_attention_packed: null argument");
    return launch_attention_packed((const bf16_t*)qkv_dev, (bf16_t*)out_dev, row_start_dev, batch, max_t, width, (hipStream_t)stream);
}

extern "C" int kemr_debug_op_attention_pooled(const void* q_dev, const void* qkv_dev, void* out_dev, const int* pool_idx_dev,
                                              const int* row_start_dev, int items, int tokens, int width, int causal, int force_long,
                                              void* stream) {
    if (!q_dev || !qkv_dev || !out_dev) KEMR_FAIL(KEMR_ERR_INVALID, "debug_op_attention_pooled: null argument");
    return launch_attention_pooled((const bf16_t*)q_dev, (const bf16_t*)qkv_dev, (bf16_t*)out_dev, pool_idx_dev, row_start_dev, items,
                                   tokens, width, causal, (hipStream_t)stream, force_long);
}

extern "C" int kemr_debug_op_attention_pooled_hd(const void* q_dev, const void* qkv_dev, void* out_dev, const int* pool_idx_dev,
                                                 const int* row_start_dev, int items, int tokens, int width, int head_dim, int causal,
                                                 int force_long, void* stream) {
    if (!q_dev || !qkv_dev || !out_dev) KEMR_FAIL(KEMR_ERR_INVALID, "debug_op_attention_pooled_hd: null argument");
    KEMR_TRY(check_head_dim("debug_op_attention_pooled_hd", head_dim, width));
    if (head_dim == 64)
        return launch_attention_pooled((const bf16_t*)q_dev, (const bf16_t*)qkv_dev, (bf16_t*)out_dev, pool_idx_dev, row_start_dev, items,
                                       tokens, width, causal, (hipStream_t)stream, force_long);
    if (pool_idx_dev || row_start_dev || force_long)
        KEMR_FAIL(KEMR_ERR_INVALID, "debug_op_attention_pooled_hd: head dim 80 takes no pooled positions, packed rows or long instantiation (vision towers of at most 288 tokens)");
    return launch_attention80_pooled((const bf16_t*)q_dev, (const bf16_t*)qkv_dev, (bf16_t*)out_dev, items, tokens, width, causal, (hipStream_t)stream);
}

extern "C" int kemr_debug_op_tail(const void* x_dev, int x_dtype, const void* delta_dev, const void* delta2_dev, const int32_t* ids_dev,
                                  const int* row_start_dev, int batch, int tokens, int width, const float* gamma_dev, const float* beta_dev,
                                  const float* proj_dev, int d, int normalize, float* out_dev, void* stream) {
    if (!x_dev || !gamma_dev || !beta_dev || !proj_dev || !out_dev) KEMR_FAIL(KEMR_ERR_INVALID, "debug_op_tail: null argument");
    if (x_dtype != KEMR_F32 && x_dtype != KEMR_BF16 && x_dtype != KEMR_F24) KEMR_FAIL(KEMR_ERR_INVALID, "debug_op_tail: bad row dtype %d", x_dtype);
    return launch_tail(x_dev, x_dtype, (const bf16_t*)delta_dev, (const bf16_t*)delta2_dev, ids_dev, batch, tokens, width, gamma_dev, beta_dev,
                       proj_dev, d, normalize, out_dev, (hipStream_t)stream, row_start_dev);
}

// ---- family 2 (BERT): the new kernels alone ----
extern "C" int kemr_debug_op_attention_varlen(const void* qkv_dev, void* out_dev, const int* row_start_dev, int batch, int max_t, int width,
                                              void* stream) {
    if (!qkv_dev || !out_dev || !row_start_dev) KEMR_FAIL(KEMR_ERR_INVALID, "debug_op_attention_varlen: null argument");
    return launch_attention_varlen((const bf16_t*)qkv_dev, (bf16_t*)out_dev, row_start_dev, batch, max_t, width, (hipStream_t)stream);
}

// family 3 (MPNet): the same launch with the [width / 64, 1023] table of biases by distance
extern "C" int kemr_debug_op_attention_varlen_bias(const void* qkv_dev, void* out_dev, const int* row_start_dev, const float* bias_by_distance_dev,
                                                   int batch, int max_t, int width, void* stream) {
    if (!qkv_dev || !out_dev || !row_start_dev || !bias_by_distance_dev) KEMR_FAIL(KEMR_ERR_INVALID, "debug_op_attention_varlen_bias: null argument");
    return launch_attention_varlen((const bf16_t*)qkv_dev, (bf16_t*)out_dev, row_start_dev, batch, max_t, width, (hipStream_t)stream, bias_by_distance_dev);
}

extern "C" int kemr_debug_op_layernorm_post(void* x_dev, int x_dtype, const void* delta_dev, const float* gamma_dev, const float* beta_dev,
                                            void* h_dev, int rows, int width, float eps, void* stream) {
    if (!x_dev || !delta_dev || !gamma_dev || !beta_dev || !h_dev) KEMR_FAIL(KEMR_ERR_INVALID, "debug_op_layernorm_post: null argument");
    return launch_layernorm_post(x_dev, x_dtype, (const bf16_t*)delta_dev, gamma_dev, beta_dev, (bf16_t*)h_dev, rows, width, (hipStream_t)stream, eps);
}

extern "C" int kemr_debug_op_pool_rows(const void* x_dev, int x_dtype, const int* row_start_dev, int batch, int width, int pooling, int normalize,
                                       float* out_dev, void* stream) {
    if (!x_dev || !row_start_dev || !out_dev) KEMR_FAIL(KEMR_ERR_INVALID, "debug_op_pool_rows: null argument");
    return launch_pool_rows(x_dev, x_dtype, row_start_dev, batch, width, pooling, normalize, out_dev, (hipStream_t)stream);
}

// ------------------------------------------------------------------------------------------------ event profiler
extern "C" int kemr_profile_begin(int max_launches) {
    if (max_launches <= 0 || max_launches > (1 << 20)) KEMR_FAIL(KEMR_ERR_INVALID, "profile_begin: bad max_launches");
    if (g_prof.on) KEMR_FAIL(KEMR_ERR_STATE, "profile_begin: already profiling");
    while ((int)g_prof.ev.size() < 2 * max_launches) {
        hipEvent_t e;
        KEMR_CHECK_HIP(hipEventCreate(&e));
        g_prof.ev.push_back(e);
    }
    g_prof.cls.assign(max_launches, 0);
    g_prof.used = 0;
    g_prof.on = true;
    return KEMR_OK;
}

extern "C" int kemr_profile_end(double* ms_per_class, int64_t* launches_per_class, int nclass) {
    if (!g_prof.on) KEMR_FAIL(KEMR_ERR_STATE, "profile_end: not profiling");
    g_prof.on = false;
    if (!ms_per_class || !launches_per_class || nclass < PROF_NCLASS) KEMR_FAIL(KEMR_ERR_INVALID, "profile_end: need %d classes", PROF_NCLASS);
    for (int i = 0; i < nclass; ++i) { ms_per_class[i] = 0; launches_per_class[i] = 0; }
    KEMR_CHECK_HIP(hipDeviceSynchronize());
    for (int i = 0; i < g_prof.used; ++i) {
        float ms = 0.f;
        KEMR_CHECK_HIP(hipEventElapsedTime(&ms, g_prof.ev[2 * i], g_prof.ev[2 * i + 1]));
        ms_per_class[g_prof.cls[i]] += ms;
        launches_per_class[g_prof.cls[i]] += 1;
    }
    return KEMR_OK;
}

// ------------------------------------------------------------------------------------------------ per-kernel test hooks
extern "C" int kemr_op_gemm(const void* a_dev, const void* w_dev, const float* bias_dev, void* c_dev, int m, int n, int k,
                            int epilogue, void* stream) {
    if (!a_dev || !w_dev || !c_dev) KEMR_FAIL(KEMR_ERR_INVALID, "op_gemm: null argument");
    if (epilogue < 0 || (epilogue > KEMR_EPI_BIAS_RESID_F32 && epilogue != KEMR_EPI_BIAS_RESADD_BF16 && epilogue != KEMR_EPI_BIAS_GELU_BF16 && epilogue != KEMR_EPI_BIAS_TGELU_BF16)) KEMR_FAIL(KEMR_ERR_INVALID, "op_gemm: bad epilogue %d", epilogue);
    GemmParams g{};
    g.A = (const bf16_t*)a_dev; g.lda = k; g.W = (const bf16_t*)w_dev; g.ldw = k; g.bias = bias_dev; g.C = c_dev; g.ldc = n;
    g.M = m; g.N = n; g.K = k;
    g.c_rows_padded = 1;           // documented requirement of this entry point: C (like A) has ceil256(m) rows
    return launch_gemm(g, epilogue, (hipStream_t)stream);
}

extern "C" int kemr_op_gemm_fp8(const void* a_dev, const void* w_dev, const float* wscale_dev, const float* bias_dev, void* c_dev,
                                int m, int n, int k, int epilogue, void* stream) {
    if (!a_dev || !w_dev || !wscale_dev || !c_dev) KEMR_FAIL(KEMR_ERR_INVALID, "op_gemm_fp8: null argument");
    GemmParams g{};
    g.A = (const bf16_t*)a_dev; g.lda = k; g.W = (const bf16_t*)w_dev; g.ldw = k; g.bias = bias_dev; g.wscale = wscale_dev;
    g.C = c_dev; g.ldc = n; g.M = m; g.N = n; g.K = k;
    g.c_rows_padded = 1;
    return launch_gemm256u_fp8(g, epilogue, (hipStream_t)stream);
}

extern "C" int kemr_op_e4m3_host(const float* in, unsigned char* out, long long n) {
    if (!in || !out || n < 0) KEMR_FAIL(KEMR_ERR_INVALID, "op_e4m3_host: bad argument");
    for (long long i = 0; i < n; ++i) out[i] = f32_to_e4m3_host(in[i]);
    return KEMR_OK;
}

extern "C" int kemr_op_layernorm(const float* x_dev, const float* gamma_dev, const float* beta_dev, void* y_dev, int rows,
                                 int width, int out_dtype, void* stream) {
    if (!x_dev || !gamma_dev || !beta_dev || !y_dev) KEMR_FAIL(KEMR_ERR_INVALID, "op_layernorm: null argument");
    return launch_layernorm((void*)x_dev, KEMR_F32, nullptr, nullptr, 0, gamma_dev, beta_dev, y_dev, rows, width, out_dtype, (hipStream_t)stream);
}

extern "C" int kemr_op_layernorm_resid(float* x_dev, const void* delta_dev, const float* gamma_dev, const float* beta_dev,
                                       void* y_dev, int rows, int width, void* stream) {
    if (!x_dev || !delta_dev || !gamma_dev || !beta_dev || !y_dev) KEMR_FAIL(KEMR_ERR_INVALID, "op_layernorm_resid: null argument");
    return launch_layernorm(x_dev, KEMR_F32, (const bf16_t*)delta_dev, nullptr, 1, gamma_dev, beta_dev, y_dev, rows, width, KEMR_BF16, (hipStream_t)stream);
}

extern "C" int kemr_op_layernorm_rows(void* x_dev, int x_dtype, const void* delta_dev, const void* delta2_dev, int writeback,
                                      const float* gamma_dev, const float* beta_dev, void* y_dev, int rows, int width,
                                      int out_dtype, void* stream) {
    if (!x_dev || !gamma_dev || !beta_dev || !y_dev) KEMR_FAIL(KEMR_ERR_INVALID, "op_layernorm_rows: null argument");
    return launch_layernorm(x_dev, x_dtype, (const bf16_t*)delta_dev, (const bf16_t*)delta2_dev, writeback, gamma_dev, beta_dev,
                            y_dev, rows, width, out_dtype, (hipStream_t)stream);
}

extern "C" int kemr_op_attention(const void* qkv_dev, void* out_dev, int batch, int t, int width, int causal, void* stream) {
    if (!qkv_dev || !out_dev) KEMR_FAIL(KEMR_ERR_INVALID, "op_attention: null argument");
    return launch_attention((const bf16_t*)qkv_dev, (bf16_t*)out_dev, batch, t, width, causal, (hipStream_t)stream);
}

// the causal packed forward as a product entry point: launch_attention_packed behind named host-side refusals
extern "C" int kemr_op_attention_packed(const void* qkv_dev, void* out_dev, const int* row_start_dev, int batch, int max_t, int width,
                                        void* stream) {
    if (!qkv_dev) KEMR_FAIL(KEMR_ERR_INVALID, "op_attention_packed: qkv is NULL");
    if (!out_dev) KEMR_FAIL(KEMR_ERR_INVALID, "op_attention_packed: out is NULL");
    if (!row_start_dev) KEMR_FAIL(KEMR_ERR_INVALID, "op_attention_packed: row_start is NULL");
    if (max_t < 1 || max_t > KEMR_MAX_TEXT_CTX)
        KEMR_FAIL(KEMR_ERR_INVALID, "op_attention_packed: max_t = %d is outside 1..%d", max_t, KEMR_MAX_TEXT_CTX);
    if (width <= 0 || width % 64 != 0)
        KEMR_FAIL(KEMR_ERR_INVALID, "op_attention_packed: width = %d is not a positive multiple of 64 (heads of 64)", width);
    if (batch < 0) KEMR_FAIL(KEMR_ERR_INVALID, "op_attention_packed: batch = %d is negative", batch);
    if (batch > 65528) KEMR_FAIL(KEMR_ERR_INVALID, "op_attention_packed: batch = %d exceeds 65528 (the grid)", batch);
    return launch_attention_packed((const bf16_t*)qkv_dev, (bf16_t*)out_dev, row_start_dev, batch, max_t, width, (hipStream_t)stream);
}

extern "C" int kemr_op_attention_hd(const void* qkv_dev, void* out_dev, int batch, int t, int width, int head_dim, int causal, void* stream) {
    if (!qkv_dev || !out_dev) KEMR_FAIL(KEMR_ERR_INVALID, "op_attention_hd: null argument");
    KEMR_TRY(check_head_dim("op_attention_hd", head_dim, width));
    if (head_dim == 64) return launch_attention((const bf16_t*)qkv_dev, (bf16_t*)out_dev, batch, t, width, causal, (hipStream_t)stream);
    return launch_attention80((const bf16_t*)qkv_dev, (bf16_t*)out_dev, batch, t, width, causal, (hipStream_t)stream);
}

// ---- KEMR_PREC_FP32X3 building blocks (panels: kemr_panel_build with nparts = 1, terms = 3) ----
extern "C" int kemr_op_layernorm_x3(const float* x_dev, const float* gamma_dev, const float* beta_dev, void* y_panel_dev, int rows,
                                    int width, void* stream) {
    if (!x_dev || !gamma_dev || !beta_dev || !y_panel_dev) KEMR_FAIL(KEMR_ERR_INVALID, "op_layernorm_x3: null argument");
    return launch_layernorm_x3(x_dev, gamma_dev, beta_dev, (bf16_t*)y_panel_dev, rows, width, (hipStream_t)stream);
}

extern "C" int kemr_op_gemm_x3(const void* a_panel_dev, const void* w_panel_dev, const float* bias_dev, void* c_dev, int m, int n,
                               int k3, int mode, void* stream) {
    if (!a_panel_dev || !w_panel_dev || !c_dev) KEMR_FAIL(KEMR_ERR_INVALID, "op_gemm_x3: null argument");
    if (mode < 0 || mode > 3) KEMR_FAIL(KEMR_ERR_INVALID, "op_gemm_x3: mode %d not in 0..3", mode);
    if (k3 <= 0 || k3 % 192) KEMR_FAIL(KEMR_ERR_INVALID, "op_gemm_x3: k3 = %d is not three blocks of a multiple of 64", k3);
    static const int epi[4] = {EPI_X3_F32, EPI_BIAS_RESID_F32, EPI_X3_QGELU, EPI_X3_GELU};
    GemmParams g{};
    g.A = (const bf16_t*)a_panel_dev; g.lda = k3; g.W = (const bf16_t*)w_panel_dev; g.ldw = k3; g.bias = bias_dev; g.C = c_dev;
    g.ldc = mode >= 2 ? 3 * n : n; g.M = m; g.N = n; g.K = k3;
    g.c_rows_padded = 1;
    return launch_gemm_x3(g, epi[mode], (hipStream_t)stream);
}

extern "C" int kemr_op_attention_x3(const float* qkv_dev, void* out_panel_dev, const int* row_start_dev, int batch, int t, int width,
                                    int causal, void* stream) {
    if (!qkv_dev || !out_panel_dev) KEMR_FAIL(KEMR_ERR_INVALID, "op_attention_x3: null argument");
    return launch_attention_x3(qkv_dev, (bf16_t*)out_panel_dev, row_start_dev, batch, t, width, causal, (hipStream_t)stream);
}

extern "C" int kemr_op_attention_x3_hd(const float* qkv_dev, void* out_panel_dev, const int* row_start_dev, int batch, int t, int width,
                                       int head_dim, int causal, void* stream) {
    if (!qkv_dev || !out_panel_dev) KEMR_FAIL(KEMR_ERR_INVALID, "op_attention_x3_hd: null argument");
    KEMR_TRY(check_head_dim("op_attention_x3_hd", head_dim, width));
    if (head_dim == 64) return launch_attention_x3(qkv_dev, (bf16_t*)out_panel_dev, row_start_dev, batch, t, width, causal, (hipStream_t)stream);
    if (row_start_dev) KEMR_FAIL(KEMR_ERR_INVALID, "op_attention_x3_hd: packed rows are causal, and head dim 80 is not served causal");
    return launch_attention80_x3(qkv_dev, (bf16_t*)out_panel_dev, batch, t, width, causal, (hipStream_t)stream);
}
