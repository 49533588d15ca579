// libkemr.so: the encoder launch sequences behind kemr_encode_* -- workspace layouts, the token fronts, the residual blocks, the tails --
// and the debug entry points that reuse the fronts.  Host-side C++ only; every kernel lives in gemm.hip / layernorm.hip / attention.hip /
// embed.hip.
#include "model.h"
#include "../../include/kemr_debug.h"

using namespace kemr;

namespace {

int stream_elem_bytes(int x_dtype) { return x_dtype == KEMR_BF16 ? 2 : (x_dtype == KEMR_F24 ? 3 : 4); }

// ---- the workspace of the bf16 path: ONE statement of its layout, for the size queries and for the carve ----
// Token-row buffers of Mp = ceil256(rows) rows, then the compact [Mc = ceil256(pooled_items), W] rows of the last block's pooled-row
// path (nothing for pooled_items == 0), then `row_starts` ints of a packed call (nothing for 0).  Byte offsets from the base.
struct Layout { size_t x, h, delta, delta2, big, pool_idx, xc, hc, qc, ac, d1c, d2c, gc, row_start, total; };

Layout ws_layout(int width, int64_t rows, int pooled_items, int x_dtype, int row_starts) {
    const int64_t Mp = round_up(rows, 256), Mc = round_up((int64_t)pooled_items, 256), W = width;
    Layout L{};
    auto take = [&](size_t& at, int64_t bytes) { at = L.total; L.total += (size_t)bytes; };
    take(L.x, round_up(Mp * W * stream_elem_bytes(x_dtype), 256));
    take(L.h, round_up(Mp * W * 2, 256));
    take(L.delta, round_up(Mp * W * 2, 256));
    take(L.delta2, round_up(Mp * W * 2, 256));
    take(L.big, round_up(Mp * W * 8, 256));
    take(L.pool_idx, round_up((int64_t)pooled_items * 4, 256));
    take(L.xc, Mc * W * 4);                            // (sized for an fp32 stream)
    take(L.hc, Mc * W * 2);
    take(L.qc, Mc * W * 2);
    take(L.ac, Mc * W * 2);
    take(L.d1c, Mc * W * 2);
    take(L.d2c, Mc * W * 2);
    take(L.gc, Mc * W * 8);
    take(L.row_start, round_up((int64_t)row_starts * 4, 256));
    return L;
}

struct Workspace {
    void* x;        // [Mp, W] residual stream, fp32 or bf16 (x_dtype)
    int x_dtype;
    bf16_t* h;      // [Mp, W] bf16: LayerNorm output / attention output (GEMM A operand)
    bf16_t* big;    // [Mp, 4W] bf16: qkv (ld 3W), MLP hidden (ld 4W), im2col patches
    bf16_t* delta;  // [Mp, W] bf16: output of the out-proj GEMM (attention update), pending until the next block's ln_1
    bf16_t* delta2; // [Mp, W] bf16: output of the fc2 GEMM (MLP update), pending until the next block's ln_1 (or the tail)
    float* x32;     // [Mp, W] fp32 front-end rows of the vision tower (patch GEMM + cls, read by ln_pre): x itself for
                    // an fp32 stream, else the (then still unused) h | delta pair, which is contiguous and as large
    // compact [Mc = ceil256(items), W] rows of the last block's pooled-row path (run_blocks)
    int* pool_idx;  // [items] row of the class / end-of-text token
    void* xc;       // residual-stream rows (x_dtype)
    bf16_t *hc, *qc, *ac, *d1c, *d2c;   // LayerNorm output, query, attention output, the two pending updates
    bf16_t* gc;     // [Mc, 4W] MLP hidden
    int* row_start; // [batch + 1] prefix sums of a packed call (row_starts_kernel), nullptr otherwise
};

int check_workspace(const void* base, size_t bytes, size_t need) {
    if (!base || bytes < need) KEMR_FAIL(KEMR_ERR_WORKSPACE, "workspace too small: %zu < %zu bytes", bytes, need);
    if ((uintptr_t)base % 256) KEMR_FAIL(KEMR_ERR_WORKSPACE, "workspace must be 256-byte aligned");
    return KEMR_OK;
}

int carve(Workspace& w, void* base, size_t bytes, const Layout& L, int x_dtype) {
    KEMR_TRY(check_workspace(base, bytes, L.total));
    char* p = (char*)base;
    w.x = p + L.x; w.x_dtype = x_dtype;
    w.h = (bf16_t*)(p + L.h); w.delta = (bf16_t*)(p + L.delta); w.delta2 = (bf16_t*)(p + L.delta2); w.big = (bf16_t*)(p + L.big);
    w.x32 = x_dtype == KEMR_F32 ? (float*)w.x : (float*)w.h;
    w.pool_idx = (int*)(p + L.pool_idx);
    w.xc = p + L.xc;
    w.hc = (bf16_t*)(p + L.hc); w.qc = (bf16_t*)(p + L.qc); w.ac = (bf16_t*)(p + L.ac);
    w.d1c = (bf16_t*)(p + L.d1c); w.d2c = (bf16_t*)(p + L.d2c); w.gc = (bf16_t*)(p + L.gc);
    w.row_start = L.total > L.row_start ? (int*)(p + L.row_start) : nullptr;
    return KEMR_OK;
}

// ---- KEMR_PREC_FP32X3: its own workspace and tower driver (nothing of the bf16 path is shared but the kernels that are fp32 already) ----
// Per token row of the Mp = ceil256(rows) allocated: x [Mp, W] fp32 (the residual stream, plain 4-byte), h [Mp, 3W] bf16 (LayerNorm
// output, then the attention output: A-side triples), qkv [Mp, 3W] fp32, big [Mp, 12W] bf16 (the MLP hidden as an A-side triple;
// the tripled im2col rows, 3 kpad <= 12W, before the blocks).  46 W bytes per row; no pooled-row area: every row runs through every
// block (option "last_block_pooled_row" is ignored in this mode).  Then the row starts of a packed call.
struct LayoutX3 { size_t x, h, qkv, big, row_start, total; };
struct WorkspaceX3 { float* x; bf16_t* h; float* qkv; bf16_t* big; int* row_start; };

LayoutX3 ws_layout_x3(int width, int64_t rows, int row_starts) {
    const int64_t Mp = round_up(rows, 256), W = width;
    LayoutX3 L{};
    auto take = [&](size_t& at, int64_t bytes) { at = L.total; L.total += (size_t)bytes; };
    take(L.x, Mp * W * 4);
    take(L.h, Mp * W * 6);
    take(L.qkv, Mp * W * 12);
    take(L.big, Mp * W * 24);
    take(L.row_start, round_up((int64_t)row_starts * 4, 256));
    return L;
}

int carve_x3(WorkspaceX3& w, void* base, size_t bytes, const LayoutX3& L) {
    KEMR_TRY(check_workspace(base, bytes, L.total));
    char* p = (char*)base;
    w.x = (float*)(p + L.x); w.h = (bf16_t*)(p + L.h); w.qkv = (float*)(p + L.qkv); w.big = (bf16_t*)(p + L.big);
    w.row_start = L.total > L.row_start ? (int*)(p + L.row_start) : nullptr;
    return KEMR_OK;
}

// ---- GEMM launches: every launch builds its parameters from scratch ----
// C[M, N] (ld ldc) = A[M, K] . W[N, K]^T (+ bias): both operands dense in K (lda = ldw = K), C with ceil256(M) writable rows like every
// workspace buffer; wscale: the per-output-channel scales of an e4m3 W (launch_gemm256u_fp8).  Everything else is zero.
GemmParams linear(const void* A, const void* W, const float* bias, void* C, int ldc, int M, int N, int K, const float* wscale = nullptr) {
    GemmParams g{};
    g.A = (const bf16_t*)A; g.lda = K; g.W = (const bf16_t*)W; g.ldw = K; g.bias = bias; g.wscale = wscale;
    g.C = C; g.ldc = ldc; g.M = M; g.N = N; g.K = K;
    g.c_rows_padded = 1;
    return g;
}

// the patch embedding over K = kpad (3 kpad: the fp32x3 triples): token rows + positional embedding, C rows remapped (no padded-row stores)
GemmParams patch_embed(const kemr_model* m, const bf16_t* patches, int K, float* C, int batch) {
    GemmParams g = linear(patches, m->conv_w, nullptr, C, m->cfg.v_width, batch * m->patches, m->cfg.v_width, K);
    g.c_rows_padded = 0;
    g.pos = m->vpos; g.patches = m->patches;
    return g;
}

// Residual blocks.  The out-proj and fc2 GEMMs do not read-modify-write the residual stream: they store `A.W^T + bias`
// as bf16 into `delta` / `delta2` (store-only epilogues) and the LayerNorms apply the updates while they read x anyway:
// ln_2 normalises x + delta without writing x; the next block's ln_1 writes x += delta + delta2 once and normalises it.
// On return both deltas of the last block are still pending; the caller's tail adds them.
//
// Option "residual_fusion" (calls of more than 512 token rows that the persistent GEMM takes whole): the out-proj and fc2
// epilogues read the x tile they overwrite and add it, both LayerNorms read x and write h only.
//  * bf16 residual stream (value >= 1, the default): EPI_BIAS_RESADD_BF16, 8 instead of 16 bytes per element and layer in the
//    LayerNorms; x is then rounded to bf16 twice per layer (after the attention update and after the MLP update) instead of once.
//  * fp32 residual stream (value 2 only): EPI_BIAS_RESID_F32, x += A.W^T + bias in fp32 in the accumulator domain -- no delta
//    buffers, no rounding of the updates at all (the store-only form rounds each update to bf16), 12 instead of 22 bytes per
//    element and layer in the LayerNorms.  NOT the default: measured (round 3, ViT-L/14 at B = 255, same device) the two GEMMs pay
//    +77 us (out-proj, 106 -> 183) and +62 us (fc2, 402 -> 464) per layer for 112 us of LayerNorm time saved -- every workgroup of
//    the persistent kernel reaches its tile boundary at the same moment, so the 0.54 GB an epilogue round moves arrive as a burst
//    at the HBM roofline with the matrix cores idle, and out-proj with 0.67 GB per launch is HBM-bound outright (122 us at best).
//
// last_pooled (option "last_block_pooled_row", store-only epilogues, fc1 not on fp8): only ONE row per item leaves a tower -- the class
// token's (ln_post(x[:, 0]) @ proj) or the end-of-text token's -- so the LAST block computes K and V for every row (they feed that
// row's attention) but the query, the attention output, out-proj, ln_2 and the MLP for the pooled rows alone: compact [items, W]
// buffers, 2 of the block's 12 W^2 of GEMM work per token row instead of 12.  The pooled rows see the same arithmetic (their GEMMs
// are smaller launches, routed to the skinny / 128-row kernels, with their summation order).
struct BlockOpts {
    int causal = 0;
    int fp8 = 0;                            // bit 0: QKV, bit 1: fc1 on e4m3 operands
    int want_resadd = 0;                    // option "residual_fusion"
    int epi_act = EPI_BIAS_QGELU_BF16;      // the fc1 epilogue (fc1_epilogue); nothing else depends on the activation
    float eps = 1e-5f;                      // every LayerNorm's epsilon
    const int* row_start = nullptr;         // text tower only: the token rows are packed, text i owning rows row_start[i] .. row_start[i + 1] - 1,
    int rows = 0;                           // `rows` in all
    int last_pooled = 0;
    const int32_t* ids = nullptr;           // causal: the pooled row is the first argmax of the item's ids
    int pool_pos = 0;                       // causal == 0: the position of the pooled row, 0 = the class token; family 1's text tower is
                                            // unmasked and pools its LAST position, so its last block runs the pooled-row form with ctx - 1
};
struct BlockResult {
    bool pending = false;                   // both deltas of the last block are left for the tail
    bool compact = false;                   // the last block ran on the pooled rows: the tail reads xc / d1c / d2c
};

int run_blocks(const TowerW& t, const Workspace& w, int batch, const BlockOpts& o, hipStream_t s, BlockResult& res) {
    const int W = t.width, M = o.row_start ? o.rows : batch * t.tokens;
    const bool fq = o.fp8 & 1, f1 = o.fp8 & 2;      // LayerNorm output = A operand of QKV / fc1: e4m3 where that GEMM runs in fp8
    const int hq = fq ? KEMR_FP8 : KEMR_BF16, h1 = f1 ? KEMR_FP8 : KEMR_BF16;
    bool resadd = o.want_resadd >= (w.x_dtype == KEMR_BF16 ? 1 : 2) && M > 512 && W % 256 == 0 && w.x_dtype != KEMR_F24;
    const int cs = w.x_dtype == KEMR_BF16 ? 2 : 4;
    const int epi_res = w.x_dtype == KEMR_BF16 ? EPI_BIAS_RESADD_BF16 : EPI_BIAS_RESID_F32;
    if (resadd)
        resadd = gemm256u_fits(linear(nullptr, nullptr, nullptr, nullptr, W, M, W, W), 2, cs) &&
                 gemm256u_fits(linear(nullptr, nullptr, nullptr, nullptr, W, M, W, 4 * W), 2, cs);
    res.pending = !resadd && t.layers > 0;
    res.compact = o.last_pooled && !resadd && !f1 && t.layers > 0 && t.tokens <= KEMR_MAX_VISION_TOKENS;
    if (res.compact) KEMR_TRY(launch_pool_index(o.causal ? o.ids : nullptr, o.row_start, batch, t.tokens, w.pool_idx, s, o.pool_pos));
    auto qkv_gemm = [&](const GemmParams& g) { return fq ? launch_gemm256u_fp8(g, EPI_BIAS_BF16, s) : launch_gemm(g, EPI_BIAS_BF16, s); };
    for (int l = 0; l < t.layers; ++l) {
        const LayerW& L = t.layer[l];
        const void* wqkv = fq ? (const void*)L.wqkv8 : (const void*)L.wqkv;         // [3W, W], one or two bytes per element
        const size_t wq_bytes = (size_t)W * W * (fq ? 1 : 2);                      // its query rows
        if (res.compact && l == t.layers - 1) {
            KEMR_TRY(launch_layernorm(w.x, w.x_dtype, l ? w.delta : nullptr, l ? w.delta2 : nullptr, 1, L.ln1_g, L.ln1_b, w.h, M, W, hq, s, o.eps));
            // K and V of every row: the weight rows W .. 3W - 1 of in_proj, into the columns W .. 3W - 1 of the qkv buffer; then the query of
            // the pooled rows from the first W weight rows (fq: both on e4m3 operands, like the QKV GEMM of the other blocks)
            KEMR_TRY(qkv_gemm(linear(w.h, (const char*)wqkv + wq_bytes, L.bqkv + W, w.big + W, 3 * W, M, 2 * W, W, fq ? L.sqkv + W : nullptr)));
            KEMR_TRY(launch_gather_pooled(w.x, w.x_dtype, w.h, hq, w.pool_idx, batch, W, w.xc, w.hc, s));
            KEMR_TRY(qkv_gemm(linear(w.hc, wqkv, L.bqkv, w.qc, W, batch, W, W, fq ? L.sqkv : nullptr)));
            if (t.head_dim == 80) KEMR_TRY(launch_attention80_pooled(w.qc, w.big, w.ac, batch, t.tokens, W, o.causal, s));
            else KEMR_TRY(launch_attention_pooled(w.qc, w.big, w.ac, w.pool_idx, o.row_start, batch, t.tokens, W, o.causal, s));
            KEMR_TRY(launch_gemm(linear(w.ac, L.wo, L.bo, w.d1c, W, batch, W, W), EPI_BIAS_BF16, s));
            KEMR_TRY(launch_layernorm(w.xc, w.x_dtype, w.d1c, nullptr, 0, L.ln2_g, L.ln2_b, w.hc, batch, W, KEMR_BF16, s, o.eps));
            KEMR_TRY(launch_gemm(linear(w.hc, L.w1, L.b1, w.gc, 4 * W, batch, 4 * W, W), o.epi_act, s));
            KEMR_TRY(launch_gemm(linear(w.gc, L.w2, L.b2, w.d2c, W, batch, W, 4 * W), EPI_BIAS_BF16, s));
            break;
        }
        if (resadd) KEMR_TRY(launch_layernorm(w.x, w.x_dtype, nullptr, nullptr, 0, L.ln1_g, L.ln1_b, w.h, M, W, hq, s, o.eps));
        else KEMR_TRY(launch_layernorm(w.x, w.x_dtype, l ? w.delta : nullptr, l ? w.delta2 : nullptr, 1, L.ln1_g, L.ln1_b, w.h, M, W, hq, s, o.eps));
        KEMR_TRY(qkv_gemm(linear(w.h, wqkv, L.bqkv, w.big, 3 * W, M, 3 * W, W, fq ? L.sqkv : nullptr)));
        if (o.row_start) KEMR_TRY(launch_attention_packed(w.big, w.h, o.row_start, batch, t.tokens, W, s));
        else if (t.head_dim == 80) KEMR_TRY(launch_attention80(w.big, w.h, batch, t.tokens, W, o.causal, s));
        else KEMR_TRY(launch_attention(w.big, w.h, batch, t.tokens, W, o.causal, s));
        KEMR_TRY(launch_gemm(linear(w.h, L.wo, L.bo, resadd ? w.x : (void*)w.delta, W, M, W, W), resadd ? epi_res : EPI_BIAS_BF16, s));
        KEMR_TRY(launch_layernorm(w.x, w.x_dtype, resadd ? nullptr : w.delta, nullptr, 0, L.ln2_g, L.ln2_b, w.h, M, W, h1, s, o.eps));
        if (f1) KEMR_TRY(launch_gemm256u_fp8(linear(w.h, L.w18, L.b1, w.big, 4 * W, M, 4 * W, W, L.s1), o.epi_act, s));
        else KEMR_TRY(launch_gemm(linear(w.h, L.w1, L.b1, w.big, 4 * W, M, 4 * W, W), o.epi_act, s));
        KEMR_TRY(launch_gemm(linear(w.big, L.w2, L.b2, resadd ? w.x : (void*)w.delta2, W, M, W, 4 * W), resadd ? epi_res : EPI_BIAS_BF16, s));
    }
    return KEMR_OK;
}

// ---- argument checks, one helper per tower: shared by the fronts (encoders, kemr_debug_*_tokens) and the fp32x3 encoders ----
// `what` prefixes the messages; out_dev is only checked for null.  batch == 0 passes (the caller returns KEMR_OK with nothing launched).
int check_image_args(const kemr_model* m, const void* pixels_dev, int batch, const void* out_dev, const char* what, bool x3_served) {
    if (!m || !pixels_dev || !out_dev) KEMR_FAIL(KEMR_ERR_INVALID, "%s: null argument", what);
    if (!m->finalized) KEMR_FAIL(KEMR_ERR_STATE, "%s: model not finalized", what);
    if (is_sentence_family(m->family)) KEMR_FAIL(KEMR_ERR_INVALID, "%s: not available for family 2 (BERT): a text-only model has no vision tower", what);
    if (m->x3 && !x3_served) KEMR_FAIL(KEMR_ERR_STATE, "%s: not available for a KEMR_PREC_FP32X3 model", what);
    if (batch < 0) KEMR_FAIL(KEMR_ERR_INVALID, "%s: negative batch", what);
    if (batch > 0 && (int64_t)batch * m->vtokens > (1 << 24)) KEMR_FAIL(KEMR_ERR_INVALID, "%s: batch %d too large", what, batch);
    return KEMR_OK;
}

// packed: lens_dev gives the lengths and `rows` (a host integer) the token rows of the call
int check_text_args(const kemr_model* m, const void* ids_dev, const void* lens_dev, int rows, int batch, bool packed, const void* out_dev,
                    const char* what, bool x3_served) {
    if (!m || !ids_dev || !out_dev || (packed && !lens_dev)) KEMR_FAIL(KEMR_ERR_INVALID, "%s: null argument", what);
    if (is_sentence_family(m->family))
        KEMR_FAIL(KEMR_ERR_INVALID, "%s: not available for family 2 (BERT): a padding mask is a length -- call kemr_encode_text_packed with the lengths (kemr_debug_bert_front for the front alone)", what);
    if (!m->finalized) KEMR_FAIL(KEMR_ERR_STATE, "%s: model not finalized", what);
    if (m->x3 && !x3_served) KEMR_FAIL(KEMR_ERR_STATE, "%s: not available for a KEMR_PREC_FP32X3 model", what);
    if (batch < 0) KEMR_FAIL(KEMR_ERR_INVALID, "%s: negative batch", what);
    if (batch == 0) return KEMR_OK;
    const int T = m->cfg.ctx;
    if ((int64_t)batch * T > (1 << 24)) KEMR_FAIL(KEMR_ERR_INVALID, "%s: batch %d too large", what, batch);
    // cfg.ctx <= KEMR_MAX_TEXT_CTX (kemr_model_create), which is what the packed attention serves; the fp32x3 attention takes packed items
    // of up to 128 rows only
    if (packed && m->x3 && T > 128)
        KEMR_FAIL(KEMR_ERR_INVALID, "%s: context length %d > 128 is not served packed for a KEMR_PREC_FP32X3 model (call kemr_encode_text)", what, T);
    if (packed && (rows < batch || (int64_t)rows > (int64_t)batch * T)) KEMR_FAIL(KEMR_ERR_INVALID, "%s: %d rows for %d texts of 1 .. %d positions", what, rows, batch, T);
    return KEMR_OK;
}

// The token fronts of the two towers, shared by the encoders and the kemr_debug_*_tokens pass-throughs (include/kemr_debug.h):
// the argument checks, the workspace carve and the kernels up to the rows the first LayerNorm reads.  batch == 0 returns KEMR_OK with
// nothing launched (the caller stops there).
// Vision: im2col, the patch-embedding GEMM (EPI_PATCH_F32: token rows + positional embedding) and the class rows -> w.x32, the
// fp32 rows [batch * tokens, v_width] ln_pre reads.
int image_front(kemr_model* m, const float* pixels_dev, int batch, const void* out_dev, void* workspace_dev, size_t workspace_bytes,
                hipStream_t s, const char* what, Workspace& w) {
    KEMR_TRY(check_image_args(m, pixels_dev, batch, out_dev, what, false));
    if (batch == 0) return KEMR_OK;
    const int W = m->cfg.v_width, T = m->vtokens;
    KEMR_TRY(carve(w, workspace_dev, workspace_bytes, ws_layout(W, (int64_t)batch * T, batch, m->res_dtype, 0), m->res_dtype));
    KEMR_TRY(launch_im2col(pixels_dev, w.big, batch, m->cfg.image_size, m->cfg.patch, m->kpad, s));
    // family 1: no class token -- row m is patch m % patches of image m / patches; vpos holds pos + the conv bias
    if (m->family == 1) return launch_gemm(patch_embed(m, w.big, m->kpad, w.x32, batch), EPI_PATCH_ROWS_F32, s);
    KEMR_TRY(launch_gemm(patch_embed(m, w.big, m->kpad, w.x32, batch), EPI_PATCH_F32, s));
    return launch_cls_rows(w.x32, m->cls, m->vpos, batch, T, W, s);
}

// Family 1's vision pooling (SiglipMultiheadAttentionPoolingHead) on h = ln_post of EVERY token row [batch * T, W]: k | v of every row
// into the k and v planes of w.big (ld 3 W), the one learned query against them (the pooled-row attention kernel's vision form),
// r = out_proj(attn), out = r + fc2(gelu_tanh(fc1(layernorm(r)))), optionally L2-normalised.  The M = batch launches take the skinny
// GEMM route; r and the MLP update are bf16 GEMM outputs like every block's updates and are summed in fp32.
int map_head(const kemr_model* m, const Workspace& w, const bf16_t* h, int batch, int normalize, float* out, hipStream_t s) {
    const int W = m->cfg.v_width, T = m->vtokens;
    KEMR_TRY(launch_gemm(linear(h, m->mh_wkv, m->mh_bkv, w.big + W, 3 * W, batch * T, 2 * W, W), EPI_BIAS_BF16, s));
    KEMR_TRY(launch_broadcast_row(m->mh_q, w.qc, batch, W, s));
    KEMR_TRY(launch_attention_pooled(w.qc, w.big, w.ac, nullptr, nullptr, batch, T, W, 0, s));
    KEMR_TRY(launch_gemm(linear(w.ac, m->mh_wo, m->mh_bo, w.d1c, W, batch, W, W), EPI_BIAS_BF16, s));
    KEMR_TRY(launch_layernorm(w.d1c, KEMR_BF16, nullptr, nullptr, 0, m->mh_ln_g, m->mh_ln_b, w.hc, batch, W, KEMR_BF16, s, m->eps));
    KEMR_TRY(launch_gemm(linear(w.hc, m->mh_w1, m->mh_b1, w.gc, 4 * W, batch, 4 * W, W), EPI_BIAS_TGELU_BF16, s));
    KEMR_TRY(launch_gemm(linear(w.gc, m->mh_w2, m->mh_b2, w.d2c, W, batch, W, 4 * W), EPI_BIAS_BF16, s));
    return launch_add_rows_out(w.d1c, w.d2c, batch, W, normalize, out, s);
}

// Text: the token + positional embedding rows of the residual stream (w.x, the model's storage type).  packed: the rows of
// kemr_encode_text_packed, w.row_start the prefix sums row_starts_kernel leaves in the workspace; otherwise batch * ctx rows.
int text_front(kemr_model* m, const int32_t* ids_dev, const int32_t* lens_dev, int rows, int batch, bool packed, const void* out_dev,
               void* workspace_dev, size_t workspace_bytes, hipStream_t s, const char* what, Workspace& w) {
    KEMR_TRY(check_text_args(m, ids_dev, lens_dev, rows, batch, packed, out_dev, what, false));
    if (batch == 0) return KEMR_OK;
    const int W = m->cfg.t_width, T = m->cfg.ctx;
    if (!packed) {
        KEMR_TRY(carve(w, workspace_dev, workspace_bytes, ws_layout(W, (int64_t)batch * T, batch, m->res_dtype, 0), m->res_dtype));
        return launch_text_embed(ids_dev, m->tok, m->tpos, w.x, w.x_dtype, batch, T, W, m->cfg.vocab, s);
    }
    KEMR_TRY(carve(w, workspace_dev, workspace_bytes, ws_layout(W, rows, batch, m->res_dtype, batch + 1), m->res_dtype));
    KEMR_TRY(launch_row_starts(lens_dev, batch, T, rows, w.row_start, s));
    return launch_text_embed(ids_dev, m->tok, m->tpos, w.x, w.x_dtype, batch, T, W, m->cfg.vocab, s, w.row_start, rows);
}

// Every GEMM contracts over the tripled K on gemm.hip's 128 x 128 kernel (launch_gemm_x3); the out-proj and fc2 epilogues add
// acc + bias into x in fp32 (EPI_BIAS_RESID_F32: nothing pending for the tail, option "residual_fusion" has no meaning here).
int run_blocks_x3(const TowerW& t, const WorkspaceX3& w, int M, int batch, int causal, int activation, hipStream_t s) {
    const int W = t.width;
    const int epi_act = activation == 1 ? EPI_X3_GELU : EPI_X3_QGELU;
    for (int l = 0; l < t.layers; ++l) {
        const LayerW& L = t.layer[l];
        KEMR_TRY(launch_layernorm_x3(w.x, L.ln1_g, L.ln1_b, w.h, M, W, s));
        KEMR_TRY(launch_gemm_x3(linear(w.h, L.wqkv, L.bqkv, w.qkv, 3 * W, M, 3 * W, 3 * W), EPI_X3_F32, s));
        if (t.head_dim == 80) KEMR_TRY(launch_attention80_x3(w.qkv, w.h, batch, t.tokens, W, causal, s));
        else KEMR_TRY(launch_attention_x3(w.qkv, w.h, w.row_start, batch, t.tokens, W, causal, s));
        KEMR_TRY(launch_gemm_x3(linear(w.h, L.wo, L.bo, w.x, W, M, W, 3 * W), EPI_BIAS_RESID_F32, s));
        KEMR_TRY(launch_layernorm_x3(w.x, L.ln2_g, L.ln2_b, w.h, M, W, s));
        KEMR_TRY(launch_gemm_x3(linear(w.h, L.w1, L.b1, w.big, 12 * W, M, 4 * W, 3 * W), epi_act, s));
        KEMR_TRY(launch_gemm_x3(linear(w.big, L.w2, L.b2, w.x, W, M, W, 12 * W), EPI_BIAS_RESID_F32, s));
    }
    return KEMR_OK;
}

int encode_image_x3(kemr_model* m, const float* pixels_dev, int batch, float* out_dev, int normalize, void* workspace_dev,
                    size_t workspace_bytes, hipStream_t s, bool pooled) {
    KEMR_TRY(check_image_args(m, pixels_dev, batch, out_dev, "encode_image", true));
    if (batch == 0) return KEMR_OK;
    const int W = m->cfg.v_width, T = m->vtokens, M = batch * T;
    WorkspaceX3 w;
    KEMR_TRY(carve_x3(w, workspace_dev, workspace_bytes, ws_layout_x3(W, M, 0)));
    KEMR_TRY(launch_im2col_x3(pixels_dev, w.big, batch, m->cfg.image_size, m->cfg.patch, m->kpad, s));
    KEMR_TRY(launch_gemm_x3(patch_embed(m, w.big, 3 * m->kpad, w.x, batch), EPI_PATCH_F32, s));
    KEMR_TRY(launch_cls_rows(w.x, m->cls, m->vpos, batch, T, W, s));
    KEMR_TRY(launch_layernorm(w.x, KEMR_F32, nullptr, nullptr, 0, m->lnpre_g, m->lnpre_b, w.x, M, W, KEMR_F32, s));
    KEMR_TRY(run_blocks_x3(m->vis, w, M, batch, 0, m->activation, s));
    return launch_tail(w.x, KEMR_F32, nullptr, nullptr, nullptr, batch, T, W, m->lnpost_g, m->lnpost_b, pooled ? nullptr : m->vproj, m->cfg.embed_dim, normalize, out_dev, s);
}

int encode_text_x3(kemr_model* m, const int32_t* ids_dev, const int32_t* lens_dev, int rows, int batch, bool packed, float* out_dev,
                   int normalize, void* workspace_dev, size_t workspace_bytes, hipStream_t s, bool pooled) {
    KEMR_TRY(check_text_args(m, ids_dev, lens_dev, rows, batch, packed, out_dev, packed ? "encode_text_packed" : "encode_text", true));
    if (batch == 0) return KEMR_OK;
    const int W = m->cfg.t_width, T = m->cfg.ctx, M = packed ? rows : batch * T;
    WorkspaceX3 w;
    KEMR_TRY(carve_x3(w, workspace_dev, workspace_bytes, ws_layout_x3(W, M, packed ? batch + 1 : 0)));
    if (packed) KEMR_TRY(launch_row_starts(lens_dev, batch, T, rows, w.row_start, s));
    KEMR_TRY(launch_text_embed(ids_dev, m->tok, m->tpos, w.x, KEMR_F32, batch, T, W, m->cfg.vocab, s, w.row_start, packed ? rows : 0));
    KEMR_TRY(run_blocks_x3(m->txt, w, M, batch, 1, m->activation, s));
    return launch_tail(w.x, KEMR_F32, nullptr, nullptr, ids_dev, batch, T, W, m->lnf_g, m->lnf_b, pooled ? nullptr : m->tproj, m->cfg.embed_dim, normalize, out_dev, s, w.row_start);
}

// ---- family 2: BERT sentence encoders (transformers.BertModel without its pooler + mean / CLS pooling) on packed rows ----
// Workspace: the token-row buffers with no pooled-row area (every row runs through every block and feeds the pooling), then the
// batch + 1 row starts.  bert_front = the argument checks, the carve, the row starts and the embedding front; every check, the
// workspace's included, comes before the first launch.
int bert_front(kemr_model* m, const int32_t* ids_dev, const int32_t* lens_dev, int rows, int batch, const void* out_dev, void* workspace_dev,
               size_t workspace_bytes, hipStream_t s, const char* what, Workspace& w) {
    if (!m || !ids_dev || !lens_dev || !out_dev) KEMR_FAIL(KEMR_ERR_INVALID, "%s: null argument", what);
    if (!is_sentence_family(m->family)) KEMR_FAIL(KEMR_ERR_INVALID, "%s: only family 2 (BERT) has this front", what);
    if (!m->finalized) KEMR_FAIL(KEMR_ERR_STATE, "%s: model not finalized", what);
    if (batch <= 0) return batch == 0 ? KEMR_OK : (set_error("%s: negative batch", what), KEMR_ERR_INVALID);
    const int W = m->cfg.t_width, T = m->cfg.ctx;
    if (batch > 65535) KEMR_FAIL(KEMR_ERR_INVALID, "%s: batch %d > 65535", what, batch);
    if (rows < batch || (int64_t)rows > (int64_t)batch * T) KEMR_FAIL(KEMR_ERR_INVALID, "%s: %d rows for %d texts of 1 .. %d positions", what, rows, batch, T);
    if (rows > (1 << 24)) KEMR_FAIL(KEMR_ERR_INVALID, "%s: %d rows in one call (at most %d)", what, rows, 1 << 24);
    KEMR_TRY(carve(w, workspace_dev, workspace_bytes, ws_layout(W, rows, 0, m->res_dtype, batch + 1), m->res_dtype));
    KEMR_TRY(launch_row_starts(lens_dev, batch, T, rows, w.row_start, s));
    return launch_bert_embed(ids_dev, m->tok, m->tpos, m->lne_g, m->lne_b, w.x, w.x_dtype, w.h, batch, T, W, m->cfg.vocab, w.row_start, rows, m->eps, s);
}

// Post-LN blocks: QKV on h, attention over the packed items, out-proj into delta (store-only), x = LN(x + delta) with h = bf16(x), fc1
// with the exact GELU, fc2 into delta2, x = LN(x + delta2) with h = bf16(x).  Options "residual_fusion", "last_block_pooled_row" and
// "activation" are not consulted.  Family 3 (MPNet) runs the same sequence; its attention launch carries the model's bias table.
int encode_bert(kemr_model* m, const int32_t* ids_dev, const int32_t* lens_dev, int rows, int batch, float* out_dev, int normalize,
                void* workspace_dev, size_t workspace_bytes, hipStream_t s) {
    Workspace w;
    KEMR_TRY(bert_front(m, ids_dev, lens_dev, rows, batch, out_dev, workspace_dev, workspace_bytes, s, "encode_text_packed", w));
    if (batch == 0) return KEMR_OK;
    const TowerW& t = m->txt;
    const int W = t.width, M = rows;
    for (int l = 0; l < t.layers; ++l) {
        const LayerW& L = t.layer[l];
        KEMR_TRY(launch_gemm(linear(w.h, L.wqkv, L.bqkv, w.big, 3 * W, M, 3 * W, W), EPI_BIAS_BF16, s));
        KEMR_TRY(launch_attention_varlen(w.big, w.h, w.row_start, batch, t.tokens, W, s, m->family == 3 ? m->rel_bias : nullptr));
        KEMR_TRY(launch_gemm(linear(w.h, L.wo, L.bo, w.delta, W, M, W, W), EPI_BIAS_BF16, s));
        KEMR_TRY(launch_layernorm_post(w.x, w.x_dtype, w.delta, L.ln1_g, L.ln1_b, w.h, M, W, s, m->eps));
        KEMR_TRY(launch_gemm(linear(w.h, L.w1, L.b1, w.big, 4 * W, M, 4 * W, W), EPI_BIAS_GELU_BF16, s));
        KEMR_TRY(launch_gemm(linear(w.big, L.w2, L.b2, w.delta2, W, M, W, 4 * W), EPI_BIAS_BF16, s));
        KEMR_TRY(launch_layernorm_post(w.x, w.x_dtype, w.delta2, L.ln2_g, L.ln2_b, w.h, M, W, s, m->eps));
    }
    return launch_pool_rows(w.x, w.x_dtype, w.row_start, batch, W, m->pooling, normalize, out_dev, s);
}

// family 1's activation is the family's (tanh GELU); option "activation" is not consulted there
int fc1_epilogue(const kemr_model* m) { return m->family == 1 ? EPI_BIAS_TGELU_BF16 : m->activation == 1 ? EPI_BIAS_GELU_BF16 : EPI_BIAS_QGELU_BF16; }

// pooled: the tail stores the pooled row of the residual stream (pending updates applied) instead of normalising and projecting it --
// kemr_encode_*_pooled; family 0 only (SigLIP's head is the attention pool over every row, BERT has no head)
int pooled_family_check(const kemr_model* m, bool pooled, const char* what) {
    if (pooled && m && m->family == 1) KEMR_FAIL(KEMR_ERR_INVALID, "%s: not available for family 1 (SigLIP): its head is the attention pool over every row, not LayerNorm + projection of one pooled row", what);
    if (pooled && m && is_sentence_family(m->family)) KEMR_FAIL(KEMR_ERR_INVALID, "%s: not available for family 2 (BERT): a sentence encoder has no projection head", what);
    return KEMR_OK;
}

int encode_image_any(kemr_model* m, const float* pixels_dev, int batch, float* out_dev, int normalize,
                     void* workspace_dev, size_t workspace_bytes, void* stream, bool pooled) {
    hipStream_t s = (hipStream_t)stream;
    KEMR_TRY(pooled_family_check(m, pooled, "encode_image_pooled"));
    if (m && is_sentence_family(m->family)) KEMR_FAIL(KEMR_ERR_INVALID, "encode_image: not available for family 2 (BERT): a text-only model has no vision tower");
    if (m && m->finalized && m->x3) return encode_image_x3(m, pixels_dev, batch, out_dev, normalize, workspace_dev, workspace_bytes, s, pooled);
    Workspace w;
    KEMR_TRY(image_front(m, pixels_dev, batch, out_dev, workspace_dev, workspace_bytes, s, "encode_image", w));
    if (batch == 0) return KEMR_OK;
    const int W = m->cfg.v_width, T = m->vtokens;
    const float* vproj = pooled ? nullptr : m->vproj;
    BlockOpts o;
    o.want_resadd = m->resadd; o.epi_act = fc1_epilogue(m);
    BlockResult r;
    if (m->family == 1) {
        // no ln_pre: the front's fp32 rows enter block 0 in the stream's storage type; every row of the last block feeds the pooling
        // head, so option "last_block_pooled_row" cannot apply; ln_post (applying the last block's pending updates) runs over all rows
        o.eps = m->eps;
        KEMR_TRY(launch_stream_cast(w.x32, w.x, w.x_dtype, (int64_t)batch * T, W, s));
        KEMR_TRY(run_blocks(m->vis, w, batch, o, s, r));
        KEMR_TRY(launch_layernorm(w.x, w.x_dtype, r.pending ? w.delta : nullptr, r.pending ? w.delta2 : nullptr, r.pending ? 1 : 0, m->lnpost_g, m->lnpost_b, w.h, batch * T, W, KEMR_BF16, s, m->eps));
        return map_head(m, w, w.h, batch, normalize, out_dev, s);
    }
    o.fp8 = m->fp8; o.last_pooled = m->last_pooled;
    KEMR_TRY(launch_layernorm(w.x32, KEMR_F32, nullptr, nullptr, 0, m->lnpre_g, m->lnpre_b, w.x, batch * T, W, w.x_dtype, s));
    KEMR_TRY(run_blocks(m->vis, w, batch, o, s, r));
    if (r.compact) return launch_tail(w.xc, w.x_dtype, w.d1c, w.d2c, nullptr, batch, 1, W, m->lnpost_g, m->lnpost_b, vproj, m->cfg.embed_dim, normalize, out_dev, s);
    return launch_tail(w.x, w.x_dtype, r.pending ? w.delta : nullptr, r.pending ? w.delta2 : nullptr, nullptr, batch, T, W, m->lnpost_g, m->lnpost_b, vproj, m->cfg.embed_dim, normalize, out_dev, s);
}

// packed: the text tower on the rows that can reach the output only.  The attention mask is causal and the pooled row is the end-of-text
// token's (reference: model.encode_text -> x[arange, text.argmax(-1)]; open_clip / CLIP text transformer with attn_mask), so the
// positions behind it never influence the embedding: text i is computed on its first lens_dev[i] positions, packed one text
// behind the other (`rows` = sum(lens) rows instead of batch * ctx through every GEMM, LayerNorm and attention launch).  With
// lens[i] >= argmax_i + 1 the embeddings are kemr_encode_text's -- the same arithmetic per row; the GEMM a launch of another M is
// routed to may sum in another order, as for another batch size (tests/test_encoder_gpu.py: 1 - cos of a few 1e-5 both ways); a
// shorter length pools the last computed row instead (memory-safe, wrong).  `rows` is a HOST integer: the tokenizer's side knows the lengths without
// asking the device (the python wrapper derives lens and rows from the same host tokens); lengths and prefix sums are clamped on the
// device (row_starts_kernel) so that no argument can index outside the workspace.
int encode_text_any(kemr_model* m, const int32_t* ids_dev, const int32_t* lens_dev, int rows, int batch, bool packed, float* out_dev,
                    int normalize, void* workspace_dev, size_t workspace_bytes, void* stream, bool pooled) {
    hipStream_t s = (hipStream_t)stream;
    KEMR_TRY(pooled_family_check(m, pooled, packed ? "encode_text_packed_pooled" : "encode_text_pooled"));
    if (!packed && m && is_sentence_family(m->family))
        KEMR_FAIL(KEMR_ERR_INVALID, "encode_text: not available for family 2 (BERT): a padding mask is a length -- call kemr_encode_text_packed with the lengths");
    if (packed && m && m->family == 1)
        KEMR_FAIL(KEMR_ERR_INVALID, "encode_text_packed: not available for family 1 (SigLIP): its text tower is unmasked and pools the last position, so a pad position is a key and no row can be left out");
    if (packed && m && is_sentence_family(m->family)) return encode_bert(m, ids_dev, lens_dev, rows, batch, out_dev, normalize, workspace_dev, workspace_bytes, s);
    if (m && m->finalized && m->x3) return encode_text_x3(m, ids_dev, lens_dev, rows, batch, packed, out_dev, normalize, workspace_dev, workspace_bytes, s, pooled);
    Workspace w;
    KEMR_TRY(text_front(m, ids_dev, lens_dev, rows, batch, packed, out_dev, workspace_dev, workspace_bytes, s, packed ? "encode_text_packed" : "encode_text", w));
    if (batch == 0) return KEMR_OK;
    const int W = m->cfg.t_width, T = m->cfg.ctx;
    BlockOpts o;
    o.want_resadd = m->resadd; o.epi_act = fc1_epilogue(m); o.last_pooled = m->last_pooled;
    BlockResult r;
    if (m->family == 1) {
        // no mask (pads are keys like every other position), the LAST position pooled whatever the ids, the head a Linear with bias
        o.eps = m->eps; o.pool_pos = T - 1;
        KEMR_TRY(run_blocks(m->txt, w, batch, o, s, r));
        if (r.compact) return launch_tail(w.xc, w.x_dtype, w.d1c, w.d2c, nullptr, batch, 1, W, m->lnf_g, m->lnf_b, m->tproj, m->cfg.embed_dim, normalize, out_dev, s, nullptr, m->eps, 0, m->tproj_b);
        return launch_tail(w.x, w.x_dtype, r.pending ? w.delta : nullptr, r.pending ? w.delta2 : nullptr, nullptr, batch, T, W, m->lnf_g, m->lnf_b, m->tproj, m->cfg.embed_dim, normalize, out_dev, s, nullptr, m->eps, T - 1, m->tproj_b);
    }
    const float* tproj = pooled ? nullptr : m->tproj;
    o.causal = 1; o.row_start = w.row_start; o.rows = rows; o.ids = ids_dev;
    KEMR_TRY(run_blocks(m->txt, w, batch, o, s, r));
    if (r.compact) return launch_tail(w.xc, w.x_dtype, w.d1c, w.d2c, nullptr, batch, 1, W, m->lnf_g, m->lnf_b, tproj, m->cfg.embed_dim, normalize, out_dev, s);
    return launch_tail(w.x, w.x_dtype, r.pending ? w.delta : nullptr, r.pending ? w.delta2 : nullptr, ids_dev, batch, T, W, m->lnf_g, m->lnf_b, tproj, m->cfg.embed_dim, normalize, out_dev, s, w.row_start);
}

}  // namespace

extern "C" size_t kemr_workspace_bytes(const kemr_model* m, int tower, int batch) {
    if (!m || batch <= 0) return 0;
    if (is_sentence_family(m->family)) return 0;                      // family 2 has the packed call only (kemr_text_packed_workspace_bytes)
    if (tower != KEMR_TOWER_VISION && tower != KEMR_TOWER_TEXT) return 0;
    const bool vision = tower == KEMR_TOWER_VISION;
    const int W = vision ? m->cfg.v_width : m->cfg.t_width;
    const int64_t rows = (int64_t)batch * (vision ? m->vtokens : m->cfg.ctx);
    return m->x3 ? ws_layout_x3(W, rows, 0).total : ws_layout(W, rows, batch, m->res_dtype, 0).total;
}

extern "C" size_t kemr_text_packed_workspace_bytes(const kemr_model* m, int rows, int batch) {
    if (!m || batch <= 0 || rows < batch) return 0;
    if (m->x3) return ws_layout_x3(m->cfg.t_width, rows, batch + 1).total;
    // buffers + pooled-row area (none for family 2) + row_start
    return ws_layout(m->cfg.t_width, rows, is_sentence_family(m->family) ? 0 : batch, m->res_dtype, batch + 1).total;
}

extern "C" int kemr_encode_image(kemr_model* m, const float* pixels_dev, int batch, float* out_dev, int normalize,
                                 void* workspace_dev, size_t workspace_bytes, void* stream) {
    return encode_image_any(m, pixels_dev, batch, out_dev, normalize, workspace_dev, workspace_bytes, stream, false);
}
extern "C" int kemr_encode_text(kemr_model* m, const int32_t* ids_dev, int batch, float* out_dev, int normalize,
                                void* workspace_dev, size_t workspace_bytes, void* stream) {
    return encode_text_any(m, ids_dev, nullptr, 0, batch, false, out_dev, normalize, workspace_dev, workspace_bytes, stream, false);
}
extern "C" int kemr_encode_text_packed(kemr_model* m, const int32_t* ids_dev, const int32_t* lens_dev, int rows, int batch, float* out_dev,
                                       int normalize, void* workspace_dev, size_t workspace_bytes, void* stream) {
    return encode_text_any(m, ids_dev, lens_dev, rows, batch, true, out_dev, normalize, workspace_dev, workspace_bytes, stream, false);
}
extern "C" int kemr_encode_image_pooled(kemr_model* m, const float* pixels_dev, int batch, float* out_dev,
                                        void* workspace_dev, size_t workspace_bytes, void* stream) {
    return encode_image_any(m, pixels_dev, batch, out_dev, 0, workspace_dev, workspace_bytes, stream, true);
}
extern "C" int kemr_encode_text_pooled(kemr_model* m, const int32_t* ids_dev, int batch, float* out_dev,
                                       void* workspace_dev, size_t workspace_bytes, void* stream) {
    return encode_text_any(m, ids_dev, nullptr, 0, batch, false, out_dev, 0, workspace_dev, workspace_bytes, stream, true);
}
extern "C" int kemr_encode_text_packed_pooled(kemr_model* m, const int32_t* ids_dev, const int32_t* lens_dev, int rows, int batch, float* out_dev,
                                              void* workspace_dev, size_t workspace_bytes, void* stream) {
    return encode_text_any(m, ids_dev, lens_dev, rows, batch, true, out_dev, 0, workspace_dev, workspace_bytes, stream, true);
}

// ------------------------------------------------------------------------------------------------ include/kemr_debug.h
// the token fronts of the encoders (image_front / text_front, the same checks and workspace), then a copy of what they leave behind
extern "C" int kemr_debug_image_tokens(kemr_model* m, const float* pixels_dev, int batch, float* out_dev, void* workspace_dev,
                                       size_t workspace_bytes, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    Workspace w;
    KEMR_TRY(image_front(m, pixels_dev, batch, out_dev, workspace_dev, workspace_bytes, s, "debug_image_tokens", w));
    if (batch == 0) return KEMR_OK;
    const size_t bytes = (size_t)batch * m->vtokens * m->cfg.v_width * 4;
    KEMR_CHECK_HIP(hipMemcpyAsync(out_dev, w.x32, bytes, hipMemcpyDeviceToDevice, s));
    return KEMR_OK;
}

// family 1's pooling head alone: h_dev = bf16 [batch * tokens, v_width] post-LayerNorm token rows (copied into the workspace, whose
// buffers have the pad rows the GEMMs read); attn_out_dev (optional) receives the attention output rows bf16 [batch, v_width]
extern "C" int kemr_debug_map_head(kemr_model* m, const void* h_dev, int batch, void* attn_out_dev, float* out_dev, int normalize,
                                   void* workspace_dev, size_t workspace_bytes, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    if (!m || !h_dev || !out_dev) KEMR_FAIL(KEMR_ERR_INVALID, "debug_map_head: null argument");
    if (!m->finalized) KEMR_FAIL(KEMR_ERR_STATE, "debug_map_head: model not finalized");
    if (m->family != 1) KEMR_FAIL(KEMR_ERR_INVALID, "debug_map_head: only family 1 (SigLIP) has a pooling head");
    if (batch <= 0) return batch == 0 ? KEMR_OK : (set_error("debug_map_head: negative batch"), KEMR_ERR_INVALID);
    if ((int64_t)batch * m->vtokens > (1 << 24)) KEMR_FAIL(KEMR_ERR_INVALID, "debug_map_head: batch %d too large", batch);
    const int W = m->cfg.v_width, T = m->vtokens;
    Workspace w;
    KEMR_TRY(carve(w, workspace_dev, workspace_bytes, ws_layout(W, (int64_t)batch * T, batch, m->res_dtype, 0), m->res_dtype));
    KEMR_CHECK_HIP(hipMemcpyAsync(w.h, h_dev, (size_t)batch * T * W * 2, hipMemcpyDeviceToDevice, s));
    KEMR_TRY(map_head(m, w, w.h, batch, normalize, out_dev, s));
    if (attn_out_dev) KEMR_CHECK_HIP(hipMemcpyAsync(attn_out_dev, w.ac, (size_t)batch * W * 2, hipMemcpyDeviceToDevice, s));
    return KEMR_OK;
}

extern "C" int kemr_debug_bert_front(kemr_model* m, const int32_t* ids_dev, const int32_t* lens_dev, int rows, int batch, void* x_out_dev,
                                     void* h_out_dev, int* row_start_out_dev, void* workspace_dev, size_t workspace_bytes, void* stream) {
    if (!h_out_dev || !row_start_out_dev) KEMR_FAIL(KEMR_ERR_INVALID, "debug_bert_front: null output");
    hipStream_t s = (hipStream_t)stream;
    Workspace w;
    KEMR_TRY(bert_front(m, ids_dev, lens_dev, rows, batch, x_out_dev, workspace_dev, workspace_bytes, s, "debug_bert_front", w));
    if (batch == 0) return KEMR_OK;
    KEMR_CHECK_HIP(hipMemcpyAsync(x_out_dev, w.x, (size_t)rows * m->cfg.t_width * stream_elem_bytes(w.x_dtype), hipMemcpyDeviceToDevice, s));
    KEMR_CHECK_HIP(hipMemcpyAsync(h_out_dev, w.h, (size_t)rows * m->cfg.t_width * 2, hipMemcpyDeviceToDevice, s));
    KEMR_CHECK_HIP(hipMemcpyAsync(row_start_out_dev, w.row_start, ((size_t)batch + 1) * 4, hipMemcpyDeviceToDevice, s));
    return KEMR_OK;
}

extern "C" int kemr_debug_text_tokens(kemr_model* m, const int32_t* ids_dev, const int32_t* lens_dev, int rows, int batch, void* out_dev,
                                      int* row_start_out_dev, void* workspace_dev, size_t workspace_bytes, void* stream) {
    const bool packed = lens_dev != nullptr;
    if (packed && !row_start_out_dev) KEMR_FAIL(KEMR_ERR_INVALID, "debug_text_tokens: null row_start output");
    hipStream_t s = (hipStream_t)stream;
    Workspace w;
    KEMR_TRY(text_front(m, ids_dev, lens_dev, rows, batch, packed, out_dev, workspace_dev, workspace_bytes, s, "debug_text_tokens", w));
    if (batch == 0) return KEMR_OK;
    const int64_t n = packed ? rows : (int64_t)batch * m->cfg.ctx;
    KEMR_CHECK_HIP(hipMemcpyAsync(out_dev, w.x, (size_t)n * m->cfg.t_width * stream_elem_bytes(w.x_dtype), hipMemcpyDeviceToDevice, s));
    if (packed) KEMR_CHECK_HIP(hipMemcpyAsync(row_start_out_dev, w.row_start, ((size_t)batch + 1) * 4, hipMemcpyDeviceToDevice, s));
    return KEMR_OK;
}
