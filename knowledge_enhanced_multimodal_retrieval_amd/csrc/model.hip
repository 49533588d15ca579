// libkemr.so: the model handle -- create, the required-tensor list, load_tensor, options, weight packing, finalize, destroy.
// Host-side C++ only.  Packing (pack_weights) is pure host code: no HIP call, the loaded tensors are left as they are.
#include "model.h"
#include "../../include/kemr_debug.h"

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>

using namespace kemr;

namespace {

constexpr int REL_DISTANCES = 2 * KEMR_MAX_BERT_CTX - 1;    // key - query in -511 .. 511

int check_cfg(const kemr_cfg& c) {
    if (c.embed_dim <= 0 || c.embed_dim > 1024) KEMR_FAIL(KEMR_ERR_INVALID, "cfg: embed_dim %d not in 1..1024", c.embed_dim);
    if (c.patch <= 0 || c.image_size <= 0 || c.image_size % c.patch) KEMR_FAIL(KEMR_ERR_INVALID, "cfg: image_size %% patch != 0");
    if (c.v_width % 256 || c.t_width % 256 || c.v_width <= 0 || c.t_width <= 0 || c.v_width > 1280 || c.t_width > 1280)
        KEMR_FAIL(KEMR_ERR_INVALID, "cfg: widths must be multiples of 256 in 256..1280 (got %d, %d)", c.v_width, c.t_width);
    if (c.v_layers <= 0 || c.t_layers <= 0 || c.vocab <= 0 || c.ctx <= 0) KEMR_FAIL(KEMR_ERR_INVALID, "cfg: non-positive field");
    const int g = c.image_size / c.patch;
    if (c.ctx > KEMR_MAX_TEXT_CTX) KEMR_FAIL(KEMR_ERR_INVALID, "cfg: sequence length > 288 not supported");
    if ((int64_t)g * g + 1 > KEMR_MAX_VISION_TOKENS)
        KEMR_FAIL(KEMR_ERR_INVALID, "cfg: vision sequence length %lld > %d not supported", (long long)g * g + 1, KEMR_MAX_VISION_TOKENS);
    const int kpad = (int)round_up(3 * c.patch * c.patch, 64);
    if (kpad > 4 * c.v_width) KEMR_FAIL(KEMR_ERR_INVALID, "cfg: patch too large for the workspace layout");
    return KEMR_OK;
}

// family 2 (BERT sentence encoders): text-only, the vision fields are 0, the embedding is the pooled stream row
int check_cfg_bert(const kemr_cfg& c) {
    if (c.image_size || c.patch || c.v_width || c.v_layers)
        KEMR_FAIL(KEMR_ERR_INVALID, "cfg: family 2 (BERT) is text-only: image_size, patch, v_width and v_layers must be 0 (got %d, %d, %d, %d)", c.image_size, c.patch, c.v_width, c.v_layers);
    if (c.t_width != 256 && c.t_width != 512 && c.t_width != 768 && c.t_width != 1024 && c.t_width != 1280)
        KEMR_FAIL(KEMR_ERR_INVALID, "cfg: family 2 (BERT) serves t_width in {256,512,768,1024,1280}, got %d", c.t_width);
    if (c.embed_dim != c.t_width)
        KEMR_FAIL(KEMR_ERR_INVALID, "cfg: family 2 (BERT) has no projection: embed_dim %d must equal t_width %d", c.embed_dim, c.t_width);
    if (c.t_layers <= 0 || c.vocab <= 0 || c.ctx <= 0) KEMR_FAIL(KEMR_ERR_INVALID, "cfg: non-positive field");
    if (c.ctx > KEMR_MAX_BERT_CTX) KEMR_FAIL(KEMR_ERR_INVALID, "cfg: family 2 (BERT) sequence length %d > %d not supported", c.ctx, KEMR_MAX_BERT_CTX);
    return KEMR_OK;
}

// The required tensors of a model family, in load order (kemr_model_create; option "family" rebuilds the list): name, shape, what the
// tensor is (TensorKind) and the pointer of the model that its device copy is bound to.  The ONE place that knows tensor names.
void build_names(kemr_model* m) {
    const kemr_cfg* cfg = &m->cfg;
    m->specs.clear();
    m->index.clear();
    auto add = [&](const std::string& n, std::vector<int64_t> shape, TensorTower tower, TensorKind kind, void* bind, int layer = -1) {
        m->index[n] = (int)m->specs.size();
        m->specs.push_back(TensorSpec{n, tower, layer, kind, bind, HostTensor{std::move(shape)}});
    };
    // pre-LN blocks: ln_1 feeds QKV, ln_2 feeds fc1 (family 2's post-LN blocks carry the same names; fp8 is not served there)
    auto blocks = [&](const std::string& prefix, TensorTower tower, TowerW& tw, int64_t w, int layers, int tokens) {
        tw.width = (int)w; tw.layers = layers; tw.tokens = tokens;
        tw.layer.assign(layers, LayerW{});
        for (int i = 0; i < layers; ++i) {
            const std::string b = prefix + ".resblocks." + std::to_string(i);
            LayerW& L = tw.layer[i];
            add(b + ".ln_1.weight", {w}, tower, KIND_LN_QKV, &L.ln1_g, i);
            add(b + ".ln_1.bias", {w}, tower, KIND_LN_QKV, &L.ln1_b, i);
            add(b + ".attn.in_proj_weight", {3 * w, w}, tower, KIND_QKV_WEIGHT, &L.wqkv, i);
            add(b + ".attn.in_proj_bias", {3 * w}, tower, KIND_QKV_BIAS, &L.bqkv, i);
            add(b + ".attn.out_proj.weight", {w, w}, tower, KIND_MATRIX, &L.wo, i);
            add(b + ".attn.out_proj.bias", {w}, tower, KIND_F32, &L.bo, i);
            add(b + ".ln_2.weight", {w}, tower, KIND_LN_FC1, &L.ln2_g, i);
            add(b + ".ln_2.bias", {w}, tower, KIND_LN_FC1, &L.ln2_b, i);
            add(b + ".mlp.c_fc.weight", {4 * w, w}, tower, KIND_FC1_WEIGHT, &L.w1, i);
            add(b + ".mlp.c_fc.bias", {4 * w}, tower, KIND_F32, &L.b1, i);
            add(b + ".mlp.c_proj.weight", {w, 4 * w}, tower, KIND_MATRIX, &L.w2, i);
            add(b + ".mlp.c_proj.bias", {w}, tower, KIND_F32, &L.b2, i);
        }
    };
    const int64_t vw = cfg->v_width, tw = cfg->t_width, D = cfg->embed_dim;
    const TensorTower V = TOWER_VISION, T = TOWER_TEXT, H = TOWER_HEAD;
    if (is_sentence_family(m->family)) {
        // BertModel without its pooler, by OpenAI-style names: ln_1 = attention.output.LayerNorm, ln_2 = output.LayerNorm (post-LN).
        // Family 3 (MPNetModel): no token types (the positional table is taken verbatim: the caller passes position_embeddings[2 : 2 + ctx]),
        // and the encoder's one relative_attention_bias for all layers
        const bool mpnet = m->family == 3;
        m->vtokens = 0;
        m->eps = mpnet ? (m->ln_eps_exp == 12 ? 1e-12f : 1e-5f) : 1e-12f;
        add("token_embedding.weight", {cfg->vocab, tw}, T, KIND_F32, &m->tok);
        add("positional_embedding", {cfg->ctx, tw}, T, mpnet ? KIND_F32 : KIND_TPOS_BERT, &m->tpos);
        if (mpnet) add("relative_attention_bias", {32, tw / 64}, T, KIND_REL_BIAS, &m->rel_bias);
        else add("token_type_embedding", {2, tw}, T, KIND_F32, nullptr);
        add("ln_embed.weight", {tw}, T, KIND_F32, &m->lne_g);
        add("ln_embed.bias", {tw}, T, KIND_F32, &m->lne_b);
        blocks("transformer", T, m->txt, tw, cfg->t_layers, cfg->ctx);
        return;
    }
    const bool sig = m->family == 1;
    m->vtokens = sig ? m->patches : m->patches + 1;
    m->eps = sig ? 1e-6f : 1e-5f;
    add("visual.conv1.weight", {vw, 3, cfg->patch, cfg->patch}, V, KIND_CONV_WEIGHT, &m->conv_w);
    if (sig) add("visual.conv1.bias", {vw}, V, KIND_F32, nullptr);
    else add("visual.class_embedding", {vw}, V, KIND_F32, &m->cls);
    add("visual.positional_embedding", {m->vtokens, vw}, V, sig ? KIND_VPOS_SIGLIP : KIND_F32, &m->vpos);
    if (!sig) {
        add("visual.ln_pre.weight", {vw}, V, KIND_F32, &m->lnpre_g);
        add("visual.ln_pre.bias", {vw}, V, KIND_F32, &m->lnpre_b);
    }
    blocks("visual.transformer", V, m->vis, vw, cfg->v_layers, m->vtokens);
    add("visual.ln_post.weight", {vw}, V, KIND_F32, &m->lnpost_g);
    add("visual.ln_post.bias", {vw}, V, KIND_F32, &m->lnpost_b);
    if (sig) {
        // the head's in_proj takes the QKV kinds like a block's, so the q rows of its device copy carry the 1/8 too.  Nothing reads those
        // q rows: the head's one query is made from the host fp32 tensors (KIND_PROBE) and mh_wkv / mh_bkv start behind them.
        const std::string h = "visual.attn_pool";
        add(h + ".probe", {vw}, H, KIND_PROBE, &m->mh_q);
        add(h + ".in_proj_weight", {3 * vw, vw}, H, KIND_QKV_WEIGHT, &m->mh_wkv);
        add(h + ".in_proj_bias", {3 * vw}, H, KIND_QKV_BIAS, &m->mh_bkv);
        add(h + ".out_proj.weight", {vw, vw}, H, KIND_MATRIX, &m->mh_wo);
        add(h + ".out_proj.bias", {vw}, H, KIND_F32, &m->mh_bo);
        add(h + ".ln.weight", {vw}, H, KIND_F32, &m->mh_ln_g);
        add(h + ".ln.bias", {vw}, H, KIND_F32, &m->mh_ln_b);
        add(h + ".mlp.c_fc.weight", {4 * vw, vw}, H, KIND_FC1_WEIGHT, &m->mh_w1);
        add(h + ".mlp.c_fc.bias", {4 * vw}, H, KIND_F32, &m->mh_b1);
        add(h + ".mlp.c_proj.weight", {vw, 4 * vw}, H, KIND_MATRIX, &m->mh_w2);
        add(h + ".mlp.c_proj.bias", {vw}, H, KIND_F32, &m->mh_b2);
    } else {
        add("visual.proj", {vw, D}, V, KIND_F32, &m->vproj);
    }
    add("token_embedding.weight", {cfg->vocab, tw}, T, KIND_F32, &m->tok);
    add("positional_embedding", {cfg->ctx, tw}, T, KIND_F32, &m->tpos);
    blocks("transformer", T, m->txt, tw, cfg->t_layers, cfg->ctx);
    add("ln_final.weight", {tw}, T, KIND_F32, &m->lnf_g);
    add("ln_final.bias", {tw}, T, KIND_F32, &m->lnf_b);
    add("text_projection", {tw, D}, T, KIND_F32, &m->tproj);
    if (sig) add("text_projection_bias", {D}, T, KIND_F32, &m->tproj_b);
}

int model_create(const kemr_cfg* cfg, int family, kemr_model** out) {
    if (!cfg || !out) KEMR_FAIL(KEMR_ERR_INVALID, "model_create: null argument");
    if (family == 3) KEMR_FAIL(KEMR_ERR_INVALID, "model_create_family: family 0 (CLIP), 1 (SigLIP) or 2 (BERT), got 3 (family 3, MPNet, is a family 2 model switched by kemr_model_set_option(m, \"family\", 3) before its first tensor is loaded)");
    if (family < 0 || family > 2) KEMR_FAIL(KEMR_ERR_INVALID, "model_create_family: family 0 (CLIP), 1 (SigLIP) or 2 (BERT), got %d", family);
    KEMR_TRY(is_sentence_family(family) ? check_cfg_bert(*cfg) : check_cfg(*cfg));
    kemr_model* m = new (std::nothrow) kemr_model();
    if (!m) KEMR_FAIL(KEMR_ERR_NOMEM, "model_create: out of memory");
    m->cfg = *cfg;
    m->family = family;
    { const char* v = getenv("KEMR_RESADD"); const int e = (v && *v) ? atoi(v) : 1; m->resadd = e < 0 ? 0 : e > 2 ? 2 : e; }
    { const char* v = getenv("KEMR_LAST_BLOCK_FULL"); m->last_pooled = (v && *v && atoi(v) != 0) ? 0 : 1; }
    { const char* v = getenv("KEMR_STREAM24"); m->stream24 = (v && *v) ? (atoi(v) != 0 ? 1 : 0) : 1; }
    if (!is_sentence_family(family)) {
        m->grid = cfg->image_size / cfg->patch;
        m->patches = m->grid * m->grid;
        m->kpad = (int)round_up(3 * cfg->patch * cfg->patch, 64);
    }
    build_names(m);
    *out = m;
    return KEMR_OK;
}

// ---- packing ----
bool is_e4m3(const TensorSpec& s, int fp8) {
    // fp8 operands in the VISION tower only (round 4): the text tower is 9 % of a gallery item's GEMM work and its embedding is ONE
    // row behind a causal softmax -- e4m3 q / k / v cost it 1 - cos 1.4e-3 against the fp32 oracle (2.9e-3 .. 5e-3 on heavy-tailed
    // weights), over north_star's 1e-3, for a 1 % gain in items/s; the image embedding averages 257 rows and stays at 2e-5 .. 1e-4.
    return s.tower == TOWER_VISION && ((s.kind == KIND_QKV_WEIGHT && (fp8 & 1)) || (s.kind == KIND_FC1_WEIGHT && (fp8 & 2)));
}

// KEMR_PREC_FP32X3: element (row, k) of a W-side triple [N, 3K] = [hi | hi | lo]
void put_x3(bf16_t* d, size_t row, size_t K, size_t k, float v) {
    const bf16_t hi = f32_to_bf16_host(v);
    uint32_t u = (uint32_t)hi << 16;
    float hf; memcpy(&hf, &u, 4);
    d[row * 3 * K + k] = hi;
    d[row * 3 * K + K + k] = hi;
    d[row * 3 * K + 2 * K + k] = f32_to_bf16_host(v - hf);
}

// A matrix [rows, cols] whose first `qrows` rows are scaled by qs in fp32 BEFORE any rounding: bf16, the fp32x3 triple, or (a_scale !=
// nullptr) e4m3 with one scale per output channel (row), scale = amax / 448, the A operand's channel scales folded into the columns.
void fill_matrix(const HostTensor& t, int64_t qrows, float qs, bool x3, const std::vector<float>* a_scale, char* dst, float* row_scale) {
    const int64_t rows = t.shape[0], cols = t.shape[1];
    for (int64_t r = 0; r < rows; ++r) {
        auto v = [&](int64_t c) { return r < qrows ? t.data[r * cols + c] * qs : t.data[r * cols + c]; };
        if (a_scale) {
            float amax = 0.f;
            for (int64_t c = 0; c < cols; ++c) amax = fmaxf(amax, fabsf(v(c) * (*a_scale)[c]));
            const float scale = amax > 0.f ? amax / 448.f : 1.0f;
            row_scale[r] = scale;
            for (int64_t c = 0; c < cols; ++c) ((uint8_t*)dst)[r * cols + c] = f32_to_e4m3_host(v(c) * (*a_scale)[c] / scale);
        } else if (x3) {
            for (int64_t c = 0; c < cols; ++c) put_x3((bf16_t*)dst, r, cols, c, v(c));
        } else {
            for (int64_t c = 0; c < cols; ++c) ((bf16_t*)dst)[r * cols + c] = f32_to_bf16_host(v(c));
        }
    }
}

const std::vector<float>& host_data(const kemr_model& m, const char* name) { return m.specs[m.index.at(name)].t.data; }

// d[i] = a[i] + row[i % w]: a vector every row of a positional table carries (added in fp32, one add per element on the device saved)
void add_row(const std::vector<float>& a, const std::vector<float>& row, size_t w, float* d) {
    for (size_t i = 0; i < a.size(); ++i) d[i] = a[i] + row[i % w];
}

void bind_weights(kemr_model* m, int fp8, const std::vector<Placement>& at) {
    const size_t vw = (size_t)m->cfg.v_width;
    for (LayerW& L : m->vis.layer) L = LayerW{};
    for (LayerW& L : m->txt.layer) L = LayerW{};
    for (size_t i = 0; i < m->specs.size(); ++i) {
        const TensorSpec& s = m->specs[i];
        const char* p = m->arena + at[i].off;
        if (is_e4m3(s, fp8)) {                             // the e4m3 copy and its row scales instead of the bf16 matrix
            LayerW& L = m->vis.layer[s.layer];
            (s.kind == KIND_QKV_WEIGHT ? L.wqkv8 : L.w18) = (const uint8_t*)p;
            (s.kind == KIND_QKV_WEIGHT ? L.sqkv : L.s1) = (const float*)(m->arena + at[i].aux);
            continue;
        }
        if (s.kind == KIND_PROBE) p = m->arena + at[i].aux;                            // mh_q: the query behind the probe
        if (s.tower == TOWER_HEAD && s.kind == KIND_QKV_WEIGHT) p += vw * vw * 2;      // mh_wkv: behind the bf16 query rows
        if (s.tower == TOWER_HEAD && s.kind == KIND_QKV_BIAS) p += vw * 4;             // mh_bkv likewise
        if (s.bind) memcpy(s.bind, &p, sizeof(p));
    }
}

}  // namespace

namespace kemr {

int relative_position_bucket(int d) {
    // n = query - key; keys behind the query (n < 0) take the upper 16 buckets; |n| < 8 is its own bucket, beyond that the eight
    // logarithmic buckets 8 .. 15 begin at the distances below (the integer form of 8 + floor(log(|n| / 8) / log(128 / 8) * 8), clamped to 15)
    static const int first[8] = {8, 12, 16, 23, 32, 46, 64, 91};
    const int n = -d, a = n < 0 ? -n : n;
    int b = a;
    if (a >= 8) {
        b = 8;
        while (b < 15 && a >= first[b - 8 + 1]) ++b;
    }
    return b + (n < 0 ? 16 : 0);
}

void expand_relative_bias(const float* weight, int heads, float* out) {
    for (int h = 0; h < heads; ++h)
        for (int d = -(KEMR_MAX_BERT_CTX - 1); d < KEMR_MAX_BERT_CTX; ++d)
            out[(size_t)h * REL_DISTANCES + d + KEMR_MAX_BERT_CTX - 1] = weight[(size_t)relative_position_bucket(d) * heads + h];
}

int fp8_bits(int precision) {
    return (precision == KEMR_PREC_FP8 || precision == KEMR_PREC_FP8_RES16) ? 1 : precision == KEMR_PREC_FP8_MLP ? 3 : 0;
}

int check_finalize(const kemr_model* m, int precision) {
    if (!m) KEMR_FAIL(KEMR_ERR_INVALID, "finalize: null model");
    if (precision < KEMR_PREC_BF16 || precision > KEMR_PREC_FP32X3)
        KEMR_FAIL(KEMR_ERR_INVALID, "finalize: unsupported precision %d", precision);
    const int fp8 = fp8_bits(precision);
    if (is_sentence_family(m->family)) {
        if (fp8) KEMR_FAIL(KEMR_ERR_INVALID, "finalize: the fp8 precisions are not served for family 2 (BERT): the e4m3 path is validated on the CLIP towers only");
        if (precision == KEMR_PREC_FP32X3) KEMR_FAIL(KEMR_ERR_INVALID, "finalize: KEMR_PREC_FP32X3 is not served for family 2 (BERT): the split-bf16 towers have no post-LN blocks");
    }
    if (fp8 && ((m->cfg.v_width % 128) || (m->cfg.t_width % 128) || m->cfg.v_width < 256 || m->cfg.t_width < 256))
        KEMR_FAIL(KEMR_ERR_INVALID, "finalize: fp8 needs tower widths that are multiples of 128 and >= 256");
    if (m->v_head_dim == 80) {
        if (m->cfg.v_width % 80) KEMR_FAIL(KEMR_ERR_INVALID, "finalize: vision_head_dim 80 needs a vision width that is a multiple of 80, got %d", m->cfg.v_width);
        if (fp8) KEMR_FAIL(KEMR_ERR_INVALID, "finalize: the fp8 precisions are not served at vision_head_dim 80 (the e4m3 QKV path is validated for heads of 64 only)");
        if (m->patches + 1 > 288)
            KEMR_FAIL(KEMR_ERR_INVALID, "finalize: vision_head_dim 80 serves towers of at most 288 tokens, this one has %d (the streaming attention kernel is head-dim-64 only)", m->patches + 1);
    }
    if (m->family == 1) {
        if (m->cfg.embed_dim != m->cfg.v_width)
            KEMR_FAIL(KEMR_ERR_INVALID, "finalize: family 1 (SigLIP) has no vision projection: embed_dim %d must equal v_width %d", m->cfg.embed_dim, m->cfg.v_width);
        if (fp8) KEMR_FAIL(KEMR_ERR_INVALID, "finalize: the fp8 precisions are not served for family 1 (SigLIP): the e4m3 path is validated on the CLIP towers only");
        if (precision == KEMR_PREC_FP32X3) KEMR_FAIL(KEMR_ERR_INVALID, "finalize: KEMR_PREC_FP32X3 is not served for family 1 (SigLIP): the split-bf16 towers have no pooling head");
        if (m->v_head_dim != 64) KEMR_FAIL(KEMR_ERR_INVALID, "finalize: family 1 (SigLIP) serves vision_head_dim 64 only, got %d", m->v_head_dim);
    }
    for (const TensorSpec& s : m->specs)
        if (!s.t.loaded) KEMR_FAIL(KEMR_ERR_STATE, "finalize: missing key '%s' (strict load)", s.name.c_str());
    return KEMR_OK;
}

// The device arena of a model that passed check_finalize: fp32 tensors verbatim, matrices as bf16 (fp32x3: every matrix [N, K] as the
// W-side triple [N, 3K] = [hi | hi | lo], conv1 over 3 kpad; vectors stay fp32), entries in spec order on multiples of 256 bytes.
// fill == false plans only: sizes and placements.
void pack_weights(const kemr_model& m, int precision, bool fill, PackedWeights& out) {
    const int fp8 = fp8_bits(precision);
    const bool x3 = precision == KEMR_PREC_FP32X3;
    const size_t mat_bytes = x3 ? 6 : 2, n = m.specs.size();
    out = PackedWeights{};
    out.at.resize(n);
    auto take = [&](size_t b) { const size_t o = out.bytes; out.bytes += (size_t)round_up((int64_t)b, 256); return o; };
    for (size_t i = 0; i < n; ++i) {
        const TensorSpec& s = m.specs[i];
        size_t numel = 1, bytes;
        for (int64_t d : s.t.shape) numel *= (size_t)d;
        switch (s.kind) {
        case KIND_CONV_WEIGHT: bytes = (size_t)m.cfg.v_width * m.kpad * mat_bytes; break;
        case KIND_MATRIX: case KIND_QKV_WEIGHT: case KIND_FC1_WEIGHT:
            if (is_e4m3(s, fp8)) { bytes = numel; out.at[i].aux = take((size_t)s.t.shape[0] * 4); }
            else bytes = numel * mat_bytes;
            break;
        case KIND_REL_BIAS: bytes = (size_t)s.t.shape[1] * REL_DISTANCES * 4; break;
        default: bytes = numel * 4;
        }
        out.at[i].off = take(bytes);
        if (s.kind == KIND_PROBE) out.at[i].aux = take(numel * 2);
    }
    if (!fill) return;

    // the attention scale 1 / sqrt(head dim), folded into the query rows of in_proj_weight / in_proj_bias in fp32 BEFORE the values are
    // rounded to bf16 (or split into hi and lo): exactly 0.125f for heads of 64 (a power of two: it commutes with every rounding), the
    // fp32 nearest to 1 / sqrt(80) for the vision tower at head dim 80
    const float v_qscale = m.v_head_dim == 80 ? (float)(1.0 / sqrt(80.0)) : 0.125f;
    auto qscale_of = [&](const TensorSpec& s) { return s.tower == TOWER_TEXT ? 0.125f : v_qscale; };
    // fp8 A operand (the LayerNorm output in front of an e4m3 GEMM): per-CHANNEL power-of-two scales s_c = 2^ceil(log2 max(|gamma_c|,
    // |beta_c|)) move the LayerNorm's gain out of the e4m3 values and into the weight columns -- gamma' = gamma / s, beta' = beta / s
    // (the LayerNorm then writes z * gamma' + beta' with |gamma'|, |beta'| <= 1: at most sqrt(W) <= 45 in magnitude, far from e4m3's
    // +-448, and gains of 0.01 no longer push the values into e4m3's subnormals), W'[:, c] = W[:, c] * s_c before the per-row
    // quantisation.  Exact in real arithmetic and in fp32 (powers of two); with gains near 1 (s = 1 or 2) the e4m3 values are the
    // same numbers shifted by one binade.  Round 3 stored z * gamma + beta with unit scale, saturating: a trained tower's gains of
    // 30-100 clipped there (round 4).
    std::vector<std::vector<float>> a_scale(2 * (size_t)m.vis.layers);      // [2 * layer + (fc1 ? 1 : 0)], empty where the GEMM is not fp8
    auto a_scale_of = [&](const TensorSpec& s) -> std::vector<float>* {
        if (s.tower != TOWER_VISION) return nullptr;
        const bool qkv = s.kind == KIND_LN_QKV || s.kind == KIND_QKV_WEIGHT, fc1 = s.kind == KIND_LN_FC1 || s.kind == KIND_FC1_WEIGHT;
        return ((qkv && (fp8 & 1)) || (fc1 && (fp8 & 2))) ? &a_scale[2 * (size_t)s.layer + (fc1 ? 1 : 0)] : nullptr;
    };
    for (const TensorSpec& s : m.specs)                    // max(|gamma_c|, |beta_c|) over the LayerNorm's two vectors ...
        if (s.kind == KIND_LN_QKV || s.kind == KIND_LN_FC1)
            if (std::vector<float>* a = a_scale_of(s)) {
                a->resize(s.t.data.size(), 0.f);
                for (size_t c = 0; c < a->size(); ++c) (*a)[c] = fmaxf((*a)[c], fabsf(s.t.data[c]));
            }
    for (std::vector<float>& sc : a_scale)                 // ... then the power of two at or above it
        for (float& a : sc) a = (a > 0.f && std::isfinite(a)) ? exp2f(fminf(12.f, fmaxf(-12.f, ceilf(log2f(a))))) : 1.0f;

    out.host.assign(out.bytes, 0);
    for (size_t i = 0; i < n; ++i) {
        const TensorSpec& s = m.specs[i];
        const HostTensor& t = s.t;
        char* dst = out.host.data() + out.at[i].off;
        const std::vector<float>* as = a_scale_of(s);
        switch (s.kind) {
        case KIND_CONV_WEIGHT: {
            const int kv = 3 * m.cfg.patch * m.cfg.patch;
            for (int r = 0; r < m.cfg.v_width; ++r)
                for (int k = 0; k < kv; ++k) {
                    if (x3) put_x3((bf16_t*)dst, r, m.kpad, k, t.data[(size_t)r * kv + k]);
                    else ((bf16_t*)dst)[(size_t)r * m.kpad + k] = f32_to_bf16_host(t.data[(size_t)r * kv + k]);
                }
            break;
        }
        case KIND_VPOS_SIGLIP:       // the patch embedding's bias rides in the positional table (x[m] = acc + pos[m % patches] + bias)
            add_row(t.data, host_data(m, "visual.conv1.bias"), (size_t)m.cfg.v_width, (float*)dst);
            break;
        case KIND_TPOS_BERT:         // every token is of type 0 (a single segment), so token_type_embedding[0] rides in the positional table
            add_row(t.data, host_data(m, "token_type_embedding"), (size_t)m.cfg.t_width, (float*)dst);
            break;
        case KIND_REL_BIAS:          // [32, heads] by bucket -> [heads, 1023] by distance: the attention kernel indexes key - query + 511
            expand_relative_bias(t.data.data(), (int)t.shape[1], (float*)dst);
            break;
        case KIND_PROBE: {
            // the pooling head's single query, the same for every image: (probe . Wq^T + bq) / 8 in fp32 (double accumulation), rounded to
            // bf16 once -- what the q rows of a block's QKV GEMM are, with the scale folded in before the rounding
            memcpy(dst, t.data.data(), t.data.size() * 4);
            const std::vector<float>&wq = host_data(m, "visual.attn_pool.in_proj_weight"), &bq = host_data(m, "visual.attn_pool.in_proj_bias");
            const size_t w = t.data.size();
            bf16_t* q = (bf16_t*)(out.host.data() + out.at[i].aux);
            for (size_t r = 0; r < w; ++r) {
                double acc = 0.0;
                for (size_t c = 0; c < w; ++c) acc += (double)t.data[c] * (double)wq[r * w + c];
                q[r] = f32_to_bf16_host(((float)acc + bq[r]) * 0.125f);
            }
            break;
        }
        case KIND_QKV_WEIGHT:
            fill_matrix(t, t.shape[1], qscale_of(s), x3, is_e4m3(s, fp8) ? as : nullptr, dst, (float*)(out.host.data() + out.at[i].aux));
            break;
        case KIND_FC1_WEIGHT:
            fill_matrix(t, 0, 1.0f, x3, is_e4m3(s, fp8) ? as : nullptr, dst, (float*)(out.host.data() + out.at[i].aux));
            break;
        case KIND_MATRIX:
            fill_matrix(t, 0, 1.0f, x3, nullptr, dst, nullptr);
            break;
        case KIND_QKV_BIAS: {
            const size_t w = t.data.size() / 3;
            const float qs = qscale_of(s);
            for (size_t c = 0; c < t.data.size(); ++c) ((float*)dst)[c] = c < w ? t.data[c] * qs : t.data[c];
            break;
        }
        case KIND_LN_QKV: case KIND_LN_FC1:
            if (as) { for (size_t c = 0; c < t.data.size(); ++c) ((float*)dst)[c] = t.data[c] / (*as)[c]; break; }
            [[fallthrough]];
        case KIND_F32:
            memcpy(dst, t.data.data(), t.data.size() * 4);
            break;
        }
    }
}

}  // namespace kemr

extern "C" int kemr_model_create(const kemr_cfg* cfg, kemr_model** out) { return model_create(cfg, 0, out); }
extern "C" int kemr_model_create_family(const kemr_cfg* cfg, int family, kemr_model** out) { return model_create(cfg, family, out); }

extern "C" int kemr_model_num_tensors(const kemr_model* m) { return m ? (int)m->specs.size() : 0; }
extern "C" const char* kemr_model_tensor_name(const kemr_model* m, int i) {
    if (!m || i < 0 || i >= (int)m->specs.size()) return nullptr;
    return m->specs[i].name.c_str();
}

extern "C" int kemr_model_load_tensor(kemr_model* m, const char* name, const void* host_ptr, int dtype,
                                      const int64_t* shape, int rank) {
    if (!m || !name || !host_ptr || (!shape && rank > 0)) KEMR_FAIL(KEMR_ERR_INVALID, "load_tensor: null argument");
    if (dtype != KEMR_F32) KEMR_FAIL(KEMR_ERR_INVALID, "load_tensor(%s): only fp32 host tensors are accepted", name);
    const std::string n(name);
    if (n == "logit_scale" || n == "input_resolution" || n == "context_length" || n == "vocab_size") return KEMR_OK;  // not on the encode path
    if (m->family == 1 && n == "logit_bias") return KEMR_OK;                    // SigLIP's second loss parameter: not on the encode path either
    auto it = m->index.find(n);
    if (it == m->index.end()) KEMR_FAIL(KEMR_ERR_INVALID, "load_tensor: unexpected key '%s' (strict load)", name);
    HostTensor& t = m->specs[it->second].t;
    bool same = (int)t.shape.size() == rank;
    int64_t numel = 1;
    for (int i = 0; same && i < rank; ++i) same = t.shape[i] == shape[i];
    if (!same) {
        std::string want, got;
        for (auto s : t.shape) want += std::to_string(s) + ",";
        for (int i = 0; i < rank; ++i) got += std::to_string(shape[i]) + ",";
        KEMR_FAIL(KEMR_ERR_INVALID, "load_tensor: size mismatch for %s: expected [%s] got [%s]", name, want.c_str(), got.c_str());
    }
    for (auto s : t.shape) numel *= s;
    t.data.assign((const float*)host_ptr, (const float*)host_ptr + numel);
    t.loaded = true;
    m->any_loaded = true;
    m->finalized = false;
    return KEMR_OK;
}

// refusals (all before any GPU call), pack on the host, upload, bind
extern "C" int kemr_model_finalize(kemr_model* m, int precision) {
    KEMR_TRY(check_finalize(m, precision));
    PackedWeights packed;
    pack_weights(*m, precision, true, packed);
    if (m->arena && m->arena_bytes != packed.bytes) { (void)hipFree(m->arena); m->arena = nullptr; }
    if (!m->arena) {
        KEMR_CHECK_HIP(hipMalloc((void**)&m->arena, packed.bytes));
        m->arena_bytes = packed.bytes;
    }
    KEMR_CHECK_HIP(hipDeviceSynchronize());   // nothing may still read the old weights
    KEMR_CHECK_HIP(hipMemcpy(m->arena, packed.host.data(), packed.bytes, hipMemcpyHostToDevice));
    bind_weights(m, fp8_bits(precision), packed.at);
    m->vis.head_dim = m->v_head_dim;
    for (TensorSpec& s : m->specs) { std::vector<float>().swap(s.t.data); s.t.loaded = false; }
    const bool x3 = precision == KEMR_PREC_FP32X3;
    m->res_dtype = (precision == KEMR_PREC_BF16_RES16 || precision == KEMR_PREC_FP8_RES16) ? KEMR_BF16 : KEMR_F32;
    if (m->stream24 && m->res_dtype == KEMR_F32 && !x3) m->res_dtype = KEMR_F24;      // option "residual_stream_24bit" (common.h f24_t)
    m->fp8 = fp8_bits(precision);
    m->x3 = x3 ? 1 : 0;
    m->finalized = true;
    return KEMR_OK;
}

// include/kemr_debug.h: the pack step of kemr_model_finalize alone, on the host (no GPU call; the loaded tensors stay loaded)
extern "C" int kemr_debug_pack_weights(const kemr_model* m, int precision, void* host_out, size_t capacity, size_t* bytes) {
    KEMR_TRY(check_finalize(m, precision));
    if (!bytes) KEMR_FAIL(KEMR_ERR_INVALID, "debug_pack_weights: null size output");
    PackedWeights packed;
    pack_weights(*m, precision, host_out != nullptr, packed);
    *bytes = packed.bytes;
    if (!host_out) return KEMR_OK;
    if (capacity < packed.bytes) KEMR_FAIL(KEMR_ERR_INVALID, "debug_pack_weights: capacity %zu < %zu bytes", capacity, packed.bytes);
    memcpy(host_out, packed.host.data(), packed.bytes);
    return KEMR_OK;
}

extern "C" int kemr_model_destroy(kemr_model* m) {
    if (!m) return KEMR_OK;
    if (m->arena) (void)hipFree(m->arena);
    delete m;
    return KEMR_OK;
}

// ------------------------------------------------------------------------------------------------ per-model options
extern "C" int kemr_model_set_option(kemr_model* m, const char* key, int value) {
    if (!m || !key) KEMR_FAIL(KEMR_ERR_INVALID, "model_set_option: null argument");
    if (!strcmp(key, "residual_fusion")) {
        if (value < 0 || value > 2) KEMR_FAIL(KEMR_ERR_INVALID, "model_set_option(residual_fusion): 0, 1 or 2, got %d", value);
        m->resadd = value;
        return KEMR_OK;
    }
    if (!strcmp(key, "residual_stream_24bit")) {
        if (value < 0 || value > 1) KEMR_FAIL(KEMR_ERR_INVALID, "model_set_option(residual_stream_24bit): 0 or 1, got %d", value);
        if (m->finalized) KEMR_FAIL(KEMR_ERR_STATE, "model_set_option(residual_stream_24bit): set it before kemr_model_finalize");
        m->stream24 = value;
        return KEMR_OK;
    }
    if (!strcmp(key, "family")) {
        if (is_sentence_family(m->family)) {
            // a sentence encoder created by kemr_model_create_family(cfg, 2): 2 (BERT) <-> 3 (MPNet) share the configuration checks and
            // differ in the tensor list, so the switch works like 0 <-> 1 does for a kemr_model_create model; nothing else is reachable
            if (value != 2 && value != 3) {
                if (m->family == 2) KEMR_FAIL(KEMR_ERR_INVALID, "model_set_option(family): a family 2 (BERT) model keeps its family (kemr_model_create_family)");
                KEMR_FAIL(KEMR_ERR_INVALID, "model_set_option(family): a family 3 (MPNet) model becomes 2 (BERT) or stays 3, got %d (families 0 and 1: kemr_model_create_family)", value);
            }
            if (m->any_loaded || m->finalized) KEMR_FAIL(KEMR_ERR_STATE, "model_set_option(family): set it before the first kemr_model_load_tensor (it decides the tensor names)");
            m->family = value;
            build_names(m);
            return KEMR_OK;
        }
        if (value == 2) KEMR_FAIL(KEMR_ERR_INVALID, "model_set_option(family): 0 (CLIP) or 1 (SigLIP), got 2 (family 2, BERT, has its own configuration checks and is decided at creation: kemr_model_create_family)");
        if (value == 3) KEMR_FAIL(KEMR_ERR_INVALID, "model_set_option(family): 0 (CLIP) or 1 (SigLIP), got 3 (family 3, MPNet, is a family-2 model -- kemr_model_create_family(cfg, 2) -- switched by this option)");
        if (value < 0 || value > 1) KEMR_FAIL(KEMR_ERR_INVALID, "model_set_option(family): 0 (CLIP) or 1 (SigLIP), got %d", value);
        if (m->any_loaded || m->finalized) KEMR_FAIL(KEMR_ERR_STATE, "model_set_option(family): set it before the first kemr_model_load_tensor (it decides the tensor names)");
        if (value == 1 && m->v_head_dim != 64) KEMR_FAIL(KEMR_ERR_INVALID, "model_set_option(family): family 1 (SigLIP) serves vision_head_dim 64 only, got %d", m->v_head_dim);
        m->family = value;
        build_names(m);
        return KEMR_OK;
    }
    if (!strcmp(key, "pooling")) {
        if (!is_sentence_family(m->family)) KEMR_FAIL(KEMR_ERR_INVALID, "model_set_option(pooling): the option exists for family 2 (BERT) only");
        if (value < 0 || value > 1) KEMR_FAIL(KEMR_ERR_INVALID, "model_set_option(pooling): 0 (mean) or 1 (first row, CLS), got %d", value);
        m->pooling = value;
        return KEMR_OK;
    }
    if (!strcmp(key, "vision_head_dim")) {
        if (is_sentence_family(m->family)) KEMR_FAIL(KEMR_ERR_INVALID, "model_set_option(vision_head_dim): family 2 (BERT) has no vision tower");
        if (m->family == 1 && value != 64) KEMR_FAIL(KEMR_ERR_INVALID, "model_set_option(vision_head_dim): family 1 (SigLIP) serves vision_head_dim 64 only, got %d", value);
        if (value != 64 && value != 80) KEMR_FAIL(KEMR_ERR_INVALID, "model_set_option(vision_head_dim): 64 or 80, got %d", value);
        if (m->finalized) KEMR_FAIL(KEMR_ERR_STATE, "model_set_option(vision_head_dim): set it before kemr_model_finalize");
        if (m->cfg.v_width % value) KEMR_FAIL(KEMR_ERR_INVALID, "model_set_option(vision_head_dim): the vision width %d is not a multiple of %d", m->cfg.v_width, value);
        m->v_head_dim = value;
        return KEMR_OK;
    }
    if (!strcmp(key, "layer_norm_eps")) {
        if (m->family != 3) KEMR_FAIL(KEMR_ERR_INVALID, "model_set_option(layer_norm_eps): the option exists for family 3 (MPNet) only");
        if (value != 5 && value != 12) KEMR_FAIL(KEMR_ERR_INVALID, "model_set_option(layer_norm_eps): 5 (1e-5) or 12 (1e-12), got %d", value);
        if (m->finalized) KEMR_FAIL(KEMR_ERR_STATE, "model_set_option(layer_norm_eps): set it before kemr_model_finalize");
        m->ln_eps_exp = value;
        m->eps = value == 12 ? 1e-12f : 1e-5f;
        return KEMR_OK;
    }
    if (!strcmp(key, "last_block_pooled_row")) {
        if (value < 0 || value > 1) KEMR_FAIL(KEMR_ERR_INVALID, "model_set_option(last_block_pooled_row): 0 or 1, got %d", value);
        m->last_pooled = value;
        return KEMR_OK;
    }
    if (!strcmp(key, "activation")) {
        if (value < 0 || value > 1) KEMR_FAIL(KEMR_ERR_INVALID, "model_set_option(activation): 0 (QuickGELU) or 1 (GELU), got %d", value);
        m->activation = value;
        return KEMR_OK;
    }
    KEMR_FAIL(KEMR_ERR_INVALID, "model_set_option: unknown key '%s'", key);
}

extern "C" int kemr_model_get_option(const kemr_model* m, const char* key, int* value) {
    if (!m || !key || !value) KEMR_FAIL(KEMR_ERR_INVALID, "model_get_option: null argument");
    if (!strcmp(key, "residual_fusion")) { *value = m->resadd; return KEMR_OK; }
    if (!strcmp(key, "last_block_pooled_row")) { *value = m->last_pooled; return KEMR_OK; }
    if (!strcmp(key, "residual_stream_24bit")) { *value = (m->finalized && !m->x3) ? (m->res_dtype == KEMR_F24) : m->stream24; return KEMR_OK; }
    if (!strcmp(key, "activation")) { *value = m->activation; return KEMR_OK; }
    if (!strcmp(key, "vision_head_dim")) { *value = m->v_head_dim; return KEMR_OK; }
    if (!strcmp(key, "family")) { *value = m->family; return KEMR_OK; }
    if (!strcmp(key, "pooling")) { *value = m->pooling; return KEMR_OK; }
    if (!strcmp(key, "layer_norm_eps")) {
        if (m->family != 3) KEMR_FAIL(KEMR_ERR_INVALID, "model_get_option(layer_norm_eps): the option exists for family 3 (MPNet) only");
        *value = m->ln_eps_exp;
        return KEMR_OK;
    }
    if (!strcmp(key, "precision_residual_bf16")) { *value = m->res_dtype == KEMR_BF16; return KEMR_OK; }
    KEMR_FAIL(KEMR_ERR_INVALID, "model_get_option: unknown key '%s'", key);
}
