// libkemr.so: model handle, weight packing and the encoder launch sequences behind the C ABI (include/kemr.h).
// Host-side C++ only; every kernel lives in gemm.hip / layernorm.hip / attention.hip / embed.hip / sim.hip.
#include "common.h"
#include "../../include/kemr_debug.h"

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
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

struct HostTensor {
    std::vector<int64_t> shape;
    std::vector<float> data;
    bool loaded = false;
};

struct LayerW {
    const float *ln1_g, *ln1_b, *ln2_g, *ln2_b, *bqkv, *bo, *b1, *b2;
    const bf16_t *wqkv, *wo, *w1, *w2;
    // KEMR_PREC_FP8: e4m3 copies of wqkv / w1 (instead of the bf16 ones) and their per-output-channel scales
    const uint8_t *wqkv8 = nullptr, *w18 = nullptr;
    const float *sqkv = nullptr, *s1 = nullptr;
};

struct TowerW {
    int width = 0, layers = 0, tokens = 0;
    int head_dim = 64;                              // 64, or 80 for the vision tower under option "vision_head_dim" (attention80.hip)
    std::vector<LayerW> layer;
};

}  // namespace kemr

using namespace kemr;

struct kemr_model {
    kemr_cfg cfg;
    std::vector<std::string> names;                 // required tensors, fixed order
    std::map<std::string, HostTensor> tensors;
    bool finalized = false;
    char* arena = nullptr;                          // device weights
    size_t arena_bytes = 0;
    int grid = 0, patches = 0, kpad = 0;
    int res_dtype = KEMR_F32;                       // storage type of the residual stream (KEMR_PREC_BF16_RES16: bf16)
    int fp8 = 0;                                    // bit 0: QKV on fp8 operands (KEMR_PREC_FP8), bit 1: fc1 too (KEMR_PREC_FP8_MLP)
    int resadd = 1;                                 // option "residual_fusion": residual add inside the out-proj / fc2 epilogues
    int last_pooled = 1;                            // option "last_block_pooled_row": the last block's query path on the pooled row only
    int activation = 0;                             // option "activation": 0 = QuickGELU, 1 = exact GELU (the fc1 epilogue of run_blocks)
    int x3 = 0;                                     // KEMR_PREC_FP32X3: split-bf16 operand triples, fp32 between the kernels (run_blocks_x3)
    int v_head_dim = 64;                            // option "vision_head_dim" (before finalize): 64, or 80 (ViT-H-14: 1280 = 16 heads of 80)
    int stream24 = 1;                               // option "residual_stream_24bit" (before finalize; default on since round 4): the fp32-class stream stored in 3 bytes
    int family = 0;                                 // option "family" (before the first load_tensor): 0 = CLIP, 1 = SigLIP (no class token / ln_pre, tanh GELU, eps 1e-6, pooling head, unmasked text);
                                                    // 2 = BERT sentence encoder (kemr_model_create_family only: text-only, post-LN blocks, eps 1e-12, mean / CLS pooling)
    int pooling = 0;                                // option "pooling" (family 2): 0 = mean of the item's rows, 1 = its first row (CLS)
    bool any_loaded = false;                        // a tensor was loaded: the name list is fixed from then on
    float eps = 1e-5f;                              // every LayerNorm's epsilon: 1e-6 for family 1
    int vtokens = 0;                                // token rows per image: patches + 1 (class token), patches for family 1
    // vision
    TowerW vis;
    const bf16_t* conv_w = nullptr;
    const float *cls = nullptr, *vpos = nullptr, *lnpre_g = nullptr, *lnpre_b = nullptr, *lnpost_g = nullptr,
                *lnpost_b = nullptr, *vproj = nullptr;
    // text
    TowerW txt;
    const float *tok = nullptr, *tpos = nullptr, *lnf_g = nullptr, *lnf_b = nullptr, *tproj = nullptr;
    // family 1: the text head's bias; the vision tower's pooling head (visual.attn_pool.*): its one query row (probe . Wq^T + bq) / 8
    // made at finalize, the k | v rows of in_proj (wkv = in_proj_weight + W * W), out_proj, LayerNorm and MLP
    const float* tproj_b = nullptr;
    const bf16_t *mh_q = nullptr, *mh_wkv = nullptr, *mh_wo = nullptr, *mh_w1 = nullptr, *mh_w2 = nullptr;
    const float *lne_g = nullptr, *lne_b = nullptr;  // family 2: the embedding LayerNorm (ln_embed.*)
    const float *mh_bkv = nullptr, *mh_bo = nullptr, *mh_ln_g = nullptr, *mh_ln_b = nullptr, *mh_b1 = nullptr, *mh_b2 = nullptr;
};

namespace {

void add_block_names(std::vector<std::string>& v, std::map<std::string, HostTensor>& t, const std::string& prefix,
                     int width, int layers) {
    auto add = [&](const std::string& n, std::vector<int64_t> shape) { v.push_back(n); t[n].shape = std::move(shape); };
    for (int i = 0; i < layers; ++i) {
        const std::string b = prefix + ".resblocks." + std::to_string(i);
        add(b + ".ln_1.weight", {width});
        add(b + ".ln_1.bias", {width});
        add(b + ".attn.in_proj_weight", {3 * width, width});
        add(b + ".attn.in_proj_bias", {3 * width});
        add(b + ".attn.out_proj.weight", {width, width});
        add(b + ".attn.out_proj.bias", {width});
        add(b + ".ln_2.weight", {width});
        add(b + ".ln_2.bias", {width});
        add(b + ".mlp.c_fc.weight", {4 * width, width});
        add(b + ".mlp.c_fc.bias", {4 * width});
        add(b + ".mlp.c_proj.weight", {width, 4 * width});
        add(b + ".mlp.c_proj.bias", {width});
    }
}

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

// the required tensors of a model family, in load order (kemr_model_create; option "family" rebuilds the list)
void build_names(kemr_model* m) {
    const kemr_cfg* cfg = &m->cfg;
    m->names.clear();
    m->tensors.clear();
    auto add = [&](const std::string& n, std::vector<int64_t> shape) { m->names.push_back(n); m->tensors[n].shape = std::move(shape); };
    const int vw = cfg->v_width, tw = cfg->t_width, D = cfg->embed_dim;
    if (m->family == 2) {
        // BertModel without its pooler, by OpenAI-style names: ln_1 = attention.output.LayerNorm, ln_2 = output.LayerNorm (post-LN)
        m->vtokens = 0;
        m->eps = 1e-12f;
        add("token_embedding.weight", {cfg->vocab, tw});
        add("positional_embedding", {cfg->ctx, tw});
        add("token_type_embedding", {2, tw});
        add("ln_embed.weight", {tw});
        add("ln_embed.bias", {tw});
        add_block_names(m->names, m->tensors, "transformer", tw, cfg->t_layers);
        return;
    }
    const bool sig = m->family == 1;
    m->vtokens = sig ? m->patches : m->patches + 1;
    m->eps = sig ? 1e-6f : 1e-5f;
    add("visual.conv1.weight", {vw, 3, cfg->patch, cfg->patch});
    if (sig) add("visual.conv1.bias", {vw});
    else add("visual.class_embedding", {vw});
    add("visual.positional_embedding", {m->vtokens, vw});
    if (!sig) {
        add("visual.ln_pre.weight", {vw});
        add("visual.ln_pre.bias", {vw});
    }
    add_block_names(m->names, m->tensors, "visual.transformer", vw, cfg->v_layers);
    add("visual.ln_post.weight", {vw});
    add("visual.ln_post.bias", {vw});
    if (sig) {
        const std::string h = "visual.attn_pool";
        add(h + ".probe", {vw});
        add(h + ".in_proj_weight", {3 * vw, vw});
        add(h + ".in_proj_bias", {3 * vw});
        add(h + ".out_proj.weight", {vw, vw});
        add(h + ".out_proj.bias", {vw});
        add(h + ".ln.weight", {vw});
        add(h + ".ln.bias", {vw});
        add(h + ".mlp.c_fc.weight", {4 * vw, vw});
        add(h + ".mlp.c_fc.bias", {4 * vw});
        add(h + ".mlp.c_proj.weight", {vw, 4 * vw});
        add(h + ".mlp.c_proj.bias", {vw});
    } else {
        add("visual.proj", {vw, D});
    }
    add("token_embedding.weight", {cfg->vocab, tw});
    add("positional_embedding", {cfg->ctx, tw});
    add_block_names(m->names, m->tensors, "transformer", tw, cfg->t_layers);
    add("ln_final.weight", {tw});
    add("ln_final.bias", {tw});
    add("text_projection", {tw, D});
    if (sig) add("text_projection_bias", {D});
}

struct ArenaPlan {
    size_t bytes = 0;
    size_t take(size_t n) { size_t o = bytes; bytes += (size_t)round_up((int64_t)n, 256); return o; }
};

}  // namespace

extern "C" const char* kemr_last_error(void) { return g_err; }
extern "C" int kemr_abi_version(void) { return KEMR_ABI_VERSION; }

static int model_create(const kemr_cfg* cfg, int family, kemr_model** out) {
    if (!cfg || !out) KEMR_FAIL(KEMR_ERR_INVALID, "model_create: null argument");
    if (family < 0 || family > 2) KEMR_FAIL(KEMR_ERR_INVALID, "model_create_family: family 0 (CLIP), 1 (SigLIP) or 2 (BERT), got %d", family);
    KEMR_TRY(family == 2 ? check_cfg_bert(*cfg) : check_cfg(*cfg));
    kemr_model* m = new (std::nothrow) kemr_model();
    if (!m) KEMR_FAIL(KEMR_ERR_NOMEM, "model_create: out of memory");
    m->cfg = *cfg;
    m->family = family;
    { const char* v = getenv("KEMR_RESADD"); const int e = (v && *v) ? atoi(v) : 1; m->resadd = e < 0 ? 0 : e > 2 ? 2 : e; }
    { const char* v = getenv("KEMR_LAST_BLOCK_FULL"); m->last_pooled = (v && *v && atoi(v) != 0) ? 0 : 1; }
    { const char* v = getenv("KEMR_STREAM24"); m->stream24 = (v && *v) ? (atoi(v) != 0 ? 1 : 0) : 1; }
    if (family != 2) {
        m->grid = cfg->image_size / cfg->patch;
        m->patches = m->grid * m->grid;
        m->kpad = (int)round_up(3 * cfg->patch * cfg->patch, 64);
    }
    build_names(m);
    *out = m;
    return KEMR_OK;
}

extern "C" int kemr_model_create(const kemr_cfg* cfg, kemr_model** out) { return model_create(cfg, 0, out); }
extern "C" int kemr_model_create_family(const kemr_cfg* cfg, int family, kemr_model** out) { return model_create(cfg, family, out); }

extern "C" int kemr_model_num_tensors(const kemr_model* m) { return m ? (int)m->names.size() : 0; }
extern "C" const char* kemr_model_tensor_name(const kemr_model* m, int i) {
    if (!m || i < 0 || i >= (int)m->names.size()) return nullptr;
    return m->names[i].c_str();
}

extern "C" int kemr_model_load_tensor(kemr_model* m, const char* name, const void* host_ptr, int dtype,
                                      const int64_t* shape, int rank) {
    if (!m || !name || !host_ptr || (!shape && rank > 0)) KEMR_FAIL(KEMR_ERR_INVALID, "load_tensor: null argument");
    if (dtype != KEMR_F32) KEMR_FAIL(KEMR_ERR_INVALID, "load_tensor(%s): only fp32 host tensors are accepted", name);
    const std::string n(name);
    if (n == "logit_scale" || n == "input_resolution" || n == "context_length" || n == "vocab_size") return KEMR_OK;  // not on the encode path
    if (m->family == 1 && n == "logit_bias") return KEMR_OK;                    // SigLIP's second loss parameter: not on the encode path either
    auto it = m->tensors.find(n);
    if (it == m->tensors.end()) KEMR_FAIL(KEMR_ERR_INVALID, "load_tensor: unexpected key '%s' (strict load)", name);
    HostTensor& t = it->second;
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

extern "C" int kemr_model_finalize(kemr_model* m, int precision) {
    if (!m) KEMR_FAIL(KEMR_ERR_INVALID, "finalize: null model");
    if (precision < KEMR_PREC_BF16 || precision > KEMR_PREC_FP32X3)
        KEMR_FAIL(KEMR_ERR_INVALID, "finalize: unsupported precision %d", precision);
    const int fp8 = (precision == KEMR_PREC_FP8 || precision == KEMR_PREC_FP8_RES16) ? 1 : precision == KEMR_PREC_FP8_MLP ? 3 : 0;
    if (m->family == 2) {
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
    for (const auto& n : m->names)
        if (!m->tensors[n].loaded) KEMR_FAIL(KEMR_ERR_STATE, "finalize: missing key '%s' (strict load)", n.c_str());
    // the attention scale 1 / sqrt(head dim), folded into the query rows of in_proj_weight / in_proj_bias in fp32 BEFORE the values are
    // rounded to bf16 (or split into hi and lo): exactly 0.125f for heads of 64 (a power of two: it commutes with every rounding), the
    // fp32 nearest to 1 / sqrt(80) for the vision tower at head dim 80
    const float v_qscale = m->v_head_dim == 80 ? (float)(1.0 / sqrt(80.0)) : 0.125f;
    auto qscale_of = [&](const std::string& n) { return n.rfind("visual.", 0) == 0 ? v_qscale : 0.125f; };
    // KEMR_PREC_FP32X3: every matrix [N, K] is packed as the W-side triple [N, 3K] = [hi | hi | lo] (conv1 over 3 kpad); vectors stay fp32
    const bool x3 = precision == KEMR_PREC_FP32X3;
    const size_t mat_bytes = x3 ? 6 : 2;
    auto put_x3 = [](bf16_t* d, size_t row, size_t K, size_t k, float v) {
        const bf16_t hi = f32_to_bf16_host(v);
        uint32_t u = (uint32_t)hi << 16;
        float hf; memcpy(&hf, &u, 4);
        d[row * 3 * K + k] = hi;
        d[row * 3 * K + K + k] = hi;
        d[row * 3 * K + 2 * K + k] = f32_to_bf16_host(v - hf);
    };

    // plan the device arena: f32 tensors verbatim, matrices as bf16
    // (family 1: visual.attn_pool.in_proj_weight / in_proj_bias take the generic in_proj_* branches below like a block's, so the q rows
    // of their device copies carry the 1/8 too.  Nothing reads those q rows: the head's one query is made from the host fp32 tensors
    // -- the "visual.attn_pool.probe" branch -- and mh_wkv / mh_bkv start behind them.)
    ArenaPlan plan;
    std::map<std::string, size_t> off;
    auto is_matrix = [](const std::string& n) {
        return n.find("in_proj_weight") != std::string::npos || n.find("out_proj.weight") != std::string::npos ||
               n.find("c_fc.weight") != std::string::npos || n.find("c_proj.weight") != std::string::npos ||
               n == "visual.conv1.weight";
    };
    // fp8 operands in the VISION tower only (round 4): the text tower is 9 % of a gallery item's GEMM work and its embedding is ONE
    // row behind a causal softmax -- e4m3 q / k / v cost it 1 - cos 1.4e-3 against the fp32 oracle (2.9e-3 .. 5e-3 on heavy-tailed
    // weights), over north_star's 1e-3, for a 1 % gain in items/s; the image embedding averages 257 rows and stays at 2e-5 .. 1e-4.
    auto is_fp8_matrix = [&](const std::string& n) {
        if (n.rfind("visual.", 0) != 0) return false;
        return ((fp8 & 1) && n.find("in_proj_weight") != std::string::npos) || ((fp8 & 2) && n.find("c_fc.weight") != std::string::npos);
    };
    for (const auto& n : m->names) {
        const HostTensor& t = m->tensors[n];
        size_t bytes;
        if (n == "visual.conv1.weight") bytes = (size_t)m->cfg.v_width * m->kpad * mat_bytes;
        else if (is_fp8_matrix(n)) { bytes = t.data.size(); off[n + "#scale"] = plan.take((size_t)t.shape[0] * 4); }
        else if (is_matrix(n)) bytes = t.data.size() * mat_bytes;
        else bytes = t.data.size() * 4;
        off[n] = plan.take(bytes);
        if (n == "visual.attn_pool.probe") off[n + "#q"] = plan.take(t.data.size() * 2);
    }
    // fp8 A operand (the LayerNorm output in front of an e4m3 GEMM): per-CHANNEL power-of-two scales s_c = 2^ceil(log2 max(|gamma_c|,
    // |beta_c|)) move the LayerNorm's gain out of the e4m3 values and into the weight columns -- gamma' = gamma / s, beta' = beta / s
    // (the LayerNorm then writes z * gamma' + beta' with |gamma'|, |beta'| <= 1: at most sqrt(W) <= 45 in magnitude, far from e4m3's
    // +-448, and gains of 0.01 no longer push the values into e4m3's subnormals), W'[:, c] = W[:, c] * s_c before the per-row
    // quantisation.  Exact in real arithmetic and in fp32 (powers of two); with gains near 1 (s = 1 or 2) the e4m3 values are the
    // same numbers shifted by one binade.  Round 3 stored z * gamma + beta with unit scale, saturating: a trained tower's gains of
    // 30-100 clipped there (round 4).
    auto ends_with = [](const std::string& a, const char* suf) { const size_t k = strlen(suf); return a.size() >= k && !a.compare(a.size() - k, k, suf); };
    auto ln_of = [&](const std::string& n) -> std::string {          // the LayerNorm whose output is matrix n's A operand
        const size_t p = n.find(".attn.in_proj_weight");
        if (p != std::string::npos) return n.substr(0, p) + ".ln_1";
        const size_t q = n.find(".mlp.c_fc.weight");
        return q != std::string::npos ? n.substr(0, q) + ".ln_2" : std::string();
    };
    std::map<std::string, std::vector<float>> a_scale;                // LayerNorm name -> s_c
    if (fp8)
        for (const auto& n : m->names)
            if (is_fp8_matrix(n)) {
                const std::string ln = ln_of(n);
                const std::vector<float>&g = m->tensors[ln + ".weight"].data, &bb = m->tensors[ln + ".bias"].data;
                std::vector<float> sc(g.size(), 1.0f);
                for (size_t c = 0; c < g.size(); ++c) {
                    const float a = fmaxf(fabsf(g[c]), fabsf(bb[c]));
                    if (a > 0.f && std::isfinite(a)) sc[c] = exp2f(fminf(12.f, fmaxf(-12.f, ceilf(log2f(a)))));
                }
                a_scale[ln] = sc;
            }
    std::vector<char> host(plan.bytes, 0);
    for (const auto& n : m->names) {
        const HostTensor& t = m->tensors[n];
        char* dst = host.data() + off[n];
        if (n == "visual.conv1.weight") {
            const int kv = 3 * m->cfg.patch * m->cfg.patch;
            bf16_t* d = (bf16_t*)dst;
            for (int r = 0; r < m->cfg.v_width; ++r)
                for (int k = 0; k < kv; ++k) {
                    if (x3) put_x3(d, r, m->kpad, k, t.data[(size_t)r * kv + k]);
                    else d[(size_t)r * m->kpad + k] = f32_to_bf16_host(t.data[(size_t)r * kv + k]);
                }
        } else if (m->family == 1 && n == "visual.positional_embedding") {
            // family 1: the patch embedding's bias rides in the positional table (x[m] = acc + pos[m % patches] + bias: one add per element)
            const std::vector<float>& cb = m->tensors["visual.conv1.bias"].data;
            float* d = (float*)dst;
            const size_t w = cb.size();
            for (size_t i = 0; i < t.data.size(); ++i) d[i] = t.data[i] + cb[i % w];
        } else if (m->family == 2 && n == "positional_embedding") {
            // family 2: every token is of type 0 (a single segment), so token_type_embedding[0] rides in the positional table, added in fp32
            const std::vector<float>& tt = m->tensors["token_type_embedding"].data;
            float* d = (float*)dst;
            const size_t w = (size_t)m->cfg.t_width;
            for (size_t i = 0; i < t.data.size(); ++i) d[i] = t.data[i] + tt[i % w];
        } else if (n == "visual.attn_pool.probe") {
            // the pooling head's single query, the same for every image: (probe . Wq^T + bq) / 8 in fp32 (double accumulation), rounded to
            // bf16 once -- what the q rows of a block's QKV GEMM are, with the scale folded in before the rounding
            memcpy(dst, t.data.data(), t.data.size() * 4);
            const std::vector<float>&wq = m->tensors["visual.attn_pool.in_proj_weight"].data, &bq = m->tensors["visual.attn_pool.in_proj_bias"].data;
            const size_t w = t.data.size();
            bf16_t* q = (bf16_t*)(host.data() + off[n + "#q"]);
            for (size_t r = 0; r < w; ++r) {
                double acc = 0.0;
                for (size_t c = 0; c < w; ++c) acc += (double)t.data[c] * (double)wq[r * w + c];
                q[r] = f32_to_bf16_host(((float)acc + bq[r]) * 0.125f);
            }
        } else if (x3 && is_matrix(n)) {
            // the attention scale in the query rows: 1/8 is a power of two and commutes with the split; 1 / sqrt(80) is applied in fp32 first
            const int64_t rows = t.shape[0], cols = t.shape[1];
            const bool qkv = n.find("in_proj_weight") != std::string::npos;
            const float qs = qscale_of(n);
            for (int64_t r = 0; r < rows; ++r)
                for (int64_t c = 0; c < cols; ++c)
                    put_x3((bf16_t*)dst, r, cols, c, (qkv && r < cols) ? t.data[r * cols + c] * qs : t.data[r * cols + c]);
        } else if (is_fp8_matrix(n)) {
            // e4m3 with one scale per output channel (row): scale = amax / 448; the attention scale 1/8 goes into the q rows
            const int64_t rows = t.shape[0], cols = t.shape[1];
            const bool qkv = n.find("in_proj_weight") != std::string::npos;
            const std::vector<float>& as = a_scale.at(ln_of(n));    // the A operand's per-channel scales, folded into the columns
            uint8_t* d = (uint8_t*)dst;
            float* sc = (float*)(host.data() + off[n + "#scale"]);
            for (int64_t r = 0; r < rows; ++r) {
                const float pre = (qkv && r < cols) ? 0.125f : 1.0f;
                float amax = 0.f;
                for (int64_t c = 0; c < cols; ++c) amax = fmaxf(amax, fabsf(t.data[r * cols + c] * pre * as[c]));
                const float scale = amax > 0.f ? amax / 448.f : 1.0f;
                sc[r] = scale;
                for (int64_t c = 0; c < cols; ++c) d[r * cols + c] = f32_to_e4m3_host(t.data[r * cols + c] * pre * as[c] / scale);
            }
        } else if (n.find("in_proj_weight") != std::string::npos) {
            // fold the attention scale 1/sqrt(64) = 0.125 (exact in bf16; 1/sqrt(80) at vision_head_dim 80) into the query rows
            const int64_t w = t.shape[1];
            const float qs = qscale_of(n);
            bf16_t* d = (bf16_t*)dst;
            for (int64_t i = 0; i < (int64_t)t.data.size(); ++i)
                d[i] = f32_to_bf16_host(i < w * w ? t.data[i] * qs : t.data[i]);
        } else if (n.find("in_proj_bias") != std::string::npos) {
            const int64_t w = t.shape[0] / 3;
            const float qs = qscale_of(n);
            float* d = (float*)dst;
            for (int64_t i = 0; i < (int64_t)t.data.size(); ++i) d[i] = i < w ? t.data[i] * qs : t.data[i];
        } else if (is_matrix(n)) {
            bf16_t* d = (bf16_t*)dst;
            for (size_t i = 0; i < t.data.size(); ++i) d[i] = f32_to_bf16_host(t.data[i]);
        } else if (fp8 && (ends_with(n, ".ln_1.weight") || ends_with(n, ".ln_1.bias") || ends_with(n, ".ln_2.weight") || ends_with(n, ".ln_2.bias")) &&
                   a_scale.count(n.substr(0, n.rfind('.')))) {
            const std::vector<float>& as = a_scale.at(n.substr(0, n.rfind('.')));
            float* d = (float*)dst;
            for (size_t c = 0; c < t.data.size(); ++c) d[c] = t.data[c] / as[c];
        } else {
            memcpy(dst, t.data.data(), t.data.size() * 4);
        }
    }
    if (m->arena && m->arena_bytes != plan.bytes) { (void)hipFree(m->arena); m->arena = nullptr; }
    if (!m->arena) {
        KEMR_CHECK_HIP(hipMalloc((void**)&m->arena, plan.bytes));
        m->arena_bytes = plan.bytes;
    }
    KEMR_CHECK_HIP(hipDeviceSynchronize());   // nothing may still read the old weights
    KEMR_CHECK_HIP(hipMemcpy(m->arena, host.data(), plan.bytes, hipMemcpyHostToDevice));

    auto F = [&](const std::string& n) { return (const float*)(m->arena + off.at(n)); };
    auto H = [&](const std::string& n) { return (const bf16_t*)(m->arena + off.at(n)); };
    auto tower = [&](TowerW& tw, const std::string& prefix, int width, int layers, int tokens, int fp8) {
        tw.width = width; tw.layers = layers; tw.tokens = tokens;
        tw.layer.resize(layers);
        for (int i = 0; i < layers; ++i) {
            const std::string b = prefix + ".resblocks." + std::to_string(i);
            LayerW& L = tw.layer[i];
            L.ln1_g = F(b + ".ln_1.weight"); L.ln1_b = F(b + ".ln_1.bias");
            L.wqkv = H(b + ".attn.in_proj_weight"); L.bqkv = F(b + ".attn.in_proj_bias");
            if (fp8 & 1) { L.wqkv8 = (const uint8_t*)L.wqkv; L.wqkv = nullptr; L.sqkv = F(b + ".attn.in_proj_weight#scale"); }
            if (fp8 & 2) { L.w18 = (const uint8_t*)H(b + ".mlp.c_fc.weight"); L.s1 = F(b + ".mlp.c_fc.weight#scale"); }
            L.wo = H(b + ".attn.out_proj.weight"); L.bo = F(b + ".attn.out_proj.bias");
            L.ln2_g = F(b + ".ln_2.weight"); L.ln2_b = F(b + ".ln_2.bias");
            L.w1 = (fp8 & 2) ? nullptr : H(b + ".mlp.c_fc.weight"); L.b1 = F(b + ".mlp.c_fc.bias");
            L.w2 = H(b + ".mlp.c_proj.weight"); L.b2 = F(b + ".mlp.c_proj.bias");
        }
    };
    tower(m->txt, "transformer", m->cfg.t_width, m->cfg.t_layers, m->cfg.ctx, 0);
    if (m->family != 2) {
        tower(m->vis, "visual.transformer", m->cfg.v_width, m->cfg.v_layers, m->vtokens, fp8);
        m->vis.head_dim = m->v_head_dim;
        m->conv_w = H("visual.conv1.weight");
        m->vpos = F("visual.positional_embedding");
        m->lnpost_g = F("visual.ln_post.weight"); m->lnpost_b = F("visual.ln_post.bias");
    }
    if (m->family == 2) {
        m->lne_g = F("ln_embed.weight"); m->lne_b = F("ln_embed.bias");
    } else if (m->family == 1) {
        const std::string h = "visual.attn_pool";
        const size_t vw = (size_t)m->cfg.v_width;
        m->cls = m->lnpre_g = m->lnpre_b = m->vproj = nullptr;
        m->mh_q = H(h + ".probe#q");
        m->mh_wkv = H(h + ".in_proj_weight") + vw * vw; m->mh_bkv = F(h + ".in_proj_bias") + vw;
        m->mh_wo = H(h + ".out_proj.weight"); m->mh_bo = F(h + ".out_proj.bias");
        m->mh_ln_g = F(h + ".ln.weight"); m->mh_ln_b = F(h + ".ln.bias");
        m->mh_w1 = H(h + ".mlp.c_fc.weight"); m->mh_b1 = F(h + ".mlp.c_fc.bias");
        m->mh_w2 = H(h + ".mlp.c_proj.weight"); m->mh_b2 = F(h + ".mlp.c_proj.bias");
        m->tproj_b = F("text_projection_bias");
    } else {
        m->cls = F("visual.class_embedding");
        m->lnpre_g = F("visual.ln_pre.weight"); m->lnpre_b = F("visual.ln_pre.bias");
        m->vproj = F("visual.proj");
        m->tproj_b = nullptr;
    }
    m->tok = F("token_embedding.weight"); m->tpos = F("positional_embedding");
    if (m->family != 2) { m->lnf_g = F("ln_final.weight"); m->lnf_b = F("ln_final.bias"); m->tproj = F("text_projection"); }

    for (auto& kv : m->tensors) { std::vector<float>().swap(kv.second.data); kv.second.loaded = false; }
    m->res_dtype = (precision == KEMR_PREC_BF16_RES16 || precision == KEMR_PREC_FP8_RES16) ? KEMR_BF16 : KEMR_F32;
    if (m->stream24 && m->res_dtype == KEMR_F32 && !x3) m->res_dtype = KEMR_F24;      // option "residual_stream_24bit" (common.h f24_t)
    m->fp8 = fp8;
    m->x3 = x3 ? 1 : 0;
    m->finalized = true;
    return KEMR_OK;
}

extern "C" int kemr_model_destroy(kemr_model* m) {
    if (!m) return KEMR_OK;
    if (m->arena) (void)hipFree(m->arena);
    delete m;
    return KEMR_OK;
}

// ------------------------------------------------------------------------------------------------ encoders
namespace {

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
};

size_t compact_bytes(int width, int items) {
    const int64_t Mc = round_up((int64_t)items, 256);
    return (size_t)(round_up((int64_t)items * 4, 256) + Mc * width * 4 + 5 * Mc * width * 2 + Mc * width * 8);
}

size_t ws_bytes_rows(int width, int64_t rows, int x_dtype) {
    const int64_t Mp = round_up(rows, 256);
    const int xb = x_dtype == KEMR_BF16 ? 2 : (x_dtype == KEMR_F24 ? 3 : 4);
    return (size_t)(round_up(Mp * width * xb, 256) + 3 * round_up(Mp * width * 2, 256) + round_up(Mp * width * 8, 256));
}

size_t ws_bytes(int width, int tokens, int batch, int x_dtype) {
    const int64_t Mp = round_up((int64_t)batch * tokens, 256);
    const int xb = x_dtype == KEMR_BF16 ? 2 : (x_dtype == KEMR_F24 ? 3 : 4);
    return (size_t)(round_up(Mp * width * xb, 256) + 3 * round_up(Mp * width * 2, 256) + round_up(Mp * width * 8, 256));
}

int carve(Workspace& w, void* base, size_t bytes, int width, int64_t rows, int items, int x_dtype) {
    const size_t need = ws_bytes_rows(width, rows, x_dtype) + compact_bytes(width, items);
    if (!base || bytes < need) KEMR_FAIL(KEMR_ERR_WORKSPACE, "workspace too small: %zu < %zu bytes", bytes, need);
    if ((uintptr_t)base % 256) KEMR_FAIL(KEMR_ERR_WORKSPACE, "workspace must be 256-byte aligned");
    const int64_t Mp = round_up(rows, 256);
    char* p = (char*)base;
    w.x = p; w.x_dtype = x_dtype; p += round_up(Mp * width * (x_dtype == KEMR_BF16 ? 2 : (x_dtype == KEMR_F24 ? 3 : 4)), 256);
    w.x32 = x_dtype == KEMR_F32 ? (float*)w.x : (float*)p;
    w.h = (bf16_t*)p; p += round_up(Mp * width * 2, 256);
    w.delta = (bf16_t*)p; p += round_up(Mp * width * 2, 256);
    w.delta2 = (bf16_t*)p; p += round_up(Mp * width * 2, 256);
    w.big = (bf16_t*)p; p += round_up(Mp * width * 8, 256);
    const int64_t Mc = round_up((int64_t)items, 256);
    w.pool_idx = (int*)p; p += round_up((int64_t)items * 4, 256);
    w.xc = p; p += Mc * width * 4;                     // (sized for an fp32 stream)
    w.hc = (bf16_t*)p; p += Mc * width * 2;
    w.qc = (bf16_t*)p; p += Mc * width * 2;
    w.ac = (bf16_t*)p; p += Mc * width * 2;
    w.d1c = (bf16_t*)p; p += Mc * width * 2;
    w.d2c = (bf16_t*)p; p += Mc * width * 2;
    w.gc = (bf16_t*)p;
    return KEMR_OK;
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
// *pending = deltas left for the tail.
// row_start / rows (text tower only): the token rows are packed, text i owning rows row_start[i] .. row_start[i + 1] - 1, `rows` in all.
//
// last_pooled (option "last_block_pooled_row", store-only epilogues, fc1 not on fp8): only ONE row per item leaves a tower -- the class
// token's (ln_post(x[:, 0]) @ proj) or the end-of-text token's -- so the LAST block computes K and V for every row (they feed that
// row's attention) but the query, the attention output, out-proj, ln_2 and the MLP for the pooled rows alone: compact [items, W]
// buffers, 2 of the block's 12 W^2 of GEMM work per token row instead of 12.  The pooled rows see the same arithmetic (their GEMMs
// are smaller launches, routed to the skinny / 128-row kernels, with their summation order).  *compact = the tail reads xc / d1c / d2c.
// epi_act: the fc1 epilogue (option "activation"), EPI_BIAS_QGELU_BF16 or EPI_BIAS_GELU_BF16; nothing else depends on the activation.
// eps: every LayerNorm's epsilon.  pool_pos (causal == 0 only): the position of the pooled row, 0 = the class token; family 1's text
// tower is unmasked and pools its LAST position, so its last block runs the pooled-row form with pool_pos = ctx - 1.
int run_blocks(const TowerW& t, const Workspace& w, int batch, int causal, int fp8, int want_resadd, int epi_act, hipStream_t s, bool* pending,
               const int* row_start = nullptr, int rows = 0, int last_pooled = 0, const int32_t* ids = nullptr, bool* compact = nullptr,
               float eps = 1e-5f, int pool_pos = 0) {
    const int W = t.width, M = row_start ? rows : batch * t.tokens;
    const bool fq = fp8 & 1, f1 = fp8 & 2;          // LayerNorm output = A operand of QKV / fc1: e4m3 where that GEMM runs in fp8
    bool resadd = want_resadd >= (w.x_dtype == KEMR_BF16 ? 1 : 2) && M > 512 && W % 256 == 0 && w.x_dtype != KEMR_F24;
    const int cs = w.x_dtype == KEMR_BF16 ? 2 : 4;
    const int epi_res = w.x_dtype == KEMR_BF16 ? EPI_BIAS_RESADD_BF16 : EPI_BIAS_RESID_F32;
    if (resadd) {
        GemmParams a{}, b{};
        a.M = b.M = M; a.N = b.N = W; a.K = W; b.K = 4 * W; a.lda = W; b.lda = 4 * W; a.ldw = W; b.ldw = 4 * W; a.ldc = b.ldc = W;
        a.c_rows_padded = b.c_rows_padded = 1;
        resadd = gemm256u_fits(a, 2, cs) && gemm256u_fits(b, 2, cs);
    }
    *pending = !resadd && t.layers > 0;
    const bool pooled = last_pooled && compact && !resadd && !f1 && t.layers > 0 && t.tokens <= KEMR_MAX_VISION_TOKENS;
    if (compact) *compact = pooled;
    if (pooled) KEMR_TRY(launch_pool_index(causal ? ids : nullptr, row_start, batch, t.tokens, w.pool_idx, s, pool_pos));
    for (int l = 0; l < t.layers; ++l) {
        const LayerW& L = t.layer[l];
        if (pooled && l == t.layers - 1) {
            KEMR_TRY(launch_layernorm(w.x, w.x_dtype, l ? w.delta : nullptr, l ? w.delta2 : nullptr, 1, L.ln1_g, L.ln1_b, w.h, M, W, fq ? KEMR_FP8 : KEMR_BF16, s, eps));
            GemmParams g{};
            g.c_rows_padded = 1;
            // K and V of every row: the weight rows W .. 3W - 1 of in_proj, into the columns W .. 3W - 1 of the qkv buffer; then the query of
            // the pooled rows from the first W weight rows (fq: both on e4m3 operands, like the QKV GEMM of the other blocks)
            g.M = M; g.A = w.h; g.lda = W; g.ldw = W; g.bias = L.bqkv + W; g.C = w.big + W; g.ldc = 3 * W; g.N = 2 * W; g.K = W;
            if (fq) { g.W = (const bf16_t*)(L.wqkv8 + (size_t)W * W); g.wscale = L.sqkv + W; KEMR_TRY(launch_gemm256u_fp8(g, EPI_BIAS_BF16, s)); }
            else { g.W = L.wqkv + (size_t)W * W; KEMR_TRY(launch_gemm(g, EPI_BIAS_BF16, s)); }
            KEMR_TRY(launch_gather_pooled(w.x, w.x_dtype, w.h, fq ? KEMR_FP8 : KEMR_BF16, w.pool_idx, batch, W, w.xc, w.hc, s));
            g.M = batch; g.A = w.hc; g.bias = L.bqkv; g.C = w.qc; g.ldc = W; g.N = W;
            if (fq) { g.W = (const bf16_t*)L.wqkv8; g.wscale = L.sqkv; KEMR_TRY(launch_gemm256u_fp8(g, EPI_BIAS_BF16, s)); g.wscale = nullptr; }
            else { g.W = L.wqkv; KEMR_TRY(launch_gemm(g, EPI_BIAS_BF16, s)); }
            if (t.head_dim == 80) KEMR_TRY(launch_attention80_pooled(w.qc, w.big, w.ac, batch, t.tokens, W, causal, s));
            else KEMR_TRY(launch_attention_pooled(w.qc, w.big, w.ac, w.pool_idx, row_start, batch, t.tokens, W, causal, s));
            g.A = w.ac; g.W = L.wo; g.bias = L.bo; g.C = w.d1c;
            KEMR_TRY(launch_gemm(g, EPI_BIAS_BF16, s));
            KEMR_TRY(launch_layernorm(w.xc, w.x_dtype, w.d1c, nullptr, 0, L.ln2_g, L.ln2_b, w.hc, batch, W, KEMR_BF16, s, eps));
            g.A = w.hc; g.W = L.w1; g.bias = L.b1; g.C = w.gc; g.ldc = 4 * W; g.N = 4 * W;
            KEMR_TRY(launch_gemm(g, epi_act, s));
            g.A = w.gc; g.lda = 4 * W; g.W = L.w2; g.ldw = 4 * W; g.bias = L.b2; g.C = w.d2c; g.ldc = W; g.N = W; g.K = 4 * W;
            KEMR_TRY(launch_gemm(g, EPI_BIAS_BF16, s));
            break;
        }
        if (resadd) KEMR_TRY(launch_layernorm(w.x, w.x_dtype, nullptr, nullptr, 0, L.ln1_g, L.ln1_b, w.h, M, W, fq ? KEMR_FP8 : KEMR_BF16, s, eps));
        else KEMR_TRY(launch_layernorm(w.x, w.x_dtype, l ? w.delta : nullptr, l ? w.delta2 : nullptr, 1, L.ln1_g, L.ln1_b, w.h, M, W, fq ? KEMR_FP8 : KEMR_BF16, s, eps));
        GemmParams g{};
        g.M = M;
        g.c_rows_padded = 1;       // every workspace buffer has ceil256(M) rows
        g.A = w.h; g.lda = W; g.W = L.wqkv; g.ldw = W; g.bias = L.bqkv; g.C = w.big; g.ldc = 3 * W; g.N = 3 * W; g.K = W;
        if (fq) {
            g.W = (const bf16_t*)L.wqkv8; g.wscale = L.sqkv;
            KEMR_TRY(launch_gemm256u_fp8(g, EPI_BIAS_BF16, s));
            g.wscale = nullptr;
        } else {
            KEMR_TRY(launch_gemm(g, EPI_BIAS_BF16, s));
        }
        if (row_start) KEMR_TRY(launch_attention_packed(w.big, w.h, row_start, batch, t.tokens, W, s));
        else if (t.head_dim == 80) KEMR_TRY(launch_attention80(w.big, w.h, batch, t.tokens, W, causal, s));
        else KEMR_TRY(launch_attention(w.big, w.h, batch, t.tokens, W, causal, s));
        g.A = w.h; g.lda = W; g.W = L.wo; g.ldw = W; g.bias = L.bo; g.C = resadd ? w.x : (void*)w.delta; g.ldc = W; g.N = W; g.K = W;
        KEMR_TRY(launch_gemm(g, resadd ? epi_res : EPI_BIAS_BF16, s));
        KEMR_TRY(launch_layernorm(w.x, w.x_dtype, resadd ? nullptr : w.delta, nullptr, 0, L.ln2_g, L.ln2_b, w.h, M, W, f1 ? KEMR_FP8 : KEMR_BF16, s, eps));
        g.A = w.h; g.lda = W; g.W = L.w1; g.ldw = W; g.bias = L.b1; g.C = w.big; g.ldc = 4 * W; g.N = 4 * W; g.K = W;
        if (f1) {
            g.W = (const bf16_t*)L.w18; g.wscale = L.s1;
            KEMR_TRY(launch_gemm256u_fp8(g, epi_act, s));
            g.wscale = nullptr;
        } else {
            KEMR_TRY(launch_gemm(g, epi_act, s));
        }
        g.A = w.big; g.lda = 4 * W; g.W = L.w2; g.ldw = 4 * W; g.bias = L.b2; g.C = resadd ? w.x : (void*)w.delta2; g.ldc = W; g.N = W; g.K = 4 * W;
        KEMR_TRY(launch_gemm(g, resadd ? epi_res : EPI_BIAS_BF16, s));
    }
    return KEMR_OK;
}

// The token fronts of the two towers, shared by the encoders and the kemr_debug_*_tokens pass-throughs (include/kemr_debug.h):
// the argument checks, the workspace carve and the kernels up to the rows the first LayerNorm reads.  `what` prefixes the
// messages; out_dev is only checked for null.  batch == 0 returns KEMR_OK with nothing launched (the caller stops there).
// Vision: im2col, the patch-embedding GEMM (EPI_PATCH_F32: token rows + positional embedding) and the class rows -> w.x32, the
// fp32 rows [batch * tokens, v_width] ln_pre reads.
int image_front(kemr_model* m, const float* pixels_dev, int batch, const void* out_dev, void* workspace_dev, size_t workspace_bytes,
                hipStream_t s, const char* what, Workspace& w) {
    if (!m || !pixels_dev || !out_dev) KEMR_FAIL(KEMR_ERR_INVALID, "%s: null argument", what);
    if (!m->finalized) KEMR_FAIL(KEMR_ERR_STATE, "%s: model not finalized", what);
    if (m->family == 2) KEMR_FAIL(KEMR_ERR_INVALID, "%s: not available for family 2 (BERT): a text-only model has no vision tower", what);
    if (m->x3) KEMR_FAIL(KEMR_ERR_STATE, "%s: not available for a KEMR_PREC_FP32X3 model", what);
    if (batch <= 0) return batch == 0 ? KEMR_OK : (set_error("%s: negative batch", what), KEMR_ERR_INVALID);
    if ((int64_t)batch * m->vtokens > (1 << 24)) KEMR_FAIL(KEMR_ERR_INVALID, "%s: batch %d too large", what, batch);
    const int W = m->cfg.v_width, T = m->vtokens;
    KEMR_TRY(carve(w, workspace_dev, workspace_bytes, W, (int64_t)batch * T, batch, m->res_dtype));
    KEMR_TRY(launch_im2col(pixels_dev, w.big, batch, m->cfg.image_size, m->cfg.patch, m->kpad, s));
    GemmParams g{};
    g.A = w.big; g.lda = m->kpad; g.W = m->conv_w; g.ldw = m->kpad; g.bias = nullptr; g.C = w.x32; g.ldc = W;
    g.pos = m->vpos; g.patches = m->patches; g.M = batch * m->patches; g.N = W; g.K = m->kpad;
    // family 1: no class token -- row m is patch m % patches of image m / patches; vpos holds pos + the conv bias
    if (m->family == 1) return launch_gemm(g, EPI_PATCH_ROWS_F32, s);
    KEMR_TRY(launch_gemm(g, EPI_PATCH_F32, s));
    return launch_cls_rows(w.x32, m->cls, m->vpos, batch, T, W, s);
}

// Family 1's vision pooling (SiglipMultiheadAttentionPoolingHead) on h = ln_post of EVERY token row [batch * T, W]: k | v of every row
// into the k and v planes of w.big (ld 3 W), the one learned query against them (the pooled-row attention kernel's vision form),
// r = out_proj(attn), out = r + fc2(gelu_tanh(fc1(layernorm(r)))), optionally L2-normalised.  The M = batch launches take the skinny
// GEMM route; r and the MLP update are bf16 GEMM outputs like every block's updates and are summed in fp32.
int map_head(const kemr_model* m, const Workspace& w, const bf16_t* h, int batch, int normalize, float* out, hipStream_t s) {
    const int W = m->cfg.v_width, T = m->vtokens;
    GemmParams g{};
    g.c_rows_padded = 1;
    g.M = batch * T; g.A = h; g.lda = W; g.W = m->mh_wkv; g.ldw = W; g.bias = m->mh_bkv; g.C = w.big + W; g.ldc = 3 * W; g.N = 2 * W; g.K = W;
    KEMR_TRY(launch_gemm(g, EPI_BIAS_BF16, s));
    KEMR_TRY(launch_broadcast_row(m->mh_q, w.qc, batch, W, s));
    KEMR_TRY(launch_attention_pooled(w.qc, w.big, w.ac, nullptr, nullptr, batch, T, W, 0, s));
    g.M = batch; g.A = w.ac; g.W = m->mh_wo; g.bias = m->mh_bo; g.C = w.d1c; g.ldc = W; g.N = W;
    KEMR_TRY(launch_gemm(g, EPI_BIAS_BF16, s));
    KEMR_TRY(launch_layernorm(w.d1c, KEMR_BF16, nullptr, nullptr, 0, m->mh_ln_g, m->mh_ln_b, w.hc, batch, W, KEMR_BF16, s, m->eps));
    g.A = w.hc; g.W = m->mh_w1; g.bias = m->mh_b1; g.C = w.gc; g.ldc = 4 * W; g.N = 4 * W;
    KEMR_TRY(launch_gemm(g, EPI_BIAS_TGELU_BF16, s));
    g.A = w.gc; g.lda = 4 * W; g.W = m->mh_w2; g.ldw = 4 * W; g.bias = m->mh_b2; g.C = w.d2c; g.ldc = W; g.N = W; g.K = 4 * W;
    KEMR_TRY(launch_gemm(g, EPI_BIAS_BF16, s));
    return launch_add_rows_out(w.d1c, w.d2c, batch, W, normalize, out, s);
}

// Text: the token + positional embedding rows of the residual stream (w.x, the model's storage type).  packed: lens_dev gives the
// lengths, `rows` the token rows (kemr_encode_text_packed) and *row_start the prefix sums row_starts_kernel leaves in the workspace;
// otherwise batch * ctx rows.
int text_front(kemr_model* m, const int32_t* ids_dev, const int32_t* lens_dev, int rows, int batch, bool packed, const void* out_dev,
               void* workspace_dev, size_t workspace_bytes, hipStream_t s, const char* what, Workspace& w, int** row_start) {
    if (!m || !ids_dev || !out_dev || (packed && !lens_dev)) KEMR_FAIL(KEMR_ERR_INVALID, "%s: null argument", what);
    if (m->family == 2)
        KEMR_FAIL(KEMR_ERR_INVALID, "%s: not available for family 2 (BERT): a padding mask is a length -- call kemr_encode_text_packed with the lengths (kemr_debug_bert_front for the front alone)", what);
    if (!m->finalized) KEMR_FAIL(KEMR_ERR_STATE, "%s: model not finalized", what);
    if (m->x3) KEMR_FAIL(KEMR_ERR_STATE, "%s: not available for a KEMR_PREC_FP32X3 model", what);
    if (batch <= 0) return batch == 0 ? KEMR_OK : (set_error("%s: negative batch", what), KEMR_ERR_INVALID);
    if ((int64_t)batch * m->cfg.ctx > (1 << 24)) KEMR_FAIL(KEMR_ERR_INVALID, "%s: batch %d too large", what, batch);
    const int W = m->cfg.t_width, T = m->cfg.ctx;
    *row_start = nullptr;
    if (!packed) {
        KEMR_TRY(carve(w, workspace_dev, workspace_bytes, W, (int64_t)batch * T, batch, m->res_dtype));
        return launch_text_embed(ids_dev, m->tok, m->tpos, w.x, w.x_dtype, batch, T, W, m->cfg.vocab, s);
    }
    if (m->cfg.ctx > 128) KEMR_FAIL(KEMR_ERR_INVALID, "%s: context length %d > 128", what, m->cfg.ctx);
    if (rows < batch || (int64_t)rows > (int64_t)batch * T) KEMR_FAIL(KEMR_ERR_INVALID, "%s: %d rows for %d texts of 1 .. %d positions", what, rows, batch, T);
    const size_t base_bytes = ws_bytes_rows(W, rows, m->res_dtype) + compact_bytes(W, batch), need = base_bytes + (size_t)round_up(((int64_t)batch + 1) * 4, 256);
    if (workspace_bytes < need) KEMR_FAIL(KEMR_ERR_WORKSPACE, "workspace too small: %zu < %zu bytes", workspace_bytes, need);
    KEMR_TRY(carve(w, workspace_dev, workspace_bytes, W, rows, batch, m->res_dtype));
    *row_start = (int*)((char*)workspace_dev + base_bytes);
    KEMR_TRY(launch_row_starts(lens_dev, batch, T, rows, *row_start, s));
    return launch_text_embed(ids_dev, m->tok, m->tpos, w.x, w.x_dtype, batch, T, W, m->cfg.vocab, s, *row_start, rows);
}

// ---- KEMR_PREC_FP32X3: its own workspace and tower driver (nothing of the bf16 path is shared but the kernels that are fp32 already) ----
// Per token row of the Mp = ceil256(rows) allocated: x [Mp, W] fp32 (the residual stream, plain 4-byte), h [Mp, 3W] bf16 (LayerNorm
// output, then the attention output: A-side triples), qkv [Mp, 3W] fp32, big [Mp, 12W] bf16 (the MLP hidden as an A-side triple;
// the tripled im2col rows, 3 kpad <= 12W, before the blocks).  46 W bytes per row; no pooled-row area: every row runs through every
// block (option "last_block_pooled_row" is ignored in this mode).
struct WorkspaceX3 { float* x; bf16_t* h; float* qkv; bf16_t* big; };

size_t ws_bytes_x3(int width, int64_t rows) {
    const int64_t Mp = round_up(rows, 256);
    return (size_t)(Mp * width * 4 + Mp * width * 6 + Mp * width * 12 + Mp * width * 24);
}

int carve_x3(WorkspaceX3& w, void* base, size_t bytes, int width, int64_t rows, size_t extra = 0) {
    const size_t need = ws_bytes_x3(width, rows) + extra;
    if (!base || bytes < need) KEMR_FAIL(KEMR_ERR_WORKSPACE, "workspace too small: %zu < %zu bytes", bytes, need);
    if ((uintptr_t)base % 256) KEMR_FAIL(KEMR_ERR_WORKSPACE, "workspace must be 256-byte aligned");
    const int64_t Mp = round_up(rows, 256);
    char* p = (char*)base;
    w.x = (float*)p; p += Mp * width * 4;
    w.h = (bf16_t*)p; p += Mp * width * 6;
    w.qkv = (float*)p; p += Mp * width * 12;
    w.big = (bf16_t*)p;
    return KEMR_OK;
}

// Every GEMM contracts over the tripled K on gemm.hip's 128 x 128 kernel (launch_gemm_x3); the out-proj and fc2 epilogues add
// acc + bias into x in fp32 (EPI_BIAS_RESID_F32: nothing pending for the tail, option "residual_fusion" has no meaning here).
int run_blocks_x3(const TowerW& t, const WorkspaceX3& w, int M, int batch, int causal, const int* row_start, int activation, hipStream_t s) {
    const int W = t.width;
    const int epi_act = activation == 1 ? EPI_X3_GELU : EPI_X3_QGELU;
    for (int l = 0; l < t.layers; ++l) {
        const LayerW& L = t.layer[l];
        KEMR_TRY(launch_layernorm_x3(w.x, L.ln1_g, L.ln1_b, w.h, M, W, s));
        GemmParams g{};
        g.M = M; g.c_rows_padded = 1;
        g.A = w.h; g.lda = 3 * W; g.W = L.wqkv; g.ldw = 3 * W; g.bias = L.bqkv; g.C = w.qkv; g.ldc = 3 * W; g.N = 3 * W; g.K = 3 * W;
        KEMR_TRY(launch_gemm_x3(g, EPI_X3_F32, s));
        if (t.head_dim == 80) KEMR_TRY(launch_attention80_x3(w.qkv, w.h, batch, t.tokens, W, causal, s));
        else KEMR_TRY(launch_attention_x3(w.qkv, w.h, row_start, batch, t.tokens, W, causal, s));
        g.W = L.wo; g.bias = L.bo; g.C = w.x; g.ldc = W; g.N = W;
        KEMR_TRY(launch_gemm_x3(g, EPI_BIAS_RESID_F32, s));
        KEMR_TRY(launch_layernorm_x3(w.x, L.ln2_g, L.ln2_b, w.h, M, W, s));
        g.W = L.w1; g.bias = L.b1; g.C = w.big; g.ldc = 12 * W; g.N = 4 * W;
        KEMR_TRY(launch_gemm_x3(g, epi_act, s));
        g.A = w.big; g.lda = 12 * W; g.W = L.w2; g.ldw = 12 * W; g.bias = L.b2; g.C = w.x; g.ldc = W; g.N = W; g.K = 12 * W;
        KEMR_TRY(launch_gemm_x3(g, EPI_BIAS_RESID_F32, s));
    }
    return KEMR_OK;
}

int encode_image_x3(kemr_model* m, const float* pixels_dev, int batch, float* out_dev, int normalize, void* workspace_dev,
                    size_t workspace_bytes, hipStream_t s, bool pooled = false) {
    if (!pixels_dev || !out_dev) KEMR_FAIL(KEMR_ERR_INVALID, "encode_image: null argument");
    if (batch <= 0) return batch == 0 ? KEMR_OK : (set_error("encode_image: negative batch"), KEMR_ERR_INVALID);
    if ((int64_t)batch * (m->patches + 1) > (1 << 24)) KEMR_FAIL(KEMR_ERR_INVALID, "encode_image: batch %d too large", batch);
    const int W = m->cfg.v_width, T = m->patches + 1, M = batch * T;
    WorkspaceX3 w;
    KEMR_TRY(carve_x3(w, workspace_dev, workspace_bytes, W, M));
    KEMR_TRY(launch_im2col_x3(pixels_dev, w.big, batch, m->cfg.image_size, m->cfg.patch, m->kpad, s));
    GemmParams g{};
    g.A = w.big; g.lda = 3 * m->kpad; g.W = m->conv_w; g.ldw = 3 * m->kpad; g.bias = nullptr; g.C = w.x; g.ldc = W;
    g.pos = m->vpos; g.patches = m->patches; g.M = batch * m->patches; g.N = W; g.K = 3 * m->kpad;
    KEMR_TRY(launch_gemm_x3(g, EPI_PATCH_F32, s));
    KEMR_TRY(launch_cls_rows(w.x, m->cls, m->vpos, batch, T, W, s));
    KEMR_TRY(launch_layernorm(w.x, KEMR_F32, nullptr, nullptr, 0, m->lnpre_g, m->lnpre_b, w.x, M, W, KEMR_F32, s));
    KEMR_TRY(run_blocks_x3(m->vis, w, M, batch, 0, nullptr, m->activation, s));
    return launch_tail(w.x, KEMR_F32, nullptr, nullptr, nullptr, batch, T, W, m->lnpost_g, m->lnpost_b, pooled ? nullptr : m->vproj, m->cfg.embed_dim, normalize, out_dev, s);
}

int encode_text_x3(kemr_model* m, const int32_t* ids_dev, const int32_t* lens_dev, int rows, int batch, bool packed, float* out_dev,
                   int normalize, void* workspace_dev, size_t workspace_bytes, hipStream_t s, bool pooled = false) {
    const char* what = packed ? "encode_text_packed" : "encode_text";
    if (!ids_dev || !out_dev || (packed && !lens_dev)) KEMR_FAIL(KEMR_ERR_INVALID, "%s: null argument", what);
    if (batch <= 0) return batch == 0 ? KEMR_OK : (set_error("%s: negative batch", what), KEMR_ERR_INVALID);
    if ((int64_t)batch * m->cfg.ctx > (1 << 24)) KEMR_FAIL(KEMR_ERR_INVALID, "%s: batch %d too large", what, batch);
    const int W = m->cfg.t_width, T = m->cfg.ctx;
    WorkspaceX3 w;
    int* row_start = nullptr;
    int M = batch * T;
    if (packed) {
        if (T > 128) KEMR_FAIL(KEMR_ERR_INVALID, "%s: context length %d > 128", what, T);
        if (rows < batch || (int64_t)rows > (int64_t)batch * T) KEMR_FAIL(KEMR_ERR_INVALID, "%s: %d rows for %d texts of 1 .. %d positions", what, rows, batch, T);
        KEMR_TRY(carve_x3(w, workspace_dev, workspace_bytes, W, rows, (size_t)round_up(((int64_t)batch + 1) * 4, 256)));
        row_start = (int*)((char*)workspace_dev + ws_bytes_x3(W, rows));
        KEMR_TRY(launch_row_starts(lens_dev, batch, T, rows, row_start, s));
        KEMR_TRY(launch_text_embed(ids_dev, m->tok, m->tpos, w.x, KEMR_F32, batch, T, W, m->cfg.vocab, s, row_start, rows));
        M = rows;
    } else {
        KEMR_TRY(carve_x3(w, workspace_dev, workspace_bytes, W, M));
        KEMR_TRY(launch_text_embed(ids_dev, m->tok, m->tpos, w.x, KEMR_F32, batch, T, W, m->cfg.vocab, s));
    }
    KEMR_TRY(run_blocks_x3(m->txt, w, M, batch, 1, row_start, m->activation, s));
    return launch_tail(w.x, KEMR_F32, nullptr, nullptr, ids_dev, batch, T, W, m->lnf_g, m->lnf_b, pooled ? nullptr : m->tproj, m->cfg.embed_dim, normalize, out_dev, s, row_start);
}

// ---- family 2: BERT sentence encoders (transformers.BertModel without its pooler + mean / CLS pooling) on packed rows ----
// Workspace: the token-row buffers of `carve` with no pooled-row area (every row runs through every block and feeds the pooling), then
// the batch + 1 row starts.  bert_front = the argument checks, the carve, the row starts and the embedding front; every check, the
// workspace's included, comes before the first launch.
size_t bert_ws_bytes(const kemr_model* m, int rows, int batch) {
    return ws_bytes_rows(m->cfg.t_width, rows, m->res_dtype) + (size_t)round_up(((int64_t)batch + 1) * 4, 256);
}

int bert_front(kemr_model* m, const int32_t* ids_dev, const int32_t* lens_dev, int rows, int batch, const void* out_dev, void* workspace_dev,
               size_t workspace_bytes, hipStream_t s, const char* what, Workspace& w, int** row_start) {
    if (!m || !ids_dev || !lens_dev || !out_dev) KEMR_FAIL(KEMR_ERR_INVALID, "%s: null argument", what);
    if (m->family != 2) KEMR_FAIL(KEMR_ERR_INVALID, "%s: only family 2 (BERT) has this front", what);
    if (!m->finalized) KEMR_FAIL(KEMR_ERR_STATE, "%s: model not finalized", what);
    if (batch <= 0) return batch == 0 ? KEMR_OK : (set_error("%s: negative batch", what), KEMR_ERR_INVALID);
    const int W = m->cfg.t_width, T = m->cfg.ctx;
    if (batch > 65535) KEMR_FAIL(KEMR_ERR_INVALID, "%s: batch %d > 65535", what, batch);
    if (rows < batch || (int64_t)rows > (int64_t)batch * T) KEMR_FAIL(KEMR_ERR_INVALID, "%s: %d rows for %d texts of 1 .. %d positions", what, rows, batch, T);
    if (rows > (1 << 24)) KEMR_FAIL(KEMR_ERR_INVALID, "%s: %d rows in one call (at most %d)", what, rows, 1 << 24);
    const size_t base_bytes = ws_bytes_rows(W, rows, m->res_dtype), need = bert_ws_bytes(m, rows, batch);
    if (!workspace_dev || workspace_bytes < need) KEMR_FAIL(KEMR_ERR_WORKSPACE, "workspace too small: %zu < %zu bytes", workspace_bytes, need);
    KEMR_TRY(carve(w, workspace_dev, workspace_bytes, W, rows, 0, m->res_dtype));
    *row_start = (int*)((char*)workspace_dev + base_bytes);
    KEMR_TRY(launch_row_starts(lens_dev, batch, T, rows, *row_start, s));
    return launch_bert_embed(ids_dev, m->tok, m->tpos, m->lne_g, m->lne_b, w.x, w.x_dtype, w.h, batch, T, W, m->cfg.vocab, *row_start, rows, m->eps, s);
}

// Post-LN blocks: QKV on h, attention over the packed items, out-proj into delta (store-only), x = LN(x + delta) with h = bf16(x), fc1
// with the exact GELU, fc2 into delta2, x = LN(x + delta2) with h = bf16(x).  Options "residual_fusion", "last_block_pooled_row" and
// "activation" are not consulted.
int encode_bert(kemr_model* m, const int32_t* ids_dev, const int32_t* lens_dev, int rows, int batch, float* out_dev, int normalize,
                void* workspace_dev, size_t workspace_bytes, hipStream_t s) {
    Workspace w;
    int* row_start = nullptr;
    KEMR_TRY(bert_front(m, ids_dev, lens_dev, rows, batch, out_dev, workspace_dev, workspace_bytes, s, "encode_text_packed", w, &row_start));
    if (batch == 0) return KEMR_OK;
    const TowerW& t = m->txt;
    const int W = t.width, M = rows;
    for (int l = 0; l < t.layers; ++l) {
        const LayerW& L = t.layer[l];
        GemmParams g{};
        g.M = M;
        g.c_rows_padded = 1;       // every workspace buffer has ceil256(M) rows
        g.A = w.h; g.lda = W; g.W = L.wqkv; g.ldw = W; g.bias = L.bqkv; g.C = w.big; g.ldc = 3 * W; g.N = 3 * W; g.K = W;
        KEMR_TRY(launch_gemm(g, EPI_BIAS_BF16, s));
        KEMR_TRY(launch_attention_varlen(w.big, w.h, row_start, batch, t.tokens, W, s));
        g.A = w.h; g.W = L.wo; g.bias = L.bo; g.C = w.delta; g.ldc = W; g.N = W;
        KEMR_TRY(launch_gemm(g, EPI_BIAS_BF16, s));
        KEMR_TRY(launch_layernorm_post(w.x, w.x_dtype, w.delta, L.ln1_g, L.ln1_b, w.h, M, W, s, m->eps));
        g.A = w.h; g.W = L.w1; g.bias = L.b1; g.C = w.big; g.ldc = 4 * W; g.N = 4 * W;
        KEMR_TRY(launch_gemm(g, EPI_BIAS_GELU_BF16, s));
        g.A = w.big; g.lda = 4 * W; g.W = L.w2; g.ldw = 4 * W; g.bias = L.b2; g.C = w.delta2; g.ldc = W; g.N = W; g.K = 4 * W;
        KEMR_TRY(launch_gemm(g, EPI_BIAS_BF16, s));
        KEMR_TRY(launch_layernorm_post(w.x, w.x_dtype, w.delta2, L.ln2_g, L.ln2_b, w.h, M, W, s, m->eps));
    }
    return launch_pool_rows(w.x, w.x_dtype, row_start, batch, W, m->pooling, normalize, out_dev, s);
}

// family 1's activation is the family's (tanh GELU); option "activation" is not consulted there
int fc1_epilogue(const kemr_model* m) { return m->family == 1 ? EPI_BIAS_TGELU_BF16 : m->activation == 1 ? EPI_BIAS_GELU_BF16 : EPI_BIAS_QGELU_BF16; }

}  // namespace

extern "C" size_t kemr_workspace_bytes(const kemr_model* m, int tower, int batch) {
    if (!m || batch <= 0) return 0;
    if (m->family == 2) return 0;                      // family 2 has the packed call only (kemr_text_packed_workspace_bytes)
    if (m->x3) {
        if (tower == KEMR_TOWER_VISION) return ws_bytes_x3(m->cfg.v_width, (int64_t)batch * (m->patches + 1));
        return tower == KEMR_TOWER_TEXT ? ws_bytes_x3(m->cfg.t_width, (int64_t)batch * m->cfg.ctx) : 0;
    }
    if (tower == KEMR_TOWER_VISION) return ws_bytes(m->cfg.v_width, m->vtokens, batch, m->res_dtype) + compact_bytes(m->cfg.v_width, batch);
    if (tower == KEMR_TOWER_TEXT) return ws_bytes(m->cfg.t_width, m->cfg.ctx, batch, m->res_dtype) + compact_bytes(m->cfg.t_width, batch);
    return 0;
}

extern "C" size_t kemr_text_packed_workspace_bytes(const kemr_model* m, int rows, int batch) {
    if (!m || batch <= 0 || rows < batch) return 0;
    if (m->family == 2) return bert_ws_bytes(m, rows, batch);                                      // buffers + row_start (no pooled-row area)
    if (m->x3) return ws_bytes_x3(m->cfg.t_width, rows) + (size_t)round_up(((int64_t)batch + 1) * 4, 256);
    return ws_bytes_rows(m->cfg.t_width, rows, m->res_dtype) + compact_bytes(m->cfg.t_width, batch) +
           (size_t)round_up(((int64_t)batch + 1) * 4, 256);                                        // buffers + pooled-row area + row_start
}

// pooled: the tail stores the pooled row of the residual stream (pending updates applied) instead of normalising and projecting it --
// kemr_encode_*_pooled; family 0 only (SigLIP's head is the attention pool over every row, BERT has no head)
static int pooled_family_check(const kemr_model* m, bool pooled, const char* what) {
    if (pooled && m && m->family == 1) KEMR_FAIL(KEMR_ERR_INVALID, "%s: not available for family 1 (SigLIP): its head is the attention pool over every row, not LayerNorm + projection of one pooled row", what);
    if (pooled && m && m->family == 2) KEMR_FAIL(KEMR_ERR_INVALID, "%s: not available for family 2 (BERT): a sentence encoder has no projection head", what);
    return KEMR_OK;
}

static int encode_image_any(kemr_model* m, const float* pixels_dev, int batch, float* out_dev, int normalize,
                            void* workspace_dev, size_t workspace_bytes, void* stream, bool pooled) {
    hipStream_t s = (hipStream_t)stream;
    KEMR_TRY(pooled_family_check(m, pooled, "encode_image_pooled"));
    const float* vproj = (pooled || !m) ? nullptr : m->vproj;
    if (m && m->family == 2) KEMR_FAIL(KEMR_ERR_INVALID, "encode_image: not available for family 2 (BERT): a text-only model has no vision tower");
    if (m && m->finalized && m->x3) return encode_image_x3(m, pixels_dev, batch, out_dev, normalize, workspace_dev, workspace_bytes, s, pooled);
    Workspace w;
    KEMR_TRY(image_front(m, pixels_dev, batch, out_dev, workspace_dev, workspace_bytes, s, "encode_image", w));
    if (batch == 0) return KEMR_OK;
    const int W = m->cfg.v_width, T = m->vtokens;
    bool vb = false, vc = false;
    if (m->family == 1) {
        // no ln_pre: the front's fp32 rows enter block 0 in the stream's storage type; every row of the last block feeds the pooling
        // head, so option "last_block_pooled_row" cannot apply; ln_post (applying the last block's pending updates) runs over all rows
        KEMR_TRY(launch_stream_cast(w.x32, w.x, w.x_dtype, (int64_t)batch * T, W, s));
        KEMR_TRY(run_blocks(m->vis, w, batch, 0, 0, m->resadd, fc1_epilogue(m), s, &vb, nullptr, 0, 0, nullptr, nullptr, m->eps));
        KEMR_TRY(launch_layernorm(w.x, w.x_dtype, vb ? w.delta : nullptr, vb ? w.delta2 : nullptr, vb ? 1 : 0, m->lnpost_g, m->lnpost_b, w.h, batch * T, W, KEMR_BF16, s, m->eps));
        return map_head(m, w, w.h, batch, normalize, out_dev, s);
    }
    KEMR_TRY(launch_layernorm(w.x32, KEMR_F32, nullptr, nullptr, 0, m->lnpre_g, m->lnpre_b, w.x, batch * T, W, w.x_dtype, s));
    KEMR_TRY(run_blocks(m->vis, w, batch, 0, m->fp8, m->resadd, fc1_epilogue(m), s, &vb, nullptr, 0, m->last_pooled, nullptr, &vc));
    if (vc) KEMR_TRY(launch_tail(w.xc, w.x_dtype, w.d1c, w.d2c, nullptr, batch, 1, W, m->lnpost_g, m->lnpost_b, vproj, m->cfg.embed_dim, normalize, out_dev, s));
    else KEMR_TRY(launch_tail(w.x, w.x_dtype, vb ? w.delta : nullptr, vb ? w.delta2 : nullptr, nullptr, batch, T, W, m->lnpost_g, m->lnpost_b, vproj, m->cfg.embed_dim, normalize, out_dev, s));
    return KEMR_OK;
}

static int encode_text_any(kemr_model* m, const int32_t* ids_dev, int batch, float* out_dev, int normalize,
                           void* workspace_dev, size_t workspace_bytes, void* stream, bool pooled) {
    hipStream_t s = (hipStream_t)stream;
    KEMR_TRY(pooled_family_check(m, pooled, "encode_text_pooled"));
    const float* tproj = (pooled || !m) ? nullptr : m->tproj;
    if (m && m->family == 2)
        KEMR_FAIL(KEMR_ERR_INVALID, "encode_text: not available for family 2 (BERT): a padding mask is a length -- call kemr_encode_text_packed with the lengths");
    if (m && m->finalized && m->x3) return encode_text_x3(m, ids_dev, nullptr, 0, batch, false, out_dev, normalize, workspace_dev, workspace_bytes, s, pooled);
    Workspace w;
    int* no_rows = nullptr;
    KEMR_TRY(text_front(m, ids_dev, nullptr, 0, batch, false, out_dev, workspace_dev, workspace_bytes, s, "encode_text", w, &no_rows));
    if (batch == 0) return KEMR_OK;
    const int W = m->cfg.t_width, T = m->cfg.ctx;
    bool tb = false, tc = false;
    if (m->family == 1) {
        // no mask (pads are keys like every other position), the LAST position pooled whatever the ids, the head a Linear with bias
        KEMR_TRY(run_blocks(m->txt, w, batch, 0, 0, m->resadd, fc1_epilogue(m), s, &tb, nullptr, 0, m->last_pooled, nullptr, &tc, m->eps, T - 1));
        if (tc) return launch_tail(w.xc, w.x_dtype, w.d1c, w.d2c, nullptr, batch, 1, W, m->lnf_g, m->lnf_b, m->tproj, m->cfg.embed_dim, normalize, out_dev, s, nullptr, m->eps, 0, m->tproj_b);
        return launch_tail(w.x, w.x_dtype, tb ? w.delta : nullptr, tb ? w.delta2 : nullptr, nullptr, batch, T, W, m->lnf_g, m->lnf_b, m->tproj, m->cfg.embed_dim, normalize, out_dev, s, nullptr, m->eps, T - 1, m->tproj_b);
    }
    KEMR_TRY(run_blocks(m->txt, w, batch, 1, 0, m->resadd, fc1_epilogue(m), s, &tb, nullptr, 0, m->last_pooled, ids_dev, &tc));
    if (tc) KEMR_TRY(launch_tail(w.xc, w.x_dtype, w.d1c, w.d2c, nullptr, batch, 1, W, m->lnf_g, m->lnf_b, tproj, m->cfg.embed_dim, normalize, out_dev, s));
    else KEMR_TRY(launch_tail(w.x, w.x_dtype, tb ? w.delta : nullptr, tb ? w.delta2 : nullptr, ids_dev, batch, T, W, m->lnf_g, m->lnf_b, tproj, m->cfg.embed_dim, normalize, out_dev, s));
    return KEMR_OK;
}

// The text tower on the rows that can reach the output only.  The attention mask is causal and the pooled row is the end-of-text
// token's (reference: model.encode_text -> x[arange, text.argmax(-1)]; open_clip / CLIP text transformer with attn_mask), so the
// positions behind it never influence the embedding: text i is computed on its first lens_dev[i] positions, packed one text
// behind the other (`rows` = sum(lens) rows instead of batch * ctx through every GEMM, LayerNorm and attention launch).  With
// lens[i] >= argmax_i + 1 the embeddings are kemr_encode_text's -- the same arithmetic per row; the GEMM a launch of another M is
// routed to may sum in another order, as for another batch size (tests/test_encoder_gpu.py: 1 - cos of a few 1e-5 both ways); a
// shorter length pools the last computed row instead (memory-safe, wrong).  `rows` is a HOST integer: the tokenizer's side knows the lengths without
// asking the device (the python wrapper derives lens and rows from the same host tokens); lengths and prefix sums are clamped on the
// device (row_starts_kernel) so that no argument can index outside the workspace.
static int encode_text_packed_any(kemr_model* m, const int32_t* ids_dev, const int32_t* lens_dev, int rows, int batch, float* out_dev,
                                  int normalize, void* workspace_dev, size_t workspace_bytes, void* stream, bool pooled) {
    hipStream_t s = (hipStream_t)stream;
    KEMR_TRY(pooled_family_check(m, pooled, "encode_text_packed_pooled"));
    const float* tproj = (pooled || !m) ? nullptr : m->tproj;
    if (m && m->family == 1)
        KEMR_FAIL(KEMR_ERR_INVALID, "encode_text_packed: not available for family 1 (SigLIP): its text tower is unmasked and pools the last position, so a pad position is a key and no row can be left out");
    if (m && m->family == 2) return encode_bert(m, ids_dev, lens_dev, rows, batch, out_dev, normalize, workspace_dev, workspace_bytes, s);
    if (m && m->finalized && m->x3) return encode_text_x3(m, ids_dev, lens_dev, rows, batch, true, out_dev, normalize, workspace_dev, workspace_bytes, s, pooled);
    Workspace w;
    int* row_start = nullptr;
    KEMR_TRY(text_front(m, ids_dev, lens_dev, rows, batch, true, out_dev, workspace_dev, workspace_bytes, s, "encode_text_packed", w, &row_start));
    if (batch == 0) return KEMR_OK;
    const int W = m->cfg.t_width, T = m->cfg.ctx;
    bool tb = false, tc = false;
    KEMR_TRY(run_blocks(m->txt, w, batch, 1, 0, m->resadd, fc1_epilogue(m), s, &tb, row_start, rows, m->last_pooled, ids_dev, &tc));
    if (tc) KEMR_TRY(launch_tail(w.xc, w.x_dtype, w.d1c, w.d2c, nullptr, batch, 1, W, m->lnf_g, m->lnf_b, tproj, m->cfg.embed_dim, normalize, out_dev, s));
    else KEMR_TRY(launch_tail(w.x, w.x_dtype, tb ? w.delta : nullptr, tb ? w.delta2 : nullptr, ids_dev, batch, T, W, m->lnf_g, m->lnf_b, tproj, m->cfg.embed_dim, normalize, out_dev, s, row_start));
    return KEMR_OK;
}

extern "C" int kemr_encode_image(kemr_model* m, const float* pixels_dev, int batch, float* out_dev, int normalize,
                                 void* workspace_dev, size_t workspace_bytes, void* stream) {
    return encode_image_any(m, pixels_dev, batch, out_dev, normalize, workspace_dev, workspace_bytes, stream, false);
}
extern "C" int kemr_encode_text(kemr_model* m, const int32_t* ids_dev, int batch, float* out_dev, int normalize,
                                void* workspace_dev, size_t workspace_bytes, void* stream) {
    return encode_text_any(m, ids_dev, batch, out_dev, normalize, workspace_dev, workspace_bytes, stream, false);
}
extern "C" int kemr_encode_text_packed(kemr_model* m, const int32_t* ids_dev, const int32_t* lens_dev, int rows, int batch, float* out_dev,
                                       int normalize, void* workspace_dev, size_t workspace_bytes, void* stream) {
    return encode_text_packed_any(m, ids_dev, lens_dev, rows, batch, out_dev, normalize, workspace_dev, workspace_bytes, stream, false);
}
extern "C" int kemr_encode_image_pooled(kemr_model* m, const float* pixels_dev, int batch, float* out_dev,
                                        void* workspace_dev, size_t workspace_bytes, void* stream) {
    return encode_image_any(m, pixels_dev, batch, out_dev, 0, workspace_dev, workspace_bytes, stream, true);
}
extern "C" int kemr_encode_text_pooled(kemr_model* m, const int32_t* ids_dev, int batch, float* out_dev,
                                       void* workspace_dev, size_t workspace_bytes, void* stream) {
    return encode_text_any(m, ids_dev, batch, out_dev, 0, workspace_dev, workspace_bytes, stream, true);
}
extern "C" int kemr_encode_text_packed_pooled(kemr_model* m, const int32_t* ids_dev, const int32_t* lens_dev, int rows, int batch, float* out_dev,
                                              void* workspace_dev, size_t workspace_bytes, void* stream) {
    return encode_text_packed_any(m, ids_dev, lens_dev, rows, batch, out_dev, 0, workspace_dev, workspace_bytes, stream, true);
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
        if (value == 2) KEMR_FAIL(KEMR_ERR_INVALID, "model_set_option(family): 0 (CLIP) or 1 (SigLIP), got 2 (family 2, BERT, has its own configuration checks and is decided at creation: kemr_model_create_family)");
        if (m->family == 2) KEMR_FAIL(KEMR_ERR_INVALID, "model_set_option(family): a family 2 (BERT) model keeps its family (kemr_model_create_family)");
        if (value < 0 || value > 1) KEMR_FAIL(KEMR_ERR_INVALID, "model_set_option(family): 0 (CLIP) or 1 (SigLIP), got %d", value);
        if (m->any_loaded || m->finalized) KEMR_FAIL(KEMR_ERR_STATE, "model_set_option(family): set it before the first kemr_model_load_tensor (it decides the tensor names)");
        if (value == 1 && m->v_head_dim != 64) KEMR_FAIL(KEMR_ERR_INVALID, "model_set_option(family): family 1 (SigLIP) serves vision_head_dim 64 only, got %d", m->v_head_dim);
        m->family = value;
        build_names(m);
        return KEMR_OK;
    }
    if (!strcmp(key, "pooling")) {
        if (m->family != 2) KEMR_FAIL(KEMR_ERR_INVALID, "model_set_option(pooling): the option exists for family 2 (BERT) only");
        if (value < 0 || value > 1) KEMR_FAIL(KEMR_ERR_INVALID, "model_set_option(pooling): 0 (mean) or 1 (first row, CLS), got %d", value);
        m->pooling = value;
        return KEMR_OK;
    }
    if (!strcmp(key, "vision_head_dim")) {
        if (m->family == 2) KEMR_FAIL(KEMR_ERR_INVALID, "model_set_option(vision_head_dim): family 2 (BERT) has no vision tower");
        if (m->family == 1 && value != 64) KEMR_FAIL(KEMR_ERR_INVALID, "model_set_option(vision_head_dim): family 1 (SigLIP) serves vision_head_dim 64 only, got %d", value);
        if (value != 64 && value != 80) KEMR_FAIL(KEMR_ERR_INVALID, "model_set_option(vision_head_dim): 64 or 80, got %d", value);
        if (m->finalized) KEMR_FAIL(KEMR_ERR_STATE, "model_set_option(vision_head_dim): set it before kemr_model_finalize");
        if (m->cfg.v_width % value) KEMR_FAIL(KEMR_ERR_INVALID, "model_set_option(vision_head_dim): the vision width %d is not a multiple of %d", m->cfg.v_width, value);
        m->v_head_dim = value;
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
    if (!strcmp(key, "precision_residual_bf16")) { *value = m->res_dtype == KEMR_BF16; return KEMR_OK; }
    KEMR_FAIL(KEMR_ERR_INVALID, "model_get_option: unknown key '%s'", key);
}

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
    KEMR_TRY(carve(w, workspace_dev, workspace_bytes, W, (int64_t)batch * T, batch, m->res_dtype));
    KEMR_CHECK_HIP(hipMemcpyAsync(w.h, h_dev, (size_t)batch * T * W * 2, hipMemcpyDeviceToDevice, s));
    KEMR_TRY(map_head(m, w, w.h, batch, normalize, out_dev, s));
    if (attn_out_dev) KEMR_CHECK_HIP(hipMemcpyAsync(attn_out_dev, w.ac, (size_t)batch * W * 2, hipMemcpyDeviceToDevice, s));
    return KEMR_OK;
}

// ---- family 2 (BERT): the new kernels alone ----
extern "C" int kemr_debug_op_attention_varlen(const void* qkv_dev, void* out_dev, const int* row_start_dev, int batch, int max_t, int width,
                                              void* stream) {
    if (!qkv_dev || !out_dev || !row_start_dev) KEMR_FAIL(KEMR_ERR_INVALID, "debug_op_attention_varlen: null argument");
    return launch_attention_varlen((const bf16_t*)qkv_dev, (bf16_t*)out_dev, row_start_dev, batch, max_t, width, (hipStream_t)stream);
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

extern "C" int kemr_debug_bert_front(kemr_model* m, const int32_t* ids_dev, const int32_t* lens_dev, int rows, int batch, void* x_out_dev,
                                     void* h_out_dev, int* row_start_out_dev, void* workspace_dev, size_t workspace_bytes, void* stream) {
    if (!h_out_dev || !row_start_out_dev) KEMR_FAIL(KEMR_ERR_INVALID, "debug_bert_front: null output");
    hipStream_t s = (hipStream_t)stream;
    Workspace w;
    int* row_start = nullptr;
    KEMR_TRY(bert_front(m, ids_dev, lens_dev, rows, batch, x_out_dev, workspace_dev, workspace_bytes, s, "debug_bert_front", w, &row_start));
    if (batch == 0) return KEMR_OK;
    const int xb = w.x_dtype == KEMR_BF16 ? 2 : (w.x_dtype == KEMR_F24 ? 3 : 4);
    KEMR_CHECK_HIP(hipMemcpyAsync(x_out_dev, w.x, (size_t)rows * m->cfg.t_width * xb, hipMemcpyDeviceToDevice, s));
    KEMR_CHECK_HIP(hipMemcpyAsync(h_out_dev, w.h, (size_t)rows * m->cfg.t_width * 2, hipMemcpyDeviceToDevice, s));
    KEMR_CHECK_HIP(hipMemcpyAsync(row_start_out_dev, row_start, ((size_t)batch + 1) * 4, hipMemcpyDeviceToDevice, s));
    return KEMR_OK;
}

extern "C" int kemr_debug_text_tokens(kemr_model* m, const int32_t* ids_dev, const int32_t* lens_dev, int rows, int batch, void* out_dev,
                                      int* row_start_out_dev, void* workspace_dev, size_t workspace_bytes, void* stream) {
    const bool packed = lens_dev != nullptr;
    if (packed && !row_start_out_dev) KEMR_FAIL(KEMR_ERR_INVALID, "debug_text_tokens: null row_start output");
    hipStream_t s = (hipStream_t)stream;
    Workspace w;
    int* row_start = nullptr;
    KEMR_TRY(text_front(m, ids_dev, lens_dev, rows, batch, packed, out_dev, workspace_dev, workspace_bytes, s, "debug_text_tokens", w, &row_start));
    if (batch == 0) return KEMR_OK;
    const int xb = w.x_dtype == KEMR_BF16 ? 2 : (w.x_dtype == KEMR_F24 ? 3 : 4);
    const int64_t n = packed ? rows : (int64_t)batch * m->cfg.ctx;
    KEMR_CHECK_HIP(hipMemcpyAsync(out_dev, w.x, (size_t)n * m->cfg.t_width * xb, hipMemcpyDeviceToDevice, s));
    if (packed) KEMR_CHECK_HIP(hipMemcpyAsync(row_start_out_dev, row_start, ((size_t)batch + 1) * 4, hipMemcpyDeviceToDevice, s));
    return KEMR_OK;
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
