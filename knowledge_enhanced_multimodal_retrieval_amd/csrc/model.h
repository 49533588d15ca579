// Internal to libkemr.so: the model handle behind include/kemr.h, shared by model.hip (create, load, pack, finalize) and encode.hip
// (the launch sequences).  Host-side C++ only.
#pragma once
#include "common.h"

#include <map>
#include <string>
#include <vector>

namespace kemr {

struct HostTensor {
    std::vector<int64_t> shape;
    std::vector<float> data;
    bool loaded = false;
};

// What a required tensor is: decided once, where build_names (model.hip) generates its name.  Sizing, filling and binding switch on the
// kind; nothing but build_names and load_tensor's lookup by full name ever looks at a name.
enum TensorTower : int { TOWER_VISION, TOWER_TEXT, TOWER_HEAD };     // TOWER_HEAD: family 1's pooling head (visual.attn_pool.*)
enum TensorKind : int {
    KIND_F32,            // fp32, verbatim
    KIND_MATRIX,         // [N, K] bf16 (KEMR_PREC_FP32X3: the W-side triple [N, 3K] = [hi | hi | lo])
    KIND_QKV_WEIGHT,     // a matrix whose first K rows (the queries) carry the attention scale; e4m3 in the vision tower under the fp8 precisions
    KIND_QKV_BIAS,       // fp32, the first third scaled likewise
    KIND_FC1_WEIGHT,     // a matrix; e4m3 in the vision tower under KEMR_PREC_FP8_MLP
    KIND_CONV_WEIGHT,    // [width, 3 * patch * patch] -> bf16 rows of kpad columns (zero pad; the triple over 3 kpad)
    KIND_LN_QKV,         // gain or bias of the LayerNorm in front of the QKV GEMM: divided by the fp8 A operand's channel scales
    KIND_LN_FC1,         // the same in front of fc1
    KIND_VPOS_SIGLIP,    // family 1's vision positional table: + visual.conv1.bias per row
    KIND_TPOS_BERT,      // family 2's positional table: + token_type_embedding[0] per row
    KIND_PROBE,          // family 1's pooling probe: verbatim, and behind it the head's one query (probe . Wq^T + bq) / 8 as bf16
    KIND_REL_BIAS,       // family 3's relative_attention_bias [32, heads]: packed as the table by distance fp32 [heads, 1023] (expand_relative_bias)
};
struct TensorSpec {
    std::string name;
    TensorTower tower;
    int layer;           // residual block, -1 outside the blocks
    TensorKind kind;
    void* bind;          // the model's pointer that receives the device address (a `const T*` member; nullptr: nothing reads the device copy)
    HostTensor t;        // t.shape is the required shape
};
// Where a tensor lies in the device arena.  aux: the fp8 row scales IN FRONT of an e4m3 matrix, the query BEHIND the probe.
struct Placement { size_t off = 0, aux = 0; };
struct PackedWeights {
    size_t bytes = 0;                   // arena size; every entry starts on a multiple of 256 bytes
    std::vector<Placement> at;          // parallel to kemr_model::specs
    std::vector<char> host;             // the arena's content (empty after a size-only plan)
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

// families 2 (BERT) and 3 (MPNet) are the sentence encoders: text-only, post-LN blocks, the packed encode call only.  What is checked or
// refused for family 2 holds for family 3 alike, with the same messages.
inline bool is_sentence_family(int family) { return family == 2 || family == 3; }
// MPNet's bucket of a distance d = key - query (transformers MPNetEncoder.relative_position_bucket at 32 buckets, max distance 128),
// by integer thresholds; and the table by distance out[h * 1023 + d + 511] = weight[bucket(d) * heads + h], d in -511 .. 511
int relative_position_bucket(int d);
void expand_relative_bias(const float* weight, int heads, float* out);

// model.hip: the refusals of kemr_model_finalize (null model, precision, family, head dim, missing keys) and the pure host packing step
int fp8_bits(int precision);
int check_finalize(const kemr_model* m, int precision);
void pack_weights(const kemr_model& m, int precision, bool fill, PackedWeights& out);

}  // namespace kemr

struct kemr_model {
    kemr_cfg cfg;
    std::vector<kemr::TensorSpec> specs;            // required tensors, fixed order
    std::map<std::string, int> index;               // name -> specs[]
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
                                                    // 3 = MPNet sentence encoder (option "family" = 3 on a model created as family 2: family 2 without token types, with a relative position bias in every
                                                    // attention score, eps 1e-5 or 1e-12 by option "layer_norm_eps")
    int pooling = 0;                                // option "pooling" (families 2, 3): 0 = mean of the item's rows, 1 = its first row (CLS)
    int ln_eps_exp = 5;                             // option "layer_norm_eps" (family 3, before finalize): 5 = 1e-5 (the published all-mpnet-base-v2), 12 = 1e-12 (MPNetConfig's default)
    bool any_loaded = false;                        // a tensor was loaded: the name list is fixed from then on
    float eps = 1e-5f;                              // every LayerNorm's epsilon: 1e-6 for family 1
    int vtokens = 0;                                // token rows per image: patches + 1 (class token), patches for family 1
    // vision
    kemr::TowerW vis;
    const kemr::bf16_t* conv_w = nullptr;
    const float *cls = nullptr, *vpos = nullptr, *lnpre_g = nullptr, *lnpre_b = nullptr, *lnpost_g = nullptr,
                *lnpost_b = nullptr, *vproj = nullptr;
    // text
    kemr::TowerW txt;
    const float *tok = nullptr, *tpos = nullptr, *lnf_g = nullptr, *lnf_b = nullptr, *tproj = nullptr;
    // family 1: the text head's bias; the vision tower's pooling head (visual.attn_pool.*): its one query row (probe . Wq^T + bq) / 8
    // made by pack_weights, the k | v rows of in_proj (wkv = in_proj_weight + W * W), out_proj, LayerNorm and MLP
    const float* tproj_b = nullptr;
    const kemr::bf16_t *mh_q = nullptr, *mh_wkv = nullptr, *mh_wo = nullptr, *mh_w1 = nullptr, *mh_w2 = nullptr;
    const float *lne_g = nullptr, *lne_b = nullptr;  // families 2, 3: the embedding LayerNorm (ln_embed.*)
    const float* rel_bias = nullptr;                 // family 3: the attention bias by distance, fp32 [heads, 1023], one table for all layers
    const float *mh_bkv = nullptr, *mh_bo = nullptr, *mh_ln_g = nullptr, *mh_ln_b = nullptr, *mh_b1 = nullptr, *mh_b2 = nullptr;
};
