/*
 * kemr.h -- C ABI of libkemr.so, the MI355X (gfx950) CLIP retrieval hot path.
 *
 * The reference (REEVALUATE/knowledge_enhanced_multimodal_retrieval) is 100 % Python and has no
 * native plugin/FFI boundary of its own: its boundary for this path is a set of Python call
 * signatures.  This header is the C ABI one level below those signatures;
 * every entry point names the reference call it replaces.  The Python host side
 * (knowledge_enhanced_multimodal_retrieval_amd/, and the drop-in `src.clip.*` mirror) binds these
 * symbols with ctypes; INTEGRATION.md shows the binding a reference maintainer would add.
 *
 * Conventions
 *  - plain C: opaque handle, raw pointers, sizes; no torch / C++ types cross the ABI.
 *  - every function returns KEMR_OK (0) or a negative kemr_status; kemr_last_error() returns a
 *    thread-local message for the last failure.  Nothing throws across the ABI.
 *  - "dev" pointers are device (HBM) pointers owned by the caller; the library never allocates on
 *    the hot path.  Scratch comes from the caller through a workspace sized by *_workspace_bytes().
 *    The library owns only the model handle and its packed weights (allocated in finalize).
 *  - all launches are asynchronous on the hipStream_t passed as `void* stream` (0 = default stream);
 *    no entry point waits for the device except the calls listed below under "calls that synchronise the host".
 *    Stream contract (tests/stream_order.py, tests/test_stream_*_gpu.py):
 *      - every kernel, memset and copy of a call is queued on the stream passed, in order, and on no other stream; the library
 *        creates no stream of its own.  A call may therefore be queued before its inputs exist (behind the work that produces them
 *        on that stream), and its arguments may be overwritten by work queued behind it.  Host arrays (the sizes and offsets of the
 *        batch transforms, the pointer arrays of kemr_panel_build) are read before the call returns.
 *      - the call returns without waiting for the device.  What a call copies host to device (the descriptor blob of the batch
 *        transforms, the tap table of the single-image transforms) leaves from pinned staging slots of the library's own; a call
 *        waits for a slot only with 64 such copies in flight.  A slot is chosen, filled and sent under one lock, so two
 *        host threads are never handed the same slot.
 *      - a finalized model handle is read-only during the encode calls: one handle may serve several streams at once when every
 *        call in flight has a workspace of its own.  Two calls that share a workspace must be ordered by the caller (the Python
 *        engines do this for their own workspace: engine.CallOrder).  kemr_model_set_option and the kemr_debug_set switches are
 *        host state read when a call is made: change them between calls, not beside them.
 *      - calls that synchronise the host, because their contract needs a host value or a quiet device: kemr_model_finalize
 *        (waits for the device, then uploads the packed weights with a blocking copy), kemr_model_destroy (frees the weights: the
 *        free waits for the device; no call that reads the handle may be pending anyway), kemr_profile_end (returns the measured
 *        times), kemr_debug_sim_lists and kemr_debug_gemm_stamps (kemr_debug.h: return what finished calls left behind); one level
 *        up, ClipEngine.encode_text with token ids on the device and no `lens` (one copy of B lengths to the host sizes the packed
 *        launches).  No other entry point waits for the device.  The event profiler (kemr_profile_begin / _end) keeps one
 *        process-wide record: profile one stream at a time.
 *      - capturing calls into a HIP graph is not part of this contract and is not tested.
 *  - no HIP call happens at library load time (fork-safe for DataLoader workers,
 *    reference: src/clip/eval/evaluator_baseline.py:83-92).
 */
#ifndef KEMR_H_
#define KEMR_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: kemr_sim_workspace_bytes takes kdim, panels are allocated with ceil256(rows) rows (kemr_panel_build zero-fills up to
 *    256), kemr_model_set_option / kemr_model_get_option, the tools' switches live in kemr_debug.h (kemr_debug_set).
 * 3: kemr_encode_text_packed / kemr_text_packed_workspace_bytes, option "last_block_pooled_row"; kemr_workspace_bytes grows by the
 *    last block's pooled-row area (callers that size their workspace with it need no change).
 * 4: the same entry points with changed defaults and semantics: option "residual_stream_24bit" defaults to 1; the fp8 precisions apply
 *    to the vision tower only and scale the e4m3 A operand per channel; kemr_preprocess_u8_batch accepts 0 x 0 items (an undecodable
 *    image: zeros after normalisation); kemr_debug_set refuses the experiment kernels the library was built without.
 *    Still 4: kemr_select_topk, kemr_sim_topk_deep, kemr_sim_topk_deep_workspace_bytes and kemr_sim_topk_deep_fused are additions, no
 *    existing entry point changed.  Option "activation" of kemr_model_set_option / kemr_model_get_option and the epilogue value
 *    KEMR_EPI_BIAS_GELU_BF16 (kemr_op_gemm, kemr_op_gemm_fp8) are additions as well: the default, 0, is the QuickGELU every existing
 *    caller gets; no entry point was added.  Still 4: option "vision_head_dim" (64, the default every existing caller gets, or 80: the
 *    vision tower of ViT-H-14) and the entry points kemr_op_attention_hd / kemr_op_attention_x3_hd are additions; kemr_cfg did not grow.
 *    Still 4: option "family" (0 = CLIP, the default every existing caller gets; 1 = SigLIP) and the epilogue value
 *    KEMR_EPI_BIAS_TGELU_BF16 (kemr_op_gemm) are additions; no entry point changed, kemr_cfg did not grow.
 *    Still 4: kemr_transform_workspace_bytes, kemr_transform_u8, kemr_transform_batch_workspace_bytes and kemr_transform_u8_batch (the
 *    image transform with its kind as an argument: CLIP's or the SigLIP family's) are additions; the four kemr_preprocess_* entry points
 *    keep their signatures and bits (they are the new ones at KEMR_TRANSFORM_CLIP).
 *    Still 4: kemr_model_create_family, model family 2 (BERT sentence encoders) behind it, KEMR_MAX_BERT_CTX and option "pooling" are
 *    additions; kemr_model_create, option "family" (0 / 1) and every existing entry point keep their behaviour and messages -- what
 *    they refuse for a family-2 model, no existing caller could reach.  kemr_cfg did not grow.
 *    Still 4: model family 3 (MPNet sentence encoders: a family-2 model under option "family" = 3, with a relative position bias in
 *    every attention score) and option "layer_norm_eps" (family 3 only) are additions; kemr_model_create_family keeps refusing 3; families 0 - 2 keep their tensors, arithmetic and
 *    messages, and no entry point changed.
 *    Still 4: kemr_op_attention_backward (the backward of kemr_op_attention, heads of 64, t <= KEMR_MAX_TEXT_CTX) is an addition; the
 *    forward kernels did not change and save nothing for it.
 *    Still 4: kemr_layernorm_backward_workspace_bytes, kemr_op_layernorm_backward (the backward of kemr_op_layernorm), kemr_op_act_forward
 *    and kemr_op_act_backward (the MLP activation on bf16) are additions; no existing entry point changed.
 *    Still 4: kemr_attention_backward_long_workspace_bytes and kemr_op_attention_backward_long (the non-causal backward of
 *    kemr_op_attention for t <= KEMR_MAX_VISION_TOKENS, streaming, with a small workspace) are additions; kemr_op_attention_backward
 *    keeps its signature, refusals, messages and bits.
 *    Still 4: kemr_op_attention_packed (the causal forward over items of different lengths packed one behind the other, what the text
 *    encoders run inside themselves) and kemr_op_attention_backward_packed (its backward, and the non-causal one, for items of up to
 *    KEMR_MAX_TEXT_CTX rows) are additions; the dense ops keep their signatures, refusals, messages and bits.
 *    Still 4: kemr_attention_backward_hd_workspace_bytes and kemr_op_attention_backward_hd (the attention backward with the head dim as
 *    an argument: heads of 80, non-causal, streaming; at 64 the existing ops) are additions; kemr_op_attention_backward,
 *    kemr_op_attention_backward_long and kemr_op_attention_hd keep their signatures, refusals, messages and bits. */
#define KEMR_ABI_VERSION 4

typedef enum kemr_status {
    KEMR_OK = 0,
    KEMR_ERR_INVALID = -1,      /* bad argument / shape the kernels do not support */
    KEMR_ERR_STATE = -2,        /* call order (e.g. encode before finalize, missing tensor) */
    KEMR_ERR_HIP = -3,          /* a HIP runtime call failed; message carries hipGetErrorString */
    KEMR_ERR_WORKSPACE = -4,    /* workspace too small / misaligned */
    KEMR_ERR_NOMEM = -5
} kemr_status;

typedef enum kemr_dtype { KEMR_F32 = 0, KEMR_BF16 = 1, KEMR_I32 = 2, KEMR_FP8 = 3 /* OCP e4m3fn */ } kemr_dtype;

/* compute precision of the encoder GEMMs (activations + weights); accumulation is always fp32 */
/* KEMR_PREC_BF16:       the default.  bf16 GEMM / attention operands, fp32 accumulation, fp32 residual stream (closest to the
 *                       reference's .float() model); the out-proj / fc2 updates are stored as bf16 and added in fp32 by the
 *                       LayerNorms (option "residual_fusion" = 2 adds them in the GEMM epilogues without rounding them).
 * KEMR_PREC_BF16_RES16: as above with the residual stream stored as bf16 between layers (what fp16/bf16 CLIP inference
 *                       does everywhere); LayerNorm statistics and the residual add stay fp32.  8 instead of 12 bytes
 *                       of HBM traffic per residual element and LayerNorm, and 16 instead of 18 workspace bytes.
 *                       For calls of more than 512 token rows the residual add runs inside the out-proj / fc2 GEMM epilogues
 *                       unless the environment holds KEMR_RESADD=0 (x is then rounded once per layer instead of twice, -3.7 %).
 * KEMR_PREC_FP8:        BASELINE config 5.  The QKV GEMMs of the VISION tower (22 % of a gallery item's FLOPs) run on fp8 e4m3
 *                       operands with the block-scaled MFMA (K = 128 per instruction, twice the bf16 rate): ln_1 writes its
 *                       output as e4m3 -- its gain moved out of the values by per-channel power-of-two scales that finalize folds
 *                       into gamma / beta and into the weight columns, so that a trained tower's gains of 30-100 do not saturate
 *                       at +-448 (round 4) --, the weights are quantised per output channel at finalize, the scale is applied
 *                       to the fp32 accumulators.  The text tower (one pooled row behind a causal softmax: e4m3 q / k / v cost
 *                       it 1 - cos 1.4e-3 .. 5e-3, over the path's 1e-3 bar) and everything else stay as KEMR_PREC_BF16.
 *                       Recall@10 stays within 0.2 points of bf16 (tests/test_encoder_gpu.py).  Vision width: multiple of 128.
 * KEMR_PREC_FP8_MLP:    the fc1 GEMMs as well (56 % of the FLOPs in fp8, +25 % encode throughput); on the synthetic
 *                       near-duplicate retrieval test this costs about one point of Recall@10 where bf16 is below 90 %
 *                       (the MLP update goes straight into the residual stream, the QKV error is averaged by the softmax),
 *                       so it is outside config 5's bar and opt-in.
 * KEMR_PREC_FP8_RES16:  KEMR_PREC_FP8 with the bf16 residual stream of KEMR_PREC_BF16_RES16 (the two savings add).
 * KEMR_PREC_FP32X3:     the fp32-grade mode ("fp32x3"): what the reference's `.float()` model computes, for practical purposes, at a
 *                       quarter to a third of the default's rate -- for evaluation runs, for validating a faster precision on one's
 *                       own checkpoint (python: engine.precision_gap), and for towers the bf16 class cannot hold to the 1e-3 bar
 *                       (uncompensated LayerNorm gains of 30-100).  Numerical contract:
 *                       - every GEMM operand, activation and weight, enters v_mfma_f32_16x16x32_bf16 as the pair hi = rne_bf16(a),
 *                         lo = rne_bf16(a - hi); every product is hi.hi + lo.hi + hi.lo with fp32 accumulation -- the convention
 *                         of the terms == 3 similarity panels: the A side is [hi | lo | hi], the W side [hi | hi | lo], both
 *                         concatenated along k, so K becomes 3K (finalize packs every matrix as [N, 3K], conv1 over 3 kpad);
 *                       - nothing between kernels is stored below fp32 except as such a pair: the residual stream is plain 4-byte
 *                         fp32 (option "residual_stream_24bit" has no effect; its stored value is still what get_option returns),
 *                         q | k | v are fp32, the LayerNorm outputs, the attention output and the MLP hidden are A-side triples;
 *                       - the out-proj and fc2 epilogues add acc + bias into the stream in fp32 (option "residual_fusion" has no
 *                         meaning here); the attention scale 1/8 stays folded into W_q and b_q (exact; at "vision_head_dim" 80 the
 *                         vision tower's 1/sqrt(80) is applied in fp32 before the split);
 *                       - attention splits Q, K, V and P into pairs and contracts with the same three products; LayerNorm
 *                         statistics, softmax, QuickGELU and the erfc-form GELU are fp32 arithmetic as in every mode; option
 *                         "activation" works as in every mode;
 *                       - option "last_block_pooled_row" is ignored: every row runs through every block, as the reference does;
 *                       - every GEMM runs on one kernel family (the 128 x 128 tile kernel), whatever the shape; fp8 is not involved.
 *                       Workspace: 46 instead of 18 bytes per token row and width element (kemr_workspace_bytes knows). */
typedef enum kemr_precision { KEMR_PREC_BF16 = 1, KEMR_PREC_BF16_RES16 = 2, KEMR_PREC_FP8 = 3, KEMR_PREC_FP8_MLP = 4, KEMR_PREC_FP8_RES16 = 5,
                              KEMR_PREC_FP32X3 = 6 } kemr_precision;

typedef enum kemr_tower { KEMR_TOWER_VISION = 0, KEMR_TOWER_TEXT = 1 } kemr_tower;

/* Longest sequences the encoders take: vision (image_size / patch)^2 + 1 tokens up to KEMR_MAX_VISION_TOKENS (a 32 x 32 patch
 * grid: ViT-L/14 at 448 px; ViT-L/14@336px has 577), the text context up to KEMR_MAX_TEXT_CTX (causal attention, 77 in CLIP, 248 in Long-CLIP).
 * Non-causal sequences of more than 288 tokens run on the streaming (flash-form) attention kernel, shorter ones on the
 * whole-sequence-in-LDS kernel; packed causal texts (kemr_encode_text_packed) of more than 128 positions on the streaming kernel's
 * causal form. */
#define KEMR_MAX_VISION_TOKENS 1025
#define KEMR_MAX_TEXT_CTX 288
/* families 2 and 3 (BERT and MPNet sentence encoders): the longest text, absolute positions 0 .. 511 (non-causal attention over packed
 * items of different lengths, csrc/attention_stream.hip; family 3's relative position bias spans the distances -511 .. 511) */
#define KEMR_MAX_BERT_CTX 512

/* Architecture numbers of an OpenAI-CLIP style model (MLP is 4*width; heads are width/64, except a vision tower under option
 * "vision_head_dim" = 80, whose heads are v_width/80: OpenCLIP's ViT-H-14 {1024,224,14,1280,32,1024,24,49408,77}).
 * ViT-L/14: {768,224,14,1024,24,768,12,49408,77}; ViT-L/14@336px: {768,336,14,1024,24,768,12,49408,77};
 * ViT-B/32: {512,224,32,768,12,512,12,49408,77}.
 * The SigLIP family (model option "family" = 1) reads the same nine numbers: embed_dim must equal v_width (the image embedding is the
 * pooling head's row, there is no vision projection), the vision tower has (image_size / patch)^2 tokens (no class token), vocab and ctx
 * are the model's (32000 / 64).  ViT-B-16-SigLIP: {768,224,16,768,12,768,12,32000,64}; ViT-L-16-SigLIP-384: {1024,384,16,1024,24,1024,24,32000,64}. */
typedef struct kemr_cfg {
    int32_t embed_dim;    /* joint embedding size D */
    int32_t image_size;   /* input resolution (square) */
    int32_t patch;        /* patch size, image_size % patch == 0 */
    int32_t v_width;      /* vision width, multiple of 256 */
    int32_t v_layers;
    int32_t t_width;      /* text width, multiple of 256 */
    int32_t t_layers;
    int32_t vocab;
    int32_t ctx;          /* text context length (77) */
} kemr_cfg;

typedef struct kemr_model kemr_model;

const char* kemr_last_error(void);
int kemr_abi_version(void);

/* ---------------------------------------------------------------------------------------------
 * Model lifecycle.  Replaces `clip.load(name, device)` + `.float()` + `load_state_dict(sd,
 * strict=True)` (reference: src/clip/model/clip_model.py:41-64).
 *   create -> load_tensor (once per state-dict entry, OpenAI-CLIP names, fp32 host memory)
 *          -> finalize (checks every required tensor is present = "strict", packs bf16 weights
 *             into device memory: the q-scale 1/sqrt(head dim) folded into W_q and b_q in fp32 before the rounding -- 1/8 for
 *             heads of 64, exact --, conv1 flattened/padded to a GEMM panel)
 *   load_tensor may be called again after finalize (fine-tuned checkpoint): call finalize again.
 * ------------------------------------------------------------------------------------------- */
int kemr_model_create(const kemr_cfg* cfg, kemr_model** out);
/* The same with the model family decided AT creation (the configuration checks depend on it): 0 and 1 are kemr_model_create followed by
 * kemr_model_set_option("family", family), exactly; 2 = a BERT sentence encoder -- transformers.BertModel without its pooler, then mean
 * or CLS pooling: intfloat/e5-base-v2 {768,0,0,0,0,768,12,30522,512}, thenlper/gte-large {1024,0,0,0,0,1024,24,30522,512} (the
 * reference's text-to-text baselines, src/clip/eval/evaluator_lm.py, baselines/evaluate_text_models.py).
 * Family 2 is text-only: image_size, patch, v_width and v_layers must be 0, embed_dim == t_width (no projection), t_width in
 * {256, 512, 768, 1024, 1280} with heads of 64 and a 4 x MLP, ctx <= KEMR_MAX_BERT_CTX.
 * Tensors (fp32, strict): token_embedding.weight [vocab, W] (word_embeddings), positional_embedding [ctx, W] (position_embeddings),
 *   token_type_embedding [2, W], ln_embed.{weight,bias} (embeddings.LayerNorm); per block transformer.resblocks.i.: attn.in_proj_weight
 *   [3W, W] / attn.in_proj_bias (query | key | value stacked), attn.out_proj.{weight,bias} (attention.output.dense), ln_1.{weight,bias}
 *   (attention.output.LayerNorm), mlp.c_fc.* (intermediate.dense), mlp.c_proj.* (output.dense), ln_2.{weight,bias} (output.LayerNorm).
 * Finalize folds 1/8 into the query rows as everywhere and adds token_type_embedding[0] to the positional table in fp32 (every token
 *   is of type 0).  Refused for family 2 with the reason in the message: the fp8 precisions and KEMR_PREC_FP32X3.
 * What the encoder computes (kemr_encode_text_packed, the only encode call of this family; kemr_encode_text -- a padding mask is a
 *   length -- and kemr_encode_image are refused, kemr_workspace_bytes is 0): per packed row x = LayerNorm(tok[id] + pos'[p]); per block
 *   (post-LN) q | k | v = h W^T + b, non-causal attention among the item's own rows, x = LayerNorm(x + out_proj(a)), x = LayerNorm(x +
 *   fc2(gelu(fc1(x)))) with the exact GELU; every LayerNorm with eps 1e-12; h, the GEMM operand, is bf16(x); the stream x is stored in
 *   the precision's type (24-bit / fp32 / bf16).  out[i] = the mean of item i's lens[i] final rows, summed in fp32 (option "pooling" 0,
 *   the default: sentence-transformers' masked mean pooling) or its first row (option "pooling" 1: CLS, as BGE uses), L2-normalised when
 *   normalize != 0.  Options "residual_fusion", "last_block_pooled_row", "activation" and "vision_head_dim" are not consulted;
 *   kemr_model_set_option("family", 2) is refused with a message naming this entry point.  A length that cuts a text short encodes the
 *   shorter text.  Workspace: kemr_text_packed_workspace_bytes (16, 17 or 18 bytes per allocated row and width element -- bf16, 24-bit or fp32
 *   stream -- + the row starts; no pooled-row area), the
 *   memory contract of the encoders below.
 * Family 3 = an MPNet sentence encoder, reached from a family-2 model: kemr_model_create_family(cfg, 2, &m), then
 * kemr_model_set_option(m, "family", 3) before the first kemr_model_load_tensor (2 <-> 3 share the configuration checks and differ in the
 * tensor list, as 0 <-> 1 do behind kemr_model_create; passing 3 to kemr_model_create_family itself is refused, as it always was, with a
 * message naming the option) -- transformers.MPNetModel without its pooler, then mean or CLS pooling:
 * sentence-transformers/all-mpnet-base-v2 {768,0,0,0,0,768,12,30527,512} (the third sentence encoder of the reference's text-to-text
 * baselines).  Everything said of family 2 holds -- the configuration checks, the packed call as the only encode call, the post-LN
 * blocks with the exact GELU, pooling, workspace, and every refusal with family 2's wording (the fp8 precisions, KEMR_PREC_FP32X3,
 * kemr_encode_text, kemr_encode_image, options "family" and "vision_head_dim") -- with these differences:
 *   Tensors: no token_type_embedding (MPNet has no token types; positional_embedding [ctx, W] is taken verbatim -- position j of a text
 *   reads row j, so the caller passes rows 2 .. 2 + ctx - 1 of MPNet's position_embeddings, whose position ids start at padding_idx + 1
 *   = 2); in addition relative_attention_bias [32, W / 64] (encoder.relative_attention_bias.weight: ONE table for all layers); the
 *   blocks' names are family 2's (attn.q | k | v stacked into in_proj, attn.o = out_proj, attention.LayerNorm = ln_1).
 *   Scores: q . k^T / 8 + bias[h][bucket(key - query)] before the softmax, in every layer.  bucket = MPNetEncoder's
 *   relative_position_bucket at 32 buckets and max distance 128, by integer thresholds: with n = query - key, 16 is added when n < 0;
 *   |n| < 8 is bucket |n|; buckets 8 .. 15 begin at |n| = 8, 12, 16, 23, 32, 46, 64, 91.  Finalize expands the 32 buckets once into a
 *   device table by distance, fp32 [heads, 1023], that the attention kernel stages per head into LDS and reads as the start value of its
 *   score accumulators (fp32, unscaled, no rounding of the bias; csrc/attention_stream.hip).
 *   LayerNorm eps: option "layer_norm_eps" below, 1e-5 by default.
 *   A text's token j sits at position j: what MPNetModel computes whenever no <pad> id occurs inside a text's length. */
int kemr_model_create_family(const kemr_cfg* cfg, int family, kemr_model** out);
int kemr_model_load_tensor(kemr_model* m, const char* name, const void* host_ptr, int dtype /*kemr_dtype, F32 only*/,
                           const int64_t* shape, int rank);
int kemr_model_finalize(kemr_model* m, int precision /*kemr_precision*/);
int kemr_model_destroy(kemr_model* m);
/* Per-model options (any time after create; take effect on the next encode call of this model, no other model is touched):
 *   "residual_fusion"  calls of more than 512 token rows add the residual inside the out-proj / fc2 GEMM epilogues instead of
 *                      storing bf16 updates that the LayerNorms apply: 0 never; 1 (default; KEMR_RESADD in the environment at
 *                      create overrides) for bf16 residual streams (x is then rounded twice per layer instead of once); 2 for
 *                      fp32 residual streams as well (x += A.W^T + b in fp32, no update is rounded at all; slower).
 *   "last_block_pooled_row"  1 (default; KEMR_LAST_BLOCK_FULL=1 in the environment at create makes it 0): one row per item leaves
 *                      a tower -- the class token's (`ln_post(x[:, 0, :]) @ proj`) or the end-of-text token's -- so the LAST
 *                      block computes K and V for every row but the query, attention output, out-proj, ln_2 and MLP for that
 *                      row alone (2 instead of 12 W^2 of GEMM work per token row in that block).  The pooled rows see the same
 *                      arithmetic in smaller launches.  Applies with store-only epilogues and fc1 on bf16 (not KEMR_PREC_FP8_MLP); 0 = every row
 *                      through every block, as the reference computes it.
 *   "residual_stream_24bit"  (set BEFORE kemr_model_finalize; default 1 since round 4, KEMR_STREAM24=0 in the environment at create
 *                      makes it 0): the fp32 residual stream of KEMR_PREC_BF16 / FP8 / FP8_MLP is stored as 24-bit floats -- the
 *                      upper three bytes of the fp32, rounded to nearest: 15 mantissa bits, 128 x finer than bf16 -- 3 instead of
 *                      4 bytes per element in the HBM-bound LayerNorm passes (+2 % on the ViT-L/14 step); every statistic and add
 *                      stays fp32 arithmetic.  The default because it meets every bar the 4-byte stream meets (1 - cos against the
 *                      fp32 oracle on plain and heavy-tailed weights, the fixed 0.2-point Recall@10 bar on ViT-B/32 and ViT-L/14,
 *                      the end-to-end margin rule: DESIGN.md section 2); 0 = the 4-byte stream (python: precision "bf16").
 *   "activation"       the MLP's activation between fc1 and fc2, in both towers: 0 (default) QuickGELU x sigmoid(1.702 x), what the
 *                      OpenAI checkpoints were trained with; 1 exact GELU 0.5 x (1 + erf(x / sqrt 2)) = torch.nn.GELU(), what the
 *                      OpenCLIP / LAION ViT-B/32, B/16 and L/14 checkpoints and Hugging Face configs with hidden_act "gelu" use.
 *                      It selects the epilogue of the fc1 GEMMs (bf16 and fp8 operands, the pooled-row last block) and nothing
 *                      else; the weights are not touched, so it may be flipped between encode calls without a finalize.
 *   "vision_head_dim"  (set BEFORE kemr_model_finalize) the head dim of the VISION tower: 64 (default) or 80, which needs v_width % 80 == 0
 *                      (1280 = 16 heads of 80: OpenCLIP / LAION ViT-H-14; the text tower keeps heads of 64).  Finalize then folds
 *                      1/sqrt(80) instead of 1/8 into the vision tower's query rows and the encoders run the head-dim-80 attention
 *                      kernels (csrc/attention80.hip).  Refused at finalize with 80: the fp8 precisions, and vision towers of more than
 *                      288 tokens (the streaming attention kernel serves heads of 64 only).  Not served at all: ViT-g / bigG (head dim
 *                      88 / widths that are no multiple of 256, MLP not 4 x width).
 *   "family"           (set BEFORE the first kemr_model_load_tensor: it rebuilds the list of required tensor names) 0 = CLIP (default),
 *                      1 = SigLIP (ViT-B/16, ViT-L/16; transformers.SiglipModel).  The names are the OpenAI-style ones wherever the tensor
 *                      exists in both models; in addition visual.conv1.bias, visual.positional_embedding [patches, W] (no class row),
 *                      visual.attn_pool.{probe [W], in_proj_weight, in_proj_bias, out_proj.weight, out_proj.bias, ln.weight, ln.bias,
 *                      mlp.c_fc.*, mlp.c_proj.*}, text_projection [t_width, D] with text_projection_bias [D]; no visual.class_embedding,
 *                      visual.ln_pre.* or visual.proj; logit_bias is ignored like logit_scale.  What the encoders then do differently:
 *                      the patch GEMM's epilogue writes x[m] = acc + pos[m % patches] + bias with no class rows and no ln_pre; every
 *                      LayerNorm uses eps 1e-6; fc1 runs the tanh-GELU epilogue (option "activation" keeps its range and messages and is
 *                      not consulted); the image embedding is the attention-pooling head over ln_post of ALL tokens (one learned query,
 *                      then r + mlp(ln(r))), so option "last_block_pooled_row" is ignored by the vision tower; the text tower has no
 *                      mask, pools position ctx - 1 whatever the ids (its last block honours "last_block_pooled_row") and its head adds
 *                      text_projection_bias.  Refused for family 1 with the reason in the message: at finalize embed_dim != v_width,
 *                      the fp8 precisions, KEMR_PREC_FP32X3 and "vision_head_dim" != 64; kemr_encode_text_packed (a pad position is a
 *                      key and the pooled row is the last one, so no row can be left out).  The family's pixels are those of its own
 *                      image transform (squash to S x S, mean = std = 0.5): KEMR_TRANSFORM_SIGLIP of kemr_transform_u8 /
 *                      kemr_transform_u8_batch below computes them on the device; the option itself does not touch the input side.
 *                      For a kemr_model_create model 2 (BERT) and 3 (MPNet) are refused here: kemr_model_create_family.  For a model
 *                      created as family 2: 2 (BERT) or 3 (MPNet: see kemr_model_create_family), likewise before the first load; 0 and 1
 *                      are refused.
 *   "pooling"          (families 2 and 3 only; any time) 0 = mean over the item's rows (default), 1 = the item's first row (CLS).
 *   "layer_norm_eps"   (family 3 only; set BEFORE kemr_model_finalize) the epsilon of every LayerNorm as its negative decimal exponent:
 *                      5 = 1e-5 (default: what the published all-mpnet-base-v2 config holds), 12 = 1e-12 (MPNetConfig's own default).
 *                      Any other value is refused, and so is the key for families 0 - 2 (set and get). */
int kemr_model_set_option(kemr_model* m, const char* key, int value);
int kemr_model_get_option(const kemr_model* m, const char* key, int* value);
/* number of required tensor names; name i via kemr_model_tensor_name (for strict-load diagnostics) */
int kemr_model_num_tensors(const kemr_model* m);
const char* kemr_model_tensor_name(const kemr_model* m, int i);

/* ---------------------------------------------------------------------------------------------
 * Encoders.  Replace `model.encode_image(images)` / `model.encode_text(tokens)` and the following
 * `x / x.norm(dim=-1, keepdim=True)` (reference: src/clip/eval/evaluator_baseline.py:107-108,
 * 113-114, 119-120; src/clip/eval/evaluator.py:121-122, 127-128, 133-134;
 * src/clip/model/fusion_model.py:287-303).
 *   pixels_dev : fp32 [B,3,S,S] contiguous NCHW, already mean/std normalised
 *   ids_dev    : int32 [B,ctx]; pooled at the first position of the row maximum (EOT); family 1: at position ctx - 1
 *   out_dev    : fp32 [B, embed_dim]; L2-normalised when normalize != 0
 *   workspace  : >= kemr_workspace_bytes(m, tower, B) bytes, 256-byte aligned, contents don't matter
 * Memory contract (tests/test_footprint_towers_gpu.py): exactly kemr_workspace_bytes is enough -- nothing before the workspace's first
 * or behind its last byte is written or can reach `out`; every workspace byte a result depends on is written by the call first (stale
 * bytes of an earlier call of another batch size or layout, NaN included, cannot reach `out`); exactly B * embed_dim floats of `out`
 * are written; nothing outside the B items of pixels / ids can reach them.  A workspace that is too small or not 256-byte aligned is
 * KEMR_ERR_WORKSPACE BEFORE anything is launched: `out` and the workspace keep their bytes.
 * ------------------------------------------------------------------------------------------- */
size_t kemr_workspace_bytes(const kemr_model* m, int tower /*kemr_tower*/, int batch);
int kemr_encode_image(kemr_model* m, const float* pixels_dev, int batch, float* out_dev, int normalize,
                      void* workspace_dev, size_t workspace_bytes, void* stream);
int kemr_encode_text(kemr_model* m, const int32_t* ids_dev, int batch, float* out_dev, int normalize,
                     void* workspace_dev, size_t workspace_bytes, void* stream);

/* The same text embeddings from the rows that can reach them.  The text transformer's mask is causal and the pooled row is the
 * end-of-text token's (reference: `x[torch.arange(x.shape[0]), text.argmax(dim=-1)] @ self.text_projection` behind the masked
 * transformer in the CLIP model `clip.load` returns; call sites as above), so positions behind that token cannot influence the
 * output: text i is computed on its first lens[i] positions only, all texts packed one behind the other (`rows` = sum of lens
 * token rows instead of B * ctx in every launch).  With lens[i] >= argmax_i + 1 the result is kemr_encode_text's up to the fp32
 * summation order of the GEMM kernel a launch of that many rows is routed to -- what another batch size changes as well.
 *   lens_dev : int32 [B] on the device, each in 1 .. ctx (clamped on the device)
 *   rows     : HOST integer, the sum of lens (the tokenizer's side knows it; B <= rows <= B * ctx is checked, and the device
 *              clamps the prefix sums into it, so no argument can make a kernel index outside the workspace)
 *   workspace: >= kemr_text_packed_workspace_bytes(m, rows, B) bytes (exactly that is enough; the memory contract of the encoders above)
 * A length shorter than argmax_i + 1 pools text i's last computed row (memory-safe, not the reference's embedding).
 * Served for family 0 at every ctx <= KEMR_MAX_TEXT_CTX (Long-CLIP's 248 positions included) in the bf16-operand and the fp8 precisions
 * (whose text tower is bf16): texts of up to 128 positions run the tile attention kernels, longer contexts the causal streaming
 * kernel (csrc/attention_stream.hip), both one launch over all packed texts.  A KEMR_PREC_FP32X3 model is served packed up to ctx =
 * 128 only: above, this call and kemr_encode_text_packed_pooled return KEMR_ERR_INVALID and kemr_encode_text is the call to make. */
size_t kemr_text_packed_workspace_bytes(const kemr_model* m, int rows, int batch);
int kemr_encode_text_packed(kemr_model* m, const int32_t* ids_dev, const int32_t* lens_dev, int rows, int batch, float* out_dev,
                            int normalize, void* workspace_dev, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Similarity + ranking.  Replaces `S = Q @ C.T`, the weighted T2I/T2T sum, and the two full
 * `np.argsort(-S)` passes of Recall@K / MRR (reference: src/clip/eval/metrics.py:13-76, 102,
 * 145-148; src/clip/eval/fusion.py:6-20) without materialising the Q x N matrix.
 *
 * Operands are "panels": bf16 [rows, kdim] row-major with kdim % 64 == 0, built by
 * kemr_panel_build from fp32 embeddings.  A panel concatenates `nparts` embedding sets along k
 * (fused T2I+T2T scoring = one contraction over [w_i*I ; w_t*T], metrics.py:148) and, with
 * terms == 3, stores the bf16 split hi/lo so that the contraction reproduces fp32 products
 * (query panel [hi | lo | hi], gallery panel [hi | hi | lo]); terms == 1 is plain bf16.
 *   kdim = nparts * terms * ceil64(D)
 * A panel buffer must be allocated with its row count rounded up to a multiple of 256
 * (kemr_panel_build zero-fills the pad rows; the kernels read whole 128- and 256-row tiles).
 * ------------------------------------------------------------------------------------------- */
typedef enum kemr_panel_side { KEMR_SIDE_QUERY = 0, KEMR_SIDE_GALLERY = 1 } kemr_panel_side;

int64_t kemr_panel_kdim(int d, int nparts, int terms);
/* parts[p] : fp32 [rows, d] dev pointers (nparts of them, host array of pointers);
 * part_scale[p] : scalar weight applied to part p (NULL = 1); row_scale[p] : optional fp32 [rows]
 * dev pointer with a per-row factor for part p (per-query gate, fusion_model.py:136-196), or NULL. */
int kemr_panel_build(const float* const* parts_dev, const float* part_scale, const float* const* row_scale_dev,
                     int nparts, int rows, int d, int terms, int side /*kemr_panel_side*/,
                     void* panel_dev /* bf16 [rows, kdim] */, void* stream);

/* Fused score + per-query top-k + rank of a ground-truth candidate.
 *   q_panel [nq,kdim], g_panel [ng,kdim]
 *   gallery_offset : global id of gallery row 0 (sharded galleries); ids written are global
 *   k <= 32; top_scores/top_idx [nq,k] sorted (score desc, id asc), padded with -inf / -1;
 *   k == 0 = rank only (top_* may be NULL, the ground truth is then required); without a bonus list this is the fast
 *            256 x 256-tile pass on the encoder GEMM's main loop (same scores, bit for bit)
 *   gt_idx  : optional int32 [nq] GLOBAL candidate id of each query's ground truth
 *   gt_score: optional fp32 [nq]; score of (query, gt) as produced by kemr_pair_scores
 *   ahead   : optional int32 [nq]; += #{j in this gallery : s_ij > s_gt or (s_ij == s_gt and id_j < gt)}
 *             (rank = 1 + sum of `ahead` over shards; caller zeroes it)
 *   bonus_*: optional sparse additive bonuses (SPARQL hits, eval/fusion.py:22-206) in CSR over
 *            queries: bonus_rowptr int32 [nq+1], bonus_col int32 (GLOBAL ids, ascending within a row),
 *            bonus_val fp32.  Weighted fusion's alpha is folded into the query panel (part_scale).
 *   Galleries of >= 8192 rows with >= 256 queries and no bonus list take their scores from the encoder GEMM's main loop as
 *   well: thresholds from the block maxima of a strided sample of the gallery (about a tenth of the rows at k = 10), one 256 x 256-tile pass that appends the
 *   candidates above a query's threshold to its lists (the rank count rides along), one selection pass.  Same scores, same
 *   order rule, same outputs bit for bit; lists that overflow re-run the slower kernel on the device (no host round trip).
 *   workspace >= kemr_sim_workspace_bytes(nq, ng, kdim, k), 256-byte aligned; exactly that is enough and its contents don't matter (every
 *   byte a result depends on is written by the call first).  Written: top_scores / top_idx [nq, k] wholly, ahead [nq] (accumulated);
 *   nothing else -- the panels, the ground truth and the CSR arrays are only read, inside their sizes.  The panels' pad rows up to
 *   ceil256 are read as parts of whole tiles, but their contents cannot reach a listed score, an id or a rank (kemr_sim_topk_deep*,
 *   kemr_scores_dense likewise) */
size_t kemr_sim_workspace_bytes(int nq, int ng, int64_t kdim, int k);
int kemr_sim_topk(const void* q_panel_dev, int nq, const void* g_panel_dev, int ng, int64_t kdim,
                  int64_t gallery_offset, int k, float* top_scores_dev, int32_t* top_idx_dev,
                  const int32_t* gt_idx_dev, const float* gt_score_dev, int32_t* ahead_dev,
                  const int32_t* bonus_rowptr_dev, const int32_t* bonus_col_dev, const float* bonus_val_dev,
                  void* workspace_dev, size_t workspace_bytes, void* stream);

/* score of listed (query row, LOCAL gallery row) pairs with exactly the arithmetic of kemr_sim_topk
 * (same MFMA k-order), so that `s_ij > s_gt` comparisons are self-consistent. out fp32 [npairs]. */
int kemr_pair_scores(const void* q_panel_dev, const void* g_panel_dev, int64_t kdim,
                     const int32_t* q_rows_dev, const int32_t* g_rows_dev, int npairs,
                     float* out_dev, void* stream);

/* Merge `nlists` sorted top-k lists per query (shards / column chunks) into one.
 * in_scores/in_idx [nq, nlists, k] -> out [nq, k]; same order rule as kemr_sim_topk. */
int kemr_topk_merge(const float* in_scores_dev, const int32_t* in_idx_dev, int nq, int nlists, int k,
                    float* out_scores_dev, int32_t* out_idx_dev, void* stream);

/* Dense score tile (for the learned fusion heads that are not GEMM epilogues and for debugging):
 * out fp32 [nq, ng] row-major = q_panel . g_panel^T with a row stride of ld_out >= ng floats (rows need no alignment): columns
 * ng .. ld_out - 1 are not written.  Reference: fusion_model.py:324-325. */
int kemr_scores_dense(const void* q_panel_dev, int nq, const void* g_panel_dev, int ng, int64_t kdim,
                      float* out_dev, int64_t ld_out, void* stream);

/* Rank an already materialised score matrix (fp32 [nq, ld], device): for every row the number of
 * candidates ranked ahead of column gt_idx[row] (written, not accumulated) and/or the sorted top-k.
 * Replaces the np.argsort passes when the caller hands over a matrix: compute_recall_at_k,
 * compute_mrr_and_mean_rank (metrics.py:13-76), compute_retrieval_metrics_fusion (metrics.py:165-185),
 * evaluate_retrieval (eval/fusion.py:6-20), evaluator_fusion.py:126.  Either output pair may be NULL.
 * scores_dev may be a row-strided view (ld >= ng; rows need no alignment); columns ng .. ld - 1 are never read.  A gt_idx outside
 * 0 .. ng - 1 writes ahead = 0.  Lists are padded with -inf / -1 where a row has fewer than k listable candidates.
 *
 * -inf and NaN scores on the k <= 32 routes (kemr_rank_dense, kemr_sim_topk, and through it the lists kemr_topk_merge is fed):
 * -inf is the PAD VALUE of the register-resident lists, and a candidate enters a list only if its score is greater than the
 * list's last entry, so a candidate whose score is -inf or NaN is NEVER LISTED -- the lists hold the candidates with a score
 * above -inf in order, then padding.  `ahead` still counts by the order rule on the raw scores (a -inf or NaN candidate is never
 * ahead of a finite ground truth).  The deep routes (kemr_select_topk, kemr_sim_topk_deep*) differ: they list every candidate with
 * an id >= 0, -inf ones behind the finite ones and NaN behind -inf.  kemr_topk_merge itself tells padding by the id (< 0), not by
 * the score: an entry (-inf, id >= 0) handed to it IS listed, behind the finite entries in id order; kemr_sim_topk never produces
 * one.  A NaN entry is not supported by kemr_topk_merge (where it lands depends on its position in the input).
 * The rule itself, its two forms and where they differ: csrc/rank_order.h. */
int kemr_rank_dense(const float* scores_dev, int nq, int ng, int64_t ld, const int32_t* gt_idx_dev,
                    int32_t* ahead_dev, int k, float* top_scores_dev, int32_t* top_idx_dev, void* stream);

/* kemr_rank_dense for ONE SHARD's columns of a score matrix whose ground truth may live on another shard (additive in ABI 4; the
 * dense learned heads over a gallery sharded across GPUs).  Candidate id of column j = id_offset + j (GLOBAL).  gt_idx holds GLOBAL
 * ids and gt_score the ground-truth pair's score, wherever it was computed.  ahead[q] (WRITTEN, not accumulated) = number of columns
 * j with id_j != gt_idx[q] that rank before (gt_score[q], gt_idx[q]) under the order rule (score descending, then lower id);
 * gt_idx[q] < 0 writes 0.  The top-k lists carry global ids.  -inf / NaN behave as on kemr_rank_dense's k <= 32 route.
 * With id_offset = 0 and gt_score[q] = S[q, gt_idx[q]] the outputs have kemr_rank_dense's bits; over any split of a matrix's columns
 * into contiguous pieces the per-piece `ahead` values sum to kemr_rank_dense's and kemr_topk_merge of the per-piece lists is its
 * list.  One workgroup per row, one pass, no atomics: a pure function of the input.  ld >= ng, rows need no alignment.
 * Refused before any launch: id_offset < 0 or id_offset + ng > INT32_MAX; ld < ng; k outside 1..32 when lists are asked for;
 * gt_idx / gt_score / ahead not all-or-none; top_scores / top_idx not both-or-none.  nq == 0 is a no-op. */
int kemr_rank_dense_shard(const float* scores_dev, int nq, int ng, int64_t ld, int64_t id_offset,
                          const int32_t* gt_idx_dev /* GLOBAL ids */, const float* gt_score_dev,
                          int32_t* ahead_dev, int k, float* top_scores_dev, int32_t* top_idx_dev, void* stream);

/* Deep ranked lists: up to KEMR_MAX_DEEP_K candidates per query, exact, by selection and a sort of the survivors instead of the
 * register-resident lists behind kemr_sim_topk / kemr_rank_dense (k <= 32).  What the online engine needs to let a SPARQL hit
 * that CLIP ranks 57th receive its bonus (reference src/retrieval.py:79-95 fuses over CLIP's own list), the shortlist that
 * kemr_cross_attention_rerank scores with the cross_attention head, Recall@100, deduplication.  Same order rule as everywhere: score descending, then lower id; lists are
 * padded with -inf / -1.  Unlike the k <= 32 routes, a candidate whose score is -inf or NaN is listed (see kemr_rank_dense).  The result is a pure function of the input (same bits on every run).  kemr_select_topk and
 * kemr_sim_topk_deep take no ground truth, `ahead` or bonus arguments; kemr_sim_topk_deep_fused is the deep route with them. */
#define KEMR_MAX_DEEP_K 1024
/* top-k of materialised rows: scores fp32 [nq, ld] (n <= ld valid columns; nothing at or beyond column n is read), idx int32
 * [nq, ld] or NULL (id = id_offset + column).  Entries with id < 0 are padding and skipped; the ids of a row must be distinct.
 * 1 <= k <= KEMR_MAX_DEEP_K; top_scores / top_idx [nq, k].  Ordering: -0.0 ties with +0.0, NaN ranks behind -inf (what
 * np.argsort(-S, kind="stable") does); the scores written are the input's own bits.  Also the merge of sharded deep lists:
 * concatenate the shards' lists along the row and pass their ids. */
int kemr_select_topk(const float* scores_dev, const int32_t* idx_dev, int nq, int n, int64_t ld, int64_t id_offset,
                     int k, float* top_scores_dev, int32_t* top_idx_dev, void* stream);
/* Scores + deep top-k without the Q x N matrix leaving the device: the queries are walked in blocks; a block's fp32 scores
 * against the whole gallery go to the workspace through the dense tile kernel (bit-identical to kemr_scores_dense,
 * kemr_pair_scores and kemr_sim_topk), the selection runs on the block.  The block is what the workspace holds, rounded down to
 * a multiple of 128 query rows of ceil4(ng) floats: kemr_sim_topk_deep_workspace_bytes returns the size for min(ceil128(nq),
 * 1024) rows, any 256-byte aligned workspace of at least 128 rows is accepted, anything smaller is KEMR_ERR_WORKSPACE.  The workspace's
 * contents don't matter; top_scores / top_idx [nq, k] are written wholly and nothing else is. */
size_t kemr_sim_topk_deep_workspace_bytes(int nq, int ng, int64_t kdim, int k);
int kemr_sim_topk_deep(const void* q_panel_dev, int nq, const void* g_panel_dev, int ng, int64_t kdim, int64_t gallery_offset,
                       int k, float* top_scores_dev, int32_t* top_idx_dev, void* workspace_dev, size_t workspace_bytes, void* stream);
/* kemr_sim_topk_deep with the knowledge side: the arguments of kemr_sim_topk in its order, 1 <= k <= KEMR_MAX_DEEP_K (rank only,
 * k == 0, stays with kemr_sim_topk), the workspace of kemr_sim_topk_deep (the bonus is applied in place on the block of scores).
 * Per block of query rows, between the score pass and the selection:
 *   bonus (rowptr int32 [nq + 1], col int32 GLOBAL ids ascending within a row, val fp32; all three or none): every entry whose
 *     column lies in [gallery_offset, gallery_offset + ng) is added to its score, entries of one column one after the other in
 *     list order in fp32 -- the fused score has the bits kemr_sim_topk computes from the same list; the lists hold fused scores;
 *   ground truth (gt_idx int32 [nq] GLOBAL ids that may lie outside this gallery, gt_score fp32 [nq] = the pair's fused score as
 *     the caller computed it, ahead int32 [nq]; all three or none): ahead[q] += the candidates of this gallery other than gt_idx[q]
 *     whose fused score ranks before (gt_score[q], gt_idx[q]) -- accumulated, so that shards sum; an integer count that does not
 *     depend on the order anything arrives in.
 * A partial triple is KEMR_ERR_INVALID; with all six NULL the call is kemr_sim_topk_deep, bit for bit. */
int kemr_sim_topk_deep_fused(const void* q_panel_dev, int nq, const void* g_panel_dev, int ng, int64_t kdim, int64_t gallery_offset,
                             int k, float* top_scores_dev, int32_t* top_idx_dev,
                             const int32_t* gt_idx_dev, const float* gt_score_dev, int32_t* ahead_dev,
                             const int32_t* bonus_rowptr_dev, const int32_t* bonus_col_dev, const float* bonus_val_dev,
                             void* workspace_dev, size_t workspace_bytes, void* stream);

/* Gate of the learned gated fusion heads in eval mode (reference src/clip/model/fusion_model.py: SimpleGatedFusion /
 * SimpleGatedFusionWithBias `sigmoid((q * w).sum(1) + b)`, GatedFusionHead `Linear(d,128) -> ReLU -> Linear(128,1) -> Sigmoid`):
 * out[r] = sigmoid(sum_c act(x[r,c] + pre_bias[c]) * w[c] + bias), act = ReLU when relu != 0 else identity; x fp32 [rows, cols]
 * (the queries, or their Linear(d,128) image from the dense kernels), pre_bias fp32 [cols] or NULL, w fp32 [cols]. */
int kemr_gate_rows(const float* x_dev, int rows, int cols, const float* pre_bias_dev, const float* w_dev, float bias, int relu,
                   float* out_dev, void* stream);

/* Learned "linear" fusion head in eval mode (reference src/clip/model/fusion_model.py:25-48):
 * out[i] = w1 . relu(W0 . [t2i[i], t2t[i]] + b0) + b1 over n score pairs (W0 fp32 [hidden,2], b0/w1 fp32 [hidden]). */
int kemr_linear_head(const float* t2i_dev, const float* t2t_dev, int64_t n, const float* w0_dev, const float* b0_dev,
                     const float* w1_dev, float b1, int hidden, float* out_dev, void* stream);

/* Pair stage of the learned "cross_attention" fusion head in eval mode (reference src/clip/model/fusion_model.py:51-133).
 * Inputs are per-query / per-candidate quantities the host precomputes with the dense kernels (see fusion_model.py of the
 * build): st_x fp32 [heads][n_c][n_q] scaled attention scores (x = image / target key), p_x fp32 [n_c][heads][hid1] =
 * W1.Wo[:,head].V_x, c0 = W1.bo + b1 [hid1], w2t = W2^T [hid1][hid2], b2 [hid2], w3 [hid2], b3.
 * out_t fp32 [n_c][n_q] = 0.5 * tanh(MLP(softmax-mixed context))  (transposed score matrix). */
int kemr_cross_attention_pairs(const float* st_i_dev, const float* st_t_dev, const float* p_i_dev, const float* p_t_dev,
                               const float* c0_dev, const float* w2t_dev, const float* b2_dev, const float* w3_dev, float b3,
                               int heads, int n_q, int n_c, int hid1, int hid2, float* out_t_dev, void* stream);

/* The "cross_attention" head on LISTED pairs (retrieve-then-rerank: the consumer of the deep lists above): for every slot (q, j),
 * j < depth, of cand_idx int32 [nq, ld] the score of query q against candidate c = cand_idx[q, j].  c < 0 is the deep lists' padding
 * and scores -inf; an id >= ng is the caller's error (it is never dereferenced and scores -inf as well).
 *   q fp32 [nq, dim]: the attention queries, already scaled by (dim / heads)^-0.5; k_x fp32 [ng, dim]: per-candidate keys
 *   (x = image / target); p_x, c0, w2t, b2, w3, b3: as kemr_cross_attention_pairs takes them (hid1 a multiple of 4, hid2 <= 64).
 * Per slot: the heads + heads dot products Q[q, head] . K_x[c, head] as fp32 FMA chains over the gathered rows, then the arithmetic
 * of kemr_cross_attention_pairs (2-way softmax per head, relu(c0 + sum_h w_i P_i + w_t P_t), hid1 -> hid2 as one ascending-k fp32
 * FMA chain on v_mfma_f32_16x16x4_f32, hid2 -> 1, 0.5 * tanh).  The dot products differ from the dense route's (which takes them
 * from the bf16-split similarity kernel) in the last bits, so scores agree with kemr_cross_attention_pairs to rounding, not bit
 * for bit.  out_scores fp32 [nq, ld]: columns < depth are each written exactly once, columns >= depth are not touched; the result
 * is a pure function of the input (same bits on every run).  1 <= depth <= KEMR_MAX_DEEP_K, depth <= ld; nq == 0 or depth == 0 is a no-op. */
int kemr_cross_attention_rerank(const float* q_dev, const float* k_i_dev, const float* k_t_dev, const float* p_i_dev,
                                const float* p_t_dev, const float* c0_dev, const float* w2t_dev, const float* b2_dev,
                                const float* w3_dev, float b3, int heads, int nq, int ng, int dim, int hid1, int hid2,
                                const int32_t* cand_idx_dev, int depth, int64_t ld, float* out_scores_dev, void* stream);

/* The knowledge side on a learned head's lists (knowledge-fused rerank: CLIP shortlist -> head on the listed pairs -> this): for
 * every slot (q, j), j < depth, of list_scores fp32 [nq, ld] / list_idx int32 [nq, ld] with id c = list_idx[q, j]
 *   c < 0 (the deep lists' padding): out = -inf;
 *   otherwise f = score_scale * s as ONE fp32 multiply (score_scale == 1.0f: the output has the input's own bits), then every entry
 *   of bonus row q whose column equals c is added to f, one after the other in list order, in fp32 -- the rule of
 *   kemr_sim_topk_deep_fused, whose CSR layout the bonus has (rowptr int32 [nq + 1], col int32 GLOBAL ids ascending within a row, val
 *   fp32; all three or none).  A column may repeat, lie outside the list or outside any gallery; a row may be empty or hold many
 *   thousands of entries (it is binary-searched; the result does not depend on its length).
 * Only columns < depth are read or written: columns >= depth of out_scores are not touched.  out_scores may alias list_scores.
 * Ground truth (gt_idx int32 [nq], ahead int32 [nq], found int32 [nq], gt_score fp32 [nq]; all four or none; WRITTEN, not accumulated):
 *   found[q] = 1 if gt_idx[q] is among the row's ids, else 0; gt_score[q] = that slot's fused score where found, -inf otherwise;
 *   ahead[q] = the slots with id >= 0 and id != gt_idx[q] that rank before (gt_score[q], gt_idx[q]) by the order rule of
 *   kemr_select_topk (score descending, -0.0 ties +0.0, lower id first on equal scores, NaN behind -inf); where the ground truth is
 *   absent, every slot with id >= 0.  So where found, ahead + 1 is the ground truth's position in kemr_select_topk(out, idx, k = depth).
 * A partial triple or quadruple is KEMR_ERR_INVALID; 1 <= depth <= KEMR_MAX_DEEP_K, ld >= depth; nq == 0 is a no-op; with both groups
 * NULL the call is scale + padding only.  One workgroup per query row, every output element has one owner, no atomics: the result is
 * a pure function of the input (same bits on every run). */
int kemr_list_fuse(const float* list_scores_dev, const int32_t* list_idx_dev, int nq, int depth, int64_t ld, float score_scale,
                   const int32_t* bonus_rowptr_dev, const int32_t* bonus_col_dev, const float* bonus_val_dev,   /* all three or none */
                   const int32_t* gt_idx_dev, int32_t* ahead_dev, int32_t* found_dev, float* gt_score_dev,      /* all four or none  */
                   float* out_scores_dev, void* stream);

/* The pooled tower rows, for training the projection heads on frozen towers: kemr_encode_image / kemr_encode_text /
 * kemr_encode_text_packed with the same arguments minus `normalize`, but out_dev is fp32 [batch, tower width] (v_width / t_width) and
 * holds the pooled row of the residual stream with the last block's pending updates applied -- exactly the values the tail feeds its
 * LayerNorm (ln_post / ln_final), BEFORE that LayerNorm and the projection.  LayerNorm + projection (+ x / ||x||) of these rows in fp32 is
 * the embedding of the counterpart call, up to the tail's own rounding.  The same workspace sizes and checks; the tail runs in a
 * store-the-row mode and leaves no state behind (the counterpart calls produce the same bits before and after).  Family 0 (CLIP) at every
 * precision; KEMR_ERR_INVALID for family 1 (SigLIP: its head is the attention pool over every row) and family 2 (BERT: no head). */
int kemr_encode_image_pooled(kemr_model* m, const float* pixels_dev, int batch, float* out_dev,
                             void* workspace_dev, size_t workspace_bytes, void* stream);
int kemr_encode_text_pooled(kemr_model* m, const int32_t* ids_dev, int batch, float* out_dev,
                            void* workspace_dev, size_t workspace_bytes, void* stream);
int kemr_encode_text_packed_pooled(kemr_model* m, const int32_t* ids_dev, const int32_t* lens_dev, int rows, int batch, float* out_dev,
                                   void* workspace_dev, size_t workspace_bytes, void* stream);

/* Fused InfoNCE (the symmetric contrastive loss of the fine-tuning recipe), forward and backward; the n x n logits are never stored.
 * For fp32 features a, b [n, d] (row-major, any norm) and z = a b^T * inv_temperature:
 *   loss_a2b = mean_i (lse_j z_ij - z_ii),  loss_b2a = mean_j (lse_i z_ij - z_jj),  loss = (loss_a2b + loss_b2a) / 2
 *   dL/dz = (softmax_rows(z) + softmax_cols(z)) / (2 n) - I / n,  grad_a = dL/dz b * inv_temperature,  grad_b = dL/dz^T a * inv_temperature
 * forward writes loss_dev fp32 [3] = loss, loss_a2b, loss_b2a and lse_dev fp32 [2 n] = the n row lse values, then the n column lse values
 * (natural logarithm); backward takes that lse_dev and OVERWRITES grad_a_dev / grad_b_dev fp32 [n, d] with the gradient of `loss` (the
 * caller scales by the upstream gradient).  Products at fp32 grade: every operand and the dL/dz tile are bf16 pairs (hi = rne(v), lo =
 * rne(v - hi), the split of kemr_panel_build's terms == 3) contracted as hi.hi + lo.hi + hi.lo with fp32 accumulation; the log-sum-exp is
 * online and max-subtracted in fp32.  No atomics, fixed reduction orders: the same inputs give the same bits on every call, and the two
 * passes of forward see the same bits of every logit.
 * 1 <= n <= 65536; d a multiple of 4, 4 <= d <= 1280; inv_temperature positive and finite; no pointer NULL.
 * Workspace (the same size for both calls; backward does not need forward's contents, only lse_dev), with n256 = ceil256(n),
 * dpad = ceil64(d), dpadT = ceil128(d), each term rounded up to 256 bytes:
 *   2 * (n256 * 2 dpad * 2)      pair panels [hi | lo] of a and b
 * + 2 * (2 dpadT * n256 * 2)     their transposes (backward's second contraction)
 * + 2 n * 16 * 2 * 4             per (row, column chunk) running maximum and sum, both passes
 * + 2 n * 4 + 2 n * 4            diagonal logits and per-row loss terms, both passes
 * 256-byte aligned; exactly that is enough and its contents don't matter (every byte that is read is written first; pad rows and pad
 * columns are zero-filled by the call and masked in the log-sum-exp).  Anything outside these ranges, a NULL pointer (KEMR_ERR_INVALID)
 * and a short or misaligned workspace (KEMR_ERR_WORKSPACE) are refused BEFORE anything is launched: the outputs and the workspace keep
 * their bytes.  kemr_infonce_workspace_bytes returns 0 for an n or d out of range. */
size_t kemr_infonce_workspace_bytes(int n, int d);
int kemr_infonce_forward(const float* a_dev, const float* b_dev, int n, int d, float inv_temperature,
                         float* loss_dev, float* lse_dev, void* workspace_dev, size_t workspace_bytes, void* stream);
int kemr_infonce_backward(const float* a_dev, const float* b_dev, const float* lse_dev, int n, int d, float inv_temperature,
                          float* grad_a_dev, float* grad_b_dev, void* workspace_dev, size_t workspace_bytes, void* stream);

/* Fused pair-score contrastive loss: the symmetric InfoNCE of kemr_infonce_forward over the scores of a learned fusion head,
 * S = head(q, img, tgt), forward and backward -- what trains the heads over frozen encoders; the n x n scores are never stored.
 * For fp32 q, img, tgt [n, d] (row-major), t2i = q img^T, t2t = q tgt^T and z = S * inv_temperature:
 *   KEMR_PAIRHEAD_GATED   s_ij = g_i t2i_ij + (1 - g_i) t2t_ij, gate_dev fp32 [n] (the head's gate per query, computed by the caller);
 *                         w0_dev .. b1_dev and hidden are ignored
 *   KEMR_PAIRHEAD_LINEAR  s_ij = b1 + sum_k w1_k max(0, w0_k0 t2i_ij + w0_k1 t2t_ij + b0_k), the arithmetic of kemr_linear_head fma for fma;
 *                         w0_dev fp32 [hidden, 2], b0_dev [hidden], w1_dev [hidden], b1_dev [1], 1 <= hidden <= 256; gate_dev is ignored
 *   loss, loss_q2g (rows), loss_g2q (columns) and lse_dev [2 n] as kemr_infonce_forward defines them
 *   G = dL/ds = ((softmax_rows(z) + softmax_cols(z)) / (2 n) - I / n) * inv_temperature
 * backward takes forward's lse_dev and OVERWRITES grad_dev with the gradient of `loss`:
 *   GATED   fp32 [n]: dL/dg_i = sum_j G_ij (t2i_ij - t2t_ij)
 *   LINEAR  fp32 [4 hidden + 1] = dL/dw0 [hidden, 2] | dL/db0 [hidden] | dL/dw1 [hidden] | dL/db1; a unit counts where its pre-activation > 0
 * No gradient goes to q, img, tgt (frozen encoders).  t2i and t2t are computed as kemr_infonce_forward computes its logits, bit for bit, and
 * both passes of forward and the backward see the same bits of every score; with g = 1 (g = 0) forward returns the bits of
 * kemr_infonce_forward(q, img) (of (q, tgt)).  No atomics, fixed reduction orders: the same inputs give the same bits on every call.
 * 1 <= n <= 65536; d a multiple of 4, 4 <= d <= 1280; inv_temperature positive and finite; no pointer that the mode reads NULL.
 * Workspace (one size for both calls; backward needs only lse_dev of forward), n256 = ceil256(n), dpad = ceil64(d),
 * tiles = ceil(n / 128), per = ceil(tiles / min(tiles, 16)), chunks = ceil(tiles / per), each term rounded up to 256 bytes:
 *   3 * (n256 * 2 dpad * 2)               pair panels [hi | lo] of q, img, tgt
 * + 2 n * 16 * 2 * 4 + 2 n * 4 + 2 n * 4  forward's chunk statistics, diagonal scores and loss terms, both passes
 * + GATED: n * 16 * 4; LINEAR: tiles * chunks * (4 hidden + 1) * 4    backward's partial sums
 * 256-byte aligned; exactly that is enough, its contents don't matter.  Anything out of range, an unknown mode, a NULL pointer
 * (KEMR_ERR_INVALID) and a short or misaligned workspace (KEMR_ERR_WORKSPACE) are refused BEFORE anything is launched: the outputs and
 * the workspace keep their bytes.  kemr_pairhead_workspace_bytes returns 0 for arguments out of range. */
#define KEMR_PAIRHEAD_GATED 0
#define KEMR_PAIRHEAD_LINEAR 1
size_t kemr_pairhead_workspace_bytes(int mode, int n, int d, int hidden);
int kemr_pairhead_forward(int mode, const float* q_dev, const float* img_dev, const float* tgt_dev, int n, int d, float inv_temperature,
                          const float* gate_dev, const float* w0_dev, const float* b0_dev, const float* w1_dev, const float* b1_dev,
                          int hidden, float* loss_dev, float* lse_dev, void* workspace_dev, size_t workspace_bytes, void* stream);
int kemr_pairhead_backward(int mode, const float* q_dev, const float* img_dev, const float* tgt_dev, const float* lse_dev, int n, int d,
                           float inv_temperature, const float* gate_dev, const float* w0_dev, const float* b0_dev, const float* w1_dev,
                           const float* b1_dev, int hidden, float* grad_dev, void* workspace_dev, size_t workspace_bytes, void* stream);

/* Optional per-kernel-class timing with hipEvents recorded on the launch stream (bench.py's roofline line).
 * Classes: 0 GEMM, 1 LayerNorm, 2 attention, 3 embed/tail, 4 similarity tile kernel.  Not thread-safe;
 * profile_end synchronises the device.  Off by default: no events are recorded on the normal path. */
#define KEMR_PROF_NCLASS 5
int kemr_profile_begin(int max_launches);
int kemr_profile_end(double* ms_per_class, int64_t* launches_per_class, int nclass);

/* ---------------------------------------------------------------------------------------------
 * Building blocks exposed for per-kernel parity tests (tests/ call these through the ABI).
 * ------------------------------------------------------------------------------------------- */
typedef enum kemr_epilogue {
    KEMR_EPI_BIAS_BF16 = 0,        /* C_bf16 = A.W^T + bias                                  */
    KEMR_EPI_BIAS_QGELU_BF16 = 1,  /* C_bf16 = quickgelu(A.W^T + bias)                       */
    KEMR_EPI_BIAS_RESID_F32 = 2,   /* X_f32 += A.W^T + bias   (in place on the residual; from 128 output tiles of 256 x 256 and more
                                      than 512 rows up the persistent kernel: C with ceil256(m) rows) */
    KEMR_EPI_BIAS_RESADD_BF16 = 4, /* X_bf16 = bf16(bf16(A.W^T + bias) + X_bf16), in place; persistent 256 x 256 kernel only:
                                      N % 256 == 0, m > 512, C with ceil256(m) rows                              */
    KEMR_EPI_BIAS_GELU_BF16 = 5,   /* C_bf16 = gelu(A.W^T + bias), exact GELU 0.5 x erfc(-x / sqrt 2) in fp32 (3 and 7 are internal, 6 is not a value) */
    KEMR_EPI_BIAS_TGELU_BF16 = 8   /* C_bf16 = gelu_tanh(A.W^T + bias): 0.5 x (1 + tanh(sqrt(2/pi) (x + 0.044715 x^3))), computed in fp32 as
                                      x sigmoid(2 sqrt(2/pi) (x + 0.044715 x^3)) (the SigLIP family's fc1; bf16 operands only) */
} kemr_epilogue;
/* A bf16 [m_alloc, k] and C [m_alloc, n] with m_alloc = m rounded up to 256 rows (pad rows of A are read; pad rows of C
 * may be written by the bf16 epilogues), W bf16 [n, k], bias fp32 [n].
 * Memory contract of kemr_op_gemm / kemr_op_gemm_fp8 (tests/test_footprint_ops_gpu.py): rows 0 .. m - 1 of C do not depend on A's pad
 * rows (they may hold NaN) nor on anything outside A's m_alloc rows, W's n rows and the bias' n floats; nothing in front of C and no
 * row >= m_alloc of C is written.  C's pad rows m .. m_alloc - 1: scratch for the bf16-store epilogues, for KEMR_EPI_BIAS_RESADD_BF16
 * and for kemr_op_gemm_fp8 (the 256-row-tile kernels store whole tiles); KEMR_EPI_BIAS_RESID_F32 leaves them as they are wherever a
 * tile kernel with row masks takes the call, i.e. everywhere but on the persistent kernel (m > 512, n % 256 == 0, k >= 128, from 128
 * output tiles of 256 x 256 up), where they are scratch. */
/* ---- image preprocessing on the GPU ------------------------------------------------
 * Replaces the per-sample host transform the reference gets from clip.load (src/clip/datasets/clip_dataset.py:110-125):
 * uint8 HWC RGB [height, width, 3] on the device -> Resize(n_px, bicubic, shorter side; Pillow's antialiased two-pass
 * filter with 8-bit intermediates, bit-exact) -> CenterCrop(n_px) -> /255 -> (x - mean) / std -> fp32 CHW [3, n_px, n_px].
 * The workspace holds the coefficient tables (uploaded by the call) and the horizontally filtered rows. */
size_t kemr_preprocess_workspace_bytes(int height, int width, int n_px);
int kemr_preprocess_u8(const unsigned char* img_dev, int height, int width, int n_px, float* out_dev,
                       void* workspace_dev, size_t workspace_bytes, void* stream);
/* A whole loader batch in ONE launch pair: `batch` uint8 HWC images of any sizes packed back to back in packed_dev
 * (image b starts at byte offsets[b] and has heights[b] x widths[b] pixels; the three arrays are HOST arrays) ->
 * out_dev fp32 [batch, 3, n_px, n_px].  Same arithmetic, bit for bit, as kemr_preprocess_u8 per image.
 * An item with heights[b] == widths[b] == 0 is one the caller could not decode: it has no bytes in packed_dev and its
 * output is 0.0f everywhere, i.e. zeros AFTER normalisation -- the tensor the reference's dataset substitutes
 * (src/clip/datasets/clip_dataset.py:120-125, torch.zeros(3, 224, 224)).  Any other non-positive size is KEMR_ERR_INVALID. */
size_t kemr_preprocess_batch_workspace_bytes(const int32_t* heights, const int32_t* widths, int batch, int n_px);
int kemr_preprocess_u8_batch(const unsigned char* packed_dev, const int64_t* offsets, const int32_t* heights,
                             const int32_t* widths, int batch, int n_px, float* out_dev, void* workspace_dev,
                             size_t workspace_bytes, void* stream);
/* The same four calls with the KIND of transform as an argument (the kemr_preprocess_* entry points are these at KEMR_TRANSFORM_CLIP):
 *   KEMR_TRANSFORM_CLIP    Resize(n_px, bicubic, shorter side) -> CenterCrop(n_px) -> / 255 -> (x - mean) / std with CLIP's constants;
 *   KEMR_TRANSFORM_SIGLIP  transformers.SiglipImageProcessor: Image.resize((n_px, n_px), BICUBIC) -- each axis resampled on its own (or
 *                          copied when its size does not change), the aspect ratio is not kept, nothing is cropped -- -> / 255 ->
 *                          (x - 0.5) / 0.5.  Bit for bit the host transform (python: preprocess.SiglipPreprocess), same kernels.
 * Any other kind: the workspace functions return 0, the launch functions KEMR_ERR_INVALID.
 * Pass order.  The kernels filter horizontally first, then vertically; the intermediate is clipped to 8 bits, so the order is part of
 * the result.  Pillow (12.2.0, measured) filters VERTICALLY first when height > 100 x width and the output is lower than the input.
 * KEMR_TRANSFORM_SIGLIP therefore refuses an image with height > 100 * width and height > n_px: the workspace functions return 0, the
 * launch functions KEMR_ERR_INVALID with a message that names the size (the batch form: and the item; the batch is refused as a
 * whole); nothing is launched, `out` and the workspace keep their bytes.  The caller computes such an image on the host.
 * (KEMR_TRANSFORM_CLIP has always filtered horizontally first and accepts such images: beyond 100:1 its bits are not Pillow's.)
 * Memory contract (tests/test_siglip_transform_gpu.py), all four launch calls, both kinds: exactly kemr_transform_workspace_bytes /
 * kemr_transform_batch_workspace_bytes is enough -- nothing before the workspace's first or behind its last byte is written or can
 * reach `out`; every workspace byte a result depends on is written by the call first (stale bytes of an earlier call of another size,
 * NaN included, cannot reach `out`); exactly 3 * n_px * n_px floats of `out` per image are written (a 0 x 0 item: 0.0f); nothing
 * outside the heights[b] * widths[b] * 3 bytes of each image -- the bytes in front of, between and behind the images of packed_dev --
 * can reach them.  A workspace that is too small or not 256-byte aligned is KEMR_ERR_WORKSPACE BEFORE anything is launched: `out` and
 * the workspace keep their bytes. */
typedef enum kemr_transform { KEMR_TRANSFORM_CLIP = 0, KEMR_TRANSFORM_SIGLIP = 1 } kemr_transform;
size_t kemr_transform_workspace_bytes(int transform /*kemr_transform*/, int height, int width, int n_px);
int kemr_transform_u8(int transform, const unsigned char* img_dev, int height, int width, int n_px, float* out_dev,
                      void* workspace_dev, size_t workspace_bytes, void* stream);
size_t kemr_transform_batch_workspace_bytes(int transform, const int32_t* heights, const int32_t* widths, int batch, int n_px);
int kemr_transform_u8_batch(int transform, const unsigned char* packed_dev, const int64_t* offsets, const int32_t* heights,
                            const int32_t* widths, int batch, int n_px, float* out_dev, void* workspace_dev,
                            size_t workspace_bytes, void* stream);

int kemr_op_gemm(const void* a_dev, const void* w_dev, const float* bias_dev, void* c_dev,
                 int m, int n, int k, int epilogue, void* stream);
int kemr_op_layernorm(const float* x_dev, const float* gamma_dev, const float* beta_dev, void* y_dev,
                      int rows, int width, int out_dtype /*KEMR_BF16|KEMR_F32*/, void* stream);
/* fp8 operands: a e4m3 [ceil256(m), k] and w e4m3 [n, k] (bytes), wscale fp32 [n] multiplies the accumulators per output
 * channel before the bias; c bf16 [ceil256(m), n]; n % 256 == 0, k % 128 == 0, k >= 256; epilogue BIAS_BF16 | BIAS_QGELU_BF16 | BIAS_GELU_BF16 */
int kemr_op_gemm_fp8(const void* a_dev, const void* w_dev, const float* wscale_dev, const float* bias_dev, void* c_dev,
                     int m, int n, int k, int epilogue, void* stream);
/* the host-side fp32 -> e4m3 conversion used when weights are packed (round to nearest even, saturating at +-448); no GPU */
int kemr_op_e4m3_host(const float* in, unsigned char* out, long long n);
/* fused residual form used inside the towers: x_f32 += delta_bf16 (written back), y_bf16 = LayerNorm(x) */
int kemr_op_layernorm_resid(float* x_dev, const void* delta_dev, const float* gamma_dev, const float* beta_dev,
                            void* y_dev, int rows, int width, void* stream);
/* general form: rows of x_dtype (KEMR_F32|KEMR_BF16); y = LayerNorm(x [+ delta [+ delta2]]) (deltas bf16, may be NULL);
 * writeback != 0 stores the sum back into x (required with delta2); without deltas x is only read, unless y_dev == x_dev.
 * Exactly rows x width elements of x, the deltas and y are touched (no pad rows: a row tile is 4 rows, masked at `rows`); without
 * writeback x keeps its bits.  Row / output types beyond the two above, for the towers and tests: x_dtype 24 (the 24-bit stream rows,
 * 3 width bytes each) and out_dtype KEMR_FP8 (e4m3 bytes) or 24 (from KEMR_F32 rows only); a delta needs a bf16 or fp8 output. */
int kemr_op_layernorm_rows(void* x_dev, int x_dtype, const void* delta_dev, const void* delta2_dev, int writeback,
                           const float* gamma_dev, const float* beta_dev, void* y_dev, int rows, int width, int out_dtype,
                           void* stream);
/* qkv bf16 [batch*t, 3*width] (heads of 64; q pre-scaled by 1/sqrt(64) = 1/8) -> out bf16 [batch*t, width]; t <= 288, or non-causal
 * t <= KEMR_MAX_VISION_TOKENS (streaming kernel); longer causal sequences are KEMR_ERR_INVALID.  No pad rows on either side: the
 * ragged last key block and query tile of an item are masked, so exactly batch * t rows of out are written and nothing before row 0 or
 * behind row batch * t - 1 of qkv can reach them (kemr_op_attention_hd, both head dims, likewise). */
int kemr_op_attention(const void* qkv_dev, void* out_dev, int batch, int t, int width, int causal, void* stream);
/* The backward of kemr_op_attention (heads of 64).  qkv bf16 [batch*t, 3*width] exactly as that op reads it (q | k | v, q pre-scaled by
 * 1/8), dout bf16 [batch*t, width] = the gradient of its output -> dqkv bf16 [batch*t, 3*width] = the gradient with respect to the three
 * planes AS GIVEN: the caller owns the 1/8 of q (d loss / d unscaled q = dq / 8).  1 <= t <= KEMR_MAX_TEXT_CTX (288), causal 0 or 1,
 * width % 64 == 0, batch >= 0 (batch == 0 launches nothing; batch * width / 64 <= 2^31 - 1, the grid); anything else, or a NULL
 * pointer, is KEMR_ERR_INVALID with a message naming the argument, refused on the host before any launch with dqkv untouched.
 * The forward saves nothing: scores, row maximum and sum and the probabilities P are recomputed from qkv in fp32, D_i = sum_j P_ij dP_ij
 * from the same values (no `out` argument).  bf16 MFMA with fp32 accumulators; P and dS are rounded to bf16 as MFMA operands, the
 * outputs to bf16 at the store, nothing else is rounded below fp32.  No workspace, no atomics: every element of dqkv has one owner
 * and one summation order, so the same inputs give the same bits on every launch.  Exactly batch * t rows of dqkv are written; the
 * ragged last tiles are masked, and nothing outside an item's own rows of qkv and dout can reach its rows of dqkv. */
int kemr_op_attention_backward(const void* qkv_dev, const void* dout_dev, void* dqkv_dev, int batch, int t, int width, int causal,
                               void* stream);
/* Causal attention (heads of 64) over items of different lengths packed one behind the other, the forward the text encoders run on
 * packed texts.  qkv bf16 [rows, 3*width] (q | k | v, q pre-scaled by 1/8) -> out bf16 [rows, width]; item b = rows row_start[b] ..
 * row_start[b + 1] - 1 of both (row_start: device int32 [batch + 1], non-decreasing; batch + 1 ints are read), every length in
 * 1 .. max_t.  1 <= max_t <= KEMR_MAX_TEXT_CTX (288), width % 64 == 0, 0 <= batch <= 65 528 (batch == 0 launches nothing); anything
 * else, or a NULL pointer, is KEMR_ERR_INVALID with a message that starts with "op_attention_packed:" and names the argument, refused
 * on the host before any launch.  max_t <= 128 runs the tile kernels, one workgroup per (item, head); above, the causal streaming
 * kernel, in which an item longer than max_t is computed as an item of its first max_t rows (its later rows of out are not written)
 * and an empty item writes nothing -- the tile kernels take lengths 1 .. max_t only.  Exactly the rows row_start[0] ..
 * row_start[batch] - 1 of out are written, nothing outside an item's own rows of qkv can reach its rows of out, and an item has the
 * same bits whatever is packed around it.  Every launch goes to `stream`. */
int kemr_op_attention_packed(const void* qkv_dev, void* out_dev, const int* row_start_dev, int batch, int max_t, int width, void* stream);
/* The backward of kemr_op_attention_packed (causal = 1), and of its non-causal counterpart (causal = 0), over the same packed layout:
 * qkv bf16 [rows, 3*width] as the forward reads it (q pre-scaled by 1/8), dout bf16 [rows, width] -> dqkv bf16 [rows, 3*width], the
 * gradient with respect to the three planes AS GIVEN: the caller owns the 1/8 of q, as with kemr_op_attention_backward.  Item b =
 * rows row_start[b] .. row_start[b + 1] - 1 of all three (row_start: device int32 [batch + 1]; batch + 1 ints are read).
 * 1 <= max_t <= KEMR_MAX_TEXT_CTX (288), width % 64 == 0, causal 0 or 1, batch >= 0 (batch == 0 launches nothing; batch * width / 64
 * <= 2^31 - 1, the grid); anything else, or a NULL qkv, dout, dqkv or row_start, is KEMR_ERR_INVALID with a message that starts with
 * "op_attention_backward_packed:" and names the argument, refused on the host before any HIP call with dqkv untouched.
 * Lengths: an empty item (length <= 0) reads and writes nothing; an item longer than max_t is computed as an item of its first max_t
 * rows and its later rows of dqkv are not written (the forward's convention).  Exactly the rows row_start[0] .. row_start[batch] - 1
 * of dqkv are written, less those rows; nothing outside an item's own rows of qkv and dout can reach its rows of dqkv.
 * The kernel is kemr_op_attention_backward's with the item's first row and length read from row_start: one workgroup per (item, head),
 * the head's Q, K, V and dO in LDS in the allocation of max_t, no workspace, no atomics, every element of dqkv owned by one wave and
 * summed in one order -- the same bits on every launch, and, per item, the bits of kemr_op_attention_backward(batch = 1, t = the
 * item's length) on the same rows at any max_t >= that length (the tiles of the larger allocation are skipped, they add nothing to
 * any sum).  Every launch goes to `stream`. */
int kemr_op_attention_backward_packed(const void* qkv_dev, const void* dout_dev, void* dqkv_dev, const int* row_start_dev, int batch,
                                      int max_t, int width, int causal, void* stream);
/* The same backward, non-causal, for sequences of any length the forward takes: 1 <= t <= KEMR_MAX_VISION_TOKENS (1025; the long
 * vision towers, ViT-L/14@336px's 577 tokens).  qkv, dout and dqkv as above; width % 64 == 0, batch >= 0 (batch == 0 launches nothing;
 * batch * width / 64 * ceil(t / 64) <= 2^31 - 1, the grid); workspace_bytes >= kemr_attention_backward_long_workspace_bytes(batch, t,
 * width) = batch * (width / 64) * t * 3 * sizeof(float) (a function of its three arguments only; 0 at batch == 0 and for arguments
 * the op refuses; the workspace may be NULL when it is 0), the workspace 4-byte aligned.  Anything else, or a NULL pointer, is
 * KEMR_ERR_INVALID with a message that starts with "op_attention_backward_long:" and names the argument, refused on the host before
 * any launch with dqkv untouched.
 * The forward saves nothing and nothing longer than 64 rows is held in LDS: a query-owned kernel streams K and V twice (an online
 * row maximum, sum and sum of e^(s - m) dP in fp32, rescaled by exp(m - m') as the forward's; then P from the final maximum and sum,
 * dS and dq) and leaves max * log2 e, 1 / sum and D of every query row of every head in the workspace, fp32 [batch * heads * t, 3];
 * a key-owned kernel streams Q, dO and those statistics once and writes dk and dv.  Rounding as above: P and dS to bf16 as MFMA
 * operands, the outputs to bf16 at the store, D from the unrounded fp32 P, nothing else below fp32.  No atomics: every element of dqkv
 * has one owner and one summation order, so the same inputs give the same bits on every launch (not the bits of
 * kemr_op_attention_backward at t <= 288: the order of the sums differs).  Exactly batch * t rows of dqkv are written and the workspace
 * only inside its stated size; the ragged last tiles are masked, and nothing outside an item's own rows of qkv and dout can reach its
 * rows of dqkv.  Every launch goes to `stream`. */
size_t kemr_attention_backward_long_workspace_bytes(int batch, int t, int width);
int kemr_op_attention_backward_long(const void* qkv_dev, const void* dout_dev, void* dqkv_dev, int batch, int t, int width,
                                    void* workspace_dev, size_t workspace_bytes, void* stream);
/* The attention backward with the head dim as an argument: the backward of kemr_op_attention_hd.
 * head_dim == 80 (the vision tower of ViT-H-14): qkv bf16 [batch*t, 3*width] exactly as kemr_op_attention_hd reads it (q | k | v, q
 * pre-scaled by 1/sqrt(80)), dout bf16 [batch*t, width] -> dqkv bf16 [batch*t, 3*width], the gradient with respect to the three planes
 * AS GIVEN: the caller owns the 1/sqrt(80) of q.  width % 80 == 0, causal == 0 (no tower has causal heads of 80), 1 <= t <=
 * KEMR_MAX_VISION_TOKENS (1025; longer than the 288 the head-dim-80 forward takes), batch >= 0 (batch == 0 launches nothing;
 * batch * width / 80 * ceil(t / 64) <= 2^31 - 1, the grid); workspace_bytes >= kemr_attention_backward_hd_workspace_bytes(batch, t,
 * width, 80) = batch * (width / 80) * t * 3 * sizeof(float), the workspace 4-byte aligned (it may be NULL when the size is 0).  Anything
 * else -- a NULL pointer, a head_dim other than 64 or 80, causal = 1 at 80, a causal that is neither 0 nor 1 -- is KEMR_ERR_INVALID
 * with a message that starts with "op_attention_backward_hd:" and names the argument, refused on the host before any HIP call with dqkv
 * untouched.  The kernels are the head-dim-80 forms of kemr_op_attention_backward_long's (csrc/attention_bwd80.hip): streaming at every
 * t -- a head's four images do not fit a CU's LDS at 257 tokens --, a query-owned kernel (K and V stream twice; dq and the statistics
 * max * log2 e, 1 / sum and D of every query row of every head, fp32 [batch * heads * t, 3], into the workspace) and a key-owned kernel
 * (Q, dO and the statistics stream once; dk and dv).  The forward saves nothing.  P and dS are rounded to bf16 as MFMA operands, the
 * outputs to bf16 at the store, D comes from the unrounded fp32 P, nothing else is below fp32.  No atomics: every element of dqkv and of
 * the workspace has one owner and one summation order, so the same inputs give the same bits on every launch.  Exactly batch * t rows
 * of dqkv are written and the workspace only inside its stated size; nothing beyond column 79 of a head, and nothing outside an item's
 * own rows of qkv and dout, is read for its rows of dqkv.  Every launch goes to `stream`.
 * head_dim == 64: the call IS kemr_op_attention_backward (causal, or t <= KEMR_MAX_TEXT_CTX: no workspace, workspace_dev and
 * workspace_bytes are ignored) or kemr_op_attention_backward_long (non-causal, longer: its workspace), with that op's bits, refusals
 * and messages; kemr_attention_backward_hd_workspace_bytes(.., 64) is 0 up to KEMR_MAX_TEXT_CTX rows and
 * kemr_attention_backward_long_workspace_bytes above.  The size function is a function of its four arguments only and returns 0 at
 * batch == 0 and for arguments the op refuses. */
size_t kemr_attention_backward_hd_workspace_bytes(int batch, int t, int width, int head_dim);
int kemr_op_attention_backward_hd(const void* qkv_dev, const void* dout_dev, void* dqkv_dev, int batch, int t, int width,
                                  int head_dim, int causal, void* workspace_dev, size_t workspace_bytes, void* stream);
/* The backward of kemr_op_layernorm. x fp32 [rows, width] exactly as the forward read it, gamma fp32 [width], dy [rows, width] = the
 * gradient of its output in dy_dtype (KEMR_BF16 where the forward wrote bf16, KEMR_F32 where it wrote fp32) -> dx fp32 [rows, width],
 * dgamma and dbeta fp32 [width].  The forward saves nothing: mean and rstd are recomputed in fp32 exactly as the forward does (two
 * passes, the same wave sums, eps 1e-5).  With g = dy gamma and x^ = (x - mean) rstd: dx = rstd (g - mean(g) - x^ mean(g x^)),
 * dgamma_j = sum over rows of dy x^, dbeta_j = sum over rows of dy; fp32 throughout, nothing is rounded below fp32.
 * width in {256, 512, 768, 1024, 1280}, rows >= 0, dy_dtype as above, workspace_bytes >= kemr_layernorm_backward_workspace_bytes(rows,
 * width) (a function of its two arguments only, monotone in rows, 0 at rows == 0; the workspace may be NULL then); x, gamma, dy, dx
 * and the workspace 16-byte aligned; anything else, or a NULL pointer, is KEMR_ERR_INVALID with a message naming the argument, refused
 * on the host before any launch with the outputs untouched.  rows == 0 zero-fills dgamma and dbeta and does not touch dx.
 * One wave per row with the row in registers; x and dy are read once.  Each workgroup keeps the dgamma / dbeta partial sums of the rows
 * it walks in registers, combines its four waves in a fixed order and stores one [2, width] slab into the workspace; a second kernel
 * sums the slabs per column in a fixed order.  No atomics: the same inputs give the same bits on every launch.  Exactly rows x width
 * elements of dx and width elements each of dgamma and dbeta are written (a ragged last row tile is masked); nothing behind row
 * rows - 1 of x or dy is read.  Every launch goes to `stream`. */
size_t kemr_layernorm_backward_workspace_bytes(int rows, int width);
int kemr_op_layernorm_backward(const float* x_dev, const float* gamma_dev, const void* dy_dev, int dy_dtype /*KEMR_BF16|KEMR_F32*/,
                               float* dx_dev, float* dgamma_dev, float* dbeta_dev, int rows, int width,
                               void* workspace_dev, size_t workspace_bytes, void* stream);
/* The MLP activation of a training step on contiguous bf16 buffers of n elements; kind 0 = QuickGELU x sigmoid(1.702 x), 1 = the exact
 * GELU 0.5 x (1 + erf(x / sqrt 2)).  forward: out = bf16(f(float(pre))) with the arithmetic of the fc1 epilogues
 * (KEMR_EPI_BIAS_QGELU_BF16 / KEMR_EPI_BIAS_GELU_BF16).  backward: dpre = bf16(float(dout) f'(float(pre))), f' = s + 1.702 x s (1 - s)
 * with s = sigmoid(1.702 x), or Phi(x) + x phi(x); fp32 arithmetic, one rounding, at the store.  n >= 0 and a multiple of 8 (16-byte
 * loads and stores; n == 0 launches nothing), 16-byte aligned buffers; another kind, a negative n, an n that is no multiple of 8 or a
 * NULL pointer is KEMR_ERR_INVALID with a message naming the argument, refused on the host before any launch.  Exactly n elements are
 * written; out may be pre itself (in place).  Every launch goes to `stream`; the same bits on every launch. */
int kemr_op_act_forward(const void* pre_dev, void* out_dev, long long n, int kind /*0 QuickGELU, 1 exact GELU*/, void* stream);
int kemr_op_act_backward(const void* pre_dev, const void* dout_dev, void* dpre_dev, long long n, int kind, void* stream);
/* the same with the head dim an argument: 64 = kemr_op_attention; 80 (q pre-scaled by 1/sqrt(80), width % 80 == 0): non-causal, t <= 288.
 * A width that is no multiple of the head dim, another head dim, causal or t > 288 at 80: KEMR_ERR_INVALID, nothing is launched. */
int kemr_op_attention_hd(const void* qkv_dev, void* out_dev, int batch, int t, int width, int head_dim, int causal, void* stream);
/* The kernels of KEMR_PREC_FP32X3.  Panels are what kemr_panel_build(nparts = 1, terms = 3, side) builds: bf16 [ceil256(rows), 3 ceil64(d)],
 * KEMR_SIDE_QUERY = the A side [hi | lo | hi], KEMR_SIDE_GALLERY = the W side [hi | hi | lo].
 * layernorm_x3: x fp32 [rows, width] -> y_panel, the A-side triple of kemr_op_layernorm(..., KEMR_F32)'s output, bit for bit;
 *   [ceil256(rows), 3 width], pad rows zero-filled. */
int kemr_op_layernorm_x3(const float* x_dev, const float* gamma_dev, const float* beta_dev, void* y_panel_dev, int rows, int width,
                         void* stream);
/* gemm_x3: a_panel [ceil256(m), k3] (A side), w_panel [n, k3] (W side), k3 = 3 k with k % 64 == 0, n % 128 == 0, bias fp32 [n] or NULL.
 *   mode 0: c fp32 [m, n] = acc + bias; 1: c fp32 [m, n] += acc + bias; 2 / 3: c = the A-side triple [ceil256(m), 3 n] bf16 of
 *   quick_gelu(acc + bias) / gelu(acc + bias), the activation in fp32 (rows m .. are not written).  One kernel family: 128 x 128 tiles.
 *   In modes 0 / 1 c has EXACTLY m rows: the last 128-row tile is masked at m, row m is not the library's.  a_panel's pad rows are read
 *   and cannot reach a row < m. */
int kemr_op_gemm_x3(const void* a_panel_dev, const void* w_panel_dev, const float* bias_dev, void* c_dev, int m, int n, int k3,
                    int mode /*0 store f32, 1 add into f32 C, 2 quick_gelu -> triple, 3 gelu -> triple*/, void* stream);
/* attention_x3: qkv fp32 [rows, 3 width] (q pre-scaled by 1/sqrt(head dim) = 1/8; heads of 64) -> out_panel, the A-side triple [rows, 3 width] bf16 of
 *   softmax(q k^T) v; rows of the panel that hold no query are not written.  row_start == NULL: batch items of t rows each, t <=
 *   KEMR_MAX_VISION_TOKENS non-causal, t <= KEMR_MAX_TEXT_CTX causal.  row_start (device int32 [batch + 1], causal only): packed
 *   items, item b = rows row_start[b] .. row_start[b + 1] - 1, at most t of them.  Same bits on every launch. */
int kemr_op_attention_x3(const float* qkv_dev, void* out_panel_dev, const int* row_start_dev, int batch, int t, int width, int causal,
                         void* stream);
/* attention_x3 with the head dim an argument: 64 = kemr_op_attention_x3; 80: non-causal, row_start NULL, t <= 288 (d padded to 96 with
 *   zeros the kernel makes, 5 output d-tiles; same three-product convention, same bits on every launch); else KEMR_ERR_INVALID. */
int kemr_op_attention_x3_hd(const float* qkv_dev, void* out_panel_dev, const int* row_start_dev, int batch, int t, int width,
                            int head_dim, int causal, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* KEMR_H_ */
