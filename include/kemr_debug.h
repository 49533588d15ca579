/*
 * kemr_debug.h -- experiment switches and diagnostics of libkemr.so for tools/ and tests/.
 *
 * NOT part of the product ABI (include/kemr.h): everything here is process-wide, not thread-safe, and may change a caller's
 * timing or route -- never its results, which tests/ check on every route.  Per-model behaviour that does change numerics
 * (the residual fusion) is a model option in kemr.h (kemr_model_set_option), not a switch here.
 */
#ifndef KEMR_DEBUG_H_
#define KEMR_DEBUG_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* One key per switch; a call touches that switch only.
 * PRODUCT library (the default build): a switch only ROUTES between kernels the product needs anyway.  The experiment kernels of
 * rounds 1-3 (earlier GEMM generations, the staggered 256x256 GEMM, the long-interval K loop, the stamped / store-dropping GEMM
 * instantiations, the attention variants) are compiled only by `python -m knowledge_enhanced_multimodal_retrieval_amd.build
 * --ab-variants`; without them every value marked [A/B] below is refused with KEMR_ERR_INVALID.  "ab_variants" (read-only) says
 * which library this is.
 *   "gemm_variant"  0 = automatic (default), 1 = 128x128x64 / 4 waves, 2 = 256x256x64 / 8 waves in lockstep,
 *                   7 = persistent 8 waves with one K-tile pipeline across tiles (the automatic choice from 128 tiles up),
 *                   8 = skinny-M split-K (automatic up to 512 rows); [A/B] 3 = 256x256x64 staggered, 4, 5, 6, 9 = earlier
 *                   persistent generations
 *   "gemm_flags"    [A/B] timing experiments of the persistent GEMM's diagnostic instantiation: 1 = drop the C stores, 4 = plain
 *                   instead of non-temporal stores, 64 (+ 32) = cycle stamps per barrier interval, 128 = whole-kernel clock
 *   "gemm_order"    tile order of the persistent GEMM: 0 = N fastest, else log2(column-group width) + 1 (default 3)
 *   "gemm_grid"     cap on the persistent GEMM's grid = the CUs it may take (0 = one workgroup per CU, the default); results do not depend on it
 *   "gemm_conc"     both wave halves' epilogues in one barrier interval: 0 never, 1 always, 2 = QuickGELU epilogue only (default)
 *   "gemm_kl"       K loop of the persistent GEMM: 0 = eight 256-cycle barrier intervals per K-tile (the product loop),
 *                   [A/B] 1 = four of 512
 *   "attn_v"        attention kernel at T = 257: 0 = the product kernel (16-query tiles, 4 waves); [A/B, csrc/attention_ab.hip]
 *                   1 = 32-query tiles on v_mfma_f32_32x32x16_bf16, 2 = eight waves per workgroup with the keys in two halves
 *                   (online softmax), 3 = as 2, one persistent workgroup per CU, the next head's K / V by LDS-DMA while this one
 *                   is computed, 4 = two query tiles per pass sharing the K / V fragments (half the LDS bytes per tile)
 *   "attn_xcd"      attention: 1 = XCD x computes the images = x (mod 8), the heads of an image next to each other in time
 *                   (default), 0 = grid order
 *   "attn_waves"    [A/B] waves per workgroup at T = 257: 0 = default (4 for attn_v 0, 16 for attn_v 3), 6 (attn_v 0), 8 (attn_v 3);
 *                   2 (attn_v 0) = the build with s_memtime stamps, which writes 8 counters per wave BEHIND the output
 *                   (tools/prof_attention.py allocates the room; nothing else may select it)
 *   "attn80_waves"  waves per workgroup of the head-dim-80 attention kernel at T = 257 (csrc/attention80.hip): 0 or 8 = eight (two per
 *                   SIMD, the default), 4 = four (one per SIMD); both instantiations are in the product library, same results bit for bit
 *   "sim_lists"     kemr_sim_topk: 0 = never the candidate-list route (nor the fast rank pass for bonus lists), 1 = where it pays
 *                   (default: from 2 048 gallery rows, 256 queries and 1.2e10 multiply-adds up), 3 = wherever it fits, 2 = as 3 and
 *                   the exact fallback forced to run after the lists
 *   "ln_nt"         LayerNorm cache hints: 3 = deltas and residual rows loaded, the ln_1 write-back of x stored non-temporally (the product
 *                   kernel); [A/B] 0 = plain (rounds 1-3), 1 = deltas only, 2 = deltas + row loads
 *   "attn_waves"    also: [A/B] 7 = the vision attention kernel with plain K / V loads (rounds 1-3), 5 = Q rows non-temporal as well,
 *                   8 (with attn_v 0) = TIMING ONLY, wrong results: the ragged 17th query tile (one valid row) is not computed
 *   "ab_variants"   read-only: 1 = the library holds the [A/B] kernels
 *   "staging_slots" read-only: pinned staging slots the transforms' host-to-device copies leave from (8 to begin with, 64 at most)
 *   "staging_grown" read-only: how often such a slot took a larger buffer and kept the one it had outgrown */
int kemr_debug_set(const char* key, int value);
int kemr_debug_get(const char* key, int* value);

/* flag / longest list / capacity / chunks / sampled rows / records per query left in `workspace` by the last kemr_sim_topk of
 * these sizes on the candidate-list route (all zero when the route does not apply; synchronises the device) */
int kemr_debug_sim_lists(const void* workspace_dev, int nq, int ng, int64_t kdim, int k, int32_t* out6);

/* cycle sums the persistent GEMM's diagnostic instantiation left behind ("gemm_flags" 64): 16 words per workgroup = the barrier
 * intervals of the K loop, K-loop tail, epilogue, tiles, K-tiles per tile.  Synchronises the device. */
int kemr_debug_gemm_stamps(unsigned* host_out, int n_words);

/* Kernels the product reaches only inside a tower, each a pass-through to its launcher (tests/test_numerics_paths_gpu.py).  Device
 * pointers; row_start_dev: batch + 1 ints, item b = the rows row_start[b] .. row_start[b + 1] - 1 (may be NULL where marked).
 * causal attention over packed items: qkv bf16 [rows, 3 width] (q pre-scaled by 1/8) -> out bf16 [rows, width], every length in
 * 1 .. max_t <= KEMR_MAX_TEXT_CTX (up to 128: the tile kernels; above: the causal streaming kernel).  Exactly the rows row_start[0] .. row_start[batch] - 1 of out are written; an item's keys are its own rows (the
 * rows before row_start[0] and the next item's cannot reach it); batch + 1 ints of row_start are read */
int kemr_debug_op_attention_packed(const void* qkv_dev, void* out_dev, const int* row_start_dev, int batch, int max_t, int width,
                                   void* stream);
/* the attention of one query row per item (the last block of a tower): q bf16 [items, width], k / v from qkv bf16 [rows, 3 width],
 * out bf16 [items, width]; keys of item b: vision (causal 0) the `tokens` rows from row_start[b] (NULL: b * tokens), text (causal 1)
 * the rows from row_start[b] (NULL: b * tokens) up to pool_idx[b], at least 1 and at most the instantiation's.  force_long = 1: the
 * 1088-key instantiation even for tokens <= 320.  Exactly items x width elements of out are written; `items` ints of pool_idx and of
 * row_start are read; no key row outside an item's can reach its output */
int kemr_debug_op_attention_pooled(const void* q_dev, const void* qkv_dev, void* out_dev, const int* pool_idx_dev,
                                   const int* row_start_dev, int items, int tokens, int width, int causal, int force_long, void* stream);
/* the same with the head dim an argument: 64 = the call above; 80 (q pre-scaled by 1/sqrt(80), width a multiple of 80): the vision form
 * only -- causal 0, pool_idx_dev, row_start_dev NULL, force_long 0, tokens <= 288; anything else, and any other head dim, is
 * KEMR_ERR_INVALID and launches nothing */
int kemr_debug_op_attention_pooled_hd(const void* q_dev, const void* qkv_dev, void* out_dev, const int* pool_idx_dev,
                                      const int* row_start_dev, int items, int tokens, int width, int head_dim, int causal, int force_long,
                                      void* stream);
/* the pooling tail: x rows of x_dtype (KEMR_F32, KEMR_BF16 or 24 = the 24-bit rows of the residual stream, W bf16 upper halves
 * then W third bytes per row) [+ delta [+ delta2]] (bf16, may be NULL) at the pooled row -- b * tokens (ids NULL) or the first
 * arg-max of ids [batch, tokens], inside row_start's rows when given (clamped to the item's last row) -- LayerNorm(gamma, beta)
 * @ proj fp32 [width, d] -> out fp32 [batch, d]; normalize != 0: each row divided by its L2 norm.  d % 4 == 0, batch <= 65535.
 * Exactly batch x d floats of out are written (a d that is no multiple of the 64-column block is masked); read: the pooled rows of x
 * and the deltas, batch x tokens ids, batch + 1 ints of row_start, width x d floats of proj */
int kemr_debug_op_tail(const void* x_dev, int x_dtype, const void* delta_dev, const void* delta2_dev, const int32_t* ids_dev,
                       const int* row_start_dev, int batch, int tokens, int width, const float* gamma_dev, const float* beta_dev,
                       const float* proj_dev, int d, int normalize, float* out_dev, void* stream);

/* The token fronts of the encoders (tests/test_numerics_front_gpu.py): the same argument checks, workspace (kemr_workspace_bytes /
 * kemr_text_packed_workspace_bytes) and launches as kemr_encode_image / kemr_encode_text / kemr_encode_text_packed up to the rows
 * the first LayerNorm reads, then a copy of those rows to out_dev.  The encoders' memory contract (include/kemr.h): a workspace of exactly
 * the stated size is enough, its contents don't matter, a small or misaligned one is refused before anything is launched.
 * image: im2col, the patch-embedding GEMM and the class rows -> fp32 [batch * tokens, v_width] (family 1: no class rows, the conv bias added).
 * text: lens_dev NULL = kemr_encode_text's batch * ctx rows, else kemr_encode_text_packed's `rows` rows and row_start_out_dev gets the
 * batch + 1 row starts; the rows in the residual stream's storage type: fp32, bf16 or 24-bit (3 t_width bytes per row: the bf16
 * upper halves, then the third bytes). */
int kemr_debug_image_tokens(struct kemr_model* m, const float* pixels_dev, int batch, float* out_dev, void* workspace_dev,
                            size_t workspace_bytes, void* stream);
int kemr_debug_text_tokens(struct kemr_model* m, const int32_t* ids_dev, const int32_t* lens_dev, int rows, int batch, void* out_dev,
                           int* row_start_out_dev, void* workspace_dev, size_t workspace_bytes, void* stream);

/* The pooling head of a family-1 (SigLIP) model alone (tests/test_siglip_ops_gpu.py): h_dev = bf16 [batch * tokens, v_width], the
 * ln_post output of every token row, is copied into the workspace (kemr_workspace_bytes of the vision tower), then the head's launches
 * as kemr_encode_image makes them -- k | v GEMM, the one learned query's attention, out-proj, LayerNorm, fc1 + tanh GELU, fc2, add
 * [, L2 normalise] -> out_dev fp32 [batch, v_width]; attn_out_dev (may be NULL) gets the attention output rows, bf16 [batch, v_width].
 * Workspace: exactly kemr_workspace_bytes is enough, contents don't matter (the pad rows of the copied h included), refusals as above */
int kemr_debug_map_head(struct kemr_model* m, const void* h_dev, int batch, void* attn_out_dev, float* out_dev, int normalize,
                        void* workspace_dev, size_t workspace_bytes, void* stream);

/* The kernels of model family 2 (BERT sentence encoders) alone (tests/test_bert_ops_gpu.py), each a pass-through to its launcher.
 * attention_varlen: NON-causal attention over packed items, qkv bf16 [rows, 3 width] (heads of 64, q pre-scaled by 1/8) -> out bf16
 *   [rows, width]; item b = the rows row_start[b] .. row_start[b + 1] - 1, 1 .. max_t <= KEMR_MAX_BERT_CTX of them.  Exactly the rows
 *   row_start[0] .. row_start[batch] - 1 of out are written; no row outside an item's own can reach its output.
 * layernorm_post: the post-LN form, o = LayerNorm(x + delta) (delta bf16 [rows, width]); x (x_dtype KEMR_F32, KEMR_BF16 or 24) is
 *   overwritten with o in its storage type, h bf16 [rows, width] = bf16(o).  Exactly rows x width elements of each are touched.
 * pool_rows: out fp32 [batch, width] = per item the mean of its rows of x (pooling 0) or its first row (pooling 1), divided by its L2
 *   norm when normalize != 0.
 * bert_front: kemr_encode_text_packed's checks, workspace and launches up to the first QKV GEMM of a family-2 model: x_out = the `rows`
 *   stream rows (the model's storage type), h_out = their bf16 copies, row_start_out = the batch + 1 row starts. */
int kemr_debug_op_attention_varlen(const void* qkv_dev, void* out_dev, const int* row_start_dev, int batch, int max_t, int width,
                                   void* stream);
/* attention_varlen_bias (model family 3, MPNet; tests/test_mpnet_ops_gpu.py): the same launch with a learned relative position bias,
 *   scores = q . k^T + bias_by_distance[h][(key - query) + 511]; bias_by_distance_dev fp32 [width / 64, 1023], read-only.  The same
 *   rows are written and the same refusals hold; a null table is refused here (kemr_debug_op_attention_varlen is the launch without). */
int kemr_debug_op_attention_varlen_bias(const void* qkv_dev, void* out_dev, const int* row_start_dev, const float* bias_by_distance_dev,
                                        int batch, int max_t, int width, void* stream);
int kemr_debug_op_layernorm_post(void* x_dev, int x_dtype, const void* delta_dev, const float* gamma_dev, const float* beta_dev,
                                 void* h_dev, int rows, int width, float eps, void* stream);
int kemr_debug_op_pool_rows(const void* x_dev, int x_dtype, const int* row_start_dev, int batch, int width, int pooling, int normalize,
                            float* out_dev, void* stream);
int kemr_debug_bert_front(struct kemr_model* m, const int32_t* ids_dev, const int32_t* lens_dev, int rows, int batch, void* x_out_dev,
                          void* h_out_dev, int* row_start_out_dev, void* workspace_dev, size_t workspace_bytes, void* stream);

/* The pack step of kemr_model_finalize alone (tests/test_pack_host.py), on the host: the bytes finalize would upload as the device arena
 * for `precision` -- every required tensor in kemr_model_tensor_name order, each entry on a multiple of 256 bytes; the per-row scales of an
 * e4m3 matrix in front of it, the pooling head's query behind the probe.  *bytes = the arena's size; host_out == NULL returns the size
 * only, else `capacity` must reach it.  The same refusals as kemr_model_finalize (codes and messages), no GPU call, and the loaded
 * tensors stay loaded: it runs on a machine without a device and kemr_model_finalize may follow. */
int kemr_debug_pack_weights(const struct kemr_model* m, int precision, void* host_out, size_t capacity, size_t* bytes);

#ifdef __cplusplus
}
#endif
#endif /* KEMR_DEBUG_H_ */
