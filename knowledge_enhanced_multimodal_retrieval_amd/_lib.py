"""ctypes binding of libkemr.so (C ABI declared in include/kemr.h).

The library is the product: there is no CPU or PyTorch fallback.  ``lib()`` raises if the shared object is
missing or does not export every declared symbol, and every wrapper in this package raises
``RuntimeError`` when a call returns a non-zero status.  Loading the library does not touch the GPU
(no HIP call happens until a model is finalised or a kernel is launched), so importing this module is
safe in forked DataLoader workers.
"""
from __future__ import annotations

import ctypes as C
import os
import threading

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(PKG_DIR, "libkemr.so")

KEMR_F32, KEMR_BF16, KEMR_I32, KEMR_FP8 = 0, 1, 2, 3
KEMR_F24 = 24               # internal: the 24-bit rows of the residual stream (csrc/common.h f24_t; debug entry points and tests only)
PREC_BF16 = 1
PREC_BF16_RES16 = 2
PREC_FP8 = 3
PREC_FP8_MLP = 4
PREC_FP8_RES16 = 5
PREC_FP32X3 = 6             # split-bf16 operand pairs, fp32 between the kernels: the fp32-grade reference mode (include/kemr.h)
# default of the product (round 4): bf16 GEMM / attention operands, fp32 accumulation, and the fp32 residual stream STORED as 24-bit
# floats (15-bit mantissa, 128 x finer than bf16: "bf16-x24"; every LayerNorm statistic and residual add is fp32 arithmetic).  It meets
# every bar the 4-byte stream ("bf16") meets -- 1 - cos against the fp32 oracle 3e-6 / 3e-5 (image / text) on plain AND heavy-tailed
# weights, the oracle anchor and the fixed 0.2-point Recall@10 bar on ViT-B/32 and ViT-L/14 (0.00 .. -0.13 points against "bf16":
# profiles/r04_recall_bar*.json), the end-to-end margin rule -- and moves 19 instead of 22 bytes per element and layer through the
# HBM-bound LayerNorm passes (+2 % items/s).  "bf16" keeps the 4-byte stream; "bf16-res16" stores it as bf16 (+4 %, Recall@10 drifts
# 0.5 points on ViT-B/32 and 3-4 points on ViT-L/14 on the stress test): opt-in through KEMR_PRECISION, never the default.
DEFAULT_PRECISION = "bf16-x24"
PRECISIONS = {"bf16": PREC_BF16, "bf16-res16": PREC_BF16_RES16, "fp8": PREC_FP8, "fp8-mlp": PREC_FP8_MLP, "fp8-res16": PREC_FP8_RES16,
              # "-x24": the same arithmetic with the fp32 residual stream stored as 24-bit floats (model option residual_stream_24bit)
              "bf16-x24": PREC_BF16, "fp8-x24": PREC_FP8,
              # every GEMM / attention operand as a bf16 pair, three products each: the reference's fp32 numbers at a third of the rate
              "fp32x3": PREC_FP32X3}
TOWER_VISION, TOWER_TEXT = 0, 1
TRANSFORM_CLIP, TRANSFORM_SIGLIP = 0, 1      # kemr_transform: the kind of kemr_transform_u8 / kemr_transform_u8_batch
SIDE_QUERY, SIDE_GALLERY = 0, 1
EPI_BIAS_BF16, EPI_BIAS_QGELU_BF16, EPI_BIAS_RESID_F32 = 0, 1, 2
EPI_BIAS_RESADD_BF16 = 4
EPI_BIAS_GELU_BF16 = 5      # exact (erf) GELU; 3 is internal to the library
EPI_BIAS_TGELU_BF16 = 8     # tanh GELU ("gelu_pytorch_tanh": the SigLIP family's fc1)
# model option "activation" (include/kemr.h): the MLP's activation, by the name Hugging Face configs give it (`hidden_act`)
ACTIVATIONS = {"quick_gelu": 0, "gelu": 1}
FAMILY_BERT = 2             # kemr_model_create_family: a BERT sentence encoder (text-only)
FAMILY_MPNET = 3            # option "family" of a FAMILY_BERT model: MPNet's relative position bias in every attention score, no token types
MPNET_DISTANCES = 2 * 512 - 1   # columns of the bias table by distance: key - query in -511 .. 511
MAX_BERT_CTX = 512          # KEMR_MAX_BERT_CTX
PAIRHEAD_GATED, PAIRHEAD_LINEAR = 0, 1      # KEMR_PAIRHEAD_*: the mode of kemr_pairhead_forward / _backward
MAX_DEEP_K = 1024           # KEMR_MAX_DEEP_K: longest list of kemr_select_topk / kemr_sim_topk_deep / kemr_sim_topk_deep_fused / kemr_cross_attention_rerank / kemr_list_fuse


class KemrCfg(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("embed_dim", "image_size", "patch", "v_width", "v_layers",
                                          "t_width", "t_layers", "vocab", "ctx")]


_vp, _i, _i64, _f, _sz = C.c_void_p, C.c_int, C.c_int64, C.c_float, C.c_size_t

# name -> (restype, argtypes); must list every symbol include/kemr.h declares (tests check this)
SIGNATURES = {
    "kemr_last_error": (C.c_char_p, []),
    "kemr_abi_version": (_i, []),
    "kemr_model_create": (_i, [C.POINTER(KemrCfg), C.POINTER(_vp)]),
    "kemr_model_create_family": (_i, [C.POINTER(KemrCfg), _i, C.POINTER(_vp)]),
    "kemr_model_load_tensor": (_i, [_vp, C.c_char_p, _vp, _i, C.POINTER(_i64), _i]),
    "kemr_model_finalize": (_i, [_vp, _i]),
    "kemr_model_destroy": (_i, [_vp]),
    "kemr_model_set_option": (_i, [_vp, C.c_char_p, _i]),
    "kemr_model_get_option": (_i, [_vp, C.c_char_p, C.POINTER(_i)]),
    "kemr_model_num_tensors": (_i, [_vp]),
    "kemr_model_tensor_name": (C.c_char_p, [_vp, _i]),
    "kemr_workspace_bytes": (_sz, [_vp, _i, _i]),
    "kemr_encode_image": (_i, [_vp, _vp, _i, _vp, _i, _vp, _sz, _vp]),
    "kemr_encode_text": (_i, [_vp, _vp, _i, _vp, _i, _vp, _sz, _vp]),
    "kemr_text_packed_workspace_bytes": (_sz, [_vp, _i, _i]),
    "kemr_encode_text_packed": (_i, [_vp, _vp, _vp, _i, _i, _vp, _i, _vp, _sz, _vp]),
    "kemr_encode_image_pooled": (_i, [_vp, _vp, _i, _vp, _vp, _sz, _vp]),
    "kemr_encode_text_pooled": (_i, [_vp, _vp, _i, _vp, _vp, _sz, _vp]),
    "kemr_encode_text_packed_pooled": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _sz, _vp]),
    "kemr_panel_kdim": (_i64, [_i, _i, _i]),
    "kemr_panel_build": (_i, [C.POINTER(_vp), C.POINTER(_f), C.POINTER(_vp), _i, _i, _i, _i, _i, _vp, _vp]),
    "kemr_sim_workspace_bytes": (_sz, [_i, _i, _i64, _i]),
    "kemr_sim_topk": (_i, [_vp, _i, _vp, _i, _i64, _i64, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "kemr_pair_scores": (_i, [_vp, _vp, _i64, _vp, _vp, _i, _vp, _vp]),
    "kemr_topk_merge": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _vp]),
    "kemr_scores_dense": (_i, [_vp, _i, _vp, _i, _i64, _vp, _i64, _vp]),
    "kemr_rank_dense": (_i, [_vp, _i, _i, _i64, _vp, _vp, _i, _vp, _vp, _vp]),
    "kemr_rank_dense_shard": (_i, [_vp, _i, _i, _i64, _i64, _vp, _vp, _vp, _i, _vp, _vp, _vp]),
    "kemr_select_topk": (_i, [_vp, _vp, _i, _i, _i64, _i64, _i, _vp, _vp, _vp]),
    "kemr_sim_topk_deep_workspace_bytes": (_sz, [_i, _i, _i64, _i]),
    "kemr_sim_topk_deep": (_i, [_vp, _i, _vp, _i, _i64, _i64, _i, _vp, _vp, _vp, _sz, _vp]),
    "kemr_sim_topk_deep_fused": (_i, [_vp, _i, _vp, _i, _i64, _i64, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "kemr_linear_head": (_i, [_vp, _vp, _i64, _vp, _vp, _vp, _f, _i, _vp, _vp]),
    "kemr_gate_rows": (_i, [_vp, _i, _i, _vp, _vp, _f, _i, _vp, _vp]),
    "kemr_cross_attention_pairs": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _f, _i, _i, _i, _i, _i, _vp, _vp]),
    "kemr_cross_attention_rerank": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _f, _i, _i, _i, _i, _i, _i, _vp, _i, _i64, _vp, _vp]),
    "kemr_list_fuse": (_i, [_vp, _vp, _i, _i, _i64, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "kemr_infonce_workspace_bytes": (_sz, [_i, _i]),
    "kemr_infonce_forward": (_i, [_vp, _vp, _i, _i, _f, _vp, _vp, _vp, _sz, _vp]),
    "kemr_infonce_backward": (_i, [_vp, _vp, _vp, _i, _i, _f, _vp, _vp, _vp, _sz, _vp]),
    "kemr_pairhead_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "kemr_pairhead_forward": (_i, [_i, _vp, _vp, _vp, _i, _i, _f, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _sz, _vp]),
    "kemr_pairhead_backward": (_i, [_i, _vp, _vp, _vp, _vp, _i, _i, _f, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _sz, _vp]),
    "kemr_profile_begin": (_i, [_i]),
    "kemr_profile_end": (_i, [C.POINTER(C.c_double), C.POINTER(_i64), _i]),
    "kemr_op_gemm": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "kemr_preprocess_workspace_bytes": (_sz, [_i, _i, _i]),
    "kemr_preprocess_u8": (_i, [_vp, _i, _i, _i, _vp, _vp, _sz, _vp]),
    "kemr_preprocess_batch_workspace_bytes": (_sz, [_vp, _vp, _i, _i]),
    "kemr_preprocess_u8_batch": (_i, [_vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _sz, _vp]),
    "kemr_transform_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "kemr_transform_u8": (_i, [_i, _vp, _i, _i, _i, _vp, _vp, _sz, _vp]),
    "kemr_transform_batch_workspace_bytes": (_sz, [_i, _vp, _vp, _i, _i]),
    "kemr_transform_u8_batch": (_i, [_i, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _sz, _vp]),
    "kemr_op_gemm_fp8": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "kemr_op_e4m3_host": (_i, [_vp, _vp, C.c_longlong]),
    "kemr_op_layernorm": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _vp]),
    "kemr_op_layernorm_resid": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _vp]),
    "kemr_op_layernorm_rows": (_i, [_vp, _i, _vp, _vp, _i, _vp, _vp, _vp, _i, _i, _i, _vp]),
    "kemr_op_attention": (_i, [_vp, _vp, _i, _i, _i, _i, _vp]),
    "kemr_op_attention_hd": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "kemr_op_attention_backward": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "kemr_op_attention_packed": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp]),
    "kemr_op_attention_backward_packed": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "kemr_attention_backward_long_workspace_bytes": (_sz, [_i, _i, _i]),
    "kemr_op_attention_backward_long": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _sz, _vp]),
    "kemr_attention_backward_hd_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "kemr_op_attention_backward_hd": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _sz, _vp]),
    "kemr_layernorm_backward_workspace_bytes": (_sz, [_i, _i]),
    "kemr_op_layernorm_backward": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _vp, _i, _i, _vp, _sz, _vp]),
    "kemr_op_act_forward": (_i, [_vp, _vp, C.c_longlong, _i, _vp]),
    "kemr_op_act_backward": (_i, [_vp, _vp, _vp, C.c_longlong, _i, _vp]),
    "kemr_op_layernorm_x3": (_i, [_vp, _vp, _vp, _vp, _i, _i, _vp]),
    "kemr_op_gemm_x3": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "kemr_op_attention_x3": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "kemr_op_attention_x3_hd": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
}

# include/kemr_debug.h: experiment switches and diagnostics for tools/ and tests/ (process-wide; not the product ABI)
DEBUG_SIGNATURES = {
    "kemr_debug_set": (_i, [C.c_char_p, _i]),
    "kemr_debug_get": (_i, [C.c_char_p, C.POINTER(_i)]),
    "kemr_debug_sim_lists": (_i, [_vp, _i, _i, _i64, _i, _vp]),
    "kemr_debug_gemm_stamps": (_i, [_vp, _i]),
    "kemr_debug_op_attention_packed": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp]),
    "kemr_debug_op_attention_pooled": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "kemr_debug_op_attention_pooled_hd": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "kemr_debug_op_tail": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _i, _i, _vp, _vp]),
    "kemr_debug_image_tokens": (_i, [_vp, _vp, _i, _vp, _vp, _sz, _vp]),
    "kemr_debug_text_tokens": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _sz, _vp]),
    "kemr_debug_map_head": (_i, [_vp, _vp, _i, _vp, _vp, _i, _vp, _sz, _vp]),
    "kemr_debug_op_attention_varlen": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp]),
    "kemr_debug_op_attention_varlen_bias": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _vp]),
    "kemr_debug_op_layernorm_post": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _i, _i, _f, _vp]),
    "kemr_debug_op_pool_rows": (_i, [_vp, _i, _vp, _i, _i, _i, _i, _vp, _vp]),
    "kemr_debug_bert_front": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _sz, _vp]),
    "kemr_debug_pack_weights": (_i, [_vp, _i, _vp, _sz, C.POINTER(_sz)]),
}
ABI_VERSION = 4

_lock = threading.Lock()
_lib = None


def lib() -> C.CDLL:
    """Load libkemr.so once; raise (never fall back) when it is absent or incomplete."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with `python -m knowledge_enhanced_multimodal_retrieval_amd.build` "
                "(hipcc, gfx950). There is no CPU fallback for this path.")
        # torch must be imported BEFORE the dlopen: PyTorch-ROCm ships its own libamdhip64.so, and libkemr.so's
        # DT_NEEDED libamdhip64.so.7 binds to whichever copy is already in the process.  Loaded the other way round the
        # process ends up with two HIP runtimes and every HIP call of libkemr fails with hipErrorNoDevice.
        import torch  # noqa: F401
        handle = C.CDLL(LIB_PATH)
        for name, (res, args) in list(SIGNATURES.items()) + list(DEBUG_SIGNATURES.items()):
            try:
                fn = getattr(handle, name)
            except AttributeError as e:
                raise RuntimeError(f"{LIB_PATH} does not export {name}; rebuild the library") from e
            fn.restype = res
            fn.argtypes = args
        if handle.kemr_abi_version() != ABI_VERSION:
            raise RuntimeError(f"libkemr.so ABI version {handle.kemr_abi_version()} != {ABI_VERSION}; rebuild the library")
        _lib = handle
        return _lib


def env_precision(environ=None) -> str:
    """The encoder precision the environment asks for: KEMR_PRECISION (a key of PRECISIONS), else DEFAULT_PRECISION.  What `clip.load`,
    `load_clip_model` and the evaluator CLIs pack their model with and record under "precision" in their result JSON."""
    name = (os.environ if environ is None else environ).get("KEMR_PRECISION", "") or DEFAULT_PRECISION
    if name not in PRECISIONS:
        raise ValueError(f"KEMR_PRECISION must be one of {sorted(PRECISIONS)}, got {name!r}")
    return name


def check_activation(activation: str) -> str:
    if activation not in ACTIVATIONS:
        raise ValueError(f"activation must be one of 'quick_gelu' (OpenAI CLIP) or 'gelu' (OpenCLIP / LAION, exact erf GELU), got {activation!r}")
    return activation


def check(status: int, what: str = "") -> None:
    if status != 0:
        msg = lib().kemr_last_error()
        raise RuntimeError(f"libkemr {what} failed ({status}): {msg.decode() if msg else '?'}")
