"""Experiment switches and diagnostics of libkemr.so (include/kemr_debug.h) for tools/ and tests/.

Process-wide and not thread-safe: nothing in the product path (engine, evaluators, retriever, dist, bench.py's timed legs)
calls into this module.  A switch changes which kernel or route runs, never what comes out (tests/ hold every route to the same
results); what does change numerics -- the residual fusion -- is a per-model option (ClipEngine.set_residual_fusion).
"""
from __future__ import annotations

import contextlib
import ctypes as C

from . import _lib

KEYS = ("gemm_variant", "gemm_flags", "gemm_order", "gemm_grid", "gemm_conc", "gemm_kl", "attn_v", "attn_xcd", "attn_waves", "attn80_waves", "sim_lists", "ln_nt")


def ab_variants() -> bool:
    """True when libkemr.so was built with the experiment kernels (``build.py --ab-variants``); the product library refuses the
    switch values that select them."""
    return get("ab_variants") == 1


def set(key: str, value: int) -> None:      # noqa: A001 (module-level verb of a tiny module)
    _lib.check(_lib.lib().kemr_debug_set(key.encode(), int(value)), f"debug_set({key})")


def get(key: str) -> int:
    v = C.c_int(0)
    _lib.check(_lib.lib().kemr_debug_get(key.encode(), C.byref(v)), f"debug_get({key})")
    return v.value


@contextlib.contextmanager
def override(**kv):
    """with debug.override(gemm_variant=2): ...  -- sets the switches, restores what they held before."""
    old = {k: get(k) for k in kv}
    try:
        for k, v in kv.items():
            set(k, v)
        yield
    finally:
        for k, v in old.items():
            set(k, v)


def set_gemm_variant(packed: int) -> None:
    """The packed form tools/ grew up with: bits 0-7 variant, 8-15 flags (both always written), 16-19 tile order + 1,
    20-21 concurrent epilogues + 1, 24-27 attention waves + 1 (written only when non-zero)."""
    set("gemm_variant", packed & 0xff)
    set("gemm_flags", (packed >> 8) & 0xff)
    if (packed >> 16) & 0xf:
        set("gemm_order", ((packed >> 16) & 0xf) - 1)
    if (packed >> 20) & 0x3:
        set("gemm_conc", ((packed >> 20) & 0x3) - 1)
    if (packed >> 24) & 0xf:
        set("attn_waves", ((packed >> 24) & 0xf) - 1)


def sim_lists(workspace, nq: int, ng: int, kdim: int, k: int):
    """flag / longest list / capacity / chunks / sampled rows / records per query of the last candidate-list search that used
    `workspace` (a torch uint8 tensor, e.g. the one engine.sim_topk(..., return_workspace=True) hands back)."""
    out = (C.c_int32 * 6)()
    _lib.check(_lib.lib().kemr_debug_sim_lists(C.c_void_p(workspace.data_ptr()), nq, ng, kdim, k, C.cast(out, C.c_void_p)),
               "debug_sim_lists")
    return list(out)


def gemm_stamps(n_words: int):
    buf = (C.c_uint * n_words)()
    _lib.check(_lib.lib().kemr_debug_gemm_stamps(buf, n_words), "debug_gemm_stamps")
    return buf


# ---- kernels a tower reaches only inside itself (tests/test_numerics_paths_gpu.py); device tensors in, outputs allocated here
def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream(device):
    import torch
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def op_attention_packed(qkv, row_start, max_t: int, width: int):
    """Causal attention over packed items: qkv bf16 [rows, 3 width], row_start int32 [batch + 1] (device) -> bf16 [rows, width]
    (rows no item owns stay 0)."""
    import torch
    out = torch.zeros((qkv.shape[0], width), dtype=torch.bfloat16, device=qkv.device)
    with torch.cuda.device(qkv.device):
        _lib.check(_lib.lib().kemr_debug_op_attention_packed(_ptr(qkv), _ptr(out), _ptr(row_start), row_start.numel() - 1, max_t,
                                                             width, _stream(qkv.device)), "debug_op_attention_packed")
    return out


def op_attention_pooled(q, qkv, pool_idx, row_start, tokens: int, causal: bool, force_long: bool = False, head_dim: int = 64):
    """One query row per item: q bf16 [items, width], k / v from qkv bf16 [rows, 3 width], pool_idx / row_start int32 (device, or
    None) -> bf16 [items, width].  head_dim 64, or 80 (the vision form only: no pool_idx / row_start, tokens <= 288)."""
    import torch
    items, width = q.shape
    out = torch.zeros((items, width), dtype=torch.bfloat16, device=q.device)
    with torch.cuda.device(q.device):
        if head_dim == 64:
            _lib.check(_lib.lib().kemr_debug_op_attention_pooled(_ptr(q), _ptr(qkv), _ptr(out), _ptr(pool_idx), _ptr(row_start), items,
                                                                 tokens, width, 1 if causal else 0, 1 if force_long else 0,
                                                                 _stream(q.device)), "debug_op_attention_pooled")
        else:
            _lib.check(_lib.lib().kemr_debug_op_attention_pooled_hd(_ptr(q), _ptr(qkv), _ptr(out), _ptr(pool_idx), _ptr(row_start), items,
                                                                    tokens, width, int(head_dim), 1 if causal else 0,
                                                                    1 if force_long else 0, _stream(q.device)), "debug_op_attention_pooled_hd")
    return out


def op_tail(x, x_dtype: int, delta, delta2, ids, row_start, batch: int, tokens: int, width: int, gamma, beta, proj,
            normalize: bool):
    """The pooling tail: rows x of x_dtype (_lib.KEMR_F32 / KEMR_BF16 / KEMR_F24) [+ delta [+ delta2]] at the pooled row ->
    LayerNorm -> @ proj fp32 [width, d] (-> / L2 norm) = fp32 [batch, d]."""
    import torch
    d = proj.shape[1]
    out = torch.zeros((batch, d), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().kemr_debug_op_tail(_ptr(x), x_dtype, _ptr(delta), _ptr(delta2), _ptr(ids), _ptr(row_start), batch,
                                                 tokens, width, _ptr(gamma), _ptr(beta), _ptr(proj), d, 1 if normalize else 0,
                                                 _ptr(out), _stream(x.device)), "debug_op_tail")
    return out


# ---- the token fronts of a ClipEngine's encoders (tests/test_numerics_front_gpu.py)
def _front_workspace(eng, need: int, fill: int):
    """The encoders' workspace, every byte `fill` (0xff: NaN in every fp32 / bf16 slot, so a row or pad column a kernel leaves
    unwritten shows up)."""
    import torch
    return torch.full((max(need, 256),), fill, dtype=torch.uint8, device=eng.device)


def image_tokens(eng, pixels, fill: int = 0xff):
    """The fp32 rows [batch * tokens, v_width] the vision tower's ln_pre reads -- im2col, the patch-embedding GEMM with its
    positional-embedding epilogue, the class rows -- for pixels fp32 [batch, 3, S, S] on the engine's device."""
    import torch
    a = eng.arch
    batch = pixels.shape[0]
    pixels = pixels.to(device=eng.device, dtype=torch.float32).contiguous()
    out = torch.empty((batch * a.v_tokens, a.v_width), dtype=torch.float32, device=eng.device)
    ws = _front_workspace(eng, int(_lib.lib().kemr_workspace_bytes(eng._h, _lib.TOWER_VISION, batch)), fill)
    with torch.cuda.device(eng.device):
        _lib.check(_lib.lib().kemr_debug_image_tokens(eng._h, _ptr(pixels), batch, _ptr(out), _ptr(ws), ws.numel(),
                                                      _stream(eng.device)), "debug_image_tokens")
    return out


def map_head(eng, h, batch: int, normalize: bool = False):
    """The pooling head of a SigLIP engine on h = bf16 [batch * tokens, v_width] (post-ln_post token rows) -> (out fp32 [batch, v_width],
    attention output bf16 [batch, v_width])."""
    import torch
    a = eng.arch
    h = h.to(device=eng.device, dtype=torch.bfloat16).contiguous()
    out = torch.empty((batch, a.v_width), dtype=torch.float32, device=eng.device)
    attn = torch.empty((batch, a.v_width), dtype=torch.bfloat16, device=eng.device)
    ws = _front_workspace(eng, int(_lib.lib().kemr_workspace_bytes(eng._h, _lib.TOWER_VISION, batch)), 0)
    with torch.cuda.device(eng.device):
        _lib.check(_lib.lib().kemr_debug_map_head(eng._h, _ptr(h), batch, _ptr(attn), _ptr(out), 1 if normalize else 0, _ptr(ws), ws.numel(),
                                                  _stream(eng.device)), "debug_map_head")
    return out, attn


def residual_dtype(eng) -> int:
    """Storage type of the engine's residual stream: _lib.KEMR_F32, KEMR_BF16 or KEMR_F24."""
    v = C.c_int(0)
    _lib.check(_lib.lib().kemr_model_get_option(eng._h, b"precision_residual_bf16", C.byref(v)), "model_get_option")
    if v.value:
        return _lib.KEMR_BF16
    _lib.check(_lib.lib().kemr_model_get_option(eng._h, b"residual_stream_24bit", C.byref(v)), "model_get_option")
    return _lib.KEMR_F24 if v.value else _lib.KEMR_F32


def text_tokens(eng, ids, lens=None, rows: int = 0, fill: int = 0xff):
    """The residual-stream rows the text tower's first LayerNorm reads.  ids int32 [batch, ctx]; lens None: kemr_encode_text's
    batch * ctx rows; lens int32 [batch] (any values) with `rows` (host int): kemr_encode_text_packed's rows.  Returns (rows, row_start):
    fp32 or bf16 [n, t_width], or the 24-bit rows as uint8 [n, 3 t_width] (engine.pack_f24_rows' layout); row_start int32 [batch + 1]
    (packed) or None."""
    import torch
    a = eng.arch
    batch = ids.shape[0]
    ids = ids.to(device=eng.device, dtype=torch.int32).contiguous()
    L = _lib.lib()
    if lens is None:
        n, need, lens_d, rs = batch * a.ctx, int(L.kemr_workspace_bytes(eng._h, _lib.TOWER_TEXT, batch)), None, None
    else:
        lens_d = torch.as_tensor(lens).to(device=eng.device, dtype=torch.int32).contiguous()
        n, need = rows, int(L.kemr_text_packed_workspace_bytes(eng._h, rows, batch))
        rs = torch.full((batch + 1,), -1, dtype=torch.int32, device=eng.device)
    dt = residual_dtype(eng)
    if dt == _lib.KEMR_F24:
        out = torch.empty((n, 3 * a.t_width), dtype=torch.uint8, device=eng.device)
    else:
        out = torch.empty((n, a.t_width), dtype=torch.bfloat16 if dt == _lib.KEMR_BF16 else torch.float32, device=eng.device)
    ws = _front_workspace(eng, need, fill)
    with torch.cuda.device(eng.device):
        _lib.check(L.kemr_debug_text_tokens(eng._h, _ptr(ids), _ptr(lens_d), rows, batch, _ptr(out), _ptr(rs), _ptr(ws), ws.numel(),
                                            _stream(eng.device)), "debug_text_tokens")
    return out, rs


# ---- the kernels of the BERT family alone (tests/test_bert_ops_gpu.py)
def op_attention_varlen(qkv, row_start, max_t: int, width: int, fill: float = 0.0):
    """Non-causal attention over packed items: qkv bf16 [rows, 3 width], row_start int32 [batch + 1] (device) -> bf16 [rows, width]
    (rows no item owns keep `fill`)."""
    import torch
    out = torch.full((qkv.shape[0], width), fill, dtype=torch.bfloat16, device=qkv.device)
    with torch.cuda.device(qkv.device):
        _lib.check(_lib.lib().kemr_debug_op_attention_varlen(_ptr(qkv), _ptr(out), _ptr(row_start), row_start.numel() - 1, max_t, width,
                                                             _stream(qkv.device)), "debug_op_attention_varlen")
    return out


def op_attention_varlen_bias(qkv, row_start, bias_by_distance, max_t: int, width: int, fill: float = 0.0):
    """op_attention_varlen with MPNet's relative position bias: bias_by_distance fp32 [width / 64, 1023] (device), entry [h][d + 511]
    added to the scores of head h at key - query = d."""
    import torch
    if bias_by_distance.dtype != torch.float32 or tuple(bias_by_distance.shape) != (width // 64, _lib.MPNET_DISTANCES) or not bias_by_distance.is_contiguous():
        raise ValueError(f"bias_by_distance must be contiguous fp32 [{width // 64}, {_lib.MPNET_DISTANCES}], got {bias_by_distance.dtype} {tuple(bias_by_distance.shape)}")
    out = torch.full((qkv.shape[0], width), fill, dtype=torch.bfloat16, device=qkv.device)
    with torch.cuda.device(qkv.device):
        _lib.check(_lib.lib().kemr_debug_op_attention_varlen_bias(_ptr(qkv), _ptr(out), _ptr(row_start), _ptr(bias_by_distance), row_start.numel() - 1,
                                                                  max_t, width, _stream(qkv.device)), "debug_op_attention_varlen_bias")
    return out


def op_layernorm_post(x, x_dtype: int, delta, gamma, beta, rows: int, width: int, eps: float):
    """The post-LN form in place on a copy of x (fp32 / bf16 [rows, width], or uint8 [rows, 3 width] 24-bit rows): -> (x', h bf16)."""
    import torch
    x = x.clone()
    h = torch.empty((rows, width), dtype=torch.bfloat16, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().kemr_debug_op_layernorm_post(_ptr(x), x_dtype, _ptr(delta), _ptr(gamma), _ptr(beta), _ptr(h), rows, width,
                                                           float(eps), _stream(x.device)), "debug_op_layernorm_post")
    return x, h


def op_pool_rows(x, x_dtype: int, row_start, width: int, pooling: int, normalize: bool):
    """The sentence encoders' pooling tail: stream rows x, row_start int32 [batch + 1] -> fp32 [batch, width]."""
    import torch
    batch = row_start.numel() - 1
    out = torch.empty((batch, width), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().kemr_debug_op_pool_rows(_ptr(x), x_dtype, _ptr(row_start), batch, width, pooling, 1 if normalize else 0,
                                                      _ptr(out), _stream(x.device)), "debug_op_pool_rows")
    return out


def bert_front(eng, ids, lens, rows: int, fill: int = 0xff):
    """The embedding front of a BertEngine: -> (stream rows: fp32 / bf16 [rows, width] or uint8 [rows, 3 width], h bf16 [rows, width],
    row_start int32 [batch + 1])."""
    import torch
    a = eng.arch
    batch = ids.shape[0]
    ids = ids.to(device=eng.device, dtype=torch.int32).contiguous()
    lens_d = torch.as_tensor(lens).to(device=eng.device, dtype=torch.int32).contiguous()
    dt = residual_dtype(eng)
    if dt == _lib.KEMR_F24:
        x = torch.empty((rows, 3 * a.width), dtype=torch.uint8, device=eng.device)
    else:
        x = torch.empty((rows, a.width), dtype=torch.bfloat16 if dt == _lib.KEMR_BF16 else torch.float32, device=eng.device)
    h = torch.empty((rows, a.width), dtype=torch.bfloat16, device=eng.device)
    rs = torch.full((batch + 1,), -1, dtype=torch.int32, device=eng.device)
    L = _lib.lib()
    ws = _front_workspace(eng, int(L.kemr_text_packed_workspace_bytes(eng._h, rows, batch)), fill)
    with torch.cuda.device(eng.device):
        _lib.check(L.kemr_debug_bert_front(eng._h, _ptr(ids), _ptr(lens_d), rows, batch, _ptr(x), _ptr(h), _ptr(rs), _ptr(ws), ws.numel(),
                                           _stream(eng.device)), "debug_bert_front")
    return x, h, rs
