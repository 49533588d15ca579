"""Hugging Face ``CLIPModel`` checkpoints (``save_pretrained`` directories) for the HIP engine.

The reference evaluates its published fine-tuned model through ``transformers.CLIPModel``
(reference: src/clip/eval/evaluator_hf.py:115,130,144,280).  That class stores the same network under other names: towers
``vision_model.*`` / ``text_model.*``, separate ``q_proj`` / ``k_proj`` / ``v_proj``, ``nn.Linear`` projections (so the matrices
are transposed), ``pre_layrnorm`` (its spelling) / ``post_layernorm`` / ``final_layer_norm``.  This module maps such a state
dict onto the OpenAI names the engine loads, and reads ``config.json`` into a :class:`ClipArch` plus the activation.

``transformers.SiglipModel`` directories (``config.json`` with ``model_type: "siglip"``) take the second route of this module:
:func:`arch_from_siglip_config` and :func:`from_siglip_state_dict` map them onto the names the engine's SigLIP family loads.

``transformers.BertModel`` directories (``model_type: "bert"``: the sentence encoders E5 and GTE of the reference's text-to-text
baselines) take the third: :func:`arch_from_bert_config` (with the sentence-transformers files ``1_Pooling/config.json`` and
``sentence_bert_config.json`` where present) and :func:`from_bert_state_dict`.

``transformers.MPNetModel`` directories (``model_type: "mpnet"``: all-mpnet-base-v2, the baselines' third sentence encoder) are read
by :func:`read_sentence_directory` alone, the route of ``SentenceEncoder.from_pretrained``: :func:`arch_from_mpnet_config`,
:func:`from_mpnet_state_dict`, and the bucket rule of MPNet's relative position bias (:func:`relative_position_bucket`,
:func:`bias_by_distance`) as the library applies it.  :func:`read_hf_directory` (``clip.load``) keeps refusing them.

Local files only: nothing here (or anywhere in the package) contacts a model hub.
"""
from __future__ import annotations

import json
import os
from typing import Dict, Mapping, Tuple

import torch

from .config import ARCHS, MPNET_EPS, BertArch, ClipArch

# what transformers.CLIPTextConfig / CLIPVisionConfig / CLIPConfig assume for a field that config.json leaves out
_TEXT_DEFAULTS = dict(hidden_size=512, intermediate_size=2048, num_attention_heads=8, num_hidden_layers=12, vocab_size=49408,
                      max_position_embeddings=77, hidden_act="quick_gelu", eos_token_id=49407)
_VISION_DEFAULTS = dict(hidden_size=768, intermediate_size=3072, num_attention_heads=12, num_hidden_layers=12, image_size=224,
                        patch_size=32, hidden_act="quick_gelu")
_ACTS = ("quick_gelu", "gelu")
WEIGHT_FILES = ("model.safetensors", "pytorch_model.bin")


def _tower(cfg: Mapping, key: str, defaults: dict) -> dict:
    sub = cfg.get(key)
    if not isinstance(sub, Mapping):
        raise ValueError(f"HF config: '{key}' is missing (not a CLIPModel config)")
    return {**defaults, **{k: v for k, v in sub.items() if v is not None}}


def arch_and_activation_from_hf_config(cfg: Mapping) -> Tuple[ClipArch, str]:
    """``config.json`` of a ``CLIPModel`` (as a dict; the kwargs of ``CLIPConfig`` work too) -> (ClipArch, "quick_gelu" | "gelu").
    Everything the kernels do not serve is refused with the name of the field: heads of another size than 64, an MLP that is not
    4 x the width, widths that are not multiples of 256, other activations, and an end-of-text id the pooling would miss."""
    t, v = _tower(cfg, "text_config", _TEXT_DEFAULTS), _tower(cfg, "vision_config", _VISION_DEFAULTS)
    for side, c in (("text_config", t), ("vision_config", v)):
        w, heads = int(c["hidden_size"]), int(c["num_attention_heads"])
        if w <= 0 or w % 256:
            raise ValueError(f"HF config: {side}.hidden_size = {w} is not a multiple of 256 (the kernels' tile)")
        if heads <= 0 or w != 64 * heads:
            raise ValueError(f"HF config: {side}.num_attention_heads = {heads} at hidden_size {w} is a head dim of "
                             f"{w / max(heads, 1):g}; Hugging Face directories are served at head dim 64 only.  ViT-H/14 (head dim 80) "
                             "is served from its OpenCLIP file -- clip.load('ViT-H-14@/path/open_clip_pytorch_model.bin', "
                             "activation='gelu'), which LAION's repositories ship next to the HF weights; ViT-g (88) is not served")
        if int(c["intermediate_size"]) != 4 * w:
            raise ValueError(f"HF config: {side}.intermediate_size = {c['intermediate_size']} is not 4 x hidden_size ({4 * w})")
        if c["hidden_act"] not in _ACTS:
            raise ValueError(f"HF config: {side}.hidden_act = {c['hidden_act']!r}; served: 'quick_gelu' and 'gelu'")
    if t["hidden_act"] != v["hidden_act"]:
        raise ValueError(f"HF config: hidden_act differs between the towers (text {t['hidden_act']!r}, vision {v['hidden_act']!r}); "
                         "the activation is one option per model")
    dims = {cfg.get("projection_dim"), t.get("projection_dim"), v.get("projection_dim")} - {None}
    if len(dims) != 1:
        raise ValueError(f"HF config: projection_dim must be given and agree between the model and its towers, got {sorted(dims)}")
    vocab, eos = int(t["vocab_size"]), int(t["eos_token_id"])
    # the engine pools the FIRST position of the row maximum.  transformers pools the first eos_token_id, or, for the legacy value 2
    # of the original conversions, argmax(input_ids): the same row when the end-of-text token is the largest id of the vocabulary.
    if eos != vocab - 1 and eos != 2:
        raise ValueError(f"HF config: text_config.eos_token_id = {eos} is neither the largest id of the vocabulary ({vocab - 1}) nor "
                         "the legacy value 2: the pooled row would not be the first position of the row maximum")
    image, patch = int(v["image_size"]), int(v["patch_size"])
    if patch <= 0 or image % patch:
        raise ValueError(f"HF config: vision_config.image_size = {image} is not a multiple of patch_size {patch}")
    arch = ClipArch(int(dims.pop()), image, patch, int(v["hidden_size"]), int(v["num_hidden_layers"]), int(t["hidden_size"]),
                    int(t["num_hidden_layers"]), vocab=vocab, ctx=int(t["max_position_embeddings"]))
    return arch, t["hidden_act"]


LONGCLIP_KEEP = 20        # positions of CLIP's own table that Long-CLIP keeps as they are


def fold_longclip_positions(sd: Mapping[str, torch.Tensor], keep: int = LONGCLIP_KEEP, ctx: int = 0) -> Dict[str, torch.Tensor]:
    """Long-CLIP's released files are OpenAI-named state dicts with TWO positional tables of the same shape ``[248, W]``:
    ``positional_embedding`` and ``positional_embedding_res``.  The published model adds ``positional_embedding * mask1 +
    positional_embedding_res * mask2`` to the token embeddings, ``mask1`` 1 on the positions 0 .. keep - 1 and ``mask2`` 1 on the
    positions keep .. 247 (keep = 20: the positions of CLIP's table the interpolation left untouched).  The table the model adds is
    therefore ``cat(positional_embedding[:keep], positional_embedding_res[keep:])``, and that is what this function returns under
    ``positional_embedding``, with ``positional_embedding_res`` removed: a dict ``CLIP.load_state_dict`` loads strictly.

    A dict without ``positional_embedding_res`` (any CLIP dict; a Long-CLIP one folded earlier) is returned as it is.  Two tables of
    different shapes, or -- with ``ctx`` given (the architecture's) -- tables of another length, are a ``ValueError`` that names both
    shapes; ``positional_embedding_res`` without ``positional_embedding`` is a ``KeyError``.  The rule is the published model code's as
    far as it is known here; it was not checked against a released file, hence ``keep`` is a parameter."""
    if "positional_embedding_res" not in sd:
        return dict(sd)
    if "positional_embedding" not in sd:
        raise KeyError("state dict: 'positional_embedding_res' without 'positional_embedding'")
    pos, res = sd["positional_embedding"], sd["positional_embedding_res"]
    if pos.dim() != 2 or tuple(pos.shape) != tuple(res.shape):
        raise ValueError(f"state dict: positional_embedding {tuple(pos.shape)} and positional_embedding_res {tuple(res.shape)} differ in shape")
    if ctx and pos.shape[0] != ctx:
        raise ValueError(f"state dict: positional_embedding {tuple(pos.shape)} and positional_embedding_res {tuple(res.shape)} do not "
                         f"hold the architecture's {ctx} positions")
    if not 0 <= keep <= pos.shape[0]:
        raise ValueError(f"fold_longclip_positions: keep = {keep} outside 0 .. {pos.shape[0]}")
    out = {k: v for k, v in sd.items() if k != "positional_embedding_res"}
    out["positional_embedding"] = torch.cat([pos[:keep], res[keep:].to(pos.dtype)], dim=0).contiguous()
    return out


def registered_name(arch: ClipArch) -> str:
    """The name ``arch`` is registered under in config.ARCHS, or "" for a shape of its own."""
    return next((n for n, a in ARCHS.items() if a == arch), "")


def from_hf_state_dict(sd: Mapping[str, torch.Tensor], arch: ClipArch) -> Dict[str, torch.Tensor]:
    """``CLIPModel.state_dict()`` -> the OpenAI-CLIP names and layouts (``CLIP.load_state_dict`` then loads it strictly): q | k | v
    concatenated into ``in_proj_*``, the two projection matrices transposed, nothing else changed.  ``position_ids`` buffers are
    ignored; a missing key and any key left over are errors that name it."""
    left = {k: v for k, v in sd.items() if not k.endswith("position_ids")}
    out: Dict[str, torch.Tensor] = {}

    def take(key: str) -> torch.Tensor:
        if key not in left:
            raise KeyError(f"HF state dict: missing key '{key}'")
        return left.pop(key)

    def blocks(src: str, dst: str, layers: int) -> None:
        for i in range(layers):
            s, d = f"{src}.encoder.layers.{i}", f"{dst}.resblocks.{i}"
            out[f"{d}.ln_1.weight"], out[f"{d}.ln_1.bias"] = take(f"{s}.layer_norm1.weight"), take(f"{s}.layer_norm1.bias")
            out[f"{d}.attn.in_proj_weight"] = torch.cat([take(f"{s}.self_attn.{p}_proj.weight") for p in "qkv"], dim=0)
            out[f"{d}.attn.in_proj_bias"] = torch.cat([take(f"{s}.self_attn.{p}_proj.bias") for p in "qkv"], dim=0)
            out[f"{d}.attn.out_proj.weight"], out[f"{d}.attn.out_proj.bias"] = take(f"{s}.self_attn.out_proj.weight"), take(f"{s}.self_attn.out_proj.bias")
            out[f"{d}.ln_2.weight"], out[f"{d}.ln_2.bias"] = take(f"{s}.layer_norm2.weight"), take(f"{s}.layer_norm2.bias")
            out[f"{d}.mlp.c_fc.weight"], out[f"{d}.mlp.c_fc.bias"] = take(f"{s}.mlp.fc1.weight"), take(f"{s}.mlp.fc1.bias")
            out[f"{d}.mlp.c_proj.weight"], out[f"{d}.mlp.c_proj.bias"] = take(f"{s}.mlp.fc2.weight"), take(f"{s}.mlp.fc2.bias")

    out["visual.conv1.weight"] = take("vision_model.embeddings.patch_embedding.weight")
    out["visual.class_embedding"] = take("vision_model.embeddings.class_embedding")
    out["visual.positional_embedding"] = take("vision_model.embeddings.position_embedding.weight")
    out["visual.ln_pre.weight"], out["visual.ln_pre.bias"] = take("vision_model.pre_layrnorm.weight"), take("vision_model.pre_layrnorm.bias")
    blocks("vision_model", "visual.transformer", arch.v_layers)
    out["visual.ln_post.weight"], out["visual.ln_post.bias"] = take("vision_model.post_layernorm.weight"), take("vision_model.post_layernorm.bias")
    out["visual.proj"] = take("visual_projection.weight").t().contiguous()
    out["token_embedding.weight"] = take("text_model.embeddings.token_embedding.weight")
    out["positional_embedding"] = take("text_model.embeddings.position_embedding.weight")
    blocks("text_model", "transformer", arch.t_layers)
    out["ln_final.weight"], out["ln_final.bias"] = take("text_model.final_layer_norm.weight"), take("text_model.final_layer_norm.bias")
    out["text_projection"] = take("text_projection.weight").t().contiguous()
    out["logit_scale"] = take("logit_scale")
    if left:
        raise KeyError(f"HF state dict: unexpected key '{sorted(left)[0]}' ({len(left)} left over; not a CLIPModel of this architecture)")
    return out


# what transformers.SiglipTextConfig / SiglipVisionConfig assume for a field that config.json leaves out
_SIGLIP_TEXT_DEFAULTS = dict(hidden_size=768, intermediate_size=3072, num_attention_heads=12, num_hidden_layers=12, vocab_size=32000,
                             max_position_embeddings=64, hidden_act="gelu_pytorch_tanh", layer_norm_eps=1e-6)
_SIGLIP_VISION_DEFAULTS = dict(hidden_size=768, intermediate_size=3072, num_attention_heads=12, num_hidden_layers=12, image_size=224,
                               patch_size=16, hidden_act="gelu_pytorch_tanh", layer_norm_eps=1e-6, vision_use_head=True)
SIGLIP_ACT = "gelu_pytorch_tanh"


def arch_from_siglip_config(cfg: Mapping) -> ClipArch:
    """``config.json`` of a ``SiglipModel`` (as a dict) -> a ClipArch of family "siglip".  Everything the kernels do not serve is
    refused with the name of the field: heads of another size than 64 (so400m: 1152 / 16 = 72), an MLP that is not 4 x the width,
    widths that are not multiples of 256, another activation than ``gelu_pytorch_tanh``, another ``layer_norm_eps`` than 1e-6, a vision
    tower without the pooling head, a text head that does not project to the vision width."""
    t, v = _tower(cfg, "text_config", _SIGLIP_TEXT_DEFAULTS), _tower(cfg, "vision_config", _SIGLIP_VISION_DEFAULTS)
    for side, c in (("text_config", t), ("vision_config", v)):
        w, heads = int(c["hidden_size"]), int(c["num_attention_heads"])
        if w <= 0 or w % 256:
            raise ValueError(f"HF config: {side}.hidden_size = {w} is not a multiple of 256 (the kernels' tile)")
        if heads <= 0 or w != 64 * heads:
            raise ValueError(f"HF config: {side}.num_attention_heads = {heads} at hidden_size {w} is a head dim of "
                             f"{w / max(heads, 1):g}; SigLIP is served at head dim 64 only (B/16 and L/16; so400m has heads of 72)")
        if int(c["intermediate_size"]) != 4 * w:
            raise ValueError(f"HF config: {side}.intermediate_size = {c['intermediate_size']} is not 4 x hidden_size ({4 * w})")
        if c["hidden_act"] != SIGLIP_ACT:
            raise ValueError(f"HF config: {side}.hidden_act = {c['hidden_act']!r}; the SigLIP family is served with {SIGLIP_ACT!r} only")
        if float(c["layer_norm_eps"]) != 1e-6:
            raise ValueError(f"HF config: {side}.layer_norm_eps = {c['layer_norm_eps']!r}; the SigLIP family is served with 1e-06 only")
    if not v.get("vision_use_head", True):
        raise ValueError("HF config: vision_config.vision_use_head = false; the engine serves the attention-pooling head only")
    vw = int(v["hidden_size"])
    proj = t.get("projection_size")
    proj = int(t["hidden_size"]) if proj is None else int(proj)
    if proj != vw:
        raise ValueError(f"HF config: text_config.projection_size = {proj} differs from vision_config.hidden_size = {vw}: the image "
                         "embedding is the pooling head's row, there is no vision projection")
    image, patch = int(v["image_size"]), int(v["patch_size"])
    if patch <= 0 or image % patch:
        raise ValueError(f"HF config: vision_config.image_size = {image} is not a multiple of patch_size {patch}")
    return ClipArch(vw, image, patch, vw, int(v["num_hidden_layers"]), int(t["hidden_size"]), int(t["num_hidden_layers"]),
                    vocab=int(t["vocab_size"]), ctx=int(t["max_position_embeddings"]), family="siglip")


def _siglip_pairs(arch: ClipArch):
    """(HF key, engine key, how) for every tensor outside the blocks; how: None = as is, "t" = transposed, "flat" = flattened."""
    h, p = "vision_model.head", "visual.attn_pool"
    return [("vision_model.embeddings.patch_embedding.weight", "visual.conv1.weight", None),
            ("vision_model.embeddings.patch_embedding.bias", "visual.conv1.bias", None),
            ("vision_model.embeddings.position_embedding.weight", "visual.positional_embedding", None),
            ("vision_model.post_layernorm.weight", "visual.ln_post.weight", None), ("vision_model.post_layernorm.bias", "visual.ln_post.bias", None),
            (f"{h}.probe", f"{p}.probe", "flat"),
            (f"{h}.attention.in_proj_weight", f"{p}.in_proj_weight", None), (f"{h}.attention.in_proj_bias", f"{p}.in_proj_bias", None),
            (f"{h}.attention.out_proj.weight", f"{p}.out_proj.weight", None), (f"{h}.attention.out_proj.bias", f"{p}.out_proj.bias", None),
            (f"{h}.layernorm.weight", f"{p}.ln.weight", None), (f"{h}.layernorm.bias", f"{p}.ln.bias", None),
            (f"{h}.mlp.fc1.weight", f"{p}.mlp.c_fc.weight", None), (f"{h}.mlp.fc1.bias", f"{p}.mlp.c_fc.bias", None),
            (f"{h}.mlp.fc2.weight", f"{p}.mlp.c_proj.weight", None), (f"{h}.mlp.fc2.bias", f"{p}.mlp.c_proj.bias", None),
            ("text_model.embeddings.token_embedding.weight", "token_embedding.weight", None),
            ("text_model.embeddings.position_embedding.weight", "positional_embedding", None),
            ("text_model.final_layer_norm.weight", "ln_final.weight", None), ("text_model.final_layer_norm.bias", "ln_final.bias", None),
            ("text_model.head.weight", "text_projection", "t"), ("text_model.head.bias", "text_projection_bias", None),
            ("logit_scale", "logit_scale", None), ("logit_bias", "logit_bias", None)]


_BLOCK_PAIRS = [("layer_norm1.weight", "ln_1.weight"), ("layer_norm1.bias", "ln_1.bias"),
                ("self_attn.out_proj.weight", "attn.out_proj.weight"), ("self_attn.out_proj.bias", "attn.out_proj.bias"),
                ("layer_norm2.weight", "ln_2.weight"), ("layer_norm2.bias", "ln_2.bias"),
                ("mlp.fc1.weight", "mlp.c_fc.weight"), ("mlp.fc1.bias", "mlp.c_fc.bias"),
                ("mlp.fc2.weight", "mlp.c_proj.weight"), ("mlp.fc2.bias", "mlp.c_proj.bias")]


def from_siglip_state_dict(sd: Mapping[str, torch.Tensor], arch: ClipArch) -> Dict[str, torch.Tensor]:
    """``SiglipModel.state_dict()`` -> the engine's SigLIP names (``SigLIP.load_state_dict`` then loads it strictly): q | k | v
    concatenated into ``in_proj_*``, ``text_model.head.weight`` transposed into ``text_projection``, ``probe`` flattened.
    ``position_ids`` buffers are ignored; a missing key and any key left over are errors that name it."""
    left = {k: v for k, v in sd.items() if not k.endswith("position_ids")}
    out: Dict[str, torch.Tensor] = {}

    def take(key: str) -> torch.Tensor:
        if key not in left:
            raise KeyError(f"HF state dict: missing key '{key}'")
        return left.pop(key)

    for src, dst, how in _siglip_pairs(arch):
        t = take(src)
        out[dst] = t.t().contiguous() if how == "t" else (t.reshape(-1) if how == "flat" else t)
    for src, dst, layers in (("vision_model", "visual.transformer", arch.v_layers), ("text_model", "transformer", arch.t_layers)):
        for i in range(layers):
            s, d = f"{src}.encoder.layers.{i}", f"{dst}.resblocks.{i}"
            out[f"{d}.attn.in_proj_weight"] = torch.cat([take(f"{s}.self_attn.{p}_proj.weight") for p in "qkv"], dim=0)
            out[f"{d}.attn.in_proj_bias"] = torch.cat([take(f"{s}.self_attn.{p}_proj.bias") for p in "qkv"], dim=0)
            for a, b in _BLOCK_PAIRS:
                out[f"{d}.{b}"] = take(f"{s}.{a}")
    if left:
        raise KeyError(f"HF state dict: unexpected key '{sorted(left)[0]}' ({len(left)} left over; not a SiglipModel of this architecture)")
    return out


def to_siglip_state_dict(sd: Mapping[str, torch.Tensor], arch: ClipArch) -> Dict[str, torch.Tensor]:
    """The way back: the engine's SigLIP names -> ``SiglipModel.state_dict()`` keys (what ``SiglipModel.load_state_dict`` takes)."""
    out: Dict[str, torch.Tensor] = {}
    for src, dst, how in _siglip_pairs(arch):
        t = sd[dst]
        out[src] = t.t().contiguous() if how == "t" else (t.reshape(1, 1, -1) if how == "flat" else t)
    for src, dst, layers, w in (("vision_model", "visual.transformer", arch.v_layers, arch.v_width), ("text_model", "transformer", arch.t_layers, arch.t_width)):
        for i in range(layers):
            s, d = f"{src}.encoder.layers.{i}", f"{dst}.resblocks.{i}"
            for j, p in enumerate("qkv"):
                out[f"{s}.self_attn.{p}_proj.weight"] = sd[f"{d}.attn.in_proj_weight"][j * w:(j + 1) * w].contiguous()
                out[f"{s}.self_attn.{p}_proj.bias"] = sd[f"{d}.attn.in_proj_bias"][j * w:(j + 1) * w].contiguous()
            for a, b in _BLOCK_PAIRS:
                out[f"{s}.{a}"] = sd[f"{d}.{b}"]
    return out


# ---- BERT sentence encoders (E5, GTE): transformers.BertModel, optionally inside a sentence-transformers directory ---------------------
_BERT_DEFAULTS = dict(hidden_size=768, intermediate_size=3072, num_attention_heads=12, num_hidden_layers=12, vocab_size=30522,
                      max_position_embeddings=512, hidden_act="gelu", layer_norm_eps=1e-12, position_embedding_type="absolute",
                      type_vocab_size=2)


def _read_json(path: str):
    with open(path) as f:
        return json.load(f)


def sentence_transformers_settings(directory) -> Tuple[str, int]:
    """(pooling, max_seq_length) a sentence-transformers directory asks for: ``1_Pooling/config.json`` (mean or CLS; anything else is
    refused) and ``sentence_bert_config.json``; ("mean", 0) where the files are absent (0 = the model's own limit)."""
    pooling, max_len = "mean", 0
    if directory:
        p = os.path.join(directory, "1_Pooling", "config.json")
        if os.path.isfile(p):
            pc = _read_json(p)
            modes = [k for k in ("pooling_mode_cls_token", "pooling_mode_mean_tokens", "pooling_mode_max_tokens", "pooling_mode_mean_sqrt_len_tokens",
                                 "pooling_mode_weightedmean_tokens", "pooling_mode_lasttoken") if pc.get(k)]
            if modes == ["pooling_mode_cls_token"]:
                pooling = "cls"
            elif modes != ["pooling_mode_mean_tokens"]:
                raise ValueError(f"1_Pooling/config.json: pooling modes {modes} are not served (mean or CLS, one of them)")
        p = os.path.join(directory, "sentence_bert_config.json")
        if os.path.isfile(p):
            max_len = int(_read_json(p).get("max_seq_length") or 0)
    return pooling, max_len


def arch_from_bert_config(cfg: Mapping, directory: str = "") -> BertArch:
    """``config.json`` of a ``BertModel`` (as a dict) -> BertArch; `directory` (optional) is searched for the sentence-transformers
    files.  Everything the kernels do not serve is refused with the reason: MPNet (its attention adds a learned relative position
    bias), relative position embeddings, widths that are no multiple of 256, heads of another size than 64, an MLP that is not 4 x the
    width, another activation than the exact GELU."""
    mt = cfg.get("model_type")
    if mt == "mpnet":
        raise ValueError("HF config: model_type 'mpnet' (all-mpnet-base-v2) is not served: its attention adds a learned relative "
                         "position bias to every score, which this route's attention launch does not take (sentence encoders load through "
                         "hf_checkpoint.read_sentence_directory / SentenceEncoder.from_pretrained, which serves it)")
    if mt != "bert":
        raise ValueError(f"HF config: model_type {mt!r} is not a BertModel")
    c = {**_BERT_DEFAULTS, **{k: v for k, v in cfg.items() if v is not None}}
    if c["position_embedding_type"] != "absolute":
        raise ValueError(f"HF config: position_embedding_type = {c['position_embedding_type']!r}; served: 'absolute' (relative positions "
                         "change every attention score)")
    w, heads = int(c["hidden_size"]), int(c["num_attention_heads"])
    if w <= 0 or w % 256:
        raise ValueError(f"HF config: hidden_size = {w} is not a multiple of 256 (the kernels' tile; e.g. MiniLM's 384 is not served)")
    if w > 1280:
        raise ValueError(f"HF config: hidden_size = {w} is beyond the widest served tower (1280)")
    if heads <= 0 or w != 64 * heads:
        raise ValueError(f"HF config: num_attention_heads = {heads} at hidden_size {w} is a head dim of {w / max(heads, 1):g}; BERT "
                         "encoders are served at head dim 64 only")
    if int(c["intermediate_size"]) != 4 * w:
        raise ValueError(f"HF config: intermediate_size = {c['intermediate_size']} is not 4 x hidden_size ({4 * w})")
    if c["hidden_act"] != "gelu":
        raise ValueError(f"HF config: hidden_act = {c['hidden_act']!r}; BERT encoders are served with the exact 'gelu' only")
    if float(c["layer_norm_eps"]) != 1e-12:
        raise ValueError(f"HF config: layer_norm_eps = {c['layer_norm_eps']!r}; BERT encoders are served with 1e-12 only")
    if int(c["type_vocab_size"]) != 2:
        raise ValueError(f"HF config: type_vocab_size = {c['type_vocab_size']}; served: 2 (every token is of type 0)")
    pooling, max_len = sentence_transformers_settings(directory)
    positions = int(c["max_position_embeddings"])
    ctx = min(max_len or positions, positions)
    if ctx > 512:
        raise ValueError(f"HF config: {ctx} positions; BERT encoders are served up to 512 (set max_seq_length in sentence_bert_config.json)")
    return BertArch(w, int(c["num_hidden_layers"]), vocab=int(c["vocab_size"]), ctx=ctx, pooling=pooling,
                    positions=positions if positions != ctx else 0)


_BERT_TOP = [("embeddings.word_embeddings.weight", "token_embedding.weight"), ("embeddings.position_embeddings.weight", "positional_embedding"),
             ("embeddings.token_type_embeddings.weight", "token_type_embedding"),
             ("embeddings.LayerNorm.weight", "ln_embed.weight"), ("embeddings.LayerNorm.bias", "ln_embed.bias")]
_BERT_BLOCK = [("attention.output.dense.weight", "attn.out_proj.weight"), ("attention.output.dense.bias", "attn.out_proj.bias"),
               ("attention.output.LayerNorm.weight", "ln_1.weight"), ("attention.output.LayerNorm.bias", "ln_1.bias"),
               ("intermediate.dense.weight", "mlp.c_fc.weight"), ("intermediate.dense.bias", "mlp.c_fc.bias"),
               ("output.dense.weight", "mlp.c_proj.weight"), ("output.dense.bias", "mlp.c_proj.bias"),
               ("output.LayerNorm.weight", "ln_2.weight"), ("output.LayerNorm.bias", "ln_2.bias")]


def from_bert_state_dict(sd: Mapping[str, torch.Tensor], arch: BertArch) -> Dict[str, torch.Tensor]:
    """``BertModel.state_dict()`` (bare keys, or ``bert.``-prefixed as a task model saves them) -> the engine's names: query | key |
    value concatenated into ``in_proj_*``, ``ln_1`` = attention.output.LayerNorm, ``ln_2`` = output.LayerNorm, the positional table cut
    to the ``arch.ctx`` positions served.  ``pooler.*``, ``position_ids`` / ``token_type_ids`` buffers and the heads of a task model
    (``cls.*``) are ignored; a missing key and any other key left over are errors that name it."""
    left = {}
    for k, v in sd.items():
        k = k[5:] if k.startswith("bert.") else k
        if k.startswith("pooler.") or k.startswith("cls.") or k.endswith("position_ids") or k.endswith("token_type_ids"):
            continue
        left[k] = v
    out: Dict[str, torch.Tensor] = {}

    def take(key: str) -> torch.Tensor:
        if key not in left:
            raise KeyError(f"HF state dict: missing key '{key}'")
        return left.pop(key)

    for src, dst in _BERT_TOP:
        out[dst] = take(src)
    out["positional_embedding"] = out["positional_embedding"][: arch.ctx].contiguous()
    for i in range(arch.layers):
        s, d = f"encoder.layer.{i}", f"transformer.resblocks.{i}"
        out[f"{d}.attn.in_proj_weight"] = torch.cat([take(f"{s}.attention.self.{p}.weight") for p in ("query", "key", "value")], dim=0)
        out[f"{d}.attn.in_proj_bias"] = torch.cat([take(f"{s}.attention.self.{p}.bias") for p in ("query", "key", "value")], dim=0)
        for a, b in _BERT_BLOCK:
            out[f"{d}.{b}"] = take(f"{s}.{a}")
    if left:
        raise KeyError(f"HF state dict: unexpected key '{sorted(left)[0]}' ({len(left)} left over; not a BertModel of this architecture)")
    return out


def to_bert_state_dict(sd: Mapping[str, torch.Tensor], arch: BertArch) -> Dict[str, torch.Tensor]:
    """The way back: the engine's names -> ``BertModel(add_pooling_layer=False).state_dict()`` keys."""
    out: Dict[str, torch.Tensor] = {src: sd[dst] for src, dst in _BERT_TOP}
    w = arch.width
    for i in range(arch.layers):
        s, d = f"encoder.layer.{i}", f"transformer.resblocks.{i}"
        for j, p in enumerate(("query", "key", "value")):
            out[f"{s}.attention.self.{p}.weight"] = sd[f"{d}.attn.in_proj_weight"][j * w:(j + 1) * w].contiguous()
            out[f"{s}.attention.self.{p}.bias"] = sd[f"{d}.attn.in_proj_bias"][j * w:(j + 1) * w].contiguous()
        for a, b in _BERT_BLOCK:
            out[f"{s}.{a}"] = sd[f"{d}.{b}"]
    return out


# ---- MPNet sentence encoders (all-mpnet-base-v2): transformers.MPNetModel ------------------------------------------------------------
_MPNET_DEFAULTS = dict(hidden_size=768, intermediate_size=3072, num_attention_heads=12, num_hidden_layers=12, vocab_size=30527,
                       max_position_embeddings=512, hidden_act="gelu", layer_norm_eps=1e-12, relative_attention_num_buckets=32, pad_token_id=1)
MPNET_BUCKETS = 32            # what MPNetEncoder.compute_position_bias passes, whatever the config says
MPNET_MAX_DISTANCE = 511      # |key - query| at 512 positions
# buckets 8 .. 15 of |query - key| begin at these distances (the integer form of 8 + floor(8 log(n / 8) / log(16)), capped at 15)
_MPNET_LOG_BUCKET_STARTS = (8, 12, 16, 23, 32, 46, 64, 91)


def relative_position_bucket(distance: int) -> int:
    """MPNet's bucket of ``distance = key - query`` (``MPNetEncoder.relative_position_bucket`` at 32 buckets, max distance 128), by
    integer thresholds: keys behind the query take buckets 16 .. 31; |distance| < 8 is its own bucket; then eight logarithmic ones."""
    n = -int(distance)
    a = abs(n)
    b = a if a < 8 else 7 + sum(1 for t in _MPNET_LOG_BUCKET_STARTS if a >= t)
    return b + (16 if n < 0 else 0)


def bias_by_distance(weight: torch.Tensor) -> torch.Tensor:
    """``encoder.relative_attention_bias.weight`` [32, heads] -> fp32 [heads, 1023]: entry [h][d + 511] is the bias head h adds to a
    score at ``key - query = d`` -- the table the library builds at finalize and the attention kernel indexes."""
    if weight.dim() != 2 or weight.shape[0] != MPNET_BUCKETS:
        raise ValueError(f"relative_attention_bias: shape {tuple(weight.shape)}; expected [{MPNET_BUCKETS}, heads]")
    idx = torch.tensor([relative_position_bucket(d) for d in range(-MPNET_MAX_DISTANCE, MPNET_MAX_DISTANCE + 1)])
    return weight.detach().float()[idx].T.contiguous()


def arch_from_mpnet_config(cfg: Mapping, directory: str = "") -> BertArch:
    """``config.json`` of an ``MPNetModel`` (as a dict) -> BertArch with ``relative_bias``; `directory` (optional) is searched for the
    sentence-transformers files.  Position ids start at padding_idx + 1 = 2, so ``max_position_embeddings`` = 514 means 512 usable
    positions.  Refused with the reason: another bucket count than 32, a LayerNorm eps other than 1e-5 / 1e-12, and what the BERT route
    refuses (width, head dim, MLP ratio, activation, more than 512 usable positions)."""
    mt = cfg.get("model_type")
    if mt != "mpnet":
        raise ValueError(f"HF config: model_type {mt!r} is not an MPNetModel")
    c = {**_MPNET_DEFAULTS, **{k: v for k, v in cfg.items() if v is not None}}
    if int(c["relative_attention_num_buckets"]) != MPNET_BUCKETS:
        raise ValueError(f"HF config: relative_attention_num_buckets = {c['relative_attention_num_buckets']}; served: 32 (MPNetEncoder computes "
                         "its bias with 32 buckets whatever the config says, so another table size cannot be a working checkpoint)")
    w, heads = int(c["hidden_size"]), int(c["num_attention_heads"])
    if w <= 0 or w % 256:
        raise ValueError(f"HF config: hidden_size = {w} is not a multiple of 256 (the kernels' tile; e.g. MiniLM's 384 is not served)")
    if w > 1280:
        raise ValueError(f"HF config: hidden_size = {w} is beyond the widest served tower (1280)")
    if heads <= 0 or w != 64 * heads:
        raise ValueError(f"HF config: num_attention_heads = {heads} at hidden_size {w} is a head dim of {w / max(heads, 1):g}; MPNet "
                         "encoders are served at head dim 64 only")
    if int(c["intermediate_size"]) != 4 * w:
        raise ValueError(f"HF config: intermediate_size = {c['intermediate_size']} is not 4 x hidden_size ({4 * w})")
    if c["hidden_act"] != "gelu":
        raise ValueError(f"HF config: hidden_act = {c['hidden_act']!r}; MPNet encoders are served with the exact 'gelu' only")
    eps = float(c["layer_norm_eps"])
    if eps not in MPNET_EPS:
        raise ValueError(f"HF config: layer_norm_eps = {c['layer_norm_eps']!r}; MPNet encoders are served with 1e-05 (all-mpnet-base-v2) "
                         "and 1e-12 (MPNetConfig's default) only")
    if int(c["pad_token_id"]) != 1:
        raise ValueError(f"HF config: pad_token_id = {c['pad_token_id']}; served: 1 (position ids start at pad_token_id + 1 = 2)")
    pooling, max_len = sentence_transformers_settings(directory)
    positions = int(c["max_position_embeddings"]) - 2
    if positions > 512:
        raise ValueError(f"HF config: max_position_embeddings = {positions + 2} is {positions} usable positions; MPNet encoders are served up "
                         "to 514 (512 usable: the bias table spans distances of -511 .. 511)")
    if positions < 1:
        raise ValueError(f"HF config: max_position_embeddings = {positions + 2} leaves no usable position (ids start at 2)")
    ctx = min(max_len or positions, positions)
    return BertArch(w, int(c["num_hidden_layers"]), vocab=int(c["vocab_size"]), ctx=ctx, pooling=pooling,
                    positions=positions if positions != ctx else 0, relative_bias=True, layer_norm_eps=eps)


_MPNET_TOP = [("embeddings.word_embeddings.weight", "token_embedding.weight"), ("embeddings.position_embeddings.weight", "positional_embedding"),
              ("embeddings.LayerNorm.weight", "ln_embed.weight"), ("embeddings.LayerNorm.bias", "ln_embed.bias"),
              ("encoder.relative_attention_bias.weight", "relative_attention_bias")]
_MPNET_BLOCK = [("attention.attn.o.weight", "attn.out_proj.weight"), ("attention.attn.o.bias", "attn.out_proj.bias"),
                ("attention.LayerNorm.weight", "ln_1.weight"), ("attention.LayerNorm.bias", "ln_1.bias")] + _BERT_BLOCK[4:]
MPNET_POSITION_OFFSET = 2     # padding_idx + 1: the row of position_embeddings that position 0 reads


def from_mpnet_state_dict(sd: Mapping[str, torch.Tensor], arch: BertArch) -> Dict[str, torch.Tensor]:
    """``MPNetModel.state_dict()`` (bare keys, or ``mpnet.``-prefixed as a task model saves them) -> the engine's names for family 3:
    q | k | v concatenated into ``in_proj_*``, ``attn.o`` = out_proj, ``ln_1`` = attention.LayerNorm, ``ln_2`` = output.LayerNorm,
    ``positional_embedding`` = rows 2 .. 2 + ctx - 1 of the positional table (position j of a text reads row j + 2), the encoder's one
    ``relative_attention_bias`` [32, heads].  ``pooler.*``, ``position_ids`` buffers and the heads of a task model (``lm_head.*``) are
    ignored; a missing key and any other key left over are errors that name it."""
    left = {}
    for k, v in sd.items():
        k = k[6:] if k.startswith("mpnet.") else k
        if k.startswith("pooler.") or k.startswith("lm_head.") or k.endswith("position_ids"):
            continue
        left[k] = v
    out: Dict[str, torch.Tensor] = {}

    def take(key: str) -> torch.Tensor:
        if key not in left:
            raise KeyError(f"HF state dict: missing key '{key}'")
        return left.pop(key)

    for src, dst in _MPNET_TOP:
        out[dst] = take(src)
    pos = out["positional_embedding"]
    if pos.shape[0] < MPNET_POSITION_OFFSET + arch.ctx:
        raise KeyError(f"HF state dict: position_embeddings has {pos.shape[0]} rows, {MPNET_POSITION_OFFSET + arch.ctx} needed for {arch.ctx} positions")
    out["positional_embedding"] = pos[MPNET_POSITION_OFFSET:MPNET_POSITION_OFFSET + arch.ctx].contiguous()
    for i in range(arch.layers):
        s, d = f"encoder.layer.{i}", f"transformer.resblocks.{i}"
        out[f"{d}.attn.in_proj_weight"] = torch.cat([take(f"{s}.attention.attn.{p}.weight") for p in ("q", "k", "v")], dim=0)
        out[f"{d}.attn.in_proj_bias"] = torch.cat([take(f"{s}.attention.attn.{p}.bias") for p in ("q", "k", "v")], dim=0)
        for a, b in _MPNET_BLOCK:
            out[f"{d}.{b}"] = take(f"{s}.{a}")
    if left:
        raise KeyError(f"HF state dict: unexpected key '{sorted(left)[0]}' ({len(left)} left over; not an MPNetModel of this architecture)")
    return out


def to_mpnet_state_dict(sd: Mapping[str, torch.Tensor], arch: BertArch, positions: int = 0) -> Dict[str, torch.Tensor]:
    """The way back (tests): the engine's names -> ``MPNetModel(add_pooling_layer=False).state_dict()`` keys.  The positional table gets
    its two leading rows back (zeros: row 1 is the padding row, row 0 is never read) and is zero-filled up to `positions` usable rows."""
    out: Dict[str, torch.Tensor] = {src: sd[dst] for src, dst in _MPNET_TOP}
    pos = sd["positional_embedding"]
    table = torch.zeros(MPNET_POSITION_OFFSET + max(positions, pos.shape[0]), pos.shape[1], dtype=pos.dtype)
    table[MPNET_POSITION_OFFSET:MPNET_POSITION_OFFSET + pos.shape[0]] = pos
    out["embeddings.position_embeddings.weight"] = table
    w = arch.width
    for i in range(arch.layers):
        s, d = f"encoder.layer.{i}", f"transformer.resblocks.{i}"
        for j, p in enumerate(("q", "k", "v")):
            out[f"{s}.attention.attn.{p}.weight"] = sd[f"{d}.attn.in_proj_weight"][j * w:(j + 1) * w].contiguous()
            out[f"{s}.attention.attn.{p}.bias"] = sd[f"{d}.attn.in_proj_bias"][j * w:(j + 1) * w].contiguous()
        for a, b in _MPNET_BLOCK:
            out[f"{s}.{a}"] = sd[f"{d}.{b}"]
    return out


def is_hf_directory(path: str) -> bool:
    return os.path.isdir(path) and os.path.isfile(os.path.join(path, "config.json"))


def _load_weights(weights: str) -> Dict[str, torch.Tensor]:
    if weights.endswith(".safetensors"):
        from safetensors.torch import load_file
        return load_file(weights)
    return torch.load(weights, map_location="cpu", weights_only=True)


def read_hf_directory(directory: str) -> Tuple[ClipArch, str, Dict[str, torch.Tensor]]:
    """(ClipArch, activation, state dict under OpenAI names) of a ``save_pretrained`` directory on the local disk."""
    cfg_path = os.path.join(directory, "config.json")
    if not os.path.isfile(cfg_path):
        raise FileNotFoundError(f"{directory!r} holds no config.json (not a save_pretrained directory)")
    weights = next((os.path.join(directory, f) for f in WEIGHT_FILES if os.path.isfile(os.path.join(directory, f))), None)
    if weights is None:
        raise FileNotFoundError(f"{directory!r} holds neither of {WEIGHT_FILES} (sharded checkpoints are not read)")
    with open(cfg_path) as f:
        cfg = json.load(f)
    if cfg.get("model_type") in ("bert", "mpnet"):      # a sentence encoder: (BertArch, "gelu", state dict under the engine's names)
        barch = arch_from_bert_config(cfg, directory)
        return barch, "gelu", from_bert_state_dict(_load_weights(weights), barch)
    siglip = cfg.get("model_type") == "siglip"          # every other model_type (and none) takes the CLIPModel route, refusals included
    if siglip:
        arch, activation = arch_from_siglip_config(cfg), SIGLIP_ACT
    else:
        arch, activation = arch_and_activation_from_hf_config(cfg)
    if weights.endswith(".safetensors"):
        from safetensors.torch import load_file
        sd = load_file(weights)
    else:
        sd = torch.load(weights, map_location="cpu", weights_only=True)
    return arch, activation, (from_siglip_state_dict if siglip else from_hf_state_dict)(sd, arch)


def read_sentence_directory(directory: str) -> Tuple[BertArch, Dict[str, torch.Tensor]]:
    """(BertArch, state dict under the engine's names) of a sentence encoder's ``save_pretrained`` directory on the local disk, with the
    sentence-transformers files honoured where present: ``model_type: "bert"`` exactly as :func:`read_hf_directory` reads it, and
    ``model_type: "mpnet"`` (``transformers.MPNetModel``, model family 3).  Any other model type is refused."""
    cfg_path = os.path.join(directory, "config.json")
    if not os.path.isfile(cfg_path):
        raise FileNotFoundError(f"{directory!r} holds no config.json (not a save_pretrained directory)")
    cfg = _read_json(cfg_path)
    mt = cfg.get("model_type")
    if mt == "bert":
        arch, _, sd = read_hf_directory(directory)
        return arch, sd
    if mt != "mpnet":
        raise ValueError(f"{directory!r} is not a sentence encoder (config.json model_type is {mt!r}; served: 'bert', 'mpnet')")
    weights = next((os.path.join(directory, f) for f in WEIGHT_FILES if os.path.isfile(os.path.join(directory, f))), None)
    if weights is None:
        raise FileNotFoundError(f"{directory!r} holds neither of {WEIGHT_FILES} (sharded checkpoints are not read)")
    arch = arch_from_mpnet_config(cfg, directory)
    return arch, from_mpnet_state_dict(_load_weights(weights), arch)
