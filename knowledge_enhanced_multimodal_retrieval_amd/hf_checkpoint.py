"""Hugging Face ``CLIPModel`` checkpoints (``save_pretrained`` directories) for the HIP engine.

The reference evaluates its published fine-tuned model through ``transformers.CLIPModel``
(reference: src/clip/eval/evaluator_hf.py:115,130,144,280).  That class stores the same network under other names: towers
``vision_model.*`` / ``text_model.*``, separate ``q_proj`` / ``k_proj`` / ``v_proj``, ``nn.Linear`` projections (so the matrices
are transposed), ``pre_layrnorm`` (its spelling) / ``post_layernorm`` / ``final_layer_norm``.  This module maps such a state
dict onto the OpenAI names the engine loads, and reads ``config.json`` into a :class:`ClipArch` plus the activation.

Local files only: nothing here (or anywhere in the package) contacts a model hub.
"""
from __future__ import annotations

import json
import os
from typing import Dict, Mapping, Tuple

import torch

from .config import ARCHS, ClipArch

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


def is_hf_directory(path: str) -> bool:
    return os.path.isdir(path) and os.path.isfile(os.path.join(path, "config.json"))


def read_hf_directory(directory: str) -> Tuple[ClipArch, str, Dict[str, torch.Tensor]]:
    """(ClipArch, activation, state dict under OpenAI names) of a ``save_pretrained`` directory on the local disk."""
    cfg_path = os.path.join(directory, "config.json")
    if not os.path.isfile(cfg_path):
        raise FileNotFoundError(f"{directory!r} holds no config.json (not a save_pretrained directory)")
    weights = next((os.path.join(directory, f) for f in WEIGHT_FILES if os.path.isfile(os.path.join(directory, f))), None)
    if weights is None:
        raise FileNotFoundError(f"{directory!r} holds neither of {WEIGHT_FILES} (sharded checkpoints are not read)")
    with open(cfg_path) as f:
        arch, activation = arch_and_activation_from_hf_config(json.load(f))
    if weights.endswith(".safetensors"):
        from safetensors.torch import load_file
        sd = load_file(weights)
    else:
        sd = torch.load(weights, map_location="cpu", weights_only=True)
    return arch, activation, from_hf_state_dict(sd, arch)
