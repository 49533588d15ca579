"""`CLIP`: an ``nn.Module`` with the attribute / state-dict layout of OpenAI-CLIP whose encoders run in libkemr.so.

The reference treats the model as a duck type: ``.eval()``, ``.float()``,
``next(model.parameters()).device``, ``.encode_image(f32[B,3,224,224])``, ``.encode_text(int[B,77])`` returning
torch tensors, ``.load_state_dict(sd, strict=True)`` / ``.state_dict()`` with OpenAI key names
(/root/reference/src/clip/model/clip_model.py:44-64, 108-119), and the attributes ``visual``, ``transformer``,
``token_embedding``, ``positional_embedding``, ``text_projection``, ``ln_final`` (``clip_model.py:193-216``).
This class holds real ``nn.Parameter``s under exactly those names (fp32 master copy, what checkpoints are saved
from) and packs them into the HIP engine lazily; the forward arithmetic never runs in PyTorch.

``encode_*`` run without autograd: there is no backward pass through the towers.  What can be trained are the projection heads on
frozen towers -- ``encode_image_pooled`` / ``encode_text_pooled`` return the rows the final LayerNorms read, ``finetune.ProjectionHeads``
trains ``visual.ln_post`` / ``visual.proj`` / ``ln_final`` / ``text_projection`` (this module's own parameters) on them, and the engine
re-packs itself after an optimizer step (``_fingerprint``).  After a write through ``p.data`` call ``refresh()``.  The TEXT tower can be
trained as well, and so can both towers end to end, by differentiable restatements of them over these same parameters
(``tower_train.TextTower`` / ``VisionTower``: attention, LayerNorm and activation backward in the library); ``encode_*`` themselves stay
without autograd.
"""
from __future__ import annotations

import os

from collections import OrderedDict
from typing import Optional

import numpy as np
import torch
from torch import nn

from .config import ClipArch, get_arch
from .engine import ClipEngine


class QuickGELU(nn.Module):
    def forward(self, x):  # pragma: no cover - parameters only; arithmetic runs in the HIP kernels
        return x * torch.sigmoid(1.702 * x)


class ResidualAttentionBlock(nn.Module):
    """Parameter container with OpenAI-CLIP names (ln_1, attn.in_proj_*, attn.out_proj.*, ln_2, mlp.c_fc, mlp.c_proj)."""

    def __init__(self, d_model: int, n_head: int, activation: str = "quick_gelu"):
        super().__init__()
        self.attn = nn.MultiheadAttention(d_model, n_head)
        self.ln_1 = nn.LayerNorm(d_model)
        self.mlp = nn.Sequential(OrderedDict([("c_fc", nn.Linear(d_model, d_model * 4)), ("gelu", nn.GELU() if activation == "gelu" else QuickGELU()),
                                              ("c_proj", nn.Linear(d_model * 4, d_model))]))
        self.ln_2 = nn.LayerNorm(d_model)


class Transformer(nn.Module):
    def __init__(self, width: int, layers: int, heads: int, activation: str = "quick_gelu"):
        super().__init__()
        self.width, self.layers = width, layers
        self.resblocks = nn.Sequential(*[ResidualAttentionBlock(width, heads, activation) for _ in range(layers)])


class VisionTransformer(nn.Module):
    def __init__(self, input_resolution: int, patch_size: int, width: int, layers: int, heads: int, output_dim: int,
                 activation: str = "quick_gelu"):
        super().__init__()
        self.input_resolution, self.output_dim = input_resolution, output_dim
        self.conv1 = nn.Conv2d(3, width, kernel_size=patch_size, stride=patch_size, bias=False)
        scale = width ** -0.5
        self.class_embedding = nn.Parameter(scale * torch.randn(width))
        self.positional_embedding = nn.Parameter(scale * torch.randn((input_resolution // patch_size) ** 2 + 1, width))
        self.ln_pre = nn.LayerNorm(width)
        self.transformer = Transformer(width, layers, heads, activation)
        self.ln_post = nn.LayerNorm(width)
        self.proj = nn.Parameter(scale * torch.randn(width, output_dim))


def _lib_default_precision() -> str:
    from ._lib import DEFAULT_PRECISION
    return DEFAULT_PRECISION


class CLIP(nn.Module):
    def __init__(self, arch: ClipArch, name: str = "", activation: str = "quick_gelu"):
        """activation: the MLP's activation, a property of the CHECKPOINT, not of the architecture: "quick_gelu" (OpenAI) or "gelu"
        (exact GELU: OpenCLIP / LAION, Hugging Face `hidden_act: gelu`).  It has no parameters: state dicts are the same."""
        super().__init__()
        from ._lib import check_activation
        self.activation = check_activation(activation)
        self.arch, self.model_name = arch, name
        self.context_length, self.vocab_size = arch.ctx, arch.vocab
        self.visual = VisionTransformer(arch.image_size, arch.patch, arch.v_width, arch.v_layers, arch.v_heads,
                                        arch.embed_dim, activation)
        self.transformer = Transformer(arch.t_width, arch.t_layers, arch.t_heads, activation)
        self.token_embedding = nn.Embedding(arch.vocab, arch.t_width)
        self.positional_embedding = nn.Parameter(torch.empty(arch.ctx, arch.t_width))
        self.ln_final = nn.LayerNorm(arch.t_width)
        self.text_projection = nn.Parameter(torch.empty(arch.t_width, arch.embed_dim))
        self.logit_scale = nn.Parameter(torch.ones([]) * np.log(1 / 0.07))
        self._engine: Optional[ClipEngine] = None
        self._gpu_pre = None
        self._packed_fp = None
        self._dirty = True
        self.initialize_parameters()

    # ------------------------------------------------------------------ init (upstream recipe: keeps activations O(1))
    def initialize_parameters(self):
        nn.init.normal_(self.token_embedding.weight, std=0.02)
        nn.init.normal_(self.positional_embedding, std=0.01)
        for tower in (self.transformer, self.visual.transformer):
            proj_std = (tower.width ** -0.5) * ((2 * tower.layers) ** -0.5)
            attn_std, fc_std = tower.width ** -0.5, (2 * tower.width) ** -0.5
            for block in tower.resblocks:
                nn.init.normal_(block.attn.in_proj_weight, std=attn_std)
                nn.init.normal_(block.attn.out_proj.weight, std=proj_std)
                nn.init.normal_(block.mlp.c_fc.weight, std=fc_std)
                nn.init.normal_(block.mlp.c_proj.weight, std=proj_std)
        nn.init.normal_(self.text_projection, std=self.arch.t_width ** -0.5)
        self._dirty = True

    @property
    def dtype(self):
        return self.visual.conv1.weight.dtype

    # ------------------------------------------------------------------ engine plumbing
    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False):
        # the scalars OpenAI's files carry, and the causal-mask buffer of OpenCLIP files (not persistent in newer releases)
        sd = {k: v for k, v in state_dict.items() if k not in ("input_resolution", "context_length", "vocab_size", "attn_mask")}
        if "positional_embedding_res" in sd:   # a Long-CLIP file as released: its two positional tables become the one the model adds
            from .hf_checkpoint import fold_longclip_positions
            sd = fold_longclip_positions(sd, ctx=self.arch.ctx)
        res = super().load_state_dict(sd, strict=strict, assign=assign)
        self._dirty = True
        return res

    def _apply(self, fn, *a, **kw):          # .to() / .float() / .cuda(): the packed copy must follow
        out = super()._apply(fn, *a, **kw)
        self._dirty = True
        return out

    def refresh(self) -> None:
        """Re-pack the current parameter values into the HIP engine at the next encode call.  `engine()` detects by itself what
        autograd's version counters see -- optimizer.step(), `p.add_()` / `p.copy_()` under no_grad, load_state_dict, .to() --
        and re-assigned storage.  It does NOT see a write through `p.data` (`p.data.copy_(w)`, `p.data.mul_(d)`: `.data` is a
        detached alias with a version counter of its own, the parameter's stays put -- EMA and hand-rolled weight loading do
        this): call `refresh()` after such a write, or set KEMR_WEIGHT_DIGEST=1, which adds a content digest (one fused norm
        over all parameters and one host read, about 0.1 ms) to every `engine()` call."""
        self._dirty = True

    def _fingerprint(self):
        """Cheap identity of the parameter values: in-place edits of the parameter itself (optimizer.step(), `p.add_()`,
        `p.copy_()`) bump its version counter, re-assignment changes its storage; see `refresh()` for what this misses.  The
        reference's trainer validates through `evaluate_clip_model_for_training` right after optimizer.step()
        (train/trainer.py:241)."""
        fp = tuple((p._version, p.data_ptr()) for p in self.parameters())
        if os.environ.get("KEMR_WEIGHT_DIGEST", "") == "1":
            params = [p.detach() for p in self.parameters()]
            digest = torch.stack(torch._foreach_norm(params)).double().cpu()       # content digest: catches writes through .data
            fp = fp + (tuple(digest.tolist()),)
        return fp

    def __deepcopy__(self, memo):
        """The packed engine is a raw library handle: a copy gets its own, built lazily (never two owners of one handle)."""
        import copy
        cls = self.__class__
        new = cls.__new__(cls)
        memo[id(self)] = new
        for k, v in self.__dict__.items():
            new.__dict__[k] = None if k in ("_engine", "_packed_fp", "_gpu_pre") else copy.deepcopy(v, memo)
        new._dirty = True
        return new

    def __getstate__(self):
        state = dict(self.__dict__)
        state["_engine"], state["_packed_fp"], state["_dirty"] = None, None, True
        state["_gpu_pre"] = None
        return state

    def _device(self) -> torch.device:
        return self.positional_embedding.device

    def _engine_activation(self) -> str:
        return self.activation

    def engine(self) -> ClipEngine:
        dev = self._device()
        if dev.type != "cuda":
            raise RuntimeError("CLIP: the model sits on %s; the encoders run only on a GPU (model.to('cuda')); there is no "
                               "CPU fallback" % dev)
        if self._engine is None or self._engine.device != dev:
            # encoder precision of the packed copy: _lib.DEFAULT_PRECISION unless KEMR_PRECISION says otherwise (bf16 | bf16-res16 | fp8 | fp8-res16 |
            # fp8-mlp | fp32x3, kemr_precision in include/kemr.h) -- an environment switch so that the reference's scripts stay unchanged
            from ._lib import env_precision
            self._engine, self._dirty = ClipEngine(self.arch, dev, precision=env_precision(), activation=self._engine_activation()), True
        if self._engine.activation != self._engine_activation():
            self._engine.set_activation(self._engine_activation())
        fp = self._fingerprint()
        if self._dirty or fp != getattr(self, "_packed_fp", None):
            self._engine.load_state_dict({k: v for k, v in self.state_dict().items() if k not in ("logit_scale", "logit_bias")})
            self._dirty, self._packed_fp = False, fp
        return self._engine

    # ------------------------------------------------------------------ the duck-typed API
    @torch.no_grad()
    def encode_image(self, image: torch.Tensor, normalize: bool = False) -> torch.Tensor:
        """``image``: float ``[B, 3, S, S]`` normalised pixels as upstream, or the :class:`preprocess.PackedRaw` batch a loader over
        ``CLIPEvalDatasetHF(split, preprocess)`` yields when the transform is deferred to the GPU -- so the reference's own loop
        (``images.to(device)`` -> ``model.encode_image(images)``, evaluator.py:118-121) runs unchanged on either."""
        from .preprocess import PackedRaw, gpu_preprocess_for
        dev = self._device()
        if isinstance(image, PackedRaw):
            if getattr(self, "_gpu_pre", None) is None or self._gpu_pre.device != dev:
                self._gpu_pre = gpu_preprocess_for(self, dev)          # the family's transform: CLIP's resize-and-crop or SigLIP's squash
            image = self._gpu_pre.batch(image)
        return self.engine().encode_image(image.to(dev), normalize=normalize)

    accepts_text_lengths = True        # encode_text(..., lens=host int tensor): evaluators.encode_dataset passes the tokenizer-side lengths

    @torch.no_grad()
    def encode_text(self, text: torch.Tensor, normalize: bool = False, lens: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Host token ids (what ``tokenize`` returns) are handed over as they are: the engine reads the text lengths from them on the
        host before the upload (engine.ClipEngine.encode_text); ids already on the GPU cost one small device-to-host copy unless the
        caller passes ``lens`` (``engine.text_lengths(host_tokens)``)."""
        return self.engine().encode_text(text, normalize=normalize, lens=lens)

    # ------------------------------------------------------------------ pooled tower rows (finetune.py: heads on frozen towers)
    @torch.no_grad()
    def encode_image_pooled(self, image: torch.Tensor) -> torch.Tensor:
        """fp32 ``[B, vision width]``: the class-token row before ``visual.ln_post`` and ``visual.proj``.  Inputs as ``encode_image``."""
        from .preprocess import PackedRaw, gpu_preprocess_for
        dev = self._device()
        if isinstance(image, PackedRaw):
            if getattr(self, "_gpu_pre", None) is None or self._gpu_pre.device != dev:
                self._gpu_pre = gpu_preprocess_for(self, dev)
            image = self._gpu_pre.batch(image)
        return self.engine().encode_image_pooled(image.to(dev))

    @torch.no_grad()
    def encode_text_pooled(self, text: torch.Tensor, lens: Optional[torch.Tensor] = None) -> torch.Tensor:
        """fp32 ``[B, text width]``: the end-of-text row before ``ln_final`` and ``text_projection``.  Inputs as ``encode_text``."""
        return self.engine().encode_text_pooled(text, lens=lens)

    # ------------------------------------------------------------------ the calls made on a transformers.CLIPModel
    @classmethod
    def from_pretrained(cls, directory: str, device=None) -> "CLIP":
        """A ``save_pretrained`` directory on the LOCAL disk (``config.json`` + ``model.safetensors`` | ``pytorch_model.bin``);
        nothing is ever fetched."""
        from .clip_api import load
        return load(directory, device=device)[0]

    @torch.no_grad()
    def get_image_features(self, pixel_values: torch.Tensor = None, **_) -> torch.Tensor:
        """``CLIPModel.get_image_features(pixel_values=...)``: the projected embeddings, not normalised."""
        return self.encode_image(pixel_values)

    @torch.no_grad()
    def get_text_features(self, input_ids: torch.Tensor = None, attention_mask=None, **_) -> torch.Tensor:
        """``CLIPModel.get_text_features(**processor(text=...))``: the projected embeddings, not normalised.  A processor pads to the
        batch's longest text: shorter rows are zero-padded to the context length here (the mask is causal and the pooled row is
        the first end-of-text token's, so neither the padding nor ``attention_mask`` can reach the result)."""
        ctx = self.context_length
        if input_ids.dim() != 2 or input_ids.shape[1] > ctx:
            raise ValueError(f"get_text_features: input_ids must be [B, <= {ctx}], got {tuple(input_ids.shape)}")
        if input_ids.shape[1] < ctx:
            input_ids = torch.nn.functional.pad(input_ids, (0, ctx - input_ids.shape[1]), value=0)
        return self.encode_text(input_ids)

    @torch.no_grad()
    def forward(self, image: torch.Tensor, text: torch.Tensor):
        """logits_per_image, logits_per_text (cosine similarities times exp(logit_scale)), as upstream CLIP.forward."""
        from . import _lib
        from . import engine as E
        img = self.encode_image(image, normalize=True)
        txt = self.encode_text(text, normalize=True)
        qp = E.build_panel([img], _lib.SIDE_QUERY, 3)
        gp = E.build_panel([txt], _lib.SIDE_GALLERY, 3)
        logits = E.scores_dense(qp, gp) * self.logit_scale.exp().to(img.device)
        return logits, logits.t()


class AttentionPool(nn.Module):
    """Parameter container of SigLIP's attention-pooling head (``visual.attn_pool.*``): a learned probe is the single query of a
    multi-head attention over the post-LayerNorm tokens; then ``r + mlp(ln(r))``."""

    def __init__(self, width: int):
        super().__init__()
        self.probe = nn.Parameter(torch.randn(width) * width ** -0.5)          # Hugging Face's [1, 1, W], flattened
        self.in_proj_weight = nn.Parameter(torch.randn(3 * width, width) * width ** -0.5)
        self.in_proj_bias = nn.Parameter(torch.zeros(3 * width))
        self.out_proj = nn.Linear(width, width)
        self.ln = nn.LayerNorm(width, eps=1e-6)
        self.mlp = nn.Sequential(OrderedDict([("c_fc", nn.Linear(width, width * 4)), ("gelu", nn.GELU(approximate="tanh")),
                                              ("c_proj", nn.Linear(width * 4, width))]))


class SiglipVisionTransformer(nn.Module):
    def __init__(self, input_resolution: int, patch_size: int, width: int, layers: int, heads: int):
        super().__init__()
        self.input_resolution, self.output_dim = input_resolution, width
        self.conv1 = nn.Conv2d(3, width, kernel_size=patch_size, stride=patch_size, bias=True)
        self.positional_embedding = nn.Parameter(width ** -0.5 * torch.randn((input_resolution // patch_size) ** 2, width))
        self.transformer = Transformer(width, layers, heads, "gelu")          # parameters only: the family's tanh GELU runs in the kernels
        self.ln_post = nn.LayerNorm(width, eps=1e-6)
        self.attn_pool = AttentionPool(width)


class SigLIP(CLIP):
    """SigLIP (ViT-B/16, ViT-L/16) with the same duck type as :class:`CLIP`: real ``nn.Parameter``s under the OpenAI-style names wherever
    the tensor exists in both models, plus ``visual.conv1.bias``, ``visual.attn_pool.*``, ``text_projection_bias`` and ``logit_bias``;
    no ``visual.class_embedding`` / ``visual.ln_pre`` / ``visual.proj``.  The encoders run in libkemr.so (model option "family" = 1)."""

    accepts_text_lengths = False       # every position is a key and the LAST one is pooled: nothing can be left out

    def __init__(self, arch: ClipArch, name: str = ""):
        if arch.family != "siglip":
            raise ValueError(f"SigLIP: arch family {arch.family!r} is not 'siglip'")
        nn.Module.__init__(self)
        self.activation = "gelu_pytorch_tanh"          # the family's; model option "activation" is not consulted
        self.arch, self.model_name = arch, name
        self.context_length, self.vocab_size = arch.ctx, arch.vocab
        self.visual = SiglipVisionTransformer(arch.image_size, arch.patch, arch.v_width, arch.v_layers, arch.v_heads)
        self.transformer = Transformer(arch.t_width, arch.t_layers, arch.t_heads, "gelu")
        self.token_embedding = nn.Embedding(arch.vocab, arch.t_width)
        self.positional_embedding = nn.Parameter(torch.empty(arch.ctx, arch.t_width))
        self.ln_final = nn.LayerNorm(arch.t_width, eps=1e-6)
        self.text_projection = nn.Parameter(torch.empty(arch.t_width, arch.embed_dim))      # head.weight transposed: y = x @ text_projection + bias
        self.text_projection_bias = nn.Parameter(torch.zeros(arch.embed_dim))
        self.logit_scale = nn.Parameter(torch.ones(1) * np.log(10.0))
        self.logit_bias = nn.Parameter(torch.ones(1) * -10.0)
        self._engine: Optional[ClipEngine] = None
        self._gpu_pre = None
        self._packed_fp = None
        self._dirty = True
        self.initialize_parameters()

    def initialize_parameters(self):
        super().initialize_parameters()
        w = self.arch.v_width
        nn.init.normal_(self.visual.attn_pool.mlp.c_fc.weight, std=(2 * w) ** -0.5)
        nn.init.normal_(self.visual.attn_pool.mlp.c_proj.weight, std=w ** -0.5 * 0.5)
        nn.init.normal_(self.visual.attn_pool.out_proj.weight, std=w ** -0.5)
        self._dirty = True

    def _engine_activation(self) -> str:
        return "quick_gelu"            # the library's default: the option stays untouched

    @classmethod
    def from_pretrained(cls, directory: str, device=None):
        """A ``save_pretrained`` directory of a ``transformers.SiglipModel`` on the LOCAL disk -> ``(model, preprocess)``."""
        from .clip_api import load
        model, preprocess = load(directory, device=device)
        if not isinstance(model, cls):
            raise ValueError(f"SigLIP.from_pretrained({directory!r}): its config.json is not a SigLIP model's")
        return model, preprocess

    @torch.no_grad()
    def get_text_features(self, input_ids: torch.Tensor = None, attention_mask=None, **_) -> torch.Tensor:
        """``SiglipModel.get_text_features``: SigLIP is trained on ``padding="max_length"``; shorter rows are padded to the context
        length with the pad id 1 here (a pad position is a key like every other, so the padding is part of the input)."""
        ctx = self.context_length
        if input_ids.dim() != 2 or input_ids.shape[1] > ctx:
            raise ValueError(f"get_text_features: input_ids must be [B, <= {ctx}], got {tuple(input_ids.shape)}")
        if input_ids.shape[1] < ctx:
            input_ids = torch.nn.functional.pad(input_ids, (0, ctx - input_ids.shape[1]), value=1)
        return self.encode_text(input_ids)

    @torch.no_grad()
    def forward(self, image: torch.Tensor, text: torch.Tensor):
        """logits_per_image, logits_per_text = cos * exp(logit_scale) + logit_bias (``sigmoid`` of it is the pair probability)."""
        li, _ = super().forward(image, text)
        li = li + self.logit_bias.to(li.device)
        return li, li.t()


def build_model(name_or_arch, device="cuda", activation: str = "quick_gelu") -> CLIP:
    arch = name_or_arch if isinstance(name_or_arch, ClipArch) else get_arch(name_or_arch)
    name = name_or_arch if isinstance(name_or_arch, str) else ""
    if arch.family == "siglip":
        return SigLIP(arch, name).to(device).eval()
    return CLIP(arch, name, activation).to(device).eval()
