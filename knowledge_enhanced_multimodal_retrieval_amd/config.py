"""Architecture presets of the CLIP models the reference evaluates
(`--model_name` choices at /root/reference/src/clip/eval/evaluator.py:264-266: ViT-B/32, ViT-B/16, ViT-L/14;
embed_dim rule at src/clip/eval/evaluator_fusion.py:192), plus ViT-L/14@336px, the higher-resolution OpenAI CLIP model, and
ViT-H-14 (OpenCLIP's spelling), LAION's ViT-H/14: the one served model whose vision heads are 80 wide instead of 64.

A second model FAMILY rides on the same dataclass: SigLIP (``family="siglip"``, OpenCLIP's names ``ViT-B-16-SigLIP*`` /
``ViT-L-16-SigLIP-*``): no class token, no ln_pre, tanh GELU, LayerNorm eps 1e-6, an attention-pooling head instead of a projection
(so ``embed_dim == v_width``), an unmasked text tower pooled at its last position, vocabulary 32000 and 64 text positions."""
from __future__ import annotations

from dataclasses import dataclass, asdict
from typing import Dict


FAMILIES = {"clip": 0, "siglip": 1}      # model option "family" (include/kemr.h)


@dataclass(frozen=True)
class ClipArch:
    embed_dim: int
    image_size: int
    patch: int
    v_width: int
    v_layers: int
    t_width: int
    t_layers: int
    vocab: int = 49408
    ctx: int = 77
    v_head_dim: int = 64          # head dim of the vision tower: 64, or 80 (ViT-H-14: 1280 = 16 heads of 80); text heads are always 64
    family: str = "clip"          # "clip", or "siglip" (model option "family" = 1 of the library; kemr_cfg did not grow)

    def __post_init__(self):
        if self.family not in FAMILIES:
            raise ValueError(f"ClipArch: family {self.family!r}; served: {list(FAMILIES)}")
        if self.family == "siglip" and (self.v_head_dim != 64 or self.embed_dim != self.v_width):
            raise ValueError(f"ClipArch: a siglip arch has vision heads of 64 and no vision projection (embed_dim {self.embed_dim} must "
                             f"equal v_width {self.v_width})")
        if self.v_head_dim not in (64, 80) or self.v_width % self.v_head_dim:
            raise ValueError(f"ClipArch: vision head dim {self.v_head_dim} at width {self.v_width}: served are heads of 64, or of 80 "
                             "at a width that is a multiple of 80")

    @property
    def v_heads(self) -> int:
        return self.v_width // self.v_head_dim

    @property
    def t_heads(self) -> int:
        return self.t_width // 64

    @property
    def grid(self) -> int:
        return self.image_size // self.patch

    @property
    def v_tokens(self) -> int:
        return self.grid * self.grid + (0 if self.family == "siglip" else 1)      # SigLIP has no class token

    @property
    def sot(self) -> int:
        return self.vocab - 2

    @property
    def eot(self) -> int:
        return self.vocab - 1

    def as_dict(self) -> Dict[str, int]:
        """The architecture as a dict: the nine numbers of kemr_cfg (include/kemr.h), and "v_head_dim" only where it is not 64, so that
        the existing entries keep the nine keys they always had.  NOT the way to build a kemr_cfg -- `KemrCfg(**arch.as_dict())` breaks for
        a head-dim-80 arch; use `cfg_dict()` (and model option "vision_head_dim" for the head dim: kemr_cfg did not grow)."""
        d = asdict(self)
        if d["v_head_dim"] == 64:
            del d["v_head_dim"]
        if d["family"] == "clip":         # likewise "family": only where it is not the default
            del d["family"]
        return d

    def cfg_dict(self) -> Dict[str, int]:
        """Exactly the fields of kemr_cfg, for every arch: what `_lib.KemrCfg(**...)`, oracle.clip_ref and the tools take."""
        d = asdict(self)
        del d["v_head_dim"], d["family"]
        return d

    # algorithmic FLOPs per item
    def image_flops(self) -> float:
        t, w, p = self.v_tokens, self.v_width, self.grid * self.grid
        per_layer = t * w * 3 * w + t * w * w + 2 * t * t * w + 2 * t * w * 4 * w
        tail = w * self.embed_dim
        if self.family == "siglip":       # the pooling head: k | v of every token, one query row's attention, out-proj and the MLP
            tail = t * w * 2 * w + 2 * t * w + w * w + 2 * w * 4 * w
        return 2.0 * (p * 3 * self.patch * self.patch * w + self.v_layers * per_layer + tail)

    def text_flops(self) -> float:
        t, w = self.ctx, self.t_width
        per_layer = t * w * 3 * w + t * w * w + 2 * t * t * w + 2 * t * w * 4 * w
        return 2.0 * (self.t_layers * per_layer + w * self.embed_dim)


@dataclass(frozen=True)
class BertArch:
    """A BERT sentence encoder (model family 2 of the library, `kemr_model_create_family`): ``transformers.BertModel`` without its
    pooler, then mean or CLS pooling.  Text-only: heads of 64, a 4 x MLP, exact GELU, LayerNorm eps 1e-12, absolute positions.
    intfloat/e5-base-v2 = BertArch(768, 12), thenlper/gte-large = BertArch(1024, 24).

    ``relative_bias=True`` says "MPNet" (model family 3, ``transformers.MPNetModel``): the same blocks with a learned relative position
    bias added to every attention score (one [32, heads] table for all layers), no token types, and ``layer_norm_eps`` 1e-5 (the
    published all-mpnet-base-v2) or 1e-12 (MPNetConfig's default).  sentence-transformers/all-mpnet-base-v2 =
    BertArch(768, 12, vocab=30527, relative_bias=True, layer_norm_eps=1e-5)."""
    width: int
    layers: int
    vocab: int = 30522
    ctx: int = 512                # positions the model serves (`max_seq_length` of a sentence-transformers directory, else max_position_embeddings)
    pooling: str = "mean"         # "mean" (masked mean pooling) or "cls"
    positions: int = 0            # rows of the checkpoint's positional table when it has more than ctx (0 = ctx)
    family: str = "bert"
    relative_bias: bool = False   # MPNet's relative position bias in every attention score (model family 3)
    layer_norm_eps: float = 1e-12

    def __post_init__(self):
        if not self.relative_bias and self.layer_norm_eps != 1e-12:
            raise ValueError(f"BertArch: layer_norm_eps {self.layer_norm_eps!r}; BERT encoders are served with 1e-12 only")
        if self.relative_bias and self.layer_norm_eps not in MPNET_EPS:
            raise ValueError(f"BertArch: layer_norm_eps {self.layer_norm_eps!r}; MPNet encoders are served with {sorted(MPNET_EPS)} only")
        if self.width not in (256, 512, 768, 1024, 1280):
            raise ValueError(f"BertArch: width {self.width}; served: 256, 512, 768, 1024, 1280 (heads of 64, multiples of 256)")
        if not 1 <= self.ctx <= 512:
            raise ValueError(f"BertArch: ctx {self.ctx} not in 1..512")
        if self.pooling not in BERT_POOLING:
            raise ValueError(f"BertArch: pooling {self.pooling!r}; served: {list(BERT_POOLING)}")

    @property
    def embed_dim(self) -> int:
        return self.width

    @property
    def heads(self) -> int:
        return self.width // 64

    @property
    def library_family(self) -> int:
        """The library's family number: 2 (BERT, `kemr_model_create_family`) or 3 (MPNet: a family-2 model with option "family" = 3)."""
        return 3 if self.relative_bias else 2

    def cfg_dict(self) -> Dict[str, int]:
        """The nine numbers of kemr_cfg for families 2 and 3: the vision fields are 0, embed_dim is the width."""
        return dict(embed_dim=self.width, image_size=0, patch=0, v_width=0, v_layers=0, t_width=self.width, t_layers=self.layers,
                    vocab=self.vocab, ctx=self.ctx)

    def text_flops(self, tokens: int) -> float:
        """Algorithmic FLOPs of one text of `tokens` tokens."""
        t, w = tokens, self.width
        return 2.0 * self.layers * (t * w * 3 * w + t * w * w + 2 * t * t * w + 2 * t * w * 4 * w)


BERT_POOLING = {"mean": 0, "cls": 1}     # model option "pooling" (include/kemr.h)
MPNET_EPS = {1e-5: 5, 1e-12: 12}         # model option "layer_norm_eps" (family 3): the exponent
BERT_ARCHS: Dict[str, BertArch] = {
    "e5-base-v2": BertArch(768, 12),
    "gte-large": BertArch(1024, 24),
    "all-mpnet-base-v2": BertArch(768, 12, vocab=30527, relative_bias=True, layer_norm_eps=1e-5),
    "tiny-bert": BertArch(256, 2, vocab=1024),       # the test fixture
}


def _siglip(image_size: int, width: int, layers: int, **kw) -> ClipArch:
    """A SigLIP arch: both towers `width` wide and `layers` deep, patch 16, joint dim = width, vocabulary 32000, 64 positions."""
    kw = {"vocab": 32000, "ctx": 64, **kw}
    return ClipArch(width, image_size, 16, width, layers, width, layers, family="siglip", **kw)


ARCHS: Dict[str, ClipArch] = {
    "ViT-L/14": ClipArch(768, 224, 14, 1024, 24, 768, 12),
    "ViT-L/14@336px": ClipArch(768, 336, 14, 1024, 24, 768, 12),      # 24 x 24 + 1 = 577 vision tokens
    "ViT-B/16": ClipArch(512, 224, 16, 768, 12, 512, 12),
    "ViT-B/32": ClipArch(512, 224, 32, 768, 12, 512, 12),
    # OpenCLIP / LAION ViT-H/14 under OpenCLIP's own name ("ViT-H/14" stays unknown): vision 1280 wide = 16 heads of 80, 32 layers, 257
    # tokens; text 1024 wide = 16 heads of 64, 24 layers; joint dim 1024; trained with the exact GELU (activation="gelu")
    "ViT-H-14": ClipArch(1024, 224, 14, 1280, 32, 1024, 24, v_head_dim=80),
    # Long-CLIP: the towers of ViT-B/16 and ViT-L/14 with a text tower of 248 positions (same state-dict names; its second positional
    # table is folded at load, hf_checkpoint.fold_longclip_positions)
    "LongCLIP-B": ClipArch(512, 224, 16, 768, 12, 512, 12, ctx=248),
    "LongCLIP-L": ClipArch(768, 224, 14, 1024, 24, 768, 12, ctx=248),
    # small shapes for tests (same structure, head dim 64)
    "tiny": ClipArch(128, 32, 8, 256, 2, 256, 2, vocab=512, ctx=16),
    "tiny-ctx248": ClipArch(128, 32, 8, 256, 2, 256, 2, vocab=512, ctx=248),      # "tiny" with Long-CLIP's 248 text positions
    # "tiny" with a 17 x 17 grid: 290 vision tokens, the smallest tower past the 288 rows of the LDS attention backward (training tests)
    "tiny-290": ClipArch(128, 136, 8, 256, 2, 256, 2, vocab=512, ctx=16),
    "tiny-long": ClipArch(256, 112, 8, 256, 3, 512, 3, vocab=1024, ctx=77),
    # the structure of ViT-H-14 (vision heads of 80 at width 1280, the only width that is a multiple of 256 and of 80): 5 and 257 tokens
    "tiny-h": ClipArch(128, 28, 14, 1280, 2, 256, 2, vocab=512, ctx=16, v_head_dim=80),
    "tiny-h-257": ClipArch(128, 224, 14, 1280, 2, 256, 2, vocab=512, ctx=16, v_head_dim=80),
    # SigLIP under OpenCLIP's names: B/16 (768 wide, 12 layers) at 224 / 256 / 384 / 512 px = 196 / 256 / 576 / 1024 tokens, L/16 (1024
    # wide, 24 layers) at 256 / 384 px
    "ViT-B-16-SigLIP": _siglip(224, 768, 12),
    "ViT-B-16-SigLIP-256": _siglip(256, 768, 12),
    "ViT-B-16-SigLIP-384": _siglip(384, 768, 12),
    "ViT-B-16-SigLIP-512": _siglip(512, 768, 12),
    "ViT-L-16-SigLIP-256": _siglip(256, 1024, 24),
    "ViT-L-16-SigLIP-384": _siglip(384, 1024, 24),
    # the same structure for tests: 16, 196 and 576 tokens (tile kernel, its 7-tile form, the streaming kernel)
    "tiny-siglip": _siglip(64, 256, 2, vocab=512, ctx=16),
    "tiny-siglip-196": _siglip(224, 256, 2, vocab=512, ctx=16),
    "tiny-siglip-576": _siglip(384, 256, 2, vocab=512, ctx=16),
}


def get_arch(name: str) -> ClipArch:
    if name not in ARCHS:
        raise RuntimeError(f"Model {name} not found; available models = {list(ARCHS)}")
    return ARCHS[name]
