"""Architecture presets of the CLIP models the reference evaluates
(`--model_name` choices at /root/reference/src/clip/eval/evaluator.py:264-266: ViT-B/32, ViT-B/16, ViT-L/14;
embed_dim rule at src/clip/eval/evaluator_fusion.py:192), plus ViT-L/14@336px, the higher-resolution OpenAI CLIP model, and
ViT-H-14 (OpenCLIP's spelling), LAION's ViT-H/14: the one served model whose vision heads are 80 wide instead of 64."""
from __future__ import annotations

from dataclasses import dataclass, asdict
from typing import Dict


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

    def __post_init__(self):
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
        return self.grid * self.grid + 1

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
        return d

    def cfg_dict(self) -> Dict[str, int]:
        """Exactly the fields of kemr_cfg, for every arch: what `_lib.KemrCfg(**...)`, oracle.clip_ref and the tools take."""
        d = asdict(self)
        del d["v_head_dim"]
        return d

    # algorithmic FLOPs per item
    def image_flops(self) -> float:
        t, w, p = self.v_tokens, self.v_width, self.grid * self.grid
        per_layer = t * w * 3 * w + t * w * w + 2 * t * t * w + 2 * t * w * 4 * w
        return 2.0 * (p * 3 * self.patch * self.patch * w + self.v_layers * per_layer + w * self.embed_dim)

    def text_flops(self) -> float:
        t, w = self.ctx, self.t_width
        per_layer = t * w * 3 * w + t * w * w + 2 * t * t * w + 2 * t * w * 4 * w
        return 2.0 * (self.t_layers * per_layer + w * self.embed_dim)


ARCHS: Dict[str, ClipArch] = {
    "ViT-L/14": ClipArch(768, 224, 14, 1024, 24, 768, 12),
    "ViT-L/14@336px": ClipArch(768, 336, 14, 1024, 24, 768, 12),      # 24 x 24 + 1 = 577 vision tokens
    "ViT-B/16": ClipArch(512, 224, 16, 768, 12, 512, 12),
    "ViT-B/32": ClipArch(512, 224, 32, 768, 12, 512, 12),
    # OpenCLIP / LAION ViT-H/14 under OpenCLIP's own name ("ViT-H/14" stays unknown): vision 1280 wide = 16 heads of 80, 32 layers, 257
    # tokens; text 1024 wide = 16 heads of 64, 24 layers; joint dim 1024; trained with the exact GELU (activation="gelu")
    "ViT-H-14": ClipArch(1024, 224, 14, 1280, 32, 1024, 24, v_head_dim=80),
    # small shapes for tests (same structure, head dim 64)
    "tiny": ClipArch(128, 32, 8, 256, 2, 256, 2, vocab=512, ctx=16),
    "tiny-long": ClipArch(256, 112, 8, 256, 3, 512, 3, vocab=1024, ctx=77),
    # the structure of ViT-H-14 (vision heads of 80 at width 1280, the only width that is a multiple of 256 and of 80): 5 and 257 tokens
    "tiny-h": ClipArch(128, 28, 14, 1280, 2, 256, 2, vocab=512, ctx=16, v_head_dim=80),
    "tiny-h-257": ClipArch(128, 224, 14, 1280, 2, 256, 2, vocab=512, ctx=16, v_head_dim=80),
}


def get_arch(name: str) -> ClipArch:
    if name not in ARCHS:
        raise RuntimeError(f"Model {name} not found; available models = {list(ARCHS)}")
    return ARCHS[name]
