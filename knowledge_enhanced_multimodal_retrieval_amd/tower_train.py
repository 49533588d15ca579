"""A differentiable CLIP text tower and the locked-image trainer (``python -m src.clip.train.trainer --lock_image_tower``).

``TextTower`` restates the text tower of a CLIP-family model in torch over the MODEL'S OWN parameters (``token_embedding``,
``positional_embedding``, ``transformer.resblocks.*``, ``ln_final``, ``text_projection``): token + positional embedding, pre-LN residual
blocks (``ln_1`` -> ``attn.in_proj_*`` -> causal attention -> ``attn.out_proj`` -> +res -> ``ln_2`` -> ``mlp.c_fc`` -> QuickGELU or exact
GELU, as the model's ``activation`` says -> ``mlp.c_proj`` -> +res), the row at the end-of-text token (what ``kemr_encode_text_pooled``
returns), then ``ln_final``, ``text_projection`` and the L2 normalisation (``finetune.project``).  Everything but the attention is
ordinary torch autograd -- LayerNorms, vendor GEMMs, an elementwise activation.  The attention is ours in both directions:

  attention="op"     ``_OpAttention``: the forward scales q by 1/8 and calls ``kemr_op_attention`` (causal), the backward calls
                     ``kemr_op_attention_backward`` (csrc/attention_bwd.hip) and scales dq by 1/8.  GPU only; the linears run under
                     bf16 autocast, LayerNorm, the residual stream and the head in fp32 over fp32 master weights.
  attention="torch"  the plain softmax formulation in torch, in the dtype of the parameters (fp32, fp64), on any device: the reference
                     of the tests and the only way the module runs without a GPU.  ``autocast=True`` gives it the same bf16 linears
                     (the yardstick the op's gradients are held to).

Running length: ``forward(ids, t)`` may run the first ``t`` positions only, ``t`` = the batch's longest text (end-of-text position + 1,
``longest``).  Under the causal mask no row up to a text's end-of-text token sees a later position, so this is exact for every row that
reaches the loss.  Family ``clip`` only (Long-CLIP's 248 positions included); SigLIP and BERT models are refused like
``finetune.ProjectionHeads`` refuses them.

``TextTowerTrainer`` is ``finetune.HeadTrainer``'s loop -- batch schedule, accumulation, ``grad_clip``, validation through the served
engine after each epoch, early stopping, ``metrics_epoch.jsonl``, checkpoints through ``clip_model.save_checkpoint`` -- with another
feature function: the image tower stays locked (its pooled rows are cached once, ``finetune.cache_image_pooled``) and goes through
``ProjectionHeads.image``; queries and targets of the batch run through the differentiable tower.  What trains: the six head tensors
plus the whole text tower.  No other vision parameter can receive a gradient: none takes part in the graph.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from .clip_model import _unwrap
from .finetune import HeadTrainer, ProjectionHeads, project

MAX_T = 288          # KEMR_MAX_TEXT_CTX: the range of kemr_op_attention (causal) and of its backward


class _OpAttention(torch.autograd.Function):
    """qkv [batch * t, 3 width] (q not yet scaled) -> bf16 [batch * t, width] through the library's two attention kernels."""

    @staticmethod
    def forward(ctx, qkv: torch.Tensor, batch: int, t: int, width: int) -> torch.Tensor:
        from . import engine
        scaled = qkv.detach().to(torch.bfloat16).clone()
        scaled[:, :width] *= 0.125                       # exact: a power of two
        ctx.save_for_backward(scaled)
        ctx.shape, ctx.in_dtype = (batch, t, width), qkv.dtype
        return engine.op_attention(scaled, batch, t, width, True)

    @staticmethod
    def backward(ctx, dout: torch.Tensor):
        from . import engine
        (scaled,) = ctx.saved_tensors
        batch, t, width = ctx.shape
        dqkv = engine.attention_backward(scaled, dout.to(torch.bfloat16).contiguous(), batch, t, width, True)
        dqkv[:, :width] *= 0.125                         # the caller's 1/8 of q (exact)
        return dqkv.to(ctx.in_dtype), None, None, None


def torch_attention(qkv: torch.Tensor, batch: int, t: int, width: int) -> torch.Tensor:
    """The plain formulation: softmax(q k^T / 8 + causal mask) v per head of 64, in qkv's dtype."""
    heads = width // 64
    q, k, v = (x.reshape(batch, t, heads, 64).transpose(1, 2) for x in qkv.split(width, dim=-1))
    s = (q * 0.125) @ k.transpose(-1, -2)
    s = s + torch.full((t, t), float("-inf"), dtype=s.dtype, device=s.device).triu_(1)
    return (torch.softmax(s, dim=-1).to(v.dtype) @ v).transpose(1, 2).reshape(batch * t, width)


def longest(ids: torch.Tensor) -> int:
    """The batch's longest text: the highest end-of-text position (first arg-max of the ids) + 1.  One host read for device ids."""
    return int(ids.argmax(dim=-1).max()) + 1


class TextTower(nn.Module):
    """See the module docstring.  ``trainable=True`` sets ``requires_grad`` on the text tower's parameters (and leaves every other
    parameter of the model as it finds it)."""

    def __init__(self, model: nn.Module, attention: str = "op", autocast: Optional[bool] = None, trainable: bool = True):
        super().__init__()
        m = _unwrap(model)
        family = getattr(getattr(m, "arch", None), "family", "clip")
        if family != "clip" or not hasattr(m, "text_projection") or not hasattr(m, "visual") or not hasattr(m.visual, "proj"):
            raise ValueError(f"TextTower: only the CLIP family's text tower is restated (this model's family: {family!r}; SigLIP pools the "
                             "last position of a bidirectional tower, BERT models are post-LN sentence encoders)")
        if attention not in ("op", "torch"):
            raise ValueError(f"TextTower: attention must be 'op' (the HIP kernels) or 'torch' (the plain formulation), got {attention!r}")
        if m.arch.t_width % 64 or m.arch.t_heads * 64 != m.arch.t_width:
            raise ValueError(f"TextTower: heads of 64 only (width {m.arch.t_width}, {m.arch.t_heads} heads)")
        self.attention = attention
        self.autocast = (attention == "op") if autocast is None else bool(autocast)
        self.activation, self.width, self.ctx = m.activation, m.arch.t_width, m.arch.ctx
        self.token_embedding, self.transformer = m.token_embedding, m.transformer              # the model's own modules and parameters
        self.positional_embedding = m.positional_embedding
        self.ln_final, self.text_projection = m.ln_final, m.text_projection
        if trainable:
            for p in self.parameters():
                p.requires_grad = True

    def named_text_parameters(self) -> Dict[str, nn.Parameter]:
        """Every parameter of the text side under its name in the model's state dict."""
        out = {"token_embedding.weight": self.token_embedding.weight, "positional_embedding": self.positional_embedding}
        out.update({f"transformer.{k}": p for k, p in self.transformer.named_parameters()})
        out.update({"ln_final.weight": self.ln_final.weight, "ln_final.bias": self.ln_final.bias, "text_projection": self.text_projection})
        return out

    def _linear(self, x: torch.Tensor, lin_w: torch.Tensor, lin_b: torch.Tensor) -> torch.Tensor:
        if self.autocast:
            with torch.autocast(x.device.type, dtype=torch.bfloat16):
                return F.linear(x, lin_w, lin_b)
        return F.linear(x, lin_w, lin_b)

    def _act(self, h: torch.Tensor) -> torch.Tensor:
        h = h.float() if h.dtype == torch.bfloat16 else h
        return F.gelu(h) if self.activation == "gelu" else h * torch.sigmoid(1.702 * h)

    def _attend(self, qkv: torch.Tensor, batch: int, t: int) -> torch.Tensor:
        """qkv [batch * t, 3 width] (q not yet scaled) -> [batch * t, width], causal.  (tools/bench_text_tower_train.py overrides this.)"""
        if self.attention == "op":
            return _OpAttention.apply(qkv, batch, t, self.width)
        return torch_attention(qkv, batch, t, self.width)

    def _block(self, x: torch.Tensor, blk: nn.Module, batch: int, t: int) -> torch.Tensor:
        w = self.width
        h = F.layer_norm(x, (w,), blk.ln_1.weight, blk.ln_1.bias, blk.ln_1.eps)
        qkv = self._linear(h, blk.attn.in_proj_weight, blk.attn.in_proj_bias)
        a = self._attend(qkv, batch, t)
        x = x + self._linear(a, blk.attn.out_proj.weight, blk.attn.out_proj.bias)
        h = F.layer_norm(x, (w,), blk.ln_2.weight, blk.ln_2.bias, blk.ln_2.eps)
        h = self._act(self._linear(h, blk.mlp.c_fc.weight, blk.mlp.c_fc.bias))
        return x + self._linear(h, blk.mlp.c_proj.weight, blk.mlp.c_proj.bias)

    def pooled(self, ids: torch.Tensor, t: Optional[int] = None) -> torch.Tensor:
        """ids int [B, ctx] -> [B, width]: the residual-stream row at each text's end-of-text token, before ``ln_final``."""
        if ids.dim() != 2 or ids.shape[1] > self.ctx:
            raise ValueError(f"TextTower: ids must be [B, <= {self.ctx}], got {tuple(ids.shape)}")
        dev = self.positional_embedding.device
        if self.attention == "op" and dev.type != "cuda":
            raise RuntimeError(f"TextTower: attention='op' must live on the GPU (got device {dev}); this path has no CPU fallback "
                               "(attention='torch' is the reference formulation)")
        ids = ids.to(dev).long()
        batch = ids.shape[0]
        eot = ids.argmax(dim=-1)
        t = ids.shape[1] if t is None else int(t)
        if not 1 <= t <= min(ids.shape[1], MAX_T):
            raise ValueError(f"TextTower: running length t = {t} is outside 1..{min(ids.shape[1], MAX_T)}")
        if t < ids.shape[1] and int(eot.max()) >= t:
            raise ValueError(f"TextTower: running length t = {t} cuts a text whose end-of-text token sits at position {int(eot.max())}")
        x = (self.token_embedding.weight[ids[:, :t]] + self.positional_embedding[:t]).reshape(batch * t, self.width)
        for blk in self.transformer.resblocks:
            x = self._block(x, blk, batch, t)
        return x.reshape(batch, t, self.width)[torch.arange(batch, device=dev), eot]

    def forward(self, ids: torch.Tensor, t: Optional[int] = None) -> torch.Tensor:
        """[B, embed_dim]: the L2-normalised text embeddings."""
        return project(self.pooled(ids, t), self.ln_final.weight, self.ln_final.bias, self.text_projection, self.ln_final.eps)


class LockedImageTuning(nn.Module):
    """What ``--lock_image_tower`` trains: ``ProjectionHeads`` (six tensors) plus the whole text tower, over the model's own parameters."""

    def __init__(self, model: nn.Module, attention: str = "op", autocast: Optional[bool] = None):
        super().__init__()
        self.heads = ProjectionHeads(model)              # freezes everything, then its six tensors
        self.tower = TextTower(model, attention=attention, autocast=autocast, trainable=True)

    def forward(self, pooled_image: torch.Tensor, query_ids: torch.Tensor, target_ids: torch.Tensor
                ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        n = query_ids.shape[0]
        ids = torch.cat([query_ids, target_ids])
        text = self.tower(ids, longest(ids))
        return self.heads.image(pooled_image), text[:n], text[n:]


class TextTowerTrainer(HeadTrainer):
    """``HeadTrainer``'s loop with ``rows`` = (cached pooled image rows fp32 [N, v_width], query ids, target ids int [N, ctx], all on the
    model's device) and ``heads`` a ``LockedImageTuning``.  A batch's activations live on the device for its backward pass, so a batch
    must be given: ``batch_size=0`` (the whole split) is refused."""

    def __init__(self, model: nn.Module, heads: LockedImageTuning, rows: Sequence[torch.Tensor], loss_fn, optimizer, scheduler=None,
                 batch_size: int = 64, **kw):
        if batch_size <= 0:
            raise ValueError(BATCH_0_REFUSED)
        super().__init__(model, heads, rows, loss_fn, optimizer, scheduler, batch_size=batch_size, **kw)


BATCH_0_REFUSED = ("--batch_size 0 (the whole split as one batch) is not served with --lock_image_tower: the text tower's backward pass "
                   "keeps the activations of a whole batch on the device, and the activations of a whole split do not fit; give a batch size")
