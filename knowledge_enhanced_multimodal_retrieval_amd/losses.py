"""Contrastive losses of the fine-tuning recipe (reference ``src/clip/train/losses.py``) on the fused InfoNCE kernels.

``InfoNCELoss`` and ``JointContrastiveLoss`` keep the reference's signatures, weight normalisation and metric keys.  The loss and its
gradient come from ``kemr_infonce_forward`` / ``kemr_infonce_backward`` (csrc/infonce.hip) through one ``torch.autograd.Function``: the
n x n logits and softmax matrices of the torch formulation are never stored, so a batch can be a whole training split.  The forward
saves the features and the 2 n log-sum-exp values; the backward recomputes the logits tile by tile.  There is no CPU path: CPU
tensors raise the engine's "no CPU fallback" error.

``FusionContrastiveLoss`` is the objective the learned fusion heads are trained on (``fusion_train.py``): the same symmetric InfoNCE over
the head's fused scores ``S = head(q, img, tgt)`` of frozen, normalised embeddings, through ``kemr_pairhead_forward`` / ``_backward``
(csrc/pairhead.hip).  The reference has no such objective (its ``train_fusion.py`` is a copy of the evaluator); this one is the project's.
"""
from __future__ import annotations

from typing import Dict, Tuple

import torch
import torch.nn as nn

from . import _lib, engine


class _InfoNCE(torch.autograd.Function):
    """(features_a, features_b, temperature) -> fp32 [3] = loss, loss_a2b, loss_b2a.  Only element 0 is differentiable: the kernel's
    backward is the gradient of `loss`, which is what both modules below return; the two halves are reported, not trained on."""

    @staticmethod
    def forward(ctx, a, b, temperature):
        a32, b32 = a.detach().float().contiguous(), b.detach().float().contiguous()
        losses, lse = engine.infonce_forward(a32, b32, temperature)
        ctx.save_for_backward(a32, b32, lse)
        ctx.temperature = temperature
        ctx.dtypes = (a.dtype, b.dtype)
        return losses

    @staticmethod
    def backward(ctx, grad_losses):
        a32, b32, lse = ctx.saved_tensors
        ga, gb = engine.infonce_backward(a32, b32, lse, ctx.temperature)
        g = grad_losses[0]
        return (ga * g).to(ctx.dtypes[0]), (gb * g).to(ctx.dtypes[1]), None


class InfoNCELoss(nn.Module):
    """Symmetric InfoNCE: mean of the a -> b and b -> a cross entropies of (a b^T) / temperature with the diagonal as labels."""

    def __init__(self, temperature: float = 0.07):
        super().__init__()
        self.temperature = temperature

    def _losses(self, features_a: torch.Tensor, features_b: torch.Tensor) -> torch.Tensor:
        return _InfoNCE.apply(features_a, features_b, float(self.temperature))

    def forward(self, features_a: torch.Tensor, features_b: torch.Tensor) -> Tuple[torch.Tensor, Dict[str, float]]:
        losses = self._losses(features_a, features_b)
        host = losses.detach().cpu().tolist()
        return losses[0], {"loss": host[0], "loss_a2b": host[1], "loss_b2a": host[2]}


class JointContrastiveLoss(nn.Module):
    """t2i_weight * InfoNCE(target, image) + t2t_weight * InfoNCE(query, target), the weights normalised to sum 1.  The target
    features take gradient from both pairs; autograd adds the two."""

    def __init__(self, temperature: float = 0.07, t2i_weight: float = 0.5, t2t_weight: float = 0.5):
        super().__init__()
        self.temperature = temperature
        self.infonce = InfoNCELoss(temperature=temperature)
        weight_sum = t2i_weight + t2t_weight
        self.t2i_weight = t2i_weight / weight_sum
        self.t2t_weight = t2t_weight / weight_sum

    def forward(self, image_features: torch.Tensor, query_features: torch.Tensor, target_features: torch.Tensor
                ) -> Tuple[torch.Tensor, Dict[str, float]]:
        loss_t2i = self.infonce._losses(target_features, image_features)[0]
        loss_t2t = self.infonce._losses(query_features, target_features)[0]
        total = self.t2i_weight * loss_t2i + self.t2t_weight * loss_t2t
        host = torch.stack([total.detach(), loss_t2i.detach(), loss_t2t.detach()]).cpu().tolist()
        return total, {"loss": host[0], "loss_t2i": host[1], "loss_t2t": host[2],
                       "t2i_weight": self.t2i_weight, "t2t_weight": self.t2t_weight}


# ------------------------------------------------------------------------------------------------ learned fusion heads
FUSION_TRAIN_MODES = {"linear": _lib.PAIRHEAD_LINEAR, "gated": _lib.PAIRHEAD_GATED, "simple_gated": _lib.PAIRHEAD_GATED,
                      "simple_gated_with_bias": _lib.PAIRHEAD_GATED}
FUSION_TRAIN_REFUSED = {
    "bilinear": "training the bilinear head is not served: its gradient needs dL/dS contracted with the gallery, and the 2 D wide operand "
                "that contraction would ride on exceeds the fused kernels' d <= 1280 at D = 768",
    "cross_attention": "training the cross_attention head is not served: it needs a backward pass through the pair kernel "
                       "(kemr_cross_attention_pairs), which does not exist",
}


def fusion_train_mode(fusion_type: str) -> int:
    """The pair-score kernel mode that trains `fusion_type`; ValueError with the reason for the heads that are not trained."""
    if fusion_type in FUSION_TRAIN_REFUSED:
        raise ValueError(FUSION_TRAIN_REFUSED[fusion_type])
    if fusion_type not in FUSION_TRAIN_MODES:
        raise ValueError(f"Unknown fusion type: {fusion_type}")
    return FUSION_TRAIN_MODES[fusion_type]


class _PairHeadGated(torch.autograd.Function):
    """(gate [n], q, img, tgt, temperature) -> fp32 [3] = loss, loss_q2g, loss_g2q; element 0 is differentiable, with respect to the gate."""

    @staticmethod
    def forward(ctx, gate, q, img, tgt, temperature):
        g32 = gate.detach().float().contiguous()
        losses, lse = engine.pairhead_forward(_lib.PAIRHEAD_GATED, q, img, tgt, temperature, gate=g32)
        ctx.save_for_backward(g32, q, img, tgt, lse)
        ctx.temperature, ctx.dtype = temperature, gate.dtype
        return losses

    @staticmethod
    def backward(ctx, grad_losses):
        g32, q, img, tgt, lse = ctx.saved_tensors
        dg = engine.pairhead_backward(_lib.PAIRHEAD_GATED, q, img, tgt, lse, ctx.temperature, gate=g32)
        return (dg * grad_losses[0]).to(ctx.dtype), None, None, None, None


class _PairHeadLinear(torch.autograd.Function):
    """(w0 [hidden, 2], b0 [hidden], w1 [1, hidden], b1 [1], q, img, tgt, temperature) -> fp32 [3]; element 0 is differentiable, with
    respect to the four parameters (the kernel's gradients, reshaped)."""

    @staticmethod
    def forward(ctx, w0, b0, w1, b1, q, img, tgt, temperature):
        lin = tuple(x.detach().float().contiguous() for x in (w0, b0, w1.reshape(-1), b1.reshape(-1)))
        losses, lse = engine.pairhead_forward(_lib.PAIRHEAD_LINEAR, q, img, tgt, temperature, linear=lin)
        ctx.save_for_backward(*lin, q, img, tgt, lse)
        ctx.temperature, ctx.like = temperature, (w0, b0, w1, b1)
        return losses

    @staticmethod
    def backward(ctx, grad_losses):
        *lin, q, img, tgt, lse = ctx.saved_tensors
        flat = engine.pairhead_backward(_lib.PAIRHEAD_LINEAR, q, img, tgt, lse, ctx.temperature, linear=tuple(lin)) * grad_losses[0]
        h = lin[1].numel()
        parts = (flat[:2 * h], flat[2 * h:3 * h], flat[3 * h:4 * h], flat[4 * h:])
        return tuple(g.reshape(p.shape).to(p.dtype) for g, p in zip(parts, ctx.like)) + (None, None, None, None)


class FusionContrastiveLoss(nn.Module):
    """Symmetric InfoNCE over a fusion head's scores: z = head(q, img, tgt) / temperature with the diagonal as labels,
    loss = (mean_i (lse_j z_ij - z_ii) + mean_j (lse_i z_ij - z_jj)) / 2.

    ``forward(fusion_model, q, img, tgt) -> (loss, {"loss", "loss_q2g", "loss_g2q"})`` for L2-normalised [n, D] device embeddings of the
    frozen encoders (no gradient goes to them).  The head is evaluated in eval mode -- its Dropout(0.1) is NOT applied -- so the function
    optimised is bit for bit the family of functions ``FusionModel.forward / rank`` serve.  linear: the kernel returns the gradients of
    ``fusion.0.weight / .bias`` and ``fusion.3.weight / .bias``; the gated heads: the kernel returns dL/dgate and torch carries it through
    the head's own ``gate()``.  bilinear and cross_attention heads and CPU inputs raise ValueError."""

    def __init__(self, temperature: float = 0.07):
        super().__init__()
        self.temperature = temperature

    def forward(self, fusion_model, q: torch.Tensor, img: torch.Tensor, tgt: torch.Tensor) -> Tuple[torch.Tensor, Dict[str, float]]:
        mode = fusion_train_mode(fusion_model.fusion_type)
        for t, name in ((q, "query"), (img, "image"), (tgt, "target")):
            if not isinstance(t, torch.Tensor) or not t.is_cuda:
                raise ValueError(f"FusionContrastiveLoss: the {name} embeddings must be a tensor on the GPU (there is no CPU path)")
        q, img, tgt = (t.detach().float().contiguous() for t in (q, img, tgt))
        head = fusion_model.fusion_head.to(q.device)
        if mode == _lib.PAIRHEAD_LINEAR:
            f = head.fusion
            losses = _PairHeadLinear.apply(f[0].weight, f[0].bias, f[3].weight, f[3].bias, q, img, tgt, float(self.temperature))
        else:
            was_training = head.training
            head.eval()                               # no dropout in the gate: the served function
            gate = head.gate(q).reshape(-1)
            head.train(was_training)
            losses = _PairHeadGated.apply(gate, q, img, tgt, float(self.temperature))
        host = losses.detach().cpu().tolist()
        return losses[0], {"loss": host[0], "loss_q2g": host[1], "loss_g2q": host[2]}
