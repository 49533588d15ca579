"""Contrastive losses of the fine-tuning recipe (reference ``src/clip/train/losses.py``) on the fused InfoNCE kernels.

``InfoNCELoss`` and ``JointContrastiveLoss`` keep the reference's signatures, weight normalisation and metric keys.  The loss and its
gradient come from ``kemr_infonce_forward`` / ``kemr_infonce_backward`` (csrc/infonce.hip) through one ``torch.autograd.Function``: the
n x n logits and softmax matrices of the torch formulation are never stored, so a batch can be a whole training split.  The forward
saves the features and the 2 n log-sum-exp values; the backward recomputes the logits tile by tile.  There is no CPU path: CPU
tensors raise the engine's "no CPU fallback" error.
"""
from __future__ import annotations

from typing import Dict, Tuple

import torch
import torch.nn as nn

from . import engine


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
