"""Learned T2I/T2T fusion heads over a frozen CLIP, with the reference's class names and state-dict keys
(/root/reference/src/clip/model/fusion_model.py: heads :9-240, ``FusionModel`` :243-331), scored by the HIP kernels.

The heads are parameter containers (so reference checkpoints load: ``fusion_head.gate_net.0.weight`` ...); the scoring
``forward(query_embed [N,D], image_embed [M,D], target_embed [M,D]) -> [N,M]`` is inference only (eval mode, dropout
inactive) and maps onto the fused similarity kernel:

* gated / simple_gated / simple_gated_with_bias: ``g*t2i + (1-g)*t2t`` = ONE contraction over ``[g*q ; (1-g)*q]`` x
  ``[img ; tgt]`` -- the per-query gate is a row scale of the query panel (``kemr_panel_build`` row_scale).  The gate
  itself (a [N,D]x[D,128] MLP or a dot product per query) is O(N*D) host-side plumbing on the device tensors.
* bilinear: ``q . (W img)^T = (q W) . img^T`` -- the D x D transform is applied to the N queries (a small contraction
  with the same kernel) instead of to the M candidates; then one weighted contraction as above.
* linear: MLP(2->128->1) of every (t2i, t2t) pair -- needs both dense matrices; ``kemr_linear_head`` applies the MLP
  element-wise on the GPU.
* cross_attention: per-pair multi-head attention of one query over two keys + out-projection + a 3-layer MLP,
  O(N*M*D^2) in the reference.  Everything but the per-head 2-way softmax weights is linear in per-candidate
  quantities, so the projections are folded per candidate (``P = W1.Wo[:,head].V``, small dense contractions with
  the similarity kernel) and ``kemr_cross_attention_pairs`` does ~21 kFLOP per pair instead of ~1.6 MFLOP.

``rank()`` gives ranks / top-k without ever forming the [N,M] matrix for the gated family and bilinear; linear and
cross_attention produce the dense matrix on the GPU and rank it with ``kemr_rank_dense``.  ``prepare_gallery()`` + ``rerank()`` are
the two-stage route for those two heads: a deep shortlist by the fused T2I + T2T score, the head on the listed pairs only
(``kemr_cross_attention_rerank``; ``kemr_pair_scores`` + ``kemr_linear_head``), sorted by ``kemr_select_topk``.  With ``bonus=`` the
knowledge side rides along: the SPARQL bonus joins the shortlist score and ``kemr_list_fuse`` ranks the list by
``head_weight * head + bonus``.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch
import torch.nn as nn

from . import _lib, engine, ranking


class SimpleGatedFusionWithBias(nn.Module):
    def __init__(self, embed_dim: int = 768):
        super().__init__()
        self.query_weight = nn.Parameter(torch.zeros(embed_dim))
        self.bias = nn.Parameter(torch.tensor(-2.0))

    def gate(self, q):
        return torch.sigmoid((q * self.query_weight).sum(dim=1, keepdim=True) + self.bias)


class SimpleGatedFusion(nn.Module):
    def __init__(self, embed_dim: int = 768):
        super().__init__()
        self.query_weight = nn.Parameter(torch.ones(embed_dim))
        self.bias = nn.Parameter(torch.zeros(1))

    def gate(self, q):
        return torch.sigmoid((q * self.query_weight).sum(dim=1, keepdim=True) + self.bias)


class GatedFusionHead(nn.Module):
    def __init__(self, embed_dim: int = 768):
        super().__init__()
        self.gate_net = nn.Sequential(nn.Linear(embed_dim, 128), nn.ReLU(), nn.Dropout(0.1), nn.Linear(128, 1), nn.Sigmoid())

    def gate(self, q):
        return self.gate_net(q)


class LinearFusionHead(nn.Module):
    def __init__(self, hidden_dim: int = 128):
        super().__init__()
        self.fusion = nn.Sequential(nn.Linear(2, hidden_dim), nn.ReLU(), nn.Dropout(0.1), nn.Linear(hidden_dim, 1))


class BilinearFusionHead(nn.Module):
    def __init__(self, embed_dim: int = 768):
        super().__init__()
        self.W_image = nn.Linear(embed_dim, embed_dim, bias=False)
        self.W_target = nn.Linear(embed_dim, embed_dim, bias=False)
        self.alpha = nn.Parameter(torch.tensor(0.5))


class CrossAttentionFusionHead(nn.Module):
    """Parameter container (reference checkpoints load); scored by ``FusionModel._cross_attention``."""

    def __init__(self, embed_dim: int = 768, num_heads: int = 8, hidden_dim: int = 256):
        super().__init__()
        self.embed_dim = embed_dim
        self.query_proj = nn.Linear(embed_dim, embed_dim)
        self.image_proj = nn.Linear(embed_dim, embed_dim)
        self.target_proj = nn.Linear(embed_dim, embed_dim)
        self.cross_attn = nn.MultiheadAttention(embed_dim=embed_dim, num_heads=num_heads, batch_first=True, dropout=0.1)
        self.score_mlp = nn.Sequential(nn.Linear(embed_dim, hidden_dim), nn.ReLU(), nn.Dropout(0.1),
                                       nn.Linear(hidden_dim, 64), nn.ReLU(), nn.Dropout(0.1), nn.Linear(64, 1))


_GATED = ("gated", "simple_gated", "simple_gated_with_bias")
_RERANK_HEADS = ("linear", "cross_attention")          # the pair heads: scored densely by forward(), on shortlists by rerank()


class HeadGallery:
    """A gallery prepared for ``FusionModel.rerank``: everything the two-stage route needs per candidate, on the device, computed
    once per gallery instead of once per query batch.

    * ``fused_panel``: the fp32x3 panel of ``[image ; target]`` that the shortlist stage scores (``engine.sim_topk_deep``);
    * linear head: ``image_panel`` / ``target_panel``, the two fp32x3 panels ``engine.pair_scores`` reads;
    * cross_attention head: ``cand`` = keys Ki, Kt [M, D], folded projections Pi, Pt [M, 8, hid1] (2 * M * 8 * hid1 * 4 bytes:
      0.7 GB at M = 43 000, hid1 = 256) and the MLP's constants.

    The cross_attention quantities are functions of the head's parameters: a HeadGallery is STALE once they change (an optimizer
    step, ``load_state_dict``); call ``refresh()`` or prepare a new one.  The linear head's parameters are read at every call."""

    def __init__(self, model: "FusionModel", image_embed, target_embed):
        self.model, self.fusion_type = model, model.fusion_type
        self.image = ranking.to_device_f32(image_embed)
        self.target = ranking.to_device_f32(target_embed, self.image.device)
        if self.image.dim() != 2 or self.image.shape != self.target.shape:
            raise ValueError("prepare_gallery: image and target embeddings must share one [M, D] shape")
        self.refresh()

    def __len__(self):
        return self.image.shape[0]

    @property
    def device(self):
        return self.image.device

    @torch.no_grad()
    def refresh(self) -> "HeadGallery":
        """Recompute every per-candidate quantity from the stored embeddings and the head's CURRENT parameters."""
        self.fused_panel = engine.build_panel([self.image, self.target], _lib.SIDE_GALLERY, 3)
        self.image_panel = self.target_panel = self.cand = None
        if self.fusion_type == "linear":
            self.image_panel = engine.build_panel([self.image], _lib.SIDE_GALLERY, 3)
            self.target_panel = engine.build_panel([self.target], _lib.SIDE_GALLERY, 3)
        else:
            self.cand = self.model._cross_attention_gallery(self.image, self.target)
        return self


class FusionModel(nn.Module):
    """Wrapper for a fusion head over a frozen CLIP encoder (``fusion_type`` as in the reference)."""

    def __init__(self, clip_model, fusion_type: str = "linear", embed_dim: int = 768):
        super().__init__()
        self.clip_model, self.fusion_type = clip_model, fusion_type
        for p in self.clip_model.parameters():
            p.requires_grad = False
        heads = {"linear": lambda: LinearFusionHead(hidden_dim=128),
                 "cross_attention": lambda: CrossAttentionFusionHead(embed_dim=embed_dim, num_heads=8, hidden_dim=256),
                 "gated": lambda: GatedFusionHead(embed_dim=embed_dim),
                 "simple_gated": lambda: SimpleGatedFusion(embed_dim=embed_dim),
                 "simple_gated_with_bias": lambda: SimpleGatedFusionWithBias(embed_dim=embed_dim),
                 "bilinear": lambda: BilinearFusionHead(embed_dim=embed_dim)}
        if fusion_type not in heads:
            raise ValueError(f"Unknown fusion type: {fusion_type}")
        self.fusion_head = heads[fusion_type]()

    # ---- encoders: encode + L2 normalise, fused in the HIP tail kernel (reference fusion_model.py:287-303)
    @torch.no_grad()
    def encode_query(self, query_tokens):
        return self.clip_model.encode_text(query_tokens, normalize=True)

    @torch.no_grad()
    def encode_target(self, target_tokens):
        return self.clip_model.encode_text(target_tokens, normalize=True)

    @torch.no_grad()
    def encode_image(self, images):
        return self.clip_model.encode_image(images, normalize=True)

    # ---- scoring
    def _parts(self, q, img, tgt):
        """(query_parts, gallery_parts, weights, row_gates) of the fused contraction for this head."""
        h = self.fusion_head
        q = ranking.to_device_f32(q)
        img, tgt = ranking.to_device_f32(img, q.device), ranking.to_device_f32(tgt, q.device)
        if self.fusion_type in _GATED:
            g = self._gate(q)
            return [q, q], [img, tgt], None, [g, 1.0 - g]
        if self.fusion_type == "bilinear":
            h = h.to(q.device)
            a = float(torch.sigmoid(h.alpha))
            wq = []
            for lin in (h.W_image, h.W_target):                      # (q W)[n, j] = <q[n, :], W[:, j]>
                qp = engine.build_panel([q], _lib.SIDE_QUERY, 3)
                wp = engine.build_panel([lin.weight.detach().t().contiguous()], _lib.SIDE_GALLERY, 3)
                wq.append(engine.scores_dense(qp, wp))
            return wq, [img, tgt], [a, 1.0 - a], None
        raise NotImplementedError

    def _gate(self, q: torch.Tensor) -> torch.Tensor:
        """The gated heads' gate in eval mode, [N] fp32 on the GPU, through the library: Linear(d, 128) by the fp32x3 dense kernel,
        everything behind it (bias, ReLU, the 128 -> 1 dot or the d -> 1 dot of the simple heads, sigmoid) in kemr_gate_rows; the
        head's own ``gate()`` (torch) is what the tests compare it with."""
        h = self.fusion_head.to(q.device).eval()
        f32 = lambda t: t.detach().float().contiguous().to(q.device)
        if hasattr(h, "gate_net"):
            x, pre = self._linear(q, h.gate_net[0].weight), f32(h.gate_net[0].bias)
            w, bias, relu = f32(h.gate_net[3].weight).reshape(-1), float(h.gate_net[3].bias.detach()), 1
        else:
            x, pre, w, bias, relu = q.float().contiguous(), None, f32(h.query_weight), float(h.bias.detach().reshape(-1)[0]), 0
        return engine.gate_rows(x, pre, w, bias, relu)

    @staticmethod
    def _linear(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
        """x @ weight.T (+ bias) through the fp32x3 dense similarity kernel (x [R,K], weight [O,K])."""
        xp = engine.build_panel([x.float().contiguous()], _lib.SIDE_QUERY, 3)
        wp = engine.build_panel([weight.detach().float().contiguous()], _lib.SIDE_GALLERY, 3)
        y = engine.scores_dense(xp, wp)
        return y if bias is None else y + bias.detach().float()

    @torch.no_grad()
    def _cross_attention_query(self, q) -> torch.Tensor:
        """Query side of the cross_attention head: the attention queries Q [N, D], already scaled by hd^-0.5."""
        h = self.fusion_head.to(q.device).eval()
        lin = self._linear
        D = q.shape[1]
        hd = D // h.cross_attn.num_heads
        Wqkv, bqkv = h.cross_attn.in_proj_weight.detach(), h.cross_attn.in_proj_bias.detach()
        qp = lin(q, h.query_proj.weight, h.query_proj.bias)
        return lin(qp, Wqkv[:D], bqkv[:D]) * (hd ** -0.5)

    @torch.no_grad()
    def _cross_attention_gallery(self, img, tgt) -> dict:
        """Candidate side of the cross_attention head, everything that does not depend on the query: the keys Ki, Kt [M, D], the
        folded projections Pi, Pt [M, H, hid1] = W1.Wo[:, head].V_x and the MLP's constants (c0, w2t, b2, w3, b3)."""
        h = self.fusion_head.to(img.device).eval()
        lin = self._linear
        M, D = img.shape
        H = h.cross_attn.num_heads
        hd = D // H
        Wqkv, bqkv = h.cross_attn.in_proj_weight.detach(), h.cross_attn.in_proj_bias.detach()
        ip = lin(img, h.image_proj.weight, h.image_proj.bias)
        tp = lin(tgt, h.target_proj.weight, h.target_proj.bias)
        Ki, Kt = lin(ip, Wqkv[D:2 * D], bqkv[D:2 * D]), lin(tp, Wqkv[D:2 * D], bqkv[D:2 * D])
        Vi, Vt = lin(ip, Wqkv[2 * D:], bqkv[2 * D:]), lin(tp, Wqkv[2 * D:], bqkv[2 * D:])
        Wo, bo = h.cross_attn.out_proj.weight.detach().float(), h.cross_attn.out_proj.bias.detach().float()
        W1, b1 = h.score_mlp[0].weight.detach().float(), h.score_mlp[0].bias.detach().float()
        W2, b2 = h.score_mlp[3].weight.detach().float(), h.score_mlp[3].bias.detach().float()
        W3, b3 = h.score_mlp[6].weight.detach().float().reshape(-1), float(h.score_mlp[6].bias.detach())
        hid1, hid2 = W1.shape[0], W2.shape[0]
        Pi = torch.empty((M, H, hid1), dtype=torch.float32, device=img.device)
        Pt = torch.empty_like(Pi)
        for hh in range(H):
            sl = slice(hh * hd, (hh + 1) * hd)
            G = lin(W1, Wo[:, sl].t().contiguous())                     # [hid1, hd] = W1 . Wo[:, head]
            Pi[:, hh] = lin(Vi[:, sl].contiguous(), G)
            Pt[:, hh] = lin(Vt[:, sl].contiguous(), G)
        c0 = (lin(bo[None, :], W1)[0] + b1).contiguous()
        return {"Ki": Ki, "Kt": Kt, "Pi": Pi, "Pt": Pt, "c0": c0, "w2t": W2.t().contiguous(), "b2": b2.contiguous(),
                "w3": W3.contiguous(), "b3": b3, "H": H, "hid1": hid1, "hid2": hid2}

    @torch.no_grad()
    def _cross_attention(self, q, img, tgt) -> torch.Tensor:
        """Eval-mode CrossAttentionFusionHead.forward (reference fusion_model.py:83-133) -> [N, M] fp32."""
        lin = self._linear
        N, D = q.shape
        M = img.shape[0]
        Q = self._cross_attention_query(q)
        c = self._cross_attention_gallery(img, tgt)
        Ki, Kt, Pi, Pt, c0, w2t, b2, W3, b3 = (c[n] for n in ("Ki", "Kt", "Pi", "Pt", "c0", "w2t", "b2", "w3", "b3"))
        H = c["H"]
        hd = D // H
        out = torch.empty((N, M), dtype=torch.float32, device=q.device)
        step = max(1, min(N, (256 << 20) // max(1, 2 * H * M * 4)))   # bound the transposed score planes to ~256 MB
        for s0 in range(0, N, step):
            Qc = Q[s0:s0 + step]
            nc = Qc.shape[0]
            sti = torch.empty((H, M, nc), dtype=torch.float32, device=q.device)
            stt = torch.empty_like(sti)
            for hh in range(H):
                sl = slice(hh * hd, (hh + 1) * hd)
                qh = Qc[:, sl].contiguous()
                sti[hh] = lin(Ki[:, sl].contiguous(), qh)               # [M, nc]: candidates x queries (transposed)
                stt[hh] = lin(Kt[:, sl].contiguous(), qh)
            out_t = engine.cross_attention_pairs(sti, stt, Pi, Pt, c0, w2t, b2, W3, b3)
            out[s0:s0 + nc] = out_t.t()
        return out

    def _linear_head(self, t2i: torch.Tensor, t2t: torch.Tensor) -> torch.Tensor:
        """The linear head's MLP(2 -> hidden -> 1) on every (t2i, t2t) pair of two equally shaped fp32 tensors (kemr_linear_head)."""
        f = self.fusion_head.fusion.to(t2i.device)
        w0, b0 = f[0].weight.detach().float().contiguous(), f[0].bias.detach().float().contiguous()
        w1, b1 = f[3].weight.detach().float().reshape(-1).contiguous(), float(f[3].bias.detach())
        return engine.linear_head(t2i.contiguous(), t2t.contiguous(), w0, b0, w1, b1)

    @torch.no_grad()
    def forward(self, query_embed, image_embed, target_embed) -> torch.Tensor:
        """-> dense [N, M] fused scores (fp32, on the GPU)."""
        if self.fusion_type == "cross_attention":
            q = ranking.to_device_f32(query_embed)
            return self._cross_attention(q, ranking.to_device_f32(image_embed, q.device),
                                         ranking.to_device_f32(target_embed, q.device))
        if self.fusion_type == "linear":
            q = ranking.to_device_f32(query_embed)
            img, tgt = ranking.to_device_f32(image_embed, q.device), ranking.to_device_f32(target_embed, q.device)
            qp = engine.build_panel([q], _lib.SIDE_QUERY, 3)
            t2i = engine.scores_dense(qp, engine.build_panel([img], _lib.SIDE_GALLERY, 3))
            t2t = engine.scores_dense(qp, engine.build_panel([tgt], _lib.SIDE_GALLERY, 3))
            return self._linear_head(t2i, t2t)
        qs, gs, weights, gates = self._parts(query_embed, image_embed, target_embed)
        qp = engine.build_panel(qs, _lib.SIDE_QUERY, 3, part_scale=weights, row_scale=gates)
        gp = engine.build_panel(gs, _lib.SIDE_GALLERY, 3)
        return engine.scores_dense(qp, gp)

    @torch.no_grad()
    def rank(self, query_embed, image_embed, target_embed, k: int = 10, gt_idx="diag"
             ) -> Tuple[Optional[torch.Tensor], torch.Tensor, torch.Tensor]:
        """Ranks / top-k under this head without the [N, M] matrix (linear: dense matrix, then a streaming rank)."""
        if self.fusion_type in ("linear", "cross_attention"):
            return ranking.ranks_of_matrix(self.forward(query_embed, image_embed, target_embed), k=k, gt_idx=gt_idx)
        qs, gs, weights, gates = self._parts(query_embed, image_embed, target_embed)
        return ranking.ranks_and_topk(qs, gs, weights=weights, row_gate=gates, k=k, gt_idx=gt_idx)

    # ---- retrieve-then-rerank: the pair heads on deep shortlists instead of on the whole [N, M] grid
    def _require_rerank_head(self, what: str) -> None:
        if self.fusion_type not in _RERANK_HEADS:
            raise ValueError(f"{what}: the {self.fusion_type!r} head folds into the fused similarity pass and ranks the WHOLE gallery "
                             f"already -- use rank(); reranking a shortlist is for {_RERANK_HEADS}")

    @torch.no_grad()
    def prepare_gallery(self, image_embed, target_embed) -> HeadGallery:
        """The per-candidate side of ``rerank`` for one gallery (``HeadGallery``; stale after the head's parameters change)."""
        self._require_rerank_head("prepare_gallery")
        return HeadGallery(self, image_embed, target_embed)

    @torch.no_grad()
    def shortlist(self, q: torch.Tensor, gallery_panel: engine.Panel, depth: int, shortlist_weights=(0.5, 0.5), bonus=None) -> torch.Tensor:
        """Stage one: the ``depth`` best candidates of every query by w_i * T2I + w_t * T2T against a ``[image ; target]`` gallery
        panel -- the ids (int32 [N, depth], -1 padded) of ``ranking.ranks_and_topk_deep([q, q], [img, tgt], weights, k=depth)``.
        ``bonus`` (CSR, as ``engine.sim_topk_deep`` takes it) is added to that score before the cut, so a hit reaches the list
        wherever CLIP alone ranks it."""
        qp = engine.build_panel([q, q], _lib.SIDE_QUERY, gallery_panel.terms, part_scale=list(shortlist_weights))
        if bonus is None:
            return engine.sim_topk_deep(qp, gallery_panel, depth)[1]
        return engine.sim_topk_deep(qp, gallery_panel, depth, bonus=bonus)[1]

    @torch.no_grad()
    def list_scores(self, q: torch.Tensor, gallery: HeadGallery, list_idx: torch.Tensor) -> torch.Tensor:
        """Stage two: this head's score of every listed pair, fp32 [N, depth]; padded slots (id < 0) hold -inf."""
        n, depth = list_idx.shape
        if self.fusion_type == "cross_attention":
            c = gallery.cand
            return engine.cross_attention_rerank(self._cross_attention_query(q), c["Ki"], c["Kt"], c["Pi"], c["Pt"], c["c0"], c["w2t"],
                                                 c["b2"], c["w3"], c["b3"], list_idx, depth)
        # linear: t2i / t2t at the listed pairs with the bits of scores_dense (include/kemr.h, kemr_pair_scores), then the MLP
        qp = engine.build_panel([q], _lib.SIDE_QUERY, 3)
        q_rows = torch.arange(n, dtype=torch.int32, device=q.device).repeat_interleave(depth)
        g_rows = list_idx.clamp(min=0).reshape(-1)
        t2i = engine.pair_scores(qp, gallery.image_panel, q_rows, g_rows)
        t2t = engine.pair_scores(qp, gallery.target_panel, q_rows, g_rows)
        return self._linear_head(t2i, t2t).view(n, depth).masked_fill_(list_idx < 0, float("-inf"))

    @torch.no_grad()
    def _rerank_lists(self, q: torch.Tensor, gallery: HeadGallery, list_idx: torch.Tensor, k: int, gt: Optional[torch.Tensor]):
        n, depth = list_idx.shape
        scores = self.list_scores(q, gallery, list_idx)
        if gt is None:
            top_s, top_i = engine.select_topk(scores, k, idx=list_idx)
            return None, top_s, top_i, scores, list_idx
        # the whole list in the project's order (score descending, then lower id), by the selection kernel: the ground truth's
        # 1-based position in it is its rank under the two-stage pipeline, and the first k entries are the top-k
        hit = list_idx == gt.view(-1, 1)
        ranking._require_finite(scores[hit], "head scores at the ground truth")
        order_s, order_i = engine.select_topk(scores, depth, idx=list_idx)
        at = order_i == gt.view(-1, 1)
        pos = (at.int() * torch.arange(1, depth + 1, dtype=torch.int32, device=q.device)).sum(dim=1).long()
        ranks = torch.where(at.any(dim=1), pos, torch.full_like(pos, depth + 1))
        return ranks, order_s[:, :k].contiguous(), order_i[:, :k].contiguous(), scores, list_idx

    @torch.no_grad()
    def _rerank_lists_fused(self, q: torch.Tensor, gallery: HeadGallery, list_idx: torch.Tensor, k: int, gt: Optional[torch.Tensor],
                            bonus, head_weight: float):
        """``_rerank_lists`` with the knowledge side: ``head_weight * head + bonus`` on the listed pairs, the ground truth's place in
        the fused list and ``found`` in the same kernel (``engine.list_fuse``), the top-k by ``engine.select_topk``."""
        depth = list_idx.shape[1]
        scores = self.list_scores(q, gallery, list_idx)
        fused, ahead, found, gt_score = engine.list_fuse(scores, list_idx, depth, head_weight, bonus, gt, out=scores)
        top_s, top_i = engine.select_topk(fused, k, idx=list_idx)
        if gt is None:
            return None, top_s, top_i, fused, list_idx
        present = found != 0
        ranking._require_finite(gt_score[present], "fused scores at the ground truth")
        ranks = torch.where(present, ahead.long() + 1, torch.full_like(ahead, depth + 1, dtype=torch.int64))
        return ranks, top_s, top_i, fused, list_idx

    @staticmethod
    def _check_bonus(bonus, n: Optional[int], what: str):
        """A bonus CSR ``(rowptr [n + 1], col, val)`` as the kernels take it, checked on the host before anything is launched
        (``n`` None: the row count is not known yet)."""
        if not isinstance(bonus, (tuple, list)) or len(bonus) != 3:
            raise ValueError(f"{what}: bonus must be the CSR triple (rowptr, col, val)")
        if n is not None and len(bonus[0]) != n + 1:
            raise ValueError(f"{what}: the bonus row pointer must have {n + 1} entries (one row per query), got {len(bonus[0])}")
        if len(bonus[1]) != len(bonus[2]):
            raise ValueError(f"{what}: bonus col and val must have one entry per hit")
        return tuple(bonus)

    @torch.no_grad()
    def rerank(self, query_embed, gallery: HeadGallery, depth: int = 200, k: int = 10, gt_idx=None, cand_idx=None,
               shortlist_weights=(0.5, 0.5), bonus=None, head_weight: float = 1.0, shortlist_bonus: bool = True):
        """Retrieve-then-rerank with the ``linear`` or ``cross_attention`` head: cut a shortlist of ``depth`` candidates per query
        with the fused score ``w_i * T2I + w_t * T2T`` (``shortlist_weights``; one pass of ``engine.sim_topk_deep`` over the
        gallery's fused panel), score only those pairs with the head, sort them (score descending, then lower id).

        ``cand_idx`` (int32 [N, depth], -1 = padding, ids < M and distinct within a row) replaces the shortlist stage.
        ``gt_idx``: None, ``"diag"`` or one gallery id per query.

        Returns ``(ranks, top_scores [N, k], top_idx [N, k], list_scores [N, depth], list_idx [N, depth])``.  ``ranks`` is None
        without ``gt_idx``; otherwise int64 [N]: the ground truth's 1-based position in the reranked list, or ``depth + 1`` where
        the shortlist does not hold it -- a LOWER BOUND of the rank the head would give it over the whole gallery.  A rank
        <= depth is the exact rank of the two-stage pipeline, so Recall@K is exact for every K <= depth.  Linear scores are
        bit-identical to ``forward()[q, ids]``; cross_attention scores agree with it to fp32 rounding (``include/kemr.h``).

        ``bonus`` (CSR ``(rowptr [N + 1], col, val)``, gallery ids ascending within a row: ``sparql_fusion.sparql_bonus``,
        ``EmbeddingStore.hits_csr``) is the knowledge-fused rerank: the shortlist is cut by the fused score PLUS the bonus (unless
        ``shortlist_bonus=False``), so a hit reaches the list wherever CLIP ranks it; the listed pairs are scored by the head; the
        list is ranked by ``head_weight * head + bonus`` (``kemr_list_fuse``: one fp32 multiply, the bonus entries added in list
        order).  ``list_scores`` then holds the fused scores and ``ranks`` the ground truth's place in the fused list.  Without
        ``bonus`` the call is the plain rerank, and ``head_weight`` must be left at 1."""
        self._require_rerank_head("rerank")
        if bonus is None and float(head_weight) != 1.0:
            raise ValueError("rerank: head_weight scales the head against a bonus; without bonus it must stay 1.0")
        if bonus is not None:
            bonus = self._check_bonus(bonus, None, "rerank")
        depth, k = int(depth), int(k)
        if not 1 <= depth <= _lib.MAX_DEEP_K:
            raise ValueError(f"rerank: depth={depth} not in 1..{_lib.MAX_DEEP_K}")
        if not 1 <= k <= depth:
            raise ValueError(f"rerank: k={k} not in 1..depth={depth}")
        if not isinstance(gallery, HeadGallery) or gallery.model is not self or gallery.fusion_type != self.fusion_type:
            raise ValueError("rerank: gallery must come from this model's prepare_gallery()")
        q = ranking.to_device_f32(query_embed, gallery.device)
        n, m = q.shape[0], len(gallery)
        if bonus is not None:
            bonus = self._check_bonus(bonus, n, "rerank")
        if cand_idx is None:
            list_idx = self.shortlist(q, gallery.fused_panel, depth, shortlist_weights, bonus if shortlist_bonus else None)
        else:
            list_idx = torch.as_tensor(cand_idx)
            if list_idx.dtype != torch.int32 or tuple(list_idx.shape) != (n, depth):
                raise ValueError(f"rerank: cand_idx must be int32 [{n}, {depth}], got {list_idx.dtype} {tuple(list_idx.shape)}")
            ids = np.sort(list_idx.cpu().numpy(), axis=1)              # validation of an external list, on the host
            if ids.size and int(ids.max()) >= m:
                raise ValueError(f"rerank: cand_idx holds id {int(ids.max())}, the gallery has {m} candidates")
            if bool(((ids[:, 1:] == ids[:, :-1]) & (ids[:, 1:] >= 0)).any()):
                raise ValueError("rerank: the ids of a cand_idx row must be distinct")
            list_idx = list_idx.to(q.device).contiguous()
        gt = None
        if gt_idx is not None:
            gt = torch.arange(n, dtype=torch.int32, device=q.device) if isinstance(gt_idx, str) \
                else torch.as_tensor(gt_idx).to(device=q.device, dtype=torch.int32).reshape(-1)
            if gt.numel() != n or bool(((gt < 0) | (gt >= m)).any()):
                raise ValueError("rerank: gt_idx must hold one gallery id per query")
        if bonus is not None:
            return self._rerank_lists_fused(q, gallery, list_idx, k, gt, bonus, float(head_weight))
        return self._rerank_lists(q, gallery, list_idx, k, gt)
