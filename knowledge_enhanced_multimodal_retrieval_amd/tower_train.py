"""Differentiable CLIP towers and their trainers (``python -m src.clip.train.trainer --lock_image_tower`` | ``--end_to_end``).

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

Packed texts: ``TextTower(..., packed=True)`` (``--packed_texts``) computes every text up to its own end-of-text token and nothing behind
it: the live positions of the batch are gathered into ``[rows, width]``, text i owning the rows ``row_start[i] .. row_start[i + 1] - 1``,
and every linear, LayerNorm and activation of the blocks runs on those rows.  The attention is ``_OpAttentionPacked``
(``kemr_op_attention_packed`` forward, ``kemr_op_attention_backward_packed`` backward, csrc/attention_bwd.hip) or, with
attention="torch", ``torch_attention_packed``.  A 16-token query no longer runs at the length of the batch's longest target; there is
no running length, so ``t`` is refused.  The result is the dense tower's up to rounding (the same rows, another layout).

Elementwise passes: ``elementwise="torch"`` (the default of ``TextTower``) runs the blocks' LayerNorms and the MLP activation as torch
autograd does -- fp32 passes over ``[rows, 4 width]`` with an fp32 copy of each kept for the backward.  ``elementwise="op"`` routes
``ln_1`` / ``ln_2`` and the activation through the library in both directions (csrc/train_ops.hip): ``_OpLayerNorm`` is
``kemr_op_layernorm`` forward (it saves the fp32 rows it read, nothing else) and ``kemr_op_layernorm_backward`` backward; ``_OpAct`` is
``kemr_op_act_forward`` / ``kemr_op_act_backward`` on the bf16 output of ``mlp.c_fc`` (it saves that bf16 pre-activation).  GPU and
bf16 autocast only.

``VisionTower`` restates the vision tower over the model's own ``visual.*`` parameters: the ``conv1`` patch embedding (a bias-free
convolution whose stride is its kernel size: unfold + linear), class token, positional embedding, ``ln_pre``, the same pre-LN blocks
with NON-causal attention (``kemr_op_attention`` / ``kemr_op_attention_backward`` at ``causal = 0``), then the class-token row -- what
``kemr_encode_image_pooled`` returns -- and ``visual.ln_post``, ``visual.proj`` and the L2 normalisation through ``finetune.project``.
``head_dims`` names the head dims the tower may have: the default, ``(64,)``, refuses ViT-H-14's heads of 80 (like the SigLIP and BERT
families); ``head_dims=HEAD_DIMS`` (64 and 80) opts in.  At 80 ``_OpAttention`` scales q by 80 ** -0.5 in fp32 and rounds it to bf16
once (the 1/8 of heads of 64 is exact), the forward is ``kemr_op_attention_hd``, the backward the streaming
``kemr_op_attention_backward_hd`` (csrc/attention_bwd80.hip) and the returned dq is the op's times 80 ** -0.5 in fp32; such a tower has
at most 288 tokens, where the head-dim-80 forward ends, whatever ``max_tokens`` says.  ``max_tokens`` bounds the sequence: the default,
``MAX_T`` = 288, is the range of ``kemr_op_attention_backward`` and refuses the 577 tokens of ViT-L/14@336px; ``max_tokens=MAX_T_LONG``
(1025, the forward's range) opts in to the long towers, whose attention backward is the streaming ``kemr_op_attention_backward_long``
(csrc/attention_bwd_stream.hip; ``engine.attention_backward`` routes by length, so towers of up to 288 tokens keep their kernel and bits).
``EndToEndTuning`` passes ``MAX_T_LONG`` and ``HEAD_DIMS``.

``EndToEndTuning`` = ``ProjectionHeads`` + ``VisionTower`` + ``TextTower``: what ``--end_to_end`` trains, every parameter of the model
but ``logit_scale`` (the loss uses ``--temperature``, as the reference's does).  ``EndToEndTrainer`` is ``HeadTrainer``'s loop over
(preprocessed pixels in pinned host memory, query ids, target ids): a batch is indexed on the host and moved to the device by
``EndToEndTuning.forward``.

``TextTowerTrainer`` is ``finetune.HeadTrainer``'s loop -- batch schedule, accumulation, ``grad_clip``, validation through the served
engine after each epoch, early stopping, ``metrics_epoch.jsonl``, checkpoints through ``clip_model.save_checkpoint`` -- with another
feature function: the image tower stays locked (its pooled rows are cached once, ``finetune.cache_image_pooled``) and goes through
``ProjectionHeads.image``; queries and targets of the batch run through the differentiable tower.  What trains: the six head tensors
plus the whole text tower.  No other vision parameter can receive a gradient: none takes part in the graph.
"""
from __future__ import annotations

from typing import Callable, Dict, NamedTuple, Optional, Sequence, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from .clip_model import _unwrap
from .finetune import HeadTrainer, ProjectionHeads, project

MAX_T = 288          # KEMR_MAX_TEXT_CTX: the range of kemr_op_attention (causal) and of its backward
MAX_T_LONG = 1025    # KEMR_MAX_VISION_TOKENS: the range of kemr_op_attention (non-causal) and of kemr_op_attention_backward_long
HEAD_DIMS = (64, 80)  # the head dims the attention ops serve in both directions; 80: non-causal only (ViT-H-14's vision tower)
MAX_T_HD80 = 288     # the range of kemr_op_attention_hd at head dim 80 (its backward goes to MAX_T_LONG)


class _OpAttention(torch.autograd.Function):
    """qkv [batch * t, 3 width] (q not yet scaled) -> bf16 [batch * t, width] through the library's two attention kernels.  Heads of 64:
    the 1/8 of q is exact in bf16.  Heads of 80: q is scaled by 80 ** -0.5 in fp32 and rounded to bf16 once; the backward scales the
    op's dq by the same factor in fp32."""

    @staticmethod
    def forward(ctx, qkv: torch.Tensor, batch: int, t: int, width: int, causal: bool, head_dim: int = 64) -> torch.Tensor:
        from . import engine
        ctx.shape, ctx.in_dtype, ctx.causal, ctx.head_dim = (batch, t, width), qkv.dtype, bool(causal), int(head_dim)
        scaled = qkv.detach().to(torch.bfloat16).clone()
        if ctx.head_dim == 64:
            scaled[:, :width] *= 0.125                   # exact: a power of two
            ctx.save_for_backward(scaled)
            return engine.op_attention(scaled, batch, t, width, ctx.causal)
        scaled[:, :width] = (qkv.detach()[:, :width].float() * ctx.head_dim ** -0.5).to(torch.bfloat16)       # one rounding
        ctx.save_for_backward(scaled)
        return engine.op_attention(scaled, batch, t, width, ctx.causal, head_dim=ctx.head_dim)

    @staticmethod
    def backward(ctx, dout: torch.Tensor):
        from . import engine
        (scaled,) = ctx.saved_tensors
        batch, t, width = ctx.shape
        if ctx.head_dim == 64:
            dqkv = engine.attention_backward(scaled, dout.to(torch.bfloat16).contiguous(), batch, t, width, ctx.causal)
            dqkv[:, :width] *= 0.125                     # the caller's 1/8 of q (exact)
            return dqkv.to(ctx.in_dtype), None, None, None, None, None
        dqkv = engine.attention_backward(scaled, dout.to(torch.bfloat16).contiguous(), batch, t, width, ctx.causal, head_dim=ctx.head_dim)
        out = dqkv.to(ctx.in_dtype)
        out[:, :width] = (dqkv[:, :width].float() * ctx.head_dim ** -0.5).to(ctx.in_dtype)      # the caller's 1/sqrt(80) of q
        return out, None, None, None, None, None


class _OpAttentionPacked(torch.autograd.Function):
    """qkv [rows, 3 width] (q not yet scaled) over packed items -> bf16 [rows, width]: ``kemr_op_attention_packed`` forward,
    ``kemr_op_attention_backward_packed`` (causal) backward.  ``row_start`` int32 [batch + 1] on qkv's device covers rows 0 .. rows - 1;
    ``segments`` = ((first item, last item + 1, max_t), ...) splits the items into consecutive runs, one call each at the run's own
    longest item (``packed_segments``).  The ops read row_start[first .. last + 1] only and write the rows of those items only; an item's
    gradient has the same bits in any call whose max_t admits it."""

    @staticmethod
    def forward(ctx, qkv: torch.Tensor, row_start: torch.Tensor, segments: Tuple[Tuple[int, int, int], ...], width: int) -> torch.Tensor:
        from . import engine
        scaled = qkv.detach().to(torch.bfloat16).clone()
        scaled[:, :width] *= 0.125                       # exact: a power of two
        ctx.save_for_backward(scaled, row_start)
        ctx.segments, ctx.width, ctx.in_dtype = segments, width, qkv.dtype
        out = torch.empty((qkv.shape[0], width), dtype=torch.bfloat16, device=qkv.device)
        for lo, hi, max_t in segments:
            engine.op_attention_packed(scaled, row_start[lo:hi + 1], max_t, width, out=out)
        return out

    @staticmethod
    def backward(ctx, dout: torch.Tensor):
        from . import engine
        scaled, row_start = ctx.saved_tensors
        dout = dout.to(torch.bfloat16).contiguous()
        dqkv = torch.empty_like(scaled)
        for lo, hi, max_t in ctx.segments:
            engine.attention_backward_packed(scaled, dout, row_start[lo:hi + 1], max_t, ctx.width, True, out=dqkv)
        dqkv[:, :ctx.width] *= 0.125                     # the caller's 1/8 of q (exact)
        return dqkv.to(ctx.in_dtype), None, None, None


class _OpLayerNorm(torch.autograd.Function):
    """x fp32 [rows, width] -> LayerNorm(x) as bf16 (a GEMM operand) or fp32 (``ln_pre``, whose output is the stream) through
    ``kemr_op_layernorm``; the backward is ``kemr_op_layernorm_backward``, which recomputes mean and rstd from the saved x."""

    @staticmethod
    def forward(ctx, x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, out_bf16: bool) -> torch.Tensor:
        from . import engine
        x, gamma = x.detach().contiguous(), gamma.detach()
        ctx.save_for_backward(x, gamma)
        ctx.out_bf16 = bool(out_bf16)
        return engine.op_layernorm(x, gamma, beta.detach(), out_bf16=ctx.out_bf16)

    @staticmethod
    def backward(ctx, dy: torch.Tensor):
        from . import engine
        x, gamma = ctx.saved_tensors
        dx, dgamma, dbeta = engine.layernorm_backward(x, gamma, dy.to(torch.bfloat16 if ctx.out_bf16 else torch.float32).contiguous())
        return dx, dgamma, dbeta, None


class _OpAct(torch.autograd.Function):
    """bf16 pre-activation -> bf16 activation (``kemr_op_act_forward``); saves the pre-activation, the backward is ``kemr_op_act_backward``."""

    @staticmethod
    def forward(ctx, pre: torch.Tensor, kind: str) -> torch.Tensor:
        from . import engine
        pre = pre.detach().contiguous()
        ctx.save_for_backward(pre)
        ctx.kind = kind
        return engine.act_forward(pre, kind)

    @staticmethod
    def backward(ctx, dout: torch.Tensor):
        from . import engine
        (pre,) = ctx.saved_tensors
        return engine.act_backward(pre, dout.to(torch.bfloat16).contiguous(), ctx.kind), None


def torch_attention(qkv: torch.Tensor, batch: int, t: int, width: int, causal: bool = True, head_dim: int = 64) -> torch.Tensor:
    """The plain formulation: softmax(q k^T / sqrt(head_dim) [+ causal mask]) v per head of ``head_dim`` (64: / 8), in qkv's dtype."""
    heads = width // head_dim
    q, k, v = (x.reshape(batch, t, heads, head_dim).transpose(1, 2) for x in qkv.split(width, dim=-1))
    s = (q * (0.125 if head_dim == 64 else head_dim ** -0.5)) @ k.transpose(-1, -2)
    if causal:
        s = s + torch.full((t, t), float("-inf"), dtype=s.dtype, device=s.device).triu_(1)
    return (torch.softmax(s, dim=-1).to(v.dtype) @ v).transpose(1, 2).reshape(batch * t, width)


def torch_attention_packed(qkv: torch.Tensor, lens: Sequence[int], width: int, causal: bool = True) -> torch.Tensor:
    """The plain formulation over packed rows: item i = the next ``lens[i]`` rows of qkv [sum(lens), 3 width], each item attending to
    itself only (``torch_attention`` per item).  Any device and dtype, differentiable: the reference of the packed op and the way the
    packed tower runs without a GPU."""
    lens = [int(n) for n in lens]
    if qkv.dim() != 2 or qkv.shape[0] != sum(lens) or any(n < 0 for n in lens):
        raise ValueError(f"torch_attention_packed: qkv has {tuple(qkv.shape)} rows, the lengths sum to {sum(lens)}")
    outs = [torch_attention(x, 1, n, width, causal) for x, n in zip(qkv.split(lens), lens) if n]
    return torch.cat(outs) if outs else qkv.new_zeros((0, width))


def packed_segments(lens: Sequence[int]) -> Tuple[Tuple[int, int, int], ...]:
    """How ``_OpAttentionPacked`` issues its calls over items of these lengths (each >= 1): one call at the longest item, or two calls over
    items [0, k) and [k, n) at each run's own longest item.  The cost of a run is taken as items x LDS allocation of its call (the
    longest item rounded up to 32 rows): a short item in a long item's launch occupies a long item's share of a compute unit.  Two
    calls are issued where some k brings that cost to 3/4 of one call's or below (the second launch has to pay for itself) -- a batch of
    short queries followed by long targets splits between them, a batch of texts of one length does not split."""
    n = len(lens)
    up = [(int(x) + 31) // 32 * 32 for x in lens]
    whole = (0, n, max(int(x) for x in lens))
    pre, suf = [0] * (n + 1), [0] * (n + 1)
    for i in range(n):
        pre[i + 1] = max(pre[i], up[i])
        suf[n - 1 - i] = max(suf[n - i], up[n - 1 - i])
    cost, k = min((k * pre[k] + (n - k) * suf[k], k) for k in range(1, n)) if n > 1 else (0, 0)
    if n < 2 or 4 * cost > 3 * n * pre[n]:
        return (whole,)
    return ((0, k, max(int(x) for x in lens[:k])), (k, n, max(int(x) for x in lens[k:])))


def longest(ids: torch.Tensor) -> int:
    """The batch's longest text: the highest end-of-text position (first arg-max of the ids) + 1.  One host read for device ids."""
    return int(ids.argmax(dim=-1).max()) + 1


class _Packed(NamedTuple):
    """The layout of a batch of packed texts: host lengths, device row_start int32 [batch + 1], the calls of the attention op."""
    lens: Tuple[int, ...]
    row_start: torch.Tensor
    segments: Tuple[Tuple[int, int, int], ...]


OP_LN_WIDTHS = (256, 512, 768, 1024, 1280)          # kemr_op_layernorm and its backward


class _Tower(nn.Module):
    """What the two towers share: the settings and one pre-LN residual block on rows [batch * t, width]."""

    causal = True
    head_dim = 64        # the text towers' always; VisionTower sets its architecture's

    def _configure(self, who: str, attention: str, elementwise: str, autocast: Optional[bool], width: int, eps: Sequence[float]) -> None:
        if attention not in ("op", "torch"):
            raise ValueError(f"{who}: attention must be 'op' (the HIP kernels) or 'torch' (the plain formulation), got {attention!r}")
        if elementwise not in ("op", "torch"):
            raise ValueError(f"{who}: elementwise must be 'op' (the HIP kernels) or 'torch' (torch autograd), got {elementwise!r}")
        self.attention, self.elementwise = attention, elementwise
        self.autocast = (attention == "op" or elementwise == "op") if autocast is None else bool(autocast)
        if elementwise == "op":
            if not self.autocast:
                raise ValueError(f"{who}: elementwise='op' runs on the bf16 outputs of autocast linears; autocast=False is not served with it")
            if width not in OP_LN_WIDTHS:
                raise ValueError(f"{who}: elementwise='op' serves widths {OP_LN_WIDTHS}, not {width}")
            if any(e != 1e-5 for e in eps):
                raise ValueError(f"{who}: elementwise='op' serves LayerNorms with eps 1e-5 (kemr_op_layernorm's)")

    def _needs_gpu(self, who: str, dev: torch.device) -> None:
        if (self.attention == "op" or self.elementwise == "op") and dev.type != "cuda":
            raise RuntimeError(f"{who}: attention='op' / elementwise='op' must live on the GPU (got device {dev}); this path has no CPU "
                               "fallback (attention='torch' with elementwise='torch' is the reference formulation)")

    def _linear(self, x: torch.Tensor, lin_w: torch.Tensor, lin_b: Optional[torch.Tensor]) -> torch.Tensor:
        if self.autocast:
            with torch.autocast(x.device.type, dtype=torch.bfloat16):
                return F.linear(x, lin_w, lin_b)
        return F.linear(x, lin_w, lin_b)

    def _ln(self, x: torch.Tensor, ln: nn.LayerNorm, out_bf16: bool = True) -> torch.Tensor:
        if self.elementwise == "op":
            return _OpLayerNorm.apply(x, ln.weight, ln.bias, out_bf16)
        return F.layer_norm(x, (x.shape[-1],), ln.weight, ln.bias, ln.eps)

    def _act(self, h: torch.Tensor) -> torch.Tensor:
        if self.elementwise == "op":
            return _OpAct.apply(h, self.activation)
        h = h.float() if h.dtype == torch.bfloat16 else h
        return F.gelu(h) if self.activation == "gelu" else h * torch.sigmoid(1.702 * h)

    def _attend(self, qkv: torch.Tensor, batch: int, t: int) -> torch.Tensor:
        """qkv [batch * t, 3 width] (q not yet scaled) -> [batch * t, width].  (tools/bench_text_tower_train.py overrides this.)"""
        if self.attention == "op":
            return _OpAttention.apply(qkv, batch, t, self.width, self.causal, self.head_dim)
        return torch_attention(qkv, batch, t, self.width, self.causal, self.head_dim)

    def _attend_packed(self, qkv: torch.Tensor, packed: "_Packed") -> torch.Tensor:
        """qkv [rows, 3 width] (q not yet scaled) over packed items -> [rows, width].  (tools/bench_text_tower_packed.py overrides this.)"""
        if self.attention == "op":
            return _OpAttentionPacked.apply(qkv, packed.row_start, packed.segments, self.width)
        return torch_attention_packed(qkv, packed.lens, self.width, self.causal)

    def _block(self, x: torch.Tensor, blk: nn.Module, attend: Callable[[torch.Tensor], torch.Tensor]) -> torch.Tensor:
        """One pre-LN residual block on rows [rows, width]; ``attend``: qkv [rows, 3 width] -> [rows, width], the layout's attention."""
        qkv = self._linear(self._ln(x, blk.ln_1), blk.attn.in_proj_weight, blk.attn.in_proj_bias)
        a = attend(qkv)
        x = x + self._linear(a, blk.attn.out_proj.weight, blk.attn.out_proj.bias)
        h = self._act(self._linear(self._ln(x, blk.ln_2), blk.mlp.c_fc.weight, blk.mlp.c_fc.bias))
        return x + self._linear(h, blk.mlp.c_proj.weight, blk.mlp.c_proj.bias)


class TextTower(_Tower):
    """See the module docstring.  ``trainable=True`` sets ``requires_grad`` on the text tower's parameters (and leaves every other
    parameter of the model as it finds it)."""

    def __init__(self, model: nn.Module, attention: str = "op", autocast: Optional[bool] = None, trainable: bool = True,
                 elementwise: str = "torch", packed: bool = False):
        super().__init__()
        self.packed = bool(packed)
        m = _unwrap(model)
        family = getattr(getattr(m, "arch", None), "family", "clip")
        if family != "clip" or not hasattr(m, "text_projection") or not hasattr(m, "visual") or not hasattr(m.visual, "proj"):
            raise ValueError(f"TextTower: only the CLIP family's text tower is restated (this model's family: {family!r}; SigLIP pools the "
                             "last position of a bidirectional tower, BERT models are post-LN sentence encoders)")
        if m.arch.t_width % 64 or m.arch.t_heads * 64 != m.arch.t_width:
            raise ValueError(f"TextTower: heads of 64 only (width {m.arch.t_width}, {m.arch.t_heads} heads)")
        self._configure("TextTower", attention, elementwise, autocast, m.arch.t_width,
                        [e for b in m.transformer.resblocks for e in (b.ln_1.eps, b.ln_2.eps)])
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

    def pooled(self, ids: torch.Tensor, t: Optional[int] = None) -> torch.Tensor:
        """ids int [B, ctx] -> [B, width]: the residual-stream row at each text's end-of-text token, before ``ln_final``."""
        if ids.dim() != 2 or ids.shape[1] > self.ctx:
            raise ValueError(f"TextTower: ids must be [B, <= {self.ctx}], got {tuple(ids.shape)}")
        dev = self.positional_embedding.device
        self._needs_gpu("TextTower", dev)
        if self.packed:
            if t is not None:
                raise ValueError(f"TextTower: packed=True computes every text up to its own end-of-text token and has no running "
                                 f"length; t = {t} is not served with it")
            return self._pooled_packed(ids, dev)
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
            x = self._block(x, blk, lambda qkv: self._attend(qkv, batch, t))
        return x.reshape(batch, t, self.width)[torch.arange(batch, device=dev), eot]

    def _pooled_packed(self, ids: torch.Tensor, dev: torch.device) -> torch.Tensor:
        """``pooled`` over packed rows: text i owns the rows row_start[i] .. row_start[i + 1] - 1 = its positions 0 .. end-of-text, and
        nothing is computed behind an end-of-text token.  The lengths are read where the ids are (one host read for device ids)."""
        lens = tuple((ids.argmax(dim=-1) + 1).tolist())
        batch, rows = len(lens), sum(lens)
        if batch == 0 or max(lens, default=0) > MAX_T:
            raise ValueError(f"TextTower: packed texts must be [B >= 1, <= {MAX_T} positions up to the end-of-text token], got "
                             f"{tuple(ids.shape)} with a longest text of {max(lens, default=0)}")
        ids = ids.to(dev, non_blocking=True).long()
        lens_dev = torch.tensor(lens, dtype=torch.long, device=dev)
        ends = lens_dev.cumsum(0)
        row_start = torch.cat([ends.new_zeros(1), ends]).to(torch.int32)
        item = torch.repeat_interleave(torch.arange(batch, device=dev), lens_dev, output_size=rows)
        pos = torch.arange(rows, device=dev) - (ends - lens_dev)[item]
        # F.embedding, not indexing: every position occurs once per text that reaches it, and the backward of an index sums a row's
        # duplicates one after the other, where embedding's splits them into partial sums
        x = F.embedding(ids[item, pos], self.token_embedding.weight) + F.embedding(pos, self.positional_embedding)
        packed = _Packed(lens, row_start, packed_segments(lens) if self.attention == "op" else ())
        for blk in self.transformer.resblocks:
            x = self._block(x, blk, lambda qkv: self._attend_packed(qkv, packed))
        return x[ends - 1]

    def forward(self, ids: torch.Tensor, t: Optional[int] = None) -> torch.Tensor:
        """[B, embed_dim]: the L2-normalised text embeddings."""
        return project(self.pooled(ids, t), self.ln_final.weight, self.ln_final.bias, self.text_projection, self.ln_final.eps)


class VisionTower(_Tower):
    """See the module docstring.  ``trainable=True`` sets ``requires_grad`` on the vision tower's parameters (and leaves every other
    parameter of the model as it finds it)."""

    causal = False

    def __init__(self, model: nn.Module, attention: str = "op", elementwise: str = "op", autocast: Optional[bool] = None,
                 trainable: bool = True, max_tokens: int = MAX_T, head_dims: Sequence[int] = (64,)):
        super().__init__()
        if not 1 <= int(max_tokens) <= MAX_T_LONG:
            raise ValueError(f"VisionTower: max_tokens = {max_tokens} is outside 1..{MAX_T_LONG} (MAX_T = {MAX_T}: the default; "
                             f"MAX_T_LONG = {MAX_T_LONG}: the long towers)")
        max_tokens = int(max_tokens)
        head_dims = tuple(int(d) for d in head_dims)
        if not head_dims or any(d not in HEAD_DIMS for d in head_dims):
            raise ValueError(f"VisionTower: head_dims = {head_dims} must be taken from HEAD_DIMS = {HEAD_DIMS} ((64,): the default; "
                             f"HEAD_DIMS: ViT-H-14's heads of 80 as well)")
        m = _unwrap(model)
        arch = getattr(m, "arch", None)
        family = getattr(arch, "family", "clip")
        if family != "clip" or not hasattr(m, "visual") or not hasattr(m.visual, "proj") or not hasattr(m.visual, "class_embedding"):
            raise ValueError(f"VisionTower: only the CLIP family's vision tower is restated (this model's family: {family!r}; SigLIP has no "
                             "class token and pools by attention, BERT models have no vision tower)")
        if arch.v_head_dim not in head_dims:
            if head_dims == (64,):
                raise ValueError(f"VisionTower: heads of 64 only (this tower: width {arch.v_width} in heads of {arch.v_head_dim}; the "
                                 "attention backward serves no other head dim)")
            raise ValueError(f"VisionTower: heads of {head_dims} only (this tower: width {arch.v_width} in heads of {arch.v_head_dim})")
        if arch.v_tokens > max_tokens:
            raise ValueError(f"VisionTower: {arch.v_tokens} tokens per image; the attention backward serves at most {max_tokens}")
        if arch.v_head_dim == 80 and arch.v_tokens > MAX_T_HD80:
            raise ValueError(f"VisionTower: {arch.v_tokens} tokens per image in heads of 80; the head-dim-80 attention forward serves at "
                             f"most {MAX_T_HD80}, whatever max_tokens says")
        self.head_dim = arch.v_head_dim
        v = m.visual
        self._configure("VisionTower", attention, elementwise, autocast, arch.v_width,
                        [v.ln_pre.eps] + [e for b in v.transformer.resblocks for e in (b.ln_1.eps, b.ln_2.eps)])
        self.activation, self.width, self.tokens, self.patch, self.image_size = m.activation, arch.v_width, arch.v_tokens, arch.patch, arch.image_size
        self.conv1, self.class_embedding, self.positional_embedding = v.conv1, v.class_embedding, v.positional_embedding
        self.ln_pre, self.transformer, self.ln_post, self.proj = v.ln_pre, v.transformer, v.ln_post, v.proj
        if trainable:
            for p in self.parameters():
                p.requires_grad = True

    def named_vision_parameters(self) -> Dict[str, nn.Parameter]:
        """Every parameter of the vision side under its name in the model's state dict."""
        out = {"visual.conv1.weight": self.conv1.weight, "visual.class_embedding": self.class_embedding,
               "visual.positional_embedding": self.positional_embedding, "visual.ln_pre.weight": self.ln_pre.weight,
               "visual.ln_pre.bias": self.ln_pre.bias}
        out.update({f"visual.transformer.{k}": p for k, p in self.transformer.named_parameters()})
        out.update({"visual.ln_post.weight": self.ln_post.weight, "visual.ln_post.bias": self.ln_post.bias, "visual.proj": self.proj})
        return out

    def pooled(self, pixels: torch.Tensor) -> torch.Tensor:
        """pixels [B, 3, S, S] (preprocessed) -> [B, width]: the class-token row of the residual stream, before ``ln_post``."""
        s, p, w, t = self.image_size, self.patch, self.width, self.tokens
        if pixels.dim() != 4 or tuple(pixels.shape[1:]) != (3, s, s):
            raise ValueError(f"VisionTower: pixels must be [B, 3, {s}, {s}], got {tuple(pixels.shape)}")
        dev = self.positional_embedding.device
        self._needs_gpu("VisionTower", dev)
        pixels = pixels.to(device=dev, dtype=self.positional_embedding.dtype)
        batch, g = pixels.shape[0], s // p
        # conv1 has no bias and its stride is its kernel size: every patch is one row of a linear layer
        patches = pixels.reshape(batch, 3, g, p, g, p).permute(0, 2, 4, 1, 3, 5).reshape(batch * g * g, 3 * p * p)
        emb = self._linear(patches, self.conv1.weight.reshape(w, 3 * p * p), None).to(pixels.dtype).reshape(batch, g * g, w)
        x = torch.cat([self.class_embedding.expand(batch, 1, w), emb], dim=1) + self.positional_embedding
        x = self._ln(x.reshape(batch * t, w), self.ln_pre, out_bf16=False)
        for blk in self.transformer.resblocks:
            x = self._block(x, blk, lambda qkv: self._attend(qkv, batch, t))
        return x.reshape(batch, t, w)[:, 0]

    def forward(self, pixels: torch.Tensor) -> torch.Tensor:
        """[B, embed_dim]: the L2-normalised image embeddings."""
        return project(self.pooled(pixels), self.ln_post.weight, self.ln_post.bias, self.proj, self.ln_post.eps)


class LockedImageTuning(nn.Module):
    """What ``--lock_image_tower`` trains: ``ProjectionHeads`` (six tensors) plus the whole text tower, over the model's own parameters."""

    def __init__(self, model: nn.Module, attention: str = "op", autocast: Optional[bool] = None, packed: bool = False):
        super().__init__()
        self.heads = ProjectionHeads(model)              # freezes everything, then its six tensors
        self.tower = TextTower(model, attention=attention, autocast=autocast, trainable=True, packed=packed)

    def forward(self, pooled_image: torch.Tensor, query_ids: torch.Tensor, target_ids: torch.Tensor
                ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        n = query_ids.shape[0]
        ids = torch.cat([query_ids, target_ids])
        text = self.tower(ids) if self.tower.packed else self.tower(ids, longest(ids))
        return self.heads.image(pooled_image), text[:n], text[n:]


class EndToEndTuning(nn.Module):
    """What ``--end_to_end`` trains: ``ProjectionHeads`` plus both towers, over the model's own parameters -- every parameter but
    ``logit_scale``, which takes no part in the graph (the loss has its own temperature) and keeps its bits."""

    def __init__(self, model: nn.Module, attention: str = "op", elementwise: str = "op", autocast: Optional[bool] = None,
                 packed: bool = False):
        super().__init__()
        self.heads = ProjectionHeads(model)              # freezes everything, then its six tensors
        self.vision = VisionTower(model, attention=attention, elementwise=elementwise, autocast=autocast, trainable=True,
                                  max_tokens=MAX_T_LONG, head_dims=HEAD_DIMS)
        self.tower = TextTower(model, attention=attention, autocast=autocast, trainable=True, elementwise=elementwise, packed=packed)

    def forward(self, pixels: torch.Tensor, query_ids: torch.Tensor, target_ids: torch.Tensor
                ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """A host (or device) batch -> (image, query, target) embeddings on the model's device."""
        dev = self.tower.positional_embedding.device
        n = query_ids.shape[0]
        ids = torch.cat([query_ids, target_ids])
        if self.tower.packed:
            text = self.tower(ids)                       # the lengths are read where the ids are: no device sync for host ids
        else:
            t = longest(ids)                             # read where the ids are: no device sync for host ids
            text = self.tower(ids.to(dev, non_blocking=True), t)
        return self.heads.image(self.vision.pooled(pixels.to(dev, non_blocking=True))), text[:n], text[n:]


class TextTowerTrainer(HeadTrainer):
    """``HeadTrainer``'s loop with ``rows`` = (cached pooled image rows fp32 [N, v_width], query ids, target ids int [N, ctx], all on the
    model's device) and ``heads`` a ``LockedImageTuning``.  A batch's activations live on the device for its backward pass, so a batch
    must be given: ``batch_size=0`` (the whole split) is refused."""

    def __init__(self, model: nn.Module, heads: LockedImageTuning, rows: Sequence[torch.Tensor], loss_fn, optimizer, scheduler=None,
                 batch_size: int = 64, **kw):
        if batch_size <= 0:
            raise ValueError(BATCH_0_REFUSED)
        super().__init__(model, heads, rows, loss_fn, optimizer, scheduler, batch_size=batch_size, **kw)


class EndToEndTrainer(HeadTrainer):
    """``HeadTrainer``'s loop with ``rows`` = (preprocessed pixels fp32 [N, 3, S, S] in pinned host memory, query ids, target ids int
    [N, ctx] on the host; ``finetune.cache_pixels``) and ``heads`` an ``EndToEndTuning``: the loop indexes a batch where the rows are
    and ``EndToEndTuning.forward`` moves it to the device.  A batch must be given: ``batch_size=0`` is refused."""

    def __init__(self, model: nn.Module, heads: EndToEndTuning, rows: Sequence[torch.Tensor], loss_fn, optimizer, scheduler=None,
                 batch_size: int = 64, **kw):
        if batch_size <= 0:
            raise ValueError(BATCH_0_REFUSED_END_TO_END)
        super().__init__(model, heads, rows, loss_fn, optimizer, scheduler, batch_size=batch_size, **kw)


BATCH_0_REFUSED_END_TO_END = ("--batch_size 0 (the whole split as one batch) is not served with --end_to_end: the towers' backward passes "
                              "keep the activations of a whole batch on the device, and the activations of a whole split do not fit; give a "
                              "batch size")
BATCH_0_REFUSED = ("--batch_size 0 (the whole split as one batch) is not served with --lock_image_tower: the text tower's backward pass "
                   "keeps the activations of a whole batch on the device, and the activations of a whole split do not fit; give a batch size")
