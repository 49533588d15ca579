"""Host-side driver of libkemr.so: model handle, encoders and the fused similarity / top-k / rank ops.

PyTorch is plumbing here (device memory, streams): every tensor that crosses into the library is passed as
``tensor.data_ptr()`` and all arithmetic of the hot path runs in the HIP kernels behind the C ABI.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os
from typing import Dict, Mapping, Optional, Sequence, Tuple

import torch

from . import _lib
from .config import ClipArch

# rows per encoder launch: picked so that batch * tokens fills whole 128/256-row GEMM tiles and the
# workspace (14 * width bytes per token) stays small; larger user batches are processed in slices.
MAX_IMAGE_BATCH = 255
MAX_TEXT_BATCH = 851
TEXT_ROW_BUDGET = 65536        # token rows per packed text call: 256 row tiles of 256


def text_lengths(ids: torch.Tensor) -> torch.Tensor:
    """Positions of every text that can reach its embedding: up to and including the pooled one, ``ids.argmax(-1) + 1`` (the
    end-of-text token has the largest id; reference pooling ``x[arange, text.argmax(dim=-1)]``).  int32 [B], on ids' device."""
    return (ids.argmax(dim=-1) + 1).to(torch.int32)


def tile_friendly_batch(tokens: int, width: int, lo: int, hi: int, num_cu: int = 256) -> int:
    """Items per encoder call, in [lo, hi], that fill the persistent GEMM's rounds best: the towers' four GEMMs have
    ceil(items * tokens / 256) x (3W | W | 4W | W) / 256 output tiles each and run ceil(tiles / CUs) rounds over the CUs, so a
    call is as fast as its emptiest round allows (255 texts of ViT-L/14: 231 out-proj tiles on 256 CUs, 90 %; 564 texts: 510
    tiles in two rounds, 99.6 %).  Weighted by the GEMMs' FLOPs; among near-equal sizes the largest (fewer launches per item:
    measured 64.6 k texts/s at 255, 66.6 k at 282, 71.4 k at 564; whole step 16 340 / 16 590 / 16 710 items/s at 255 / 565 / 848)."""
    effs = {}
    for items in range(lo, hi + 1):
        row_tiles = -(-items * tokens // 256)
        num = den = 0.0
        for n_mult, weight in ((3, 3.0), (1, 1.0), (4, 4.0), (1, 4.0)):      # QKV, out-proj, fc1, fc2 (K = 4W)
            tiles = row_tiles * (n_mult * width // 256)
            num += weight * (items * tokens / 256.0) * (n_mult * width / 256.0)      # useful tile-equivalents
            den += weight * -(-tiles // num_cu) * num_cu                             # tile slots of the rounds it takes
        effs[items] = num / den
    top = max(effs.values())
    return max(i for i, e in effs.items() if e >= top - 2e-3)


def image_call_items(arch: ClipArch) -> int:
    """Images per vision-encoder call.  Towers of at most 288 tokens: MAX_IMAGE_BATCH (255 images of ViT-L/14 = 256 row tiles).
    Longer towers (ViT-L/14@336px: 577 tokens) keep about the same token rows per call, 255 * 257 = 65 535, and take the item
    count in [half, all] of that which fills the persistent GEMM's rounds best (tile_friendly_batch: 85 images at 577 x 1024)."""
    t = arch.v_tokens
    if t <= 288:
        return MAX_IMAGE_BATCH
    hi = max(1, MAX_IMAGE_BATCH * 257 // t)
    return tile_friendly_batch(t, arch.v_width, max(1, hi // 2), hi)


def _stream_ptr(device: torch.device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


class CallOrder:
    """Orders the calls of ONE object that keeps a workspace across calls (ClipEngine, BertEngine, the GPU preprocessors).  The library
    orders a call on the stream it is given and nowhere else (include/kemr.h "Stream contract"), so two calls of one object made under
    two ``torch.cuda.stream(...)`` contexts would share the scratch buffer with nothing between them.  ``begin`` makes the current
    stream wait for the object's previous call when that call was queued on another stream (one event wait on the device, only then);
    ``end`` records the event the next call may have to wait for.  ``retire`` keeps a workspace that a larger one replaced referenced
    until the call that replaced it has finished: freed earlier, the caching allocator could hand the block out while a call queued on
    another stream than the block's own is still pending.  Nothing here synchronises the host.  A call made while its stream is being
    captured into a graph takes no part (an event recorded inside a capture cannot be waited for outside it; capture is not part of
    the stream contract)."""

    def __init__(self):
        self._event: Optional[torch.cuda.Event] = None
        self._stream = None
        self._capturing = False
        self._old: list = []             # workspaces replaced during the current call
        self._retired: list = []         # (event recorded behind the call that replaced them, those workspaces)

    def begin(self, device: torch.device):
        cur = torch.cuda.current_stream(device)
        self._capturing = torch.cuda.is_current_stream_capturing()
        if self._capturing:
            return cur
        if self._event is not None and cur != self._stream:
            cur.wait_event(self._event)
        if self._retired:
            self._retired = [r for r in self._retired if not r[0].query()]
        return cur

    def retire(self, ws: Optional[torch.Tensor]) -> None:
        if ws is not None:
            self._old.append(ws)

    def end(self, cur) -> None:
        if self._capturing:
            return
        if self._event is None:
            self._event = torch.cuda.Event()
        self._event.record(cur)
        self._stream = cur
        if self._old:
            done = torch.cuda.Event()
            done.record(cur)
            self._retired.append((done, self._old))
            self._old = []

    @contextlib.contextmanager
    def call(self, device: torch.device):
        """``with order.call(device) as stream:`` -- begin, the launches, end.  ``end`` runs as well when a launch raises in the
        middle of a call: what is queued by then is ordered for the next call, and workspaces retired by then wait for it."""
        cur = self.begin(device)
        try:
            yield cur
        finally:
            self.end(cur)


def _require_cuda(t: torch.Tensor, what: str) -> None:
    if not t.is_cuda:
        raise RuntimeError(f"{what} must live on the GPU (got device {t.device}); this path has no CPU fallback")


class ClipEngine:
    """One packed CLIP model (both towers) in HBM."""

    def __init__(self, arch: ClipArch, device: torch.device | str = "cuda:0", precision: str = _lib.DEFAULT_PRECISION,
                 activation: str = "quick_gelu"):
        """precision: "bf16-x24" (default: bf16 operands, fp32 accumulation, the fp32 residual stream stored as 24-bit floats -- model
        option residual_stream_24bit), "bf16" (the stream as 4-byte fp32), "bf16-res16" (bf16 residual stream, opt-in), "fp8" / "fp8-x24"
        (the vision tower's QKV GEMMs on fp8 operands, BASELINE config 5), "fp8-res16" or "fp8-mlp" (fc1 too).  See kemr_precision in
        include/kemr.h and _lib.DEFAULT_PRECISION.  "fp32x3": every GEMM / attention operand as a bf16 pair (hi, lo) with three products
        each, fp32 between the kernels -- the reference's fp32 numbers for practical purposes at a quarter to a third of the default's
        rate; what `precision_gap` measures the faster precisions against.
        activation: "quick_gelu" (the OpenAI checkpoints) or "gelu" (exact GELU: OpenCLIP / LAION and Hugging Face `hidden_act: gelu`
        checkpoints) -- model option "activation"."""
        _lib.check_activation(activation)
        if precision not in _lib.PRECISIONS:
            raise ValueError(f"precision must be one of {sorted(_lib.PRECISIONS)}, got {precision!r}")
        self.precision = precision
        self.arch = arch
        self.image_batch = image_call_items(arch)        # images per kemr_encode_image call
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("ClipEngine needs a GPU device; the HIP path has no CPU fallback")
        self._L = _lib.lib()
        cfg = _lib.KemrCfg(**arch.cfg_dict())
        h = C.c_void_p()
        _lib.check(self._L.kemr_model_create(C.byref(cfg), C.byref(h)), "model_create")
        self._h = h
        if arch.v_head_dim != 64:                        # before finalize: it decides the scale folded into the vision tower's query rows
            _lib.check(self._L.kemr_model_set_option(self._h, b"vision_head_dim", arch.v_head_dim), "model_set_option")
        self.family = arch.family
        if arch.family != "clip":                        # right after create: it decides the tensor names (refused after the first load_tensor)
            from .config import FAMILIES
            _lib.check(self._L.kemr_model_set_option(self._h, b"family", FAMILIES[arch.family]), "model_set_option")
        self.activation = "quick_gelu"                   # the library's default; the option is only touched when something else is asked for
        if activation != self.activation:                # (family "siglip": its tanh GELU is the family's, the option is not consulted)
            self.set_activation(activation)
        self._ws: Dict[object, torch.Tensor] = {}
        self._order = CallOrder()                        # the workspaces are reused: calls made under different streams are ordered
        self._state: Optional[Mapping[str, torch.Tensor]] = None
        self.ready = False
        self.pack_text = os.environ.get("KEMR_TEXT_PACKED", "1") != "0"     # encode_text: only the positions up to the end-of-text token
        if arch.family == "siglip":                      # unmasked text tower pooled at the last position: every position counts
            self.pack_text = False

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            try:
                self._L.kemr_model_destroy(h)
            except Exception:
                pass

    def set_activation(self, activation: str) -> None:
        """Option "activation" of THIS model: "quick_gelu" or "gelu", the epilogue of the fc1 GEMMs from the next encode call on (the
        packed weights do not depend on it)."""
        code = _lib.ACTIVATIONS[_lib.check_activation(activation)]
        _lib.check(self._L.kemr_model_set_option(self._h, b"activation", code), "model_set_option")
        self.activation = activation

    def set_residual_fusion(self, level) -> None:
        """Option "residual_fusion" of THIS model (include/kemr.h kemr_model_set_option): 0 / False = the out-proj / fc2 GEMMs store
        bf16 updates that the LayerNorms apply; 1 / True = bf16 residual streams add them in the GEMM epilogues (default); 2 = fp32
        residual streams too (nothing is rounded; slower)."""
        _lib.check(self._L.kemr_model_set_option(self._h, b"residual_fusion", int(level)), "model_set_option")

    def set_last_block_pooled_row(self, on: bool) -> None:
        """Option "last_block_pooled_row" of THIS model (default on): the last block of a tower computes its query path -- attention
        output, out-proj, ln_2, MLP -- for the one row per item that leaves the tower (class / end-of-text token) instead of for all
        of them; off = every row, as the reference does.  Store-only epilogues only (not the bf16-stream modes' fused residual add), and
        not with fc1 on fp8 ("fp8-mlp")."""
        _lib.check(self._L.kemr_model_set_option(self._h, b"last_block_pooled_row", 1 if on else 0), "model_set_option")

    def last_block_pooled_row(self) -> bool:
        v = C.c_int(0)
        _lib.check(self._L.kemr_model_get_option(self._h, b"last_block_pooled_row", C.byref(v)), "model_get_option")
        return bool(v.value)

    def residual_fusion(self) -> int:
        """The option's value (0 / 1 / 2)."""
        v = C.c_int(0)
        _lib.check(self._L.kemr_model_get_option(self._h, b"residual_fusion", C.byref(v)), "model_get_option")
        return v.value

    def residual_fusion_active(self) -> bool:
        """Whether large calls of THIS engine add the residual inside the GEMM epilogues (option and stream type together)."""
        if self.precision.endswith("-x24") or self.precision == "fp32x3":
            return False                                   # 24-bit stream rows: store-only epilogues, whatever the option says; fp32x3: the option has no meaning
        return self.residual_fusion() >= (1 if self.precision.endswith("res16") else 2)

    # ------------------------------------------------------------------ weights
    def tensor_names(self) -> Sequence[str]:
        n = self._L.kemr_model_num_tensors(self._h)
        return [self._L.kemr_model_tensor_name(self._h, i).decode() for i in range(n)]

    def load_state_dict(self, sd: Mapping[str, torch.Tensor]) -> None:
        """Strict load of an OpenAI-CLIP style state dict (any float dtype, any device) + pack to HBM."""
        self._state = dict(sd)          # references, not copies: what `precision_gap` packs a second engine from
        for name, t in sd.items():
            if not torch.is_tensor(t):
                continue
            host = t.detach().to(device="cpu", dtype=torch.float32).contiguous()
            shape = (C.c_int64 * max(host.dim(), 1))(*host.shape)
            _lib.check(self._L.kemr_model_load_tensor(self._h, name.encode(), C.c_void_p(host.data_ptr()), _lib.KEMR_F32,
                                                      shape, host.dim()), f"load_tensor({name})")
        # "-x24" names the 24-bit stream (the product's default), "bf16" / "fp8" / "fp8-mlp" the 4-byte one; idle for the bf16 streams
        _lib.check(self._L.kemr_model_set_option(self._h, b"residual_stream_24bit", 1 if self.precision.endswith("-x24") else 0), "model_set_option")
        with torch.cuda.device(self.device):
            _lib.check(self._L.kemr_model_finalize(self._h, _lib.PRECISIONS[self.precision]), "model_finalize")
        self.ready = True

    # ------------------------------------------------------------------ encoders
    def _workspace(self, tower: int, batch: int) -> torch.Tensor:
        need = int(self._L.kemr_workspace_bytes(self._h, tower, batch))
        ws = self._ws.get(tower)
        if ws is None or ws.numel() < need:
            self._order.retire(ws)
            ws = torch.empty(need, dtype=torch.uint8, device=self.device)
            self._ws[tower] = ws
        return ws

    def _encode(self, fn, tower: int, x: torch.Tensor, max_batch: int, normalize: bool, pooled_width: Optional[int] = None) -> torch.Tensor:
        """pooled_width: `fn` is the kemr_encode_*_pooled form (no `normalize` argument, rows of the tower's width)."""
        if not self.ready:
            raise RuntimeError("ClipEngine: load_state_dict() must be called before encoding")
        n = x.shape[0]
        out = torch.empty((n, pooled_width or self.arch.embed_dim), dtype=torch.float32, device=self.device)
        if n == 0:
            return out
        with torch.cuda.device(self.device), self._order.call(self.device) as cur:
            stream = cur.cuda_stream
            ws = self._workspace(tower, min(n, max_batch))
            for s in range(0, n, max_batch):
                xb = x[s:s + max_batch]
                tail = (C.c_void_p(ws.data_ptr()), ws.numel(), C.c_void_p(stream))
                head = (self._h, C.c_void_p(xb.data_ptr()), xb.shape[0], C.c_void_p(out[s:].data_ptr()))
                _lib.check(fn(*head, *tail) if pooled_width else fn(*head, 1 if normalize else 0, *tail), "encode")
        return out

    def encode_image(self, pixels: torch.Tensor, normalize: bool = False) -> torch.Tensor:
        a = self.arch
        _require_cuda(pixels, "pixels")
        if pixels.dim() != 4 or tuple(pixels.shape[1:]) != (3, a.image_size, a.image_size):
            raise RuntimeError(f"encode_image expects [B,3,{a.image_size},{a.image_size}], got {tuple(pixels.shape)}")
        pixels = pixels.to(dtype=torch.float32).contiguous()
        return self._encode(self._L.kemr_encode_image, _lib.TOWER_VISION, pixels, self.image_batch, normalize)

    def _refuse_pooled(self, what: str) -> None:
        if self.arch.family != "clip":
            raise RuntimeError(f"{what}: pooled tower rows are served for the CLIP family only (SigLIP's head is the attention pool "
                               f"over every row, BERT has no head); this model's family is {self.arch.family!r}")

    def encode_image_pooled(self, pixels: torch.Tensor) -> torch.Tensor:
        """fp32 [B, v_width]: the class-token row of the residual stream BEFORE ln_post and the projection (kemr_encode_image_pooled);
        ``(ln_post(rows) @ visual.proj)`` is ``encode_image(pixels)``.  What a head trained on frozen towers takes as its input."""
        a = self.arch
        self._refuse_pooled("encode_image_pooled")
        _require_cuda(pixels, "pixels")
        if pixels.dim() != 4 or tuple(pixels.shape[1:]) != (3, a.image_size, a.image_size):
            raise RuntimeError(f"encode_image_pooled expects [B,3,{a.image_size},{a.image_size}], got {tuple(pixels.shape)}")
        pixels = pixels.to(dtype=torch.float32).contiguous()
        return self._encode(self._L.kemr_encode_image_pooled, _lib.TOWER_VISION, pixels, self.image_batch, False, pooled_width=a.v_width)

    def encode_text_pooled(self, ids: torch.Tensor, lens: Optional[torch.Tensor] = None) -> torch.Tensor:
        """fp32 [B, t_width]: the end-of-text row BEFORE ln_final and the projection (kemr_encode_text_pooled / _packed_pooled, chosen
        like encode_text chooses between the dense and the packed call)."""
        self._refuse_pooled("encode_text_pooled")
        return self.encode_text(ids, lens=lens, _pooled=True)

    def encode_text(self, ids: torch.Tensor, normalize: bool = False, lens: Optional[torch.Tensor] = None, _pooled: bool = False) -> torch.Tensor:
        """``model.encode_text(tokens)`` (+ the optional L2 normalisation).  The rows behind a text's end-of-text token cannot reach
        its embedding (causal mask, pooled at ``tokens.argmax(-1)``), so by default only the first ``lens[i] = argmax_i + 1``
        positions of every text are computed, packed one text behind the other (kemr_encode_text_packed: the same embeddings --
        up to the summation order of the GEMM kernel a launch of that many rows is routed to, as with another batch size -- from
        sum(lens) instead of B * ctx token rows in every launch).  The lengths must be known on the HOST to size the launches:

        * ``ids`` on the host (what a tokenizer returns): lengths are taken from it there, then it is uploaded -- no device sync;
        * ``ids`` on the GPU with ``lens`` (host int tensor [B], ``text_lengths(host_tokens)``): no device sync;
        * ``ids`` on the GPU alone: one small device-to-host copy (B ints) per call, unless ``KEMR_TEXT_PACK_SYNC=0``, which sends
          such calls through the full-context kernel instead.

        ``KEMR_TEXT_PACKED=0`` (or ``self.pack_text = False``) computes every position, as the reference does."""
        a = self.arch
        if ids.dim() != 2 or ids.shape[1] != a.ctx:
            raise RuntimeError(f"encode_text expects [B,{a.ctx}] token ids, got {tuple(ids.shape)}")
        if not self.ready:
            raise RuntimeError("ClipEngine: load_state_dict() must be called before encoding")
        # never the packed entry point for SigLIP (the library refuses it); an fp32x3 model is served packed up to 128 positions only
        # (include/kemr.h), every other precision at every context the library takes (Long-CLIP's 248 among them)
        pack = self.pack_text and a.family != "siglip" and (a.ctx <= 128 or self.precision != "fp32x3")
        if pack and not ids.is_cuda:
            # host ids: the lengths are free to compute; caller-supplied ones may only LENGTHEN a text (a length short of the
            # end-of-text token would pool the wrong row: ADVICE r3)
            own = text_lengths(ids)
            if lens is None:
                lens = own
            else:
                given = torch.as_tensor(lens, device="cpu").reshape(-1).to(own.dtype)
                if given.numel() != own.numel():
                    raise RuntimeError(f"encode_text: {given.numel()} lengths for {own.numel()} texts")
                lens = torch.maximum(given, own)
        ids = ids.to(device=self.device, dtype=torch.int32, non_blocking=True).contiguous()
        _require_cuda(ids, "token ids")
        if pack and lens is None and os.environ.get("KEMR_TEXT_PACK_SYNC", "1") != "0":
            lens = text_lengths(ids).cpu()                    # the one synchronising copy of this path
        if not pack or lens is None:
            if _pooled:
                return self._encode(self._L.kemr_encode_text_pooled, _lib.TOWER_TEXT, ids, MAX_TEXT_BATCH, False, pooled_width=a.t_width)
            return self._encode(self._L.kemr_encode_text, _lib.TOWER_TEXT, ids, MAX_TEXT_BATCH, normalize)
        n = ids.shape[0]
        lens = torch.as_tensor(lens, dtype=torch.int32, device="cpu").reshape(-1).clamp(1, a.ctx).contiguous()
        if lens.numel() != n:
            raise RuntimeError(f"encode_text: {lens.numel()} lengths for {n} texts")
        out = torch.empty((n, a.t_width if _pooled else a.embed_dim), dtype=torch.float32, device=self.device)
        if n == 0:
            return out
        lens_dev = lens.to(self.device, non_blocking=True)
        # calls of at most TEXT_ROW_BUDGET token rows (256 row tiles of the persistent GEMM: whole rounds, engine.tile_friendly_batch)
        csum = torch.cumsum(lens.to(torch.int64), 0).tolist()
        with torch.cuda.device(self.device), self._order.call(self.device) as cur:
            stream = cur.cuda_stream
            s0, base = 0, 0
            while s0 < n:
                s1 = s0 + 1
                while s1 < n and csum[s1] - base <= TEXT_ROW_BUDGET and s1 - s0 < 65528:
                    s1 += 1
                rows = csum[s1 - 1] - base
                need = int(self._L.kemr_text_packed_workspace_bytes(self._h, rows, s1 - s0))
                ws = self._ws.get("text_packed")
                if ws is None or ws.numel() < need:
                    self._order.retire(ws)
                    ws = self._ws["text_packed"] = torch.empty(max(need, int(self._L.kemr_text_packed_workspace_bytes(
                        self._h, min(TEXT_ROW_BUDGET, n * a.ctx), min(n, 65528)))), dtype=torch.uint8, device=self.device)
                head = (self._h, C.c_void_p(ids[s0:].data_ptr()), C.c_void_p(lens_dev[s0:].data_ptr()), rows, s1 - s0, C.c_void_p(out[s0:].data_ptr()))
                tail = (C.c_void_p(ws.data_ptr()), ws.numel(), C.c_void_p(stream))
                if _pooled:
                    _lib.check(self._L.kemr_encode_text_packed_pooled(*head, *tail), "encode_text_packed_pooled")
                else:
                    _lib.check(self._L.kemr_encode_text_packed(*head, 1 if normalize else 0, *tail), "encode_text_packed")
                s0, base = s1, csum[s1 - 1]
        return out


class BertEngine:
    """One packed BERT sentence encoder (model family 2 of the library) in HBM: ``transformers.BertModel`` without its pooler, then mean
    or CLS pooling -- E5, GTE, BGE; or, for an arch with ``relative_bias``, an MPNet one (family 3: all-mpnet-base-v2, whose attention
    scores carry a learned relative position bias; state dict by hf_checkpoint.from_mpnet_state_dict).  ``encode_ids`` is `kemr_encode_text_packed`: the texts of a call are packed one behind the other,
    each on its own ``lens[i]`` positions (a padding mask is a length), so a call costs sum(lens) token rows, not B x the longest."""

    ROW_BUDGET = 65536           # token rows per packed call: 256 row tiles of the persistent GEMM (TEXT_ROW_BUDGET's reasoning)

    def __init__(self, arch, device: torch.device | str = "cuda:0", precision: str = _lib.DEFAULT_PRECISION):
        if precision not in ("bf16-x24", "bf16", "bf16-res16"):
            raise ValueError(f"BertEngine: precision {precision!r}; served: 'bf16-x24' (default), 'bf16', 'bf16-res16' (the fp8 precisions and "
                             "fp32x3 are not served for this family)")
        self.precision, self.arch = precision, arch
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("BertEngine needs a GPU device; the HIP path has no CPU fallback")
        self._L = _lib.lib()
        cfg = _lib.KemrCfg(**arch.cfg_dict())
        h = C.c_void_p()
        mpnet = bool(getattr(arch, "relative_bias", False))
        _lib.check(self._L.kemr_model_create_family(C.byref(cfg), _lib.FAMILY_BERT, C.byref(h)), "model_create_family")
        self._h = h
        from .config import BERT_POOLING, MPNET_EPS
        if mpnet:                                      # family 3 is a family-2 model switched before its first tensor is loaded
            _lib.check(self._L.kemr_model_set_option(self._h, b"family", _lib.FAMILY_MPNET), "model_set_option")
            _lib.check(self._L.kemr_model_set_option(self._h, b"layer_norm_eps", MPNET_EPS[arch.layer_norm_eps]), "model_set_option")
        _lib.check(self._L.kemr_model_set_option(self._h, b"pooling", BERT_POOLING[arch.pooling]), "model_set_option")
        self._ws: Optional[torch.Tensor] = None
        self._order = CallOrder()
        self.ready = False

    __del__ = ClipEngine.__del__
    tensor_names = ClipEngine.tensor_names

    def set_pooling(self, pooling: str) -> None:
        from .config import BERT_POOLING
        if pooling not in BERT_POOLING:
            raise ValueError(f"pooling {pooling!r}; served: {list(BERT_POOLING)}")
        _lib.check(self._L.kemr_model_set_option(self._h, b"pooling", BERT_POOLING[pooling]), "model_set_option")

    def load_state_dict(self, sd: Mapping[str, torch.Tensor]) -> None:
        """Strict load of a state dict under the engine's names (hf_checkpoint.from_bert_state_dict) + pack to HBM."""
        for name, t in sd.items():
            host = t.detach().to(device="cpu", dtype=torch.float32).contiguous()
            shape = (C.c_int64 * max(host.dim(), 1))(*host.shape)
            _lib.check(self._L.kemr_model_load_tensor(self._h, name.encode(), C.c_void_p(host.data_ptr()), _lib.KEMR_F32, shape, host.dim()),
                       f"load_tensor({name})")
        _lib.check(self._L.kemr_model_set_option(self._h, b"residual_stream_24bit", 1 if self.precision.endswith("-x24") else 0), "model_set_option")
        with torch.cuda.device(self.device):
            _lib.check(self._L.kemr_model_finalize(self._h, _lib.PRECISIONS[self.precision]), "model_finalize")
        self.ready = True

    def encode_ids(self, ids: torch.Tensor, lens, normalize: bool = False) -> torch.Tensor:
        """ids int [B, ctx] (host or device; positions behind a text's length are never read), lens int [B] on the HOST (what the
        tokenizer returned) -> fp32 [B, width] on the device, in input order."""
        a = self.arch
        if not self.ready:
            raise RuntimeError("BertEngine: load_state_dict() must be called before encoding")
        if ids.dim() != 2 or ids.shape[1] != a.ctx:
            raise RuntimeError(f"encode_ids expects [B,{a.ctx}] token ids, got {tuple(ids.shape)}")
        n = ids.shape[0]
        lens = torch.as_tensor(lens, device="cpu").reshape(-1).to(torch.int32).clamp(1, a.ctx).contiguous()
        if lens.numel() != n:
            raise RuntimeError(f"encode_ids: {lens.numel()} lengths for {n} texts")
        ids = ids.to(device=self.device, dtype=torch.int32, non_blocking=True).contiguous()
        out = torch.empty((n, a.width), dtype=torch.float32, device=self.device)
        if n == 0:
            return out
        lens_dev = lens.to(self.device, non_blocking=True)
        csum = torch.cumsum(lens.to(torch.int64), 0).tolist()
        with torch.cuda.device(self.device), self._order.call(self.device) as cur:
            stream = cur.cuda_stream
            s0, base = 0, 0
            while s0 < n:
                s1 = s0 + 1
                while s1 < n and csum[s1] - base <= self.ROW_BUDGET and s1 - s0 < 65528:
                    s1 += 1
                rows = csum[s1 - 1] - base
                need = int(self._L.kemr_text_packed_workspace_bytes(self._h, rows, s1 - s0))
                if self._ws is None or self._ws.numel() < need:
                    self._order.retire(self._ws)
                    self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
                _lib.check(self._L.kemr_encode_text_packed(self._h, C.c_void_p(ids[s0:].data_ptr()), C.c_void_p(lens_dev[s0:].data_ptr()),
                                                           rows, s1 - s0, C.c_void_p(out[s0:].data_ptr()), 1 if normalize else 0,
                                                           C.c_void_p(self._ws.data_ptr()), self._ws.numel(), C.c_void_p(stream)),
                           "encode_text_packed")
                s0, base = s1, csum[s1 - 1]
        return out


def precision_gap(model_or_engine, pixels: Optional[torch.Tensor], ids: Optional[torch.Tensor], fast: str = _lib.DEFAULT_PRECISION,
                  exact: str = "fp32x3") -> Dict[str, Dict[str, object]]:
    """Is `fast` safe for THIS checkpoint on THIS data?  Packs the same weights twice, at precision `fast` and at `exact` (the
    fp32-grade "fp32x3"), encodes `pixels` ([B, 3, S, S] normalised) and `ids` ([B, ctx] token ids; either may be None) with both and
    returns, per tower, the per-embedding 1 - cos between the two:

        {"image": {"one_minus_cos": fp64 tensor [B] (CPU), "worst": float, "median": float, "argmax": int}, "text": {...},
         "fast": fast, "exact": exact}

    `model_or_engine`: a `CLIP` module (its state dict and activation) or a `ClipEngine` that has loaded one.  Two engines of its
    own are built and dropped; the one handed in is not touched.  The path's bar is 1e-3: a worst value near
    or above it means the checkpoint is in the regime bf16 operands cannot hold (LayerNorm gains of 30-100 that the following
    weights do not compensate) and should be served at `exact`."""
    if isinstance(model_or_engine, ClipEngine):
        if model_or_engine._state is None:
            raise RuntimeError("precision_gap: the engine has not loaded a state dict")
        arch, device, activation, sd = model_or_engine.arch, model_or_engine.device, model_or_engine.activation, model_or_engine._state
    else:
        arch, activation = model_or_engine.arch, model_or_engine.activation
        device = next(model_or_engine.parameters()).device
        sd = {k: v for k, v in model_or_engine.state_dict().items() if k != "logit_scale"}
    embs = {}
    for prec in (fast, exact):
        eng = ClipEngine(arch, device, precision=prec, activation=activation)
        eng.load_state_dict(sd)
        embs[prec] = (eng.encode_image(pixels.to(device)).double().cpu() if pixels is not None else None,
                      eng.encode_text(ids).double().cpu() if ids is not None else None)
        del eng
    out: Dict[str, Dict[str, object]] = {"fast": fast, "exact": exact}
    for i, tower in enumerate(("image", "text")):
        a, b = embs[fast][i], embs[exact][i]
        if a is None:
            continue
        gap = 1.0 - torch.nn.functional.cosine_similarity(a, b, dim=-1)      # fp64 on the CPU, the expression the tests measure with
        out[tower] = {"one_minus_cos": gap, "worst": float(gap.max()), "median": float(gap.median()), "argmax": int(gap.argmax())}
    return out


# ====================================================================== similarity / ranking ops

def rows_alloc(rows: int) -> int:
    return (rows + 255) // 256 * 256


class Panel:
    """bf16 operand of the fused similarity kernels: [rows (padded to 256), kdim]."""

    def __init__(self, data: torch.Tensor, rows: int, kdim: int, terms: int, side: int):
        self.data, self.rows, self.kdim, self.terms, self.side = data, rows, kdim, terms, side

    @property
    def device(self):
        return self.data.device


def build_panel(parts: Sequence[torch.Tensor], side: int, terms: int = 3,
                part_scale: Optional[Sequence[float]] = None,
                row_scale: Optional[Sequence[Optional[torch.Tensor]]] = None) -> Panel:
    """Concatenate weighted embedding sets along k and split to bf16 (see include/kemr.h)."""
    L = _lib.lib()
    parts = [p.to(torch.float32).contiguous() for p in parts]
    for p in parts:
        _require_cuda(p, "embeddings")
    rows, d = parts[0].shape
    if any(tuple(p.shape) != (rows, d) for p in parts):
        raise RuntimeError("build_panel: all parts must share one [rows, d] shape")
    n = len(parts)
    kdim = int(L.kemr_panel_kdim(d, n, terms))
    if kdim <= 0:
        raise RuntimeError(f"build_panel: unsupported d={d} nparts={n} terms={terms}")
    dev = parts[0].device
    out = torch.empty((rows_alloc(max(rows, 1)), kdim), dtype=torch.bfloat16, device=dev)
    pp = (C.c_void_p * n)(*[p.data_ptr() for p in parts])
    ps = (C.c_float * n)(*(list(part_scale) if part_scale is not None else [1.0] * n))
    keep = []
    if row_scale is not None:
        rs = []
        for r in row_scale:
            if r is None:
                rs.append(None)
            else:
                r = r.to(device=dev, dtype=torch.float32).contiguous().view(-1)
                if r.numel() != rows:
                    raise RuntimeError("build_panel: row_scale must have one entry per row")
                keep.append(r)
                rs.append(r.data_ptr())
        prs = (C.c_void_p * n)(*rs)
    else:
        prs = None
    with torch.cuda.device(dev):
        _lib.check(L.kemr_panel_build(pp, ps, prs, n, rows, d, terms, side, C.c_void_p(out.data_ptr()),
                                      C.c_void_p(_stream_ptr(dev))), "panel_build")
    return Panel(out, rows, kdim, terms, side)


def _opt_ptr(t: Optional[torch.Tensor]):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def pair_scores(qp: Panel, gp: Panel, q_rows: torch.Tensor, g_rows: torch.Tensor) -> torch.Tensor:
    L = _lib.lib()
    q_rows = q_rows.to(device=qp.device, dtype=torch.int32).contiguous()
    g_rows = g_rows.to(device=qp.device, dtype=torch.int32).contiguous()
    n = q_rows.numel()
    out = torch.empty(n, dtype=torch.float32, device=qp.device)
    if n:
        with torch.cuda.device(qp.device):
            _lib.check(L.kemr_pair_scores(C.c_void_p(qp.data.data_ptr()), C.c_void_p(gp.data.data_ptr()), qp.kdim,
                                          C.c_void_p(q_rows.data_ptr()), C.c_void_p(g_rows.data_ptr()), n,
                                          C.c_void_p(out.data_ptr()), C.c_void_p(_stream_ptr(qp.device))), "pair_scores")
    return out


def sim_topk(qp: Panel, gp: Panel, k: int, gallery_offset: int = 0,
             gt_idx: Optional[torch.Tensor] = None, gt_score: Optional[torch.Tensor] = None,
             ahead: Optional[torch.Tensor] = None,
             bonus: Optional[Tuple[torch.Tensor, torch.Tensor, torch.Tensor]] = None,
             return_workspace: bool = False):
    """Fused scores + top-k (+ `ahead` counts when a ground truth is given). Returns (scores [nq,k], ids [nq,k]).
    k == 0 = rank only (needs the ground truth; the returned tensors are empty).  return_workspace (tools/): the call's
    scratch tensor as a third result (debug.sim_lists reads the candidate-list statistics out of it); otherwise the scratch
    goes back to the caching allocator with the call (2.3 GB at 43 k x 43 k)."""
    L = _lib.lib()
    if qp.kdim != gp.kdim:
        raise RuntimeError(f"sim_topk: panel kdim mismatch ({qp.kdim} vs {gp.kdim})")
    dev = qp.device
    nq, ng = qp.rows, gp.rows
    top_s = torch.empty((nq, k), dtype=torch.float32, device=dev)
    top_i = torch.empty((nq, k), dtype=torch.int32, device=dev)
    if nq == 0:
        return top_s, top_i
    if ng == 0:
        return top_s.fill_(float("-inf")), top_i.fill_(-1)
    ws = torch.empty(max(int(L.kemr_sim_workspace_bytes(nq, ng, qp.kdim, k)), 256), dtype=torch.uint8, device=dev)
    if gt_idx is not None:
        if gt_score is None or ahead is None:
            raise RuntimeError("sim_topk: gt_idx needs gt_score and ahead")
        gt_idx = gt_idx.to(device=dev, dtype=torch.int32).contiguous()
        gt_score = gt_score.to(device=dev, dtype=torch.float32).contiguous()
        if ahead.dtype != torch.int32 or not ahead.is_contiguous() or ahead.device != dev:
            raise RuntimeError("sim_topk: ahead must be a contiguous int32 tensor on the panel's device")
    b_ptr = b_col = b_val = None
    if bonus is not None and len(bonus[1]) == 0:      # no hit at all: same as no bonus (empty tensors have no address)
        bonus = None
    if bonus is not None:
        b_ptr, b_col, b_val = (torch.as_tensor(bonus[0]).to(device=dev, dtype=torch.int32).contiguous(),
                               torch.as_tensor(bonus[1]).to(device=dev, dtype=torch.int32).contiguous(),
                               torch.as_tensor(bonus[2]).to(device=dev, dtype=torch.float32).contiguous())
        if b_ptr.numel() != nq + 1:
            raise RuntimeError("sim_topk: bonus row pointer must have nq + 1 entries")
    with torch.cuda.device(dev):
        _lib.check(L.kemr_sim_topk(C.c_void_p(qp.data.data_ptr()), nq, C.c_void_p(gp.data.data_ptr()), ng, qp.kdim,
                                   gallery_offset, k, C.c_void_p(top_s.data_ptr()), C.c_void_p(top_i.data_ptr()),
                                   _opt_ptr(gt_idx), _opt_ptr(gt_score), _opt_ptr(ahead),
                                   _opt_ptr(b_ptr), _opt_ptr(b_col), _opt_ptr(b_val),
                                   C.c_void_p(ws.data_ptr()), ws.numel(), C.c_void_p(_stream_ptr(dev))), "sim_topk")
    if return_workspace:
        return top_s, top_i, ws
    return top_s, top_i


def _f32_rows(scores: torch.Tensor) -> Tuple[torch.Tensor, int]:
    """A [nq, n] score matrix as the kernels read it: fp32, unit column stride, and the row stride ``ld`` of the ABI (row-strided views
    are read in place)."""
    scores = scores.to(torch.float32)
    if scores.stride(-1) != 1 or (scores.shape[0] > 1 and scores.stride(0) < scores.shape[1]):
        scores = scores.contiguous()
    nq, n = scores.shape
    return scores, (scores.stride(0) if nq > 1 else max(n, 1))


def _rank_outputs(nq: int, ng: int, k: int, with_ahead: bool, dev) -> Tuple[Optional[torch.Tensor], Optional[torch.Tensor], Optional[torch.Tensor]]:
    """(ahead, top scores, top ids) of the dense rankers: zeros, and lists that are padding already where there is no column."""
    ahead = torch.zeros(nq, dtype=torch.int32, device=dev) if with_ahead else None
    if k <= 0:
        return ahead, None, None
    if ng == 0:
        return ahead, torch.full((nq, k), float("-inf"), dtype=torch.float32, device=dev), torch.full((nq, k), -1, dtype=torch.int32, device=dev)
    return ahead, torch.empty((nq, k), dtype=torch.float32, device=dev), torch.empty((nq, k), dtype=torch.int32, device=dev)


def topk_merge(scores: torch.Tensor, idx: torch.Tensor, k: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """[nq, nlists, k] candidate lists -> [nq, k] (score desc, id asc)."""
    L = _lib.lib()
    _require_cuda(scores, "scores")
    nq, nlists, kk = scores.shape
    if kk != k or tuple(idx.shape) != tuple(scores.shape):
        raise RuntimeError("topk_merge: expected scores/idx of shape [nq, nlists, k]")
    scores = scores.to(torch.float32).contiguous()
    idx = idx.to(torch.int32).contiguous()
    out_s = torch.empty((nq, k), dtype=torch.float32, device=scores.device)
    out_i = torch.empty((nq, k), dtype=torch.int32, device=scores.device)
    if nq:
        with torch.cuda.device(scores.device):
            _lib.check(L.kemr_topk_merge(C.c_void_p(scores.data_ptr()), C.c_void_p(idx.data_ptr()), nq, nlists, k,
                                         C.c_void_p(out_s.data_ptr()), C.c_void_p(out_i.data_ptr()),
                                         C.c_void_p(_stream_ptr(scores.device))), "topk_merge")
    return out_s, out_i


def select_topk(scores: torch.Tensor, k: int, idx: Optional[torch.Tensor] = None, id_offset: int = 0
                ) -> Tuple[torch.Tensor, torch.Tensor]:
    """Deep top-k (1 <= k <= 1024) of a materialised fp32 matrix [nq, n] on the GPU: (scores [nq, k], ids [nq, k]), score
    descending then lower id, padded with -inf / -1.  ids: ``idx`` (int32, same shape and row stride as ``scores``; entries < 0
    are skipped, the ids of a row are distinct) or ``id_offset + column``.  Row-strided views are read in place."""
    L = _lib.lib()
    _require_cuda(scores, "score matrix")
    if scores.dim() != 2:
        raise RuntimeError("select_topk: expected a [nq, n] score matrix")
    scores, ld = _f32_rows(scores)
    nq, n = scores.shape
    dev = scores.device
    if idx is not None:
        if tuple(idx.shape) != (nq, n):
            raise RuntimeError("select_topk: idx must have the shape of scores")
        idx = idx.to(device=dev, dtype=torch.int32)
        if idx.stride(-1) != 1 or (nq > 1 and idx.stride(0) != ld):
            scores, idx, ld = scores.contiguous(), idx.contiguous(), max(n, 1)
    if not 1 <= k <= _lib.MAX_DEEP_K:
        raise RuntimeError(f"select_topk: k={k} not in 1..{_lib.MAX_DEEP_K}")
    top_s = torch.empty((nq, k), dtype=torch.float32, device=dev)
    top_i = torch.empty((nq, k), dtype=torch.int32, device=dev)
    if nq == 0:
        return top_s, top_i
    if n == 0:
        return top_s.fill_(float("-inf")), top_i.fill_(-1)
    with torch.cuda.device(dev):
        _lib.check(L.kemr_select_topk(C.c_void_p(scores.data_ptr()), _opt_ptr(idx), nq, n, ld, id_offset, k,
                                      C.c_void_p(top_s.data_ptr()), C.c_void_p(top_i.data_ptr()), C.c_void_p(_stream_ptr(dev))),
                   "select_topk")
    return top_s, top_i


def sim_topk_deep(qp: Panel, gp: Panel, k: int, gallery_offset: int = 0, query_block: Optional[int] = None,
                  gt_idx: Optional[torch.Tensor] = None, gt_score: Optional[torch.Tensor] = None,
                  ahead: Optional[torch.Tensor] = None,
                  bonus: Optional[Tuple[torch.Tensor, torch.Tensor, torch.Tensor]] = None
                  ) -> Tuple[torch.Tensor, torch.Tensor]:
    """Scores + exact top-k for 1 <= k <= 1024: (scores [nq, k], global ids [nq, k]), the scores bit-identical to ``scores_dense`` /
    ``pair_scores`` / ``sim_topk``.  The queries are walked in blocks of what the workspace holds (default: up to 1024 rows of fp32
    scores against the whole gallery); ``query_block`` sizes the workspace for that many rows instead (tests: several blocks).

    ``bonus`` (CSR ``(rowptr [nq + 1], col, val)``, GLOBAL column ids ascending within a row) is added to the scores before the
    selection, and with ``gt_idx`` (GLOBAL ids) / ``gt_score`` / ``ahead`` (int32, accumulated) the candidates ranked before the
    ground truth are counted on the fused scores in the same call (``kemr_sim_topk_deep_fused``): the arguments, conversions and
    checks of ``sim_topk``.  Without them the call is ``kemr_sim_topk_deep``."""
    L = _lib.lib()
    if qp.kdim != gp.kdim:
        raise RuntimeError(f"sim_topk_deep: panel kdim mismatch ({qp.kdim} vs {gp.kdim})")
    if not 1 <= k <= _lib.MAX_DEEP_K:
        raise RuntimeError(f"sim_topk_deep: k={k} not in 1..{_lib.MAX_DEEP_K}")
    dev = qp.device
    nq, ng = qp.rows, gp.rows
    top_s = torch.empty((nq, k), dtype=torch.float32, device=dev)
    top_i = torch.empty((nq, k), dtype=torch.int32, device=dev)
    if nq == 0:
        return top_s, top_i
    if ng == 0:
        return top_s.fill_(float("-inf")), top_i.fill_(-1)
    if gt_idx is not None:
        if gt_score is None or ahead is None:
            raise RuntimeError("sim_topk_deep: gt_idx needs gt_score and ahead")
        gt_idx = gt_idx.to(device=dev, dtype=torch.int32).contiguous()
        gt_score = gt_score.to(device=dev, dtype=torch.float32).contiguous()
        if ahead.dtype != torch.int32 or not ahead.is_contiguous() or ahead.device != dev:
            raise RuntimeError("sim_topk_deep: ahead must be a contiguous int32 tensor on the panel's device")
        if gt_idx.numel() != nq or gt_score.numel() != nq or ahead.numel() != nq:
            raise RuntimeError("sim_topk_deep: gt_idx, gt_score and ahead must have one entry per query")
    b_ptr = b_col = b_val = None
    if bonus is not None and len(bonus[1]) == 0:      # no hit at all: same as no bonus (empty tensors have no address)
        bonus = None
    if bonus is not None:
        b_ptr, b_col, b_val = (torch.as_tensor(bonus[0]).to(device=dev, dtype=torch.int32).contiguous(),
                               torch.as_tensor(bonus[1]).to(device=dev, dtype=torch.int32).contiguous(),
                               torch.as_tensor(bonus[2]).to(device=dev, dtype=torch.float32).contiguous())
        if b_ptr.numel() != nq + 1:
            raise RuntimeError("sim_topk_deep: bonus row pointer must have nq + 1 entries")
        if b_val.numel() != b_col.numel():
            raise RuntimeError("sim_topk_deep: bonus col and val must have one entry per hit")
    if query_block is None:
        nbytes = int(L.kemr_sim_topk_deep_workspace_bytes(nq, ng, qp.kdim, k))
    else:
        nbytes = int(L.kemr_sim_topk_deep_workspace_bytes(128, ng, qp.kdim, k)) // 128 * int(query_block)
    ws = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        if gt_idx is None and ahead is None and gt_score is None and bonus is None:
            _lib.check(L.kemr_sim_topk_deep(C.c_void_p(qp.data.data_ptr()), nq, C.c_void_p(gp.data.data_ptr()), ng, qp.kdim,
                                            gallery_offset, k, C.c_void_p(top_s.data_ptr()), C.c_void_p(top_i.data_ptr()),
                                            C.c_void_p(ws.data_ptr()), ws.numel(), C.c_void_p(_stream_ptr(dev))), "sim_topk_deep")
        else:
            _lib.check(L.kemr_sim_topk_deep_fused(C.c_void_p(qp.data.data_ptr()), nq, C.c_void_p(gp.data.data_ptr()), ng, qp.kdim,
                                                  gallery_offset, k, C.c_void_p(top_s.data_ptr()), C.c_void_p(top_i.data_ptr()),
                                                  _opt_ptr(gt_idx), _opt_ptr(gt_score), _opt_ptr(ahead),
                                                  _opt_ptr(b_ptr), _opt_ptr(b_col), _opt_ptr(b_val),
                                                  C.c_void_p(ws.data_ptr()), ws.numel(), C.c_void_p(_stream_ptr(dev))),
                       "sim_topk_deep_fused")
    return top_s, top_i


def cross_attention_rerank(q: torch.Tensor, k_i: torch.Tensor, k_t: torch.Tensor, p_i: torch.Tensor, p_t: torch.Tensor,
                           c0: torch.Tensor, w2t: torch.Tensor, b2: torch.Tensor, w3: torch.Tensor, b3: float,
                           cand_idx: torch.Tensor, depth: Optional[int] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The cross_attention head on listed pairs (``kemr_cross_attention_rerank``): fp32 [nq, ld] scores of query ``q`` against the
    candidates ``cand_idx`` (int32 [nq, ld], row stride ld, ids < 0 = padding -> -inf) in the first ``depth`` (default: all) columns.
    q [nq, dim] scaled attention queries, k_x [ng, dim], p_x [ng, heads, hid1], c0 [hid1], w2t [hid1, hid2], b2 / w3 [hid2]: what
    ``FusionModel`` precomputes per query / per candidate.  ``out`` (fp32 [nq, ld], contiguous): written in place in its first
    ``depth`` columns, the rest is left as it is; without it a new tensor whose columns >= depth hold -inf."""
    L = _lib.lib()
    _require_cuda(q, "attention queries")
    dev = q.device
    f32 = lambda t: t.to(device=dev, dtype=torch.float32).contiguous()
    q, k_i, k_t, p_i, p_t, c0, w2t, b2, w3 = (f32(t) for t in (q, k_i, k_t, p_i, p_t, c0, w2t, b2, w3))
    cand_idx = cand_idx.to(device=dev, dtype=torch.int32).contiguous()
    if q.dim() != 2 or cand_idx.dim() != 2 or cand_idx.shape[0] != q.shape[0]:
        raise RuntimeError("cross_attention_rerank: q [nq, dim] and cand_idx [nq, ld] must describe the same queries")
    nq, dim = q.shape
    ld = cand_idx.shape[1]
    depth = ld if depth is None else int(depth)
    ng, heads, hid1 = p_i.shape
    hid2 = w2t.shape[1]
    if tuple(k_i.shape) != (ng, dim) or tuple(k_t.shape) != (ng, dim) or tuple(p_t.shape) != (ng, heads, hid1) or \
            tuple(w2t.shape) != (hid1, hid2) or c0.numel() != hid1 or b2.numel() != hid2 or w3.numel() != hid2:
        raise RuntimeError("cross_attention_rerank: candidate-side tensors do not fit together")
    if out is None:
        out = torch.full((nq, ld), float("-inf"), dtype=torch.float32, device=dev)
    elif out.dtype != torch.float32 or tuple(out.shape) != (nq, ld) or not out.is_contiguous() or out.device != dev:
        raise RuntimeError("cross_attention_rerank: out must be a contiguous fp32 [nq, ld] tensor on the queries' device")
    if nq and depth:
        with torch.cuda.device(dev):
            _lib.check(L.kemr_cross_attention_rerank(
                C.c_void_p(q.data_ptr()), C.c_void_p(k_i.data_ptr()), C.c_void_p(k_t.data_ptr()), C.c_void_p(p_i.data_ptr()),
                C.c_void_p(p_t.data_ptr()), C.c_void_p(c0.data_ptr()), C.c_void_p(w2t.data_ptr()), C.c_void_p(b2.data_ptr()),
                C.c_void_p(w3.data_ptr()), float(b3), heads, nq, ng, dim, hid1, hid2, C.c_void_p(cand_idx.data_ptr()), depth, ld,
                C.c_void_p(out.data_ptr()), C.c_void_p(_stream_ptr(dev))), "cross_attention_rerank")
    return out


def list_fuse(scores: torch.Tensor, idx: torch.Tensor, depth: Optional[int] = None, scale: float = 1.0,
              bonus: Optional[Tuple[torch.Tensor, torch.Tensor, torch.Tensor]] = None, gt_idx: Optional[torch.Tensor] = None,
              out: Optional[torch.Tensor] = None
              ) -> Tuple[torch.Tensor, Optional[torch.Tensor], Optional[torch.Tensor], Optional[torch.Tensor]]:
    """The knowledge side on listed scores (``kemr_list_fuse``): ``scale * scores + bonus`` in the first ``depth`` (default: all)
    columns of the contiguous fp32 [nq, ld] ``scores`` whose candidates are ``idx`` (int32 [nq, ld], ids < 0 = padding -> -inf).
    ``bonus``: the CSR ``(rowptr [nq + 1], col, val)`` of ``sim_topk_deep`` (GLOBAL column ids ascending within a row).  ``gt_idx``
    (one id per query): also the ground truth's place in the fused list.  ``out`` (contiguous fp32 [nq, ld], may be ``scores``
    itself): written in its first ``depth`` columns, the rest is left as it is; without it a new tensor whose columns >= depth hold
    -inf.  Returns ``(fused, ahead, found, gt_score)``, the last three None without ``gt_idx``: int32 [nq] slots ranked before the
    ground truth (every listed slot where it is absent), int32 [nq] 1 where the row lists it, fp32 [nq] its fused score (-inf where
    absent) -- where found, ``ahead + 1`` is its position in ``select_topk(fused, depth, idx=idx)``."""
    L = _lib.lib()
    _require_cuda(scores, "listed scores")
    dev = scores.device
    if scores.dim() != 2 or idx.dim() != 2 or tuple(idx.shape) != tuple(scores.shape):
        raise RuntimeError("list_fuse: scores and idx must share one [nq, ld] shape")
    if scores.dtype != torch.float32 or not scores.is_contiguous():
        raise RuntimeError("list_fuse: scores must be a contiguous fp32 tensor")
    idx = idx.to(device=dev, dtype=torch.int32).contiguous()
    nq, ld = scores.shape
    depth = ld if depth is None else int(depth)
    if nq and not 1 <= depth <= min(ld, _lib.MAX_DEEP_K):
        raise RuntimeError(f"list_fuse: depth={depth} not in 1..min(ld={ld}, {_lib.MAX_DEEP_K})")
    if out is None:
        out = torch.full((nq, ld), float("-inf"), dtype=torch.float32, device=dev)
    elif out.dtype != torch.float32 or tuple(out.shape) != (nq, ld) or not out.is_contiguous() or out.device != dev:
        raise RuntimeError("list_fuse: out must be a contiguous fp32 [nq, ld] tensor on the scores' device")
    b_ptr = b_col = b_val = None
    if bonus is not None and len(bonus[1]) == 0:      # no hit at all: same as no bonus (empty tensors have no address)
        bonus = None
    if bonus is not None:
        b_ptr, b_col, b_val = (torch.as_tensor(bonus[0]).to(device=dev, dtype=torch.int32).contiguous(),
                               torch.as_tensor(bonus[1]).to(device=dev, dtype=torch.int32).contiguous(),
                               torch.as_tensor(bonus[2]).to(device=dev, dtype=torch.float32).contiguous())
        if b_ptr.numel() != nq + 1:
            raise RuntimeError("list_fuse: bonus row pointer must have nq + 1 entries")
        if b_val.numel() != b_col.numel():
            raise RuntimeError("list_fuse: bonus col and val must have one entry per hit")
    gt = ahead = found = gt_score = None
    if gt_idx is not None:
        gt = torch.as_tensor(gt_idx).to(device=dev, dtype=torch.int32).contiguous().reshape(-1)
        if gt.numel() != nq:
            raise RuntimeError("list_fuse: gt_idx must have one entry per query")
        ahead = torch.empty(nq, dtype=torch.int32, device=dev)
        found = torch.empty(nq, dtype=torch.int32, device=dev)
        gt_score = torch.empty(nq, dtype=torch.float32, device=dev)
    if nq:
        with torch.cuda.device(dev):
            _lib.check(L.kemr_list_fuse(C.c_void_p(scores.data_ptr()), C.c_void_p(idx.data_ptr()), nq, depth, ld, float(scale),
                                        _opt_ptr(b_ptr), _opt_ptr(b_col), _opt_ptr(b_val),
                                        _opt_ptr(gt), _opt_ptr(ahead), _opt_ptr(found), _opt_ptr(gt_score),
                                        C.c_void_p(out.data_ptr()), C.c_void_p(_stream_ptr(dev))), "list_fuse")
    return out, ahead, found, gt_score


def scores_dense(qp: Panel, gp: Panel) -> torch.Tensor:
    """Dense fp32 score matrix [nq, ng] (fusion heads that need every pair; debugging)."""
    L = _lib.lib()
    if qp.kdim != gp.kdim:
        raise RuntimeError("scores_dense: panel kdim mismatch")
    out = torch.empty((qp.rows, gp.rows), dtype=torch.float32, device=qp.device)
    if qp.rows and gp.rows:
        with torch.cuda.device(qp.device):
            _lib.check(L.kemr_scores_dense(C.c_void_p(qp.data.data_ptr()), qp.rows, C.c_void_p(gp.data.data_ptr()), gp.rows,
                                           qp.kdim, C.c_void_p(out.data_ptr()), gp.rows,
                                           C.c_void_p(_stream_ptr(qp.device))), "scores_dense")
    return out


def rank_dense(scores: torch.Tensor, gt_idx: Optional[torch.Tensor] = None, k: int = 0
               ) -> Tuple[Optional[torch.Tensor], Optional[torch.Tensor], Optional[torch.Tensor]]:
    """Rank a materialised fp32 score matrix on the GPU: returns (ahead [nq] or None, top scores, top ids).  Row-strided views are
    read in place (``stride(0)`` is the ABI's ``ld``).  The lists are padded with -inf / -1 where a row has fewer than k candidates
    (an empty gallery: padding only, ahead = 0); a candidate whose score is -inf or NaN is never listed (include/kemr.h)."""
    L = _lib.lib()
    _require_cuda(scores, "score matrix")
    scores, ld = _f32_rows(scores)
    nq, ng = scores.shape
    dev = scores.device
    gt = None if gt_idx is None else gt_idx.to(device=dev, dtype=torch.int32).contiguous()
    ahead, top_s, top_i = _rank_outputs(nq, ng, k, gt is not None, dev)
    if nq and ng:
        with torch.cuda.device(dev):
            _lib.check(L.kemr_rank_dense(C.c_void_p(scores.data_ptr()), nq, ng, ld, _opt_ptr(gt), _opt_ptr(ahead),
                                         k, _opt_ptr(top_s), _opt_ptr(top_i), C.c_void_p(_stream_ptr(dev))), "rank_dense")
    return ahead, top_s, top_i


def rank_dense_shard(scores: torch.Tensor, id_offset: int = 0, gt_idx: Optional[torch.Tensor] = None,
                     gt_score: Optional[torch.Tensor] = None, k: int = 0
                     ) -> Tuple[Optional[torch.Tensor], Optional[torch.Tensor], Optional[torch.Tensor]]:
    """``rank_dense`` for ONE SHARD's columns of a score matrix (``kemr_rank_dense_shard``): column j is the candidate with the GLOBAL
    id ``id_offset + j``; ``gt_idx`` holds GLOBAL ids (on this shard or not, < 0 = none) and ``gt_score`` the ground-truth pairs'
    scores.  Returns (ahead int32 [nq] or None: this shard's columns ranked before the ground truth, top scores, top GLOBAL ids);
    the per-shard ``ahead`` values sum to ``rank_dense``'s and ``topk_merge`` of the per-shard lists is its list.  An empty shard
    (no columns) gives ahead = 0 and padding."""
    L = _lib.lib()
    _require_cuda(scores, "score matrix")
    scores, ld = _f32_rows(scores)
    nq, ng = scores.shape
    dev = scores.device
    if (gt_idx is None) != (gt_score is None):
        raise RuntimeError("rank_dense_shard: gt_idx and gt_score together")
    gt = sgt = None
    if gt_idx is not None:
        gt = gt_idx.to(device=dev, dtype=torch.int32).contiguous()
        sgt = gt_score.to(device=dev, dtype=torch.float32).contiguous()
        if gt.numel() != nq or sgt.numel() != nq:
            raise RuntimeError("rank_dense_shard: gt_idx and gt_score must have one entry per query")
    ahead, top_s, top_i = _rank_outputs(nq, ng, k, gt is not None, dev)
    if nq and ng:
        with torch.cuda.device(dev):
            _lib.check(L.kemr_rank_dense_shard(C.c_void_p(scores.data_ptr()), nq, ng, ld, int(id_offset), _opt_ptr(gt), _opt_ptr(sgt),
                                               _opt_ptr(ahead), k, _opt_ptr(top_s), _opt_ptr(top_i), C.c_void_p(_stream_ptr(dev))),
                       "rank_dense_shard")
    return ahead, top_s, top_i


def gate_rows(x: torch.Tensor, pre: Optional[torch.Tensor], w: torch.Tensor, bias: float, relu: bool,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``kemr_gate_rows``: sigmoid(sum_c act(x[r, c] + pre[c]) w[c] + bias) per row of the contiguous fp32 x [rows, cols] -> fp32
    [rows] (``out``: a contiguous fp32 tensor of at least ``rows`` elements, written in its first ``rows``)."""
    L = _lib.lib()
    _require_cuda(x, "gate input")
    rows, cols = x.shape
    if out is None:
        out = torch.empty(rows, dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(L.kemr_gate_rows(C.c_void_p(x.data_ptr()), rows, cols, _opt_ptr(pre), C.c_void_p(w.data_ptr()), float(bias),
                                    int(bool(relu)), C.c_void_p(out.data_ptr()), C.c_void_p(_stream_ptr(x.device))), "gate_rows")
    return out


def linear_head(t2i: torch.Tensor, t2t: torch.Tensor, w0: torch.Tensor, b0: torch.Tensor, w1: torch.Tensor, b1: float,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``kemr_linear_head``: b1 + w1 . relu(W0 . [t2i, t2t] + b0) on every element of two equally shaped contiguous fp32 tensors
    (w0 [hidden, 2], b0 / w1 [hidden], all contiguous fp32 on t2i's device); ``out``: at least ``t2i.numel()`` fp32 elements."""
    L = _lib.lib()
    _require_cuda(t2i, "t2i scores")
    if out is None:
        out = torch.empty_like(t2i)
    with torch.cuda.device(t2i.device):
        _lib.check(L.kemr_linear_head(C.c_void_p(t2i.data_ptr()), C.c_void_p(t2t.data_ptr()), t2i.numel(), C.c_void_p(w0.data_ptr()),
                                      C.c_void_p(b0.data_ptr()), C.c_void_p(w1.data_ptr()), float(b1), w0.shape[0],
                                      C.c_void_p(out.data_ptr()), C.c_void_p(_stream_ptr(t2i.device))), "linear_head")
    return out


def cross_attention_pairs(st_i: torch.Tensor, st_t: torch.Tensor, p_i: torch.Tensor, p_t: torch.Tensor, c0: torch.Tensor,
                          w2t: torch.Tensor, b2: torch.Tensor, w3: torch.Tensor, b3: float, heads: Optional[int] = None,
                          hid1: Optional[int] = None, hid2: Optional[int] = None, out_t: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``kemr_cross_attention_pairs`` on contiguous fp32 device tensors: st_x [heads, n_c, n_q], p_x [n_c, heads, hid1], c0 [hid1],
    w2t [hid1, hid2], b2 / w3 [hid2] -> out_t fp32 [n_c, n_q] (``out_t``: at least n_c * n_q fp32 elements).  heads / hid1 / hid2
    default to the tensors' shapes; the tests pass sizes the ABI refuses."""
    L = _lib.lib()
    _require_cuda(st_i, "score planes")
    n_c, n_q = st_i.shape[1], st_i.shape[2]
    heads = st_i.shape[0] if heads is None else heads
    hid1 = w2t.shape[0] if hid1 is None else hid1
    hid2 = w2t.shape[1] if hid2 is None else hid2
    if out_t is None:
        out_t = torch.empty((n_c, n_q), dtype=torch.float32, device=st_i.device)
    with torch.cuda.device(st_i.device):
        _lib.check(L.kemr_cross_attention_pairs(
            C.c_void_p(st_i.data_ptr()), C.c_void_p(st_t.data_ptr()), C.c_void_p(p_i.data_ptr()), C.c_void_p(p_t.data_ptr()),
            C.c_void_p(c0.data_ptr()), C.c_void_p(w2t.data_ptr()), C.c_void_p(b2.data_ptr()), C.c_void_p(w3.data_ptr()), float(b3),
            heads, n_q, n_c, hid1, hid2, C.c_void_p(out_t.data_ptr()), C.c_void_p(_stream_ptr(st_i.device))), "cross_attention_pairs")
    return out_t


# ---------------------------------------------------------------------- per-kernel hooks used by tests
def set_gemm_variant(variant: int) -> None:
    """tools/ and tests/: see debug.set_gemm_variant (include/kemr_debug.h; nothing in the product path calls this)."""
    from . import debug
    debug.set_gemm_variant(variant)


def op_gemm(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], m: int, epilogue: int,
            c: Optional[torch.Tensor] = None) -> torch.Tensor:
    """a: bf16 [m_alloc, k] (m_alloc multiple of 256), w: bf16 [n, k]; returns C (bf16 [m_alloc, n] or the fp32 residual)."""
    L = _lib.lib()
    n, k = w.shape
    if c is None:
        c = torch.zeros((a.shape[0], n), dtype=torch.bfloat16 if epilogue != _lib.EPI_BIAS_RESID_F32 else torch.float32,
                        device=a.device)
    with torch.cuda.device(a.device):
        _lib.check(L.kemr_op_gemm(C.c_void_p(a.data_ptr()), C.c_void_p(w.data_ptr()), _opt_ptr(bias), C.c_void_p(c.data_ptr()),
                                  m, n, k, epilogue, C.c_void_p(_stream_ptr(a.device))), "op_gemm")
    return c


def op_gemm_fp8(a: torch.Tensor, w: torch.Tensor, wscale: torch.Tensor, bias: Optional[torch.Tensor], m: int,
                epilogue: int) -> torch.Tensor:
    """a, w: torch.float8_e4m3fn [ceil256(m), k] / [n, k]; returns bf16 [ceil256(m), n] = epi(a.w^T * wscale + bias)."""
    L = _lib.lib()
    n, k = w.shape
    c = torch.zeros((a.shape[0], n), dtype=torch.bfloat16, device=a.device)
    with torch.cuda.device(a.device):
        _lib.check(L.kemr_op_gemm_fp8(C.c_void_p(a.data_ptr()), C.c_void_p(w.data_ptr()), C.c_void_p(wscale.data_ptr()),
                                      _opt_ptr(bias), C.c_void_p(c.data_ptr()), m, n, k, epilogue,
                                      C.c_void_p(_stream_ptr(a.device))), "op_gemm_fp8")
    return c


def op_layernorm(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, out_bf16: bool = True) -> torch.Tensor:
    L = _lib.lib()
    rows, width = x.shape
    y = torch.empty((rows, width), dtype=torch.bfloat16 if out_bf16 else torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(L.kemr_op_layernorm(C.c_void_p(x.data_ptr()), C.c_void_p(gamma.data_ptr()), C.c_void_p(beta.data_ptr()),
                                       C.c_void_p(y.data_ptr()), rows, width, _lib.KEMR_BF16 if out_bf16 else _lib.KEMR_F32,
                                       C.c_void_p(_stream_ptr(x.device))), "op_layernorm")
    return y


def op_layernorm_resid(x: torch.Tensor, delta: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor) -> torch.Tensor:
    """x (fp32, updated in place) += delta (bf16); returns LayerNorm(x) as bf16."""
    L = _lib.lib()
    rows, width = x.shape
    y = torch.empty((rows, width), dtype=torch.bfloat16, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(L.kemr_op_layernorm_resid(C.c_void_p(x.data_ptr()), C.c_void_p(delta.data_ptr()), C.c_void_p(gamma.data_ptr()),
                                             C.c_void_p(beta.data_ptr()), C.c_void_p(y.data_ptr()), rows, width,
                                             C.c_void_p(_stream_ptr(x.device))), "op_layernorm_resid")
    return y


def op_layernorm_rows(x: torch.Tensor, delta: Optional[torch.Tensor], gamma: torch.Tensor, beta: torch.Tensor,
                      out_bf16: bool = True, delta2: Optional[torch.Tensor] = None, writeback: bool = True,
                      out_fp8: bool = False) -> torch.Tensor:
    """General form: x is fp32 or bf16 rows; returns LayerNorm(x [+ delta [+ delta2]]) (deltas bf16); with `writeback`
    the sum is stored back into x in x's dtype."""
    L = _lib.lib()
    rows, width = x.shape
    if x.dtype not in (torch.float32, torch.bfloat16):
        raise RuntimeError("op_layernorm_rows: x must be fp32 or bf16")
    ydt = torch.float8_e4m3fn if out_fp8 else (torch.bfloat16 if out_bf16 else torch.float32)
    y = torch.empty((rows, width), dtype=ydt, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(L.kemr_op_layernorm_rows(C.c_void_p(x.data_ptr()), _lib.KEMR_BF16 if x.dtype == torch.bfloat16 else _lib.KEMR_F32,
                                            _opt_ptr(delta), _opt_ptr(delta2), 1 if writeback else 0,
                                            C.c_void_p(gamma.data_ptr()), C.c_void_p(beta.data_ptr()),
                                            C.c_void_p(y.data_ptr()), rows, width,
                                            _lib.KEMR_FP8 if out_fp8 else (_lib.KEMR_BF16 if out_bf16 else _lib.KEMR_F32),
                                            C.c_void_p(_stream_ptr(x.device))), "op_layernorm_rows")
    return y


def pack_f24_rows(x: torch.Tensor) -> torch.Tensor:
    """fp32 [rows, W] -> the library's 24-bit-float rows (csrc/common.h f24_t): uint8 [rows, 3 W], a row = its W bf16 upper halves
    (little endian) followed by its W third bytes; round to nearest on the 24 kept bits.  Tests / tools."""
    bits = (x.contiguous().view(torch.int32).to(torch.int64) & 0xffffffff) + 0x80
    hi = ((bits >> 16) & 0xffff)
    lo = ((bits >> 8) & 0xff).to(torch.uint8)
    hi_bytes = torch.stack([(hi & 0xff).to(torch.uint8), (hi >> 8).to(torch.uint8)], dim=-1).reshape(x.shape[0], -1)
    return torch.cat([hi_bytes, lo], dim=1).contiguous()


def unpack_f24_rows(rows24: torch.Tensor, width: int) -> torch.Tensor:
    """The inverse of pack_f24_rows (exact): uint8 [rows, 3 W] -> fp32 [rows, W]."""
    hb = rows24[:, :2 * width].reshape(-1, width, 2).to(torch.int64)
    lo = rows24[:, 2 * width:].to(torch.int64)
    bits = (hb[..., 1] << 24) | (hb[..., 0] << 16) | (lo << 8)
    bits = torch.where(bits >= 2 ** 31, bits - 2 ** 32, bits)
    return bits.to(torch.int32).view(torch.float32)


def op_layernorm_rows_f24(x24: torch.Tensor, width: int, delta: Optional[torch.Tensor], gamma: torch.Tensor, beta: torch.Tensor,
                          delta2: Optional[torch.Tensor] = None, writeback: bool = True) -> torch.Tensor:
    """op_layernorm_rows on 24-bit-float rows (pack_f24_rows layout, updated in place with `writeback`); bf16 output."""
    L = _lib.lib()
    rows = x24.shape[0]
    y = torch.empty((rows, width), dtype=torch.bfloat16, device=x24.device)
    with torch.cuda.device(x24.device):
        _lib.check(L.kemr_op_layernorm_rows(C.c_void_p(x24.data_ptr()), 24, _opt_ptr(delta), _opt_ptr(delta2), 1 if writeback else 0,
                                            C.c_void_p(gamma.data_ptr()), C.c_void_p(beta.data_ptr()), C.c_void_p(y.data_ptr()), rows, width,
                                            _lib.KEMR_BF16, C.c_void_p(_stream_ptr(x24.device))), "op_layernorm_rows")
    return y


def op_attention(qkv: torch.Tensor, batch: int, t: int, width: int, causal: bool, head_dim: int = 64) -> torch.Tensor:
    """qkv bf16 [batch * t, 3 width] (q pre-scaled by 1 / sqrt(head_dim)) -> bf16 [batch * t, width].  head_dim 64, or 80 (non-causal,
    t <= 288, width a multiple of 80)."""
    L = _lib.lib()
    out = torch.empty((batch * t, width), dtype=torch.bfloat16, device=qkv.device)
    with torch.cuda.device(qkv.device):
        if head_dim == 64:
            _lib.check(L.kemr_op_attention(C.c_void_p(qkv.data_ptr()), C.c_void_p(out.data_ptr()), batch, t, width,
                                           1 if causal else 0, C.c_void_p(_stream_ptr(qkv.device))), "op_attention")
        else:
            _lib.check(L.kemr_op_attention_hd(C.c_void_p(qkv.data_ptr()), C.c_void_p(out.data_ptr()), batch, t, width, int(head_dim),
                                              1 if causal else 0, C.c_void_p(_stream_ptr(qkv.device))), "op_attention_hd")
    return out


ATTENTION_BACKWARD_LDS_T = 288     # KEMR_MAX_TEXT_CTX: up to here kemr_op_attention_backward (a head in LDS), beyond it the streaming op


def attention_backward(qkv: torch.Tensor, dout: torch.Tensor, batch: int, t: int, width: int, causal: bool, head_dim: int = 64) -> torch.Tensor:
    """The backward of op_attention (heads of 64): qkv bf16 [batch * t, 3 width] as the forward read it (q pre-scaled by 1/8),
    dout bf16 [batch * t, width] -> dqkv bf16 [batch * t, 3 width], the gradient with respect to the planes as given (the caller owns
    the 1/8 of q).  Recomputes the probabilities from qkv; the same bits on every launch.  Routed by shape: t <= 288, causal or not, is
    ``kemr_op_attention_backward`` (no workspace); non-causal 289 <= t <= 1025 is ``kemr_op_attention_backward_long`` (streaming, with
    a workspace of three fp32 per query row and head, a torch allocation on qkv's device and the current stream); causal t > 288 is
    refused by the first op, as the forward refuses it.  ``head_dim=80`` (q pre-scaled by 1/sqrt(80), non-causal, t <= 1025) is
    ``kemr_op_attention_backward_hd``, streaming at every length with the same kind of workspace; any other head dim, and
    ``causal=True`` at 80, are refused with that op's message."""
    _require_cuda(qkv, "attention_backward: qkv")
    _require_cuda(dout, "attention_backward: dout")
    if qkv.dtype != torch.bfloat16 or dout.dtype != torch.bfloat16 or not qkv.is_contiguous() or not dout.is_contiguous():
        raise RuntimeError("attention_backward: qkv and dout must be contiguous bf16")
    if qkv.device != dout.device or tuple(qkv.shape) != (batch * t, 3 * width) or tuple(dout.shape) != (batch * t, width):
        raise RuntimeError(f"attention_backward: qkv must be [{batch * t}, {3 * width}] and dout [{batch * t}, {width}] on one device, got "
                           f"{tuple(qkv.shape)} and {tuple(dout.shape)}")
    dqkv = torch.empty_like(qkv)
    L = _lib.lib()
    with torch.cuda.device(qkv.device):
        if head_dim != 64:
            need = int(L.kemr_attention_backward_hd_workspace_bytes(batch, t, width, int(head_dim)))
            ws = torch.empty(max(need, 4), dtype=torch.uint8, device=qkv.device)
            _lib.check(L.kemr_op_attention_backward_hd(C.c_void_p(qkv.data_ptr()), C.c_void_p(dout.data_ptr()), C.c_void_p(dqkv.data_ptr()),
                                                       batch, t, width, int(head_dim), 1 if causal else 0, C.c_void_p(ws.data_ptr()), need,
                                                       C.c_void_p(_stream_ptr(qkv.device))), "op_attention_backward_hd")
        elif causal or t <= ATTENTION_BACKWARD_LDS_T:
            _lib.check(L.kemr_op_attention_backward(C.c_void_p(qkv.data_ptr()), C.c_void_p(dout.data_ptr()), C.c_void_p(dqkv.data_ptr()),
                                                    batch, t, width, 1 if causal else 0, C.c_void_p(_stream_ptr(qkv.device))),
                       "op_attention_backward")
        else:
            need = int(L.kemr_attention_backward_long_workspace_bytes(batch, t, width))
            ws = torch.empty(max(need, 4), dtype=torch.uint8, device=qkv.device)
            _lib.check(L.kemr_op_attention_backward_long(C.c_void_p(qkv.data_ptr()), C.c_void_p(dout.data_ptr()), C.c_void_p(dqkv.data_ptr()),
                                                         batch, t, width, C.c_void_p(ws.data_ptr()), need,
                                                         C.c_void_p(_stream_ptr(qkv.device))), "op_attention_backward_long")
    return dqkv


def _check_packed(who: str, qkv: torch.Tensor, row_start: torch.Tensor, width: int, dout: Optional[torch.Tensor] = None) -> None:
    """What the two packed attention wrappers check before they hand pointers to the library."""
    tensors = [(qkv, "qkv"), (row_start, "row_start")] + ([(dout, "dout")] if dout is not None else [])
    for t, what in tensors:
        _require_cuda(t, f"{who}: {what}")
    if qkv.dtype != torch.bfloat16 or not qkv.is_contiguous() or (dout is not None and (dout.dtype != torch.bfloat16 or not dout.is_contiguous())):
        raise RuntimeError(f"{who}: qkv{'' if dout is None else ' and dout'} must be contiguous bf16")
    if row_start.dtype != torch.int32 or row_start.dim() != 1 or row_start.numel() < 1 or not row_start.is_contiguous():
        raise RuntimeError(f"{who}: row_start must be contiguous int32 [batch + 1], got {row_start.dtype} {tuple(row_start.shape)}")
    if qkv.dim() != 2 or qkv.shape[1] != 3 * width or any(t.device != qkv.device for t, _ in tensors) or \
            (dout is not None and tuple(dout.shape) != (qkv.shape[0], width)):
        raise RuntimeError(f"{who}: qkv must be [rows, {3 * width}]{'' if dout is None else f', dout [rows, {width}]'} and row_start on the "
                           f"same device, got {[tuple(t.shape) for t, _ in tensors]} on {[str(t.device) for t, _ in tensors]}")


def _check_packed_out(who: str, out: torch.Tensor, qkv: torch.Tensor, shape: Tuple[int, ...]) -> None:
    if out.dtype != torch.bfloat16 or not out.is_contiguous() or out.device != qkv.device or tuple(out.shape) != tuple(shape):
        raise RuntimeError(f"{who}: out must be contiguous bf16 {tuple(shape)} on qkv's device, got {out.dtype} {tuple(out.shape)} on {out.device}")


def op_attention_packed(qkv: torch.Tensor, row_start: torch.Tensor, max_t: int, width: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Causal attention over packed items (``kemr_op_attention_packed``): qkv bf16 [rows, 3 width] (q pre-scaled by 1/8), row_start
    int32 [batch + 1] on the same device, item b = rows row_start[b] .. row_start[b + 1] - 1, every length in 1 .. max_t <= 288 ->
    bf16 [rows, width].  The caller's row_start must stay inside ``rows``: the library reads it on the device.  Rows no item owns are
    left as they are: as allocated, or as ``out`` (bf16 [rows, width], contiguous, for calls over sub-ranges of the items) has them."""
    _check_packed("op_attention_packed", qkv, row_start, width)
    if out is None:
        out = torch.empty((qkv.shape[0], width), dtype=torch.bfloat16, device=qkv.device)
    _check_packed_out("op_attention_packed", out, qkv, (qkv.shape[0], width))
    with torch.cuda.device(qkv.device):
        _lib.check(_lib.lib().kemr_op_attention_packed(C.c_void_p(qkv.data_ptr()), C.c_void_p(out.data_ptr()), C.c_void_p(row_start.data_ptr()),
                                                       row_start.numel() - 1, int(max_t), int(width), C.c_void_p(_stream_ptr(qkv.device))),
                   "op_attention_packed")
    return out


def attention_backward_packed(qkv: torch.Tensor, dout: torch.Tensor, row_start: torch.Tensor, max_t: int, width: int,
                              causal: bool, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The backward of op_attention_packed (``kemr_op_attention_backward_packed``; causal or not): qkv bf16 [rows, 3 width] as the
    forward read it, dout bf16 [rows, width], row_start int32 [batch + 1] -> dqkv bf16 [rows, 3 width], the gradient with respect to the
    planes as given (the caller owns the 1/8 of q).  Per item the bits of ``attention_backward(item rows, 1, length, ...)``; the same
    bits on every launch.  Rows no item owns are left as they are: as allocated, or as ``out`` (like qkv) has them."""
    _check_packed("attention_backward_packed", qkv, row_start, width, dout)
    dqkv = torch.empty_like(qkv) if out is None else out
    _check_packed_out("attention_backward_packed", dqkv, qkv, tuple(qkv.shape))
    with torch.cuda.device(qkv.device):
        _lib.check(_lib.lib().kemr_op_attention_backward_packed(C.c_void_p(qkv.data_ptr()), C.c_void_p(dout.data_ptr()),
                                                                C.c_void_p(dqkv.data_ptr()), C.c_void_p(row_start.data_ptr()),
                                                                row_start.numel() - 1, int(max_t), int(width), 1 if causal else 0,
                                                                C.c_void_p(_stream_ptr(qkv.device))), "op_attention_backward_packed")
    return dqkv


def layernorm_backward(x: torch.Tensor, gamma: torch.Tensor, dy: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The backward of op_layernorm: x fp32 [rows, width] as the forward read it, gamma fp32 [width], dy bf16 or fp32 [rows, width] ->
    (dx fp32 [rows, width], dgamma fp32 [width], dbeta fp32 [width]).  Mean and rstd are recomputed; no atomics, the same bits on every
    launch (``kemr_op_layernorm_backward``).  The workspace is a torch allocation on the current stream."""
    for t, what in ((x, "x"), (gamma, "gamma"), (dy, "dy")):
        _require_cuda(t, f"layernorm_backward: {what}")
    if x.dtype != torch.float32 or gamma.dtype != torch.float32 or dy.dtype not in (torch.bfloat16, torch.float32):
        raise RuntimeError("layernorm_backward: x and gamma must be fp32, dy bf16 or fp32")
    if x.dim() != 2 or tuple(dy.shape) != tuple(x.shape) or tuple(gamma.shape) != (x.shape[1],) or not (x.device == gamma.device == dy.device):
        raise RuntimeError(f"layernorm_backward: x and dy must be [rows, width] and gamma [width] on one device, got {tuple(x.shape)}, "
                           f"{tuple(dy.shape)} and {tuple(gamma.shape)}")
    if not (x.is_contiguous() and gamma.is_contiguous() and dy.is_contiguous()):
        raise RuntimeError("layernorm_backward: x, gamma and dy must be contiguous")
    L = _lib.lib()
    rows, width = x.shape
    dx = torch.empty_like(x)
    if rows == 0:                                        # an empty tensor has no address to hand over; the op's own answer for no rows
        return dx, torch.zeros_like(gamma), torch.zeros_like(gamma)
    dgamma, dbeta = torch.empty_like(gamma), torch.empty_like(gamma)
    need =int(L.kemr_layernorm_backward_workspace_bytes(rows, width))
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(L.kemr_op_layernorm_backward(C.c_void_p(x.data_ptr()), C.c_void_p(gamma.data_ptr()), C.c_void_p(dy.data_ptr()),
                                                _lib.KEMR_BF16 if dy.dtype == torch.bfloat16 else _lib.KEMR_F32,
                                                C.c_void_p(dx.data_ptr()), C.c_void_p(dgamma.data_ptr()), C.c_void_p(dbeta.data_ptr()),
                                                rows, width, C.c_void_p(ws.data_ptr()), need, C.c_void_p(_stream_ptr(x.device))),
                   "op_layernorm_backward")
    return dx, dgamma, dbeta


ACT_KINDS = {"quick_gelu": 0, "gelu": 1}


def _act_args(what: str, kind, *tensors: torch.Tensor) -> int:
    k = ACT_KINDS.get(kind, kind)
    if k not in (0, 1):
        raise RuntimeError(f"{what}: kind must be 'quick_gelu' (0) or 'gelu' (1), got {kind!r}")
    for t in tensors:
        _require_cuda(t, what)
        if t.dtype != torch.bfloat16 or not t.is_contiguous():
            raise RuntimeError(f"{what}: the buffers must be contiguous bf16")
        if tuple(t.shape) != tuple(tensors[0].shape) or t.device != tensors[0].device:
            raise RuntimeError(f"{what}: the buffers must have one shape on one device, got {[tuple(u.shape) for u in tensors]}")
    if tensors[0].numel() % 8:
        raise RuntimeError(f"{what}: {tensors[0].numel()} elements are not a multiple of 8")
    return k


def act_forward(pre: torch.Tensor, kind) -> torch.Tensor:
    """bf16 pre-activation -> bf16(f(float(pre))), f = QuickGELU ('quick_gelu', 0) or the exact GELU ('gelu', 1): ``kemr_op_act_forward``."""
    k = _act_args("act_forward", kind, pre)
    out = torch.empty_like(pre)
    with torch.cuda.device(pre.device):
        _lib.check(_lib.lib().kemr_op_act_forward(C.c_void_p(pre.data_ptr()), C.c_void_p(out.data_ptr()), pre.numel(), k,
                                                  C.c_void_p(_stream_ptr(pre.device))), "op_act_forward")
    return out


def act_backward(pre: torch.Tensor, dout: torch.Tensor, kind) -> torch.Tensor:
    """The backward of act_forward: bf16(float(dout) f'(float(pre))) (``kemr_op_act_backward``)."""
    k = _act_args("act_backward", kind, pre, dout)
    dpre = torch.empty_like(pre)
    with torch.cuda.device(pre.device):
        _lib.check(_lib.lib().kemr_op_act_backward(C.c_void_p(pre.data_ptr()), C.c_void_p(dout.data_ptr()), C.c_void_p(dpre.data_ptr()),
                                                   pre.numel(), k, C.c_void_p(_stream_ptr(pre.device))), "op_act_backward")
    return dpre


def op_layernorm_x3(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor) -> torch.Tensor:
    """fp32 [rows, width] -> the A-side triple [hi | lo | hi] of LayerNorm(x): bf16 [ceil256(rows), 3 width], pad rows zero."""
    L = _lib.lib()
    rows, width = x.shape
    y = torch.full((rows_alloc(rows), 3 * width), float("nan"), dtype=torch.bfloat16, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(L.kemr_op_layernorm_x3(C.c_void_p(x.data_ptr()), C.c_void_p(gamma.data_ptr()), C.c_void_p(beta.data_ptr()),
                                          C.c_void_p(y.data_ptr()), rows, width, C.c_void_p(_stream_ptr(x.device))), "op_layernorm_x3")
    return y


def op_gemm_x3(a_panel: torch.Tensor, w_panel: torch.Tensor, bias: Optional[torch.Tensor], m: int, mode: int,
               c: Optional[torch.Tensor] = None) -> torch.Tensor:
    """a_panel bf16 [ceil256(m), 3k] (build_panel(..., SIDE_QUERY, 3).data), w_panel bf16 [>= n, 3k] (SIDE_GALLERY; n = its row count
    unless `c` says otherwise).  mode 0: fp32 [m, n] = acc + bias; 1: c += acc + bias (c required); 2 / 3: the A-side triple
    bf16 [ceil256(m), 3n] of quick_gelu / gelu(acc + bias), rows m .. left as allocated (zero)."""
    L = _lib.lib()
    n, k3 = w_panel.shape
    if c is None:
        if mode == 1:
            raise RuntimeError("op_gemm_x3: mode 1 accumulates into a given c")
        c = (torch.zeros((m, n), dtype=torch.float32, device=a_panel.device) if mode == 0 else
             torch.zeros((rows_alloc(m), 3 * n), dtype=torch.bfloat16, device=a_panel.device))
    elif mode < 2:
        n = c.shape[1]
    with torch.cuda.device(a_panel.device):
        _lib.check(L.kemr_op_gemm_x3(C.c_void_p(a_panel.data_ptr()), C.c_void_p(w_panel.data_ptr()), _opt_ptr(bias), C.c_void_p(c.data_ptr()),
                                     m, n, k3, mode, C.c_void_p(_stream_ptr(a_panel.device))), "op_gemm_x3")
    return c


def op_attention_x3(qkv: torch.Tensor, batch: int, t: int, width: int, causal: bool, row_start: Optional[torch.Tensor] = None,
                    head_dim: int = 64) -> torch.Tensor:
    """qkv fp32 [rows, 3 width] (q pre-scaled) -> the A-side triple bf16 [rows, 3 width] of the attention output.  row_start (int32
    [batch + 1] on the device): packed causal items of at most t rows.  head_dim 64, or 80 (non-causal, no packed rows, t <= 288)."""
    L = _lib.lib()
    out = torch.zeros((qkv.shape[0], 3 * width), dtype=torch.bfloat16, device=qkv.device)
    with torch.cuda.device(qkv.device):
        if head_dim == 64:
            _lib.check(L.kemr_op_attention_x3(C.c_void_p(qkv.data_ptr()), C.c_void_p(out.data_ptr()), _opt_ptr(row_start), batch, t, width,
                                              1 if causal else 0, C.c_void_p(_stream_ptr(qkv.device))), "op_attention_x3")
        else:
            _lib.check(L.kemr_op_attention_x3_hd(C.c_void_p(qkv.data_ptr()), C.c_void_p(out.data_ptr()), _opt_ptr(row_start), batch, t, width,
                                                 int(head_dim), 1 if causal else 0, C.c_void_p(_stream_ptr(qkv.device))), "op_attention_x3_hd")
    return out


# ------------------------------------------------------------------------------------------------ fused InfoNCE (csrc/infonce.hip)
def _infonce_args(a: torch.Tensor, b: torch.Tensor, what: str) -> Tuple[int, int]:
    _require_cuda(a, f"{what}: features_a")
    _require_cuda(b, f"{what}: features_b")
    if a.dim() != 2 or a.shape != b.shape or a.device != b.device:
        raise RuntimeError(f"{what}: features must be two [n, d] tensors on one device, got {tuple(a.shape)} and {tuple(b.shape)}")
    if a.dtype != torch.float32 or b.dtype != torch.float32 or not a.is_contiguous() or not b.is_contiguous():
        raise RuntimeError(f"{what}: features must be contiguous fp32")
    return int(a.shape[0]), int(a.shape[1])


def infonce_workspace_bytes(n: int, d: int) -> int:
    need = int(_lib.lib().kemr_infonce_workspace_bytes(n, d))
    if need == 0:
        raise RuntimeError(f"infonce: n={n} must be in 1..65536 and d={d} a multiple of 4 in 4..1280")
    return need


def infonce_forward(a: torch.Tensor, b: torch.Tensor, temperature: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """(losses fp32 [3] = loss, loss_a2b, loss_b2a; lse fp32 [2 n] = row lse, column lse) of z = a b^T / temperature; z is never stored."""
    n, d = _infonce_args(a, b, "infonce_forward")
    ws = torch.empty(infonce_workspace_bytes(n, d), dtype=torch.uint8, device=a.device)
    loss = torch.empty(3, dtype=torch.float32, device=a.device)
    lse = torch.empty(2 * n, dtype=torch.float32, device=a.device)
    with torch.cuda.device(a.device):
        _lib.check(_lib.lib().kemr_infonce_forward(C.c_void_p(a.data_ptr()), C.c_void_p(b.data_ptr()), n, d, 1.0 / float(temperature),
                                                   C.c_void_p(loss.data_ptr()), C.c_void_p(lse.data_ptr()), C.c_void_p(ws.data_ptr()),
                                                   ws.numel(), C.c_void_p(_stream_ptr(a.device))), "infonce_forward")
    return loss, lse


def infonce_backward(a: torch.Tensor, b: torch.Tensor, lse: torch.Tensor, temperature: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """(d loss / d a, d loss / d b), fp32 [n, d] each, from the lse values infonce_forward saved."""
    n, d = _infonce_args(a, b, "infonce_backward")
    _require_cuda(lse, "infonce_backward: lse")
    if lse.dtype != torch.float32 or lse.numel() != 2 * n or not lse.is_contiguous():
        raise RuntimeError("infonce_backward: lse must be the contiguous fp32 [2 n] tensor of infonce_forward")
    ws = torch.empty(infonce_workspace_bytes(n, d), dtype=torch.uint8, device=a.device)
    ga, gb = torch.empty_like(a), torch.empty_like(b)
    with torch.cuda.device(a.device):
        _lib.check(_lib.lib().kemr_infonce_backward(C.c_void_p(a.data_ptr()), C.c_void_p(b.data_ptr()), C.c_void_p(lse.data_ptr()), n, d,
                                                    1.0 / float(temperature), C.c_void_p(ga.data_ptr()), C.c_void_p(gb.data_ptr()),
                                                    C.c_void_p(ws.data_ptr()), ws.numel(), C.c_void_p(_stream_ptr(a.device))),
                   "infonce_backward")
    return ga, gb


# ------------------------------------------------------------------------------------------------ fused pair-score contrastive loss (csrc/pairhead.hip)
def _pairhead_args(mode: int, q: torch.Tensor, img: torch.Tensor, tgt: torch.Tensor, gate, linear, what: str):
    """Checks of both pairhead calls; returns (n, d, hidden, the five head pointers as c_void_p)."""
    for t, name in ((q, "q"), (img, "img"), (tgt, "tgt")):
        _require_cuda(t, f"{what}: {name}")
    if q.dim() != 2 or q.shape != img.shape or q.shape != tgt.shape or q.device != img.device or q.device != tgt.device:
        raise RuntimeError(f"{what}: q, img, tgt must be three [n, d] tensors on one device, got {tuple(q.shape)}, {tuple(img.shape)}, "
                           f"{tuple(tgt.shape)}")
    heads = []
    if mode == _lib.PAIRHEAD_GATED:
        if gate is None or linear is not None:
            raise RuntimeError(f"{what}: the gated mode takes gate= (fp32 [n]) and no linear=")
        heads, shapes, hidden = [gate], [(q.shape[0],)], 0
    elif mode == _lib.PAIRHEAD_LINEAR:
        if linear is None or gate is not None or len(linear) != 4:
            raise RuntimeError(f"{what}: the linear mode takes linear=(w0 [hidden, 2], b0 [hidden], w1 [hidden], b1 [1]) and no gate=")
        heads, hidden = list(linear), int(linear[1].numel())
        shapes = [(hidden, 2), (hidden,), (hidden,), (1,)]
    else:
        raise RuntimeError(f"{what}: mode={mode} is neither PAIRHEAD_GATED nor PAIRHEAD_LINEAR")
    for t in [q, img, tgt] + heads:
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise RuntimeError(f"{what}: every tensor must be contiguous fp32")
    for t, shape in zip(heads, shapes):
        _require_cuda(t, f"{what}: head parameters")
        if tuple(t.shape) != shape or t.device != q.device:
            raise RuntimeError(f"{what}: a head tensor has shape {tuple(t.shape)}, expected {shape} on {q.device}")
    ptr = [C.c_void_p(t.data_ptr()) for t in heads]
    ptrs = ptr + [None] * 4 if mode == _lib.PAIRHEAD_GATED else [None] + ptr
    return int(q.shape[0]), int(q.shape[1]), hidden, ptrs


def pairhead_workspace_bytes(mode: int, n: int, d: int, hidden: int = 0) -> int:
    need = int(_lib.lib().kemr_pairhead_workspace_bytes(mode, n, d, hidden))
    if need == 0:
        raise RuntimeError(f"pairhead: mode={mode} must be 0 (gated) or 1 (linear), n={n} in 1..65536, d={d} a multiple of 4 in 4..1280 "
                           f"and, for the linear head, hidden={hidden} in 1..256")
    return need


def pairhead_forward(mode: int, q: torch.Tensor, img: torch.Tensor, tgt: torch.Tensor, temperature: float, gate=None, linear=None
                     ) -> Tuple[torch.Tensor, torch.Tensor]:
    """(losses fp32 [3] = loss, loss_q2g, loss_g2q; lse fp32 [2 n]) of the symmetric InfoNCE over S = head(q, img, tgt) / temperature
    (``kemr_pairhead_forward``); S is never stored.  ``gate`` fp32 [n] (PAIRHEAD_GATED) or ``linear`` = (w0, b0, w1, b1) (PAIRHEAD_LINEAR)."""
    n, d, hidden, hp = _pairhead_args(mode, q, img, tgt, gate, linear, "pairhead_forward")
    ws = torch.empty(pairhead_workspace_bytes(mode, n, d, hidden), dtype=torch.uint8, device=q.device)
    loss = torch.empty(3, dtype=torch.float32, device=q.device)
    lse = torch.empty(2 * n, dtype=torch.float32, device=q.device)
    with torch.cuda.device(q.device):
        _lib.check(_lib.lib().kemr_pairhead_forward(mode, C.c_void_p(q.data_ptr()), C.c_void_p(img.data_ptr()), C.c_void_p(tgt.data_ptr()), n, d,
                                                    1.0 / float(temperature), *hp, hidden, C.c_void_p(loss.data_ptr()),
                                                    C.c_void_p(lse.data_ptr()), C.c_void_p(ws.data_ptr()), ws.numel(),
                                                    C.c_void_p(_stream_ptr(q.device))), "pairhead_forward")
    return loss, lse


def pairhead_backward(mode: int, q: torch.Tensor, img: torch.Tensor, tgt: torch.Tensor, lse: torch.Tensor, temperature: float, gate=None,
                      linear=None) -> torch.Tensor:
    """The gradient of pairhead_forward's `loss` from the lse values it saved: fp32 [n] = dL/dgate (PAIRHEAD_GATED) or fp32
    [4 hidden + 1] = dL/dw0 | dL/db0 | dL/dw1 | dL/db1 (PAIRHEAD_LINEAR)."""
    n, d, hidden, hp = _pairhead_args(mode, q, img, tgt, gate, linear, "pairhead_backward")
    _require_cuda(lse, "pairhead_backward: lse")
    if lse.dtype != torch.float32 or lse.numel() != 2 * n or not lse.is_contiguous():
        raise RuntimeError("pairhead_backward: lse must be the contiguous fp32 [2 n] tensor of pairhead_forward")
    ws = torch.empty(pairhead_workspace_bytes(mode, n, d, hidden), dtype=torch.uint8, device=q.device)
    grad = torch.empty(n if mode == _lib.PAIRHEAD_GATED else 4 * hidden + 1, dtype=torch.float32, device=q.device)
    with torch.cuda.device(q.device):
        _lib.check(_lib.lib().kemr_pairhead_backward(mode, C.c_void_p(q.data_ptr()), C.c_void_p(img.data_ptr()), C.c_void_p(tgt.data_ptr()),
                                                     C.c_void_p(lse.data_ptr()), n, d, 1.0 / float(temperature), *hp, hidden,
                                                     C.c_void_p(grad.data_ptr()), C.c_void_p(ws.data_ptr()), ws.numel(),
                                                     C.c_void_p(_stream_ptr(q.device))), "pairhead_backward")
    return grad
