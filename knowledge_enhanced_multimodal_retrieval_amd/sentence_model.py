"""``SentenceTransformer``'s surface, as the reference's text-to-text baselines use it, on the HIP engine.

The reference loads ``intfloat/e5-base-v2`` and ``thenlper/gte-large`` through ``SentenceTransformer(name, device=...)`` and calls
``model.encode(texts, convert_to_tensor=True, device=device, show_progress_bar=False, normalize_embeddings=True)``
(reference: src/clip/eval/evaluator_lm.py:92-109, baselines/evaluate_text_models.py:142-150).  :class:`SentenceEncoder` takes those
calls: a local checkpoint directory in (``transformers`` or sentence-transformers layout), embeddings out, computed by
``BertEngine`` -- every text on its own length, packed (no padded positions are computed).

The reference's third sentence encoder, ``sentence-transformers/all-mpnet-base-v2`` (``transformers.MPNetModel``), loads the same way:
its learned relative position bias rides in the packed attention kernel's score accumulators (model family 3 of the library).  The
engine places token j of a text at position j, which is what MPNet's position ids (built from the non-pad ids) give whenever no
``<pad>`` id occurs inside a text's length -- tokenizers never emit one there; a text that held one would differ from Hugging Face.

Local files only.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Union

import numpy as np
import torch

from . import _lib
from .config import BertArch
from .engine import BertEngine
from .hf_checkpoint import read_sentence_directory
from .tokenizer import bert_tokenizer, pad_id_lists


def length_sorted_order(lengths: Sequence[int]) -> List[int]:
    """The order ``SentenceTransformer.encode`` works in: longest text first (stable: equal lengths keep their input order)."""
    return sorted(range(len(lengths)), key=lambda i: -lengths[i])


class SentenceEncoder:
    """A BERT or MPNet sentence encoder on the GPU with ``SentenceTransformer.encode``'s contract."""

    def __init__(self, arch: BertArch, state_dict, tokenize, device=None, precision: str = _lib.DEFAULT_PRECISION):
        """`tokenize`: a ``tokenizer.BertTokenize`` (or any object with ``encode_lists(texts) -> list of id lists``, each at most
        ``arch.ctx`` long, special tokens included)."""
        self.arch, self.tokenize = arch, tokenize
        self.device = torch.device(device if device is not None else "cuda:0")
        self.engine = BertEngine(arch, self.device, precision)
        self.engine.load_state_dict(state_dict)
        self.max_seq_length = arch.ctx

    @classmethod
    def from_pretrained(cls, directory: str, device=None, precision: str = _lib.DEFAULT_PRECISION) -> "SentenceEncoder":
        """A ``save_pretrained`` directory of a ``BertModel`` or an ``MPNetModel`` (``config.json``, weights, ``tokenizer.json``),
        optionally with the sentence-transformers files ``1_Pooling/config.json`` and ``sentence_bert_config.json``."""
        arch, sd = read_sentence_directory(directory)
        return cls(arch, sd, bert_tokenizer(directory, arch.ctx), device, precision)

    # SentenceTransformer is an nn.Module: the reference calls .to(device) and .eval() on it
    def to(self, device=None, *args, **kw) -> "SentenceEncoder":
        if device is not None and torch.device(device).type == "cuda":
            d = torch.device(device)
            d = torch.device("cuda", d.index if d.index is not None else (self.device.index or 0))
            if d != self.device:
                raise RuntimeError(f"SentenceEncoder lives on {self.device}; load it there (from_pretrained(..., device=...)) instead of moving it to {d}")
        elif device is not None and not isinstance(device, torch.dtype):
            raise RuntimeError("SentenceEncoder runs on the GPU only; there is no CPU fallback")
        return self

    def eval(self) -> "SentenceEncoder":
        return self

    def get_sentence_embedding_dimension(self) -> int:
        return self.arch.width

    @torch.no_grad()
    def encode(self, sentences: Union[str, Sequence[str]], batch_size: int = 32, convert_to_tensor: bool = False,
               convert_to_numpy: bool = True, normalize_embeddings: bool = False, device=None, show_progress_bar: bool = False):
        """``SentenceTransformer.encode``: a string -> one vector, a list -> one row per sentence IN INPUT ORDER.  Returns a float32
        numpy array, a torch tensor on the model's device (``convert_to_tensor``), or a list of tensors (both flags off).  Inside, the
        sentences are sorted by length (longest first, as sentence-transformers does) and cut into calls of ``batch_size`` sentences
        or more -- the engine packs them, so ``batch_size`` is a lower bound, not a padding decision."""
        self.to(device)
        single = isinstance(sentences, str)
        texts = [sentences] if single else list(sentences)
        id_lists = self.tokenize.encode_lists(texts)
        order = length_sorted_order([len(x) for x in id_lists])
        ids, lens = pad_id_lists([id_lists[i] for i in order], self.arch.ctx)
        emb_sorted = self.engine.encode_ids(ids, lens, normalize=normalize_embeddings)
        emb = torch.empty_like(emb_sorted)
        if order:
            emb[torch.as_tensor(order, device=emb.device)] = emb_sorted
        if single:
            emb = emb[0]
        if convert_to_tensor:
            return emb
        if convert_to_numpy:
            return emb.cpu().numpy()
        return [emb] if single else list(emb)
