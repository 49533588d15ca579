"""`clip.tokenize` for the build: byte-level BPE of openai/CLIP, restated from its published algorithm.

The reference calls ``clip.tokenize(texts, truncate=True)`` (/root/reference/src/clip/eval/evaluator_baseline.py:112,118;
src/clip/eval/evaluator.py:126,132) and feeds the ``[B, 77]`` ids to ``encode_text``.  The tokenizer needs the merge
table ``bpe_simple_vocab_16e6.txt.gz`` that ships with the ``clip`` package; it is not part of this repository (no
network in the build container).  It is looked up in this order:

1. ``$KEMR_BPE_VOCAB``, 2. ``<this package>/bpe_simple_vocab_16e6.txt.gz``, 3. ``<repo>/clip/bpe_simple_vocab_16e6.txt.gz``,
4. ``~/.cache/clip/bpe_simple_vocab_16e6.txt.gz``.

Without the table a deterministic **hash tokenizer** is used (word -> stable id in [1, SOT)), with a warning: ids are
then not OpenAI's, which is fine for synthetic benchmarking / plumbing tests and wrong for pretrained weights.
``ftfy`` is not installed here; text cleaning is ``html.unescape`` + whitespace collapse + lower-casing.
"""
from __future__ import annotations

import gzip
import hashlib
import html
import os
import warnings
from functools import lru_cache
from typing import List, Sequence, Union

import regex as re
import torch

SOT, EOT, CONTEXT = 49406, 49407, 77
_PAT = re.compile(r"""<\|startoftext\|>|<\|endoftext\|>|'s|'t|'re|'ve|'m|'ll|'d|[\p{L}]+|[\p{N}]|[^\s\p{L}\p{N}]+""",
                  re.IGNORECASE)


def _vocab_candidates():
    here = os.path.dirname(os.path.abspath(__file__))
    name = "bpe_simple_vocab_16e6.txt.gz"
    env = os.environ.get("KEMR_BPE_VOCAB")
    return [p for p in (env, os.path.join(here, name), os.path.join(os.path.dirname(here), "clip", name),
                        os.path.expanduser(os.path.join("~", ".cache", "clip", name))) if p]


def find_vocab():
    for p in _vocab_candidates():
        if os.path.exists(p):
            return p
    return None


@lru_cache()
def bytes_to_unicode():
    bs = list(range(ord("!"), ord("~") + 1)) + list(range(ord("¡"), ord("¬") + 1)) + list(range(ord("®"), ord("ÿ") + 1))
    cs = bs[:]
    n = 0
    for b in range(2 ** 8):
        if b not in bs:
            bs.append(b)
            cs.append(2 ** 8 + n)
            n += 1
    return dict(zip(bs, [chr(c) for c in cs]))


def _pairs(word):
    return set(zip(word[:-1], word[1:]))


def clean(text: str) -> str:
    text = html.unescape(html.unescape(text)).strip()
    return re.sub(r"\s+", " ", text).strip().lower()


class BPETokenizer:
    """Byte-level BPE with the 49 408-entry CLIP vocabulary (256 bytes, 256 end-of-word bytes, merges, 2 specials)."""

    def __init__(self, bpe_path: str):
        self.path = bpe_path
        self.byte_encoder = bytes_to_unicode()
        merges = gzip.open(bpe_path).read().decode("utf-8").split("\n")
        merges = [tuple(m.split()) for m in merges[1:49152 - 256 - 2 + 1]]
        vocab = list(self.byte_encoder.values())
        vocab = vocab + [v + "</w>" for v in vocab]
        vocab.extend("".join(m) for m in merges)
        vocab.extend(["<|startoftext|>", "<|endoftext|>"])
        self.encoder = dict(zip(vocab, range(len(vocab))))
        self.bpe_ranks = dict(zip(merges, range(len(merges))))
        self.cache = {"<|startoftext|>": "<|startoftext|>", "<|endoftext|>": "<|endoftext|>"}

    def bpe(self, token: str) -> str:
        if token in self.cache:
            return self.cache[token]
        word = tuple(token[:-1]) + (token[-1] + "</w>",)
        pairs = _pairs(word)
        if not pairs:
            return token + "</w>"
        while True:
            bigram = min(pairs, key=lambda p: self.bpe_ranks.get(p, float("inf")))
            if bigram not in self.bpe_ranks:
                break
            first, second = bigram
            new, i = [], 0
            while i < len(word):
                try:
                    j = word.index(first, i)
                except ValueError:
                    new.extend(word[i:])
                    break
                new.extend(word[i:j])
                i = j
                if word[i] == first and i < len(word) - 1 and word[i + 1] == second:
                    new.append(first + second)
                    i += 2
                else:
                    new.append(word[i])
                    i += 1
            word = tuple(new)
            if len(word) == 1:
                break
            pairs = _pairs(word)
        out = " ".join(word)
        self.cache[token] = out
        return out

    def encode(self, text: str) -> List[int]:
        ids: List[int] = []
        for tok in re.findall(_PAT, clean(text)):
            tok = "".join(self.byte_encoder[b] for b in tok.encode("utf-8"))
            ids.extend(self.encoder[t] for t in self.bpe(tok).split(" "))
        return ids


class HashTokenizer:
    """Offline stand-in: one stable id per word piece (NOT OpenAI's ids; see module docstring)."""

    def encode(self, text: str) -> List[int]:
        out = []
        for tok in re.findall(_PAT, clean(text)):
            h = int.from_bytes(hashlib.blake2s(tok.encode("utf-8"), digest_size=4).digest(), "little")
            out.append(1 + h % (SOT - 1))
        return out


_tokenizer = None
_allow_hash = False


def allow_hash_tokenizer(flag: bool = True) -> None:
    """Opt in to the hash tokenizer when the BPE vocabulary is absent (synthetic-data runs, tests)."""
    global _allow_hash
    _allow_hash = bool(flag)


def hash_tokenizer_allowed() -> bool:
    return _allow_hash or os.environ.get("KEMR_ALLOW_HASH_TOKENIZER", "") == "1"


def get_tokenizer():
    """The BPE tokenizer when its vocabulary file is found; without it: an error, unless the hash tokenizer was allowed
    explicitly (its ids are not OpenAI's: text embeddings of a pretrained model would be meaningless)."""
    global _tokenizer
    if _tokenizer is None or (isinstance(_tokenizer, HashTokenizer) and not hash_tokenizer_allowed()):
        path = find_vocab()
        if path:
            _tokenizer = BPETokenizer(path)
        elif hash_tokenizer_allowed():
            warnings.warn("CLIP BPE vocabulary not found (%s): using the deterministic hash tokenizer (explicitly allowed); "
                          "token ids are not OpenAI's" % ", ".join(_vocab_candidates()), RuntimeWarning, stacklevel=2)
            _tokenizer = HashTokenizer()
        else:
            raise FileNotFoundError(
                "CLIP BPE vocabulary not found (%s).  Put bpe_simple_vocab_16e6.txt.gz there, or opt in to the hash tokenizer "
                "(synthetic-data runs: --synthetic, tokenizer.allow_hash_tokenizer(), KEMR_ALLOW_HASH_TOKENIZER=1)"
                % ", ".join(_vocab_candidates()))
    return _tokenizer


def tokenizer_name() -> str:
    t = get_tokenizer()
    return "bpe(%s)" % t.path if isinstance(t, BPETokenizer) else "hash (NOT OpenAI ids)"


def tokenize(texts: Union[str, Sequence[str]], context_length: int = CONTEXT, truncate: bool = False) -> torch.Tensor:
    """-> int32 [len(texts), context_length]: SOT, ids..., EOT, zero padding; over-long inputs are cut and end in EOT
    when ``truncate`` else raise (upstream ``clip.tokenize`` contract)."""
    if isinstance(texts, str):
        texts = [texts]
    tok = get_tokenizer()
    out = torch.zeros(len(texts), context_length, dtype=torch.int32)
    for i, text in enumerate(texts):
        ids = [SOT] + tok.encode(text) + [EOT]
        if len(ids) > context_length:
            if not truncate:
                raise RuntimeError(f"Input {text} is too long for context length {context_length}")
            ids = ids[:context_length]
            ids[-1] = EOT
        out[i, :len(ids)] = torch.tensor(ids, dtype=torch.int32)
    return out


class ClipTokenize:
    """``tokenize_fn`` of a CLIP-family model whose text tower is not 77 positions long (Long-CLIP: 248): CLIP's BPE with
    ``context_length`` positions, over-long texts cut and ended in EOT -> int32 ``[B, context_length]``.  A module-level class with one
    integer of state: picklable, so it survives the loader workers' start method."""

    def __init__(self, context_length: int):
        self.context_length = int(context_length)

    def __call__(self, texts: Union[str, Sequence[str]]) -> torch.Tensor:
        return tokenize([texts] if isinstance(texts, str) else list(texts), context_length=self.context_length, truncate=True)

    def __eq__(self, other):
        return isinstance(other, ClipTokenize) and other.context_length == self.context_length

    def __hash__(self):
        return hash(("ClipTokenize", self.context_length))


# ---- SigLIP: a callable for the `tokenize_fn=` parameters (evaluators, EmbeddingStore.build, CLIPRetriever) -------------------------
SIGLIP_CONTEXT = 64
SIGLIP_EOS = 1          # "</s>"; the pad id as well (SigLIP pads with it, and a pad position is a key like every other)


def siglip_canonicalize(text: str) -> str:
    """``SiglipTokenizer.canonicalize_text``: lower-case, ``string.punctuation`` removed, whitespace collapsed and stripped."""
    import string
    text = text.lower().translate(str.maketrans("", "", string.punctuation))
    return re.sub(r"\s+", " ", text).strip()


class SiglipTokenize:
    """``tokenize_fn`` of a SigLIP checkpoint directory: canonicalise, encode with the ``tokenizers`` package from the directory's
    ``tokenizer.json``, append the end-of-sequence id 1, cut to ``context_length`` keeping that id, pad with id 1 -> int32
    ``[B, context_length]``.  Picklable (loader workers): the ``tokenizers`` object is rebuilt from the path on first use.
    ``sentencepiece`` is not a dependency: a directory that holds only ``spiece.model`` cannot be read."""

    def __init__(self, directory: str, context_length: int = SIGLIP_CONTEXT):
        path = os.path.join(directory, "tokenizer.json") if os.path.isdir(directory) else directory
        if not os.path.isfile(path):
            if os.path.isfile(os.path.join(os.path.dirname(path), "spiece.model")):
                raise FileNotFoundError(f"{directory!r} holds spiece.model but no tokenizer.json: reading a SentencePiece model needs the "
                                        "sentencepiece package, which this build does not depend on.  Save the fast tokenizer "
                                        "(tokenizer.json) next to it, or pass pre-tokenised ids")
            raise FileNotFoundError(f"{path!r} does not exist (a SigLIP directory's tokenizer.json)")
        self.path, self.context_length = path, int(context_length)
        self._tok = None

    def __getstate__(self):
        return {"path": self.path, "context_length": self.context_length, "_tok": None}

    def _tokenizer(self):
        if self._tok is None:
            from tokenizers import Tokenizer
            tok = Tokenizer.from_file(self.path)
            tok.no_padding()
            tok.no_truncation()
            self._tok = tok
        return self._tok

    def __call__(self, texts: Union[str, Sequence[str]]) -> torch.Tensor:
        if isinstance(texts, str):
            texts = [texts]
        n = self.context_length
        out = torch.full((len(texts), n), SIGLIP_EOS, dtype=torch.int32)
        tok = self._tokenizer()
        for i, t in enumerate(texts):
            ids = tok.encode(siglip_canonicalize(t), add_special_tokens=False).ids
            ids = [j for j in ids if j != SIGLIP_EOS][: n - 1] + [SIGLIP_EOS]
            out[i, : len(ids)] = torch.tensor(ids, dtype=torch.int32)
        return out


def siglip_tokenizer(directory: str, context_length: int = SIGLIP_CONTEXT) -> SiglipTokenize:
    return SiglipTokenize(directory, context_length)


# ---- BERT sentence encoders (E5, GTE): WordPiece from the directory's tokenizer.json ------------------------------------------------
class BertTokenize:
    """Tokenizer of a BERT checkpoint directory: the ``tokenizers`` package on the directory's ``tokenizer.json`` (its normaliser,
    WordPiece model and ``[CLS] ... [SEP]`` post-processor as saved), truncated to ``max_length`` keeping ``[SEP]`` -> (ids int32
    ``[B, max_length]`` zero-padded, lengths int32 ``[B]``).  The lengths ARE the padding mask: the engine computes a text on its first
    ``lens[i]`` positions only.  Picklable: the ``tokenizers`` object is rebuilt from the path on first use."""

    def __init__(self, directory: str, max_length: int = 512):
        path = os.path.join(directory, "tokenizer.json") if os.path.isdir(directory) else directory
        if not os.path.isfile(path):
            raise FileNotFoundError(f"{path!r} does not exist (a BERT directory's tokenizer.json; vocab.txt alone is not read)")
        if not 2 <= int(max_length) <= 512:
            raise ValueError(f"bert_tokenizer: max_length {max_length} not in 2..512")
        self.path, self.max_length = path, int(max_length)
        self._tok = None

    def __getstate__(self):
        return {"path": self.path, "max_length": self.max_length, "_tok": None}

    def _tokenizer(self):
        if self._tok is None:
            from tokenizers import Tokenizer
            tok = Tokenizer.from_file(self.path)
            tok.no_padding()
            tok.enable_truncation(max_length=self.max_length)
            self._tok = tok
        return self._tok

    def encode_lists(self, texts: Sequence[str]):
        """The id lists themselves (ragged), for callers that sort by length before they pad."""
        return [e.ids for e in self._tokenizer().encode_batch([str(t) for t in texts], add_special_tokens=True)]

    def __call__(self, texts: Union[str, Sequence[str]]):
        if isinstance(texts, str):
            texts = [texts]
        return pad_id_lists(self.encode_lists(texts), self.max_length)


def pad_id_lists(id_lists, max_length: int):
    """Ragged id lists -> (int32 [B, max_length] zero-padded, int32 [B] lengths); an empty list counts as one pad token."""
    out = torch.zeros(len(id_lists), max_length, dtype=torch.int32)
    lens = torch.ones(len(id_lists), dtype=torch.int32)
    for i, ids in enumerate(id_lists):
        if len(ids) > max_length:
            raise RuntimeError(f"{len(ids)} ids for {max_length} positions")
        if ids:
            out[i, : len(ids)] = torch.tensor(ids, dtype=torch.int32)
            lens[i] = len(ids)
    return out, lens


def bert_tokenizer(directory: str, max_length: int = 512) -> BertTokenize:
    return BertTokenize(directory, max_length)
