"""A CPU statement of the BERT sentence encoders (model family 2: ``transformers.BertModel`` without its pooler, then mean or CLS
pooling) on the engine's tensor names, and the fixtures the BERT tests share.  Not a test module; no GPU, no library.

``encode`` states what ``BertModel`` + sentence-transformers' pooling compute (tests/test_bert_host.py holds it to them).  Every text
is computed on its own ``lens[i]`` positions and nothing else -- a padding mask is a length -- so the result cannot depend on how far
a batch is padded.

The model fixture is ``BertConfig(vocab_size=1024, hidden_size=256, num_hidden_layers=2, num_attention_heads=4,
intermediate_size=1024, max_position_embeddings=512)`` with seeded random weights; ``save_directory`` writes it with
``save_pretrained`` and puts a small WordPiece ``tokenizer.json`` next to it.
"""
import json
import os

import torch
import torch.nn.functional as F

from knowledge_enhanced_multimodal_retrieval_amd import hf_checkpoint
from knowledge_enhanced_multimodal_retrieval_amd.config import BertArch

ARCH = BertArch(256, 2, vocab=1024, ctx=512)
EPS = 1e-12
# the edges of a 16-query tile, a 64-key chunk and a 128-query block, and the two extremes: 2 418 rows in one packed call
LENGTHS = [1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512]
SHUFFLED = [LENGTHS[i] for i in torch.randperm(len(LENGTHS), generator=torch.Generator().manual_seed(7)).tolist()]
CLS, SEP = 2, 3


def bert_config(arch=ARCH, positions=None):
    from transformers import BertConfig
    return BertConfig(vocab_size=arch.vocab, hidden_size=arch.width, num_hidden_layers=arch.layers, num_attention_heads=arch.heads,
                      intermediate_size=4 * arch.width, max_position_embeddings=positions or arch.ctx)


def tensor_shapes(arch=ARCH):
    w = arch.width
    shapes = {"token_embedding.weight": (arch.vocab, w), "positional_embedding": (arch.ctx, w), "token_type_embedding": (2, w),
              "ln_embed.weight": (w,), "ln_embed.bias": (w,)}
    for i in range(arch.layers):
        b = f"transformer.resblocks.{i}"
        shapes.update({f"{b}.attn.in_proj_weight": (3 * w, w), f"{b}.attn.in_proj_bias": (3 * w,), f"{b}.attn.out_proj.weight": (w, w),
                       f"{b}.attn.out_proj.bias": (w,), f"{b}.ln_1.weight": (w,), f"{b}.ln_1.bias": (w,),
                       f"{b}.mlp.c_fc.weight": (4 * w, w), f"{b}.mlp.c_fc.bias": (4 * w,), f"{b}.mlp.c_proj.weight": (w, 4 * w),
                       f"{b}.mlp.c_proj.bias": (w,), f"{b}.ln_2.weight": (w,), f"{b}.ln_2.bias": (w,)})
    return shapes


def random_state_dict(arch=ARCH, seed=0):
    """Seeded fp32 weights under the engine's names, scaled so that activations stay O(1) (the scales of tests/siglip_ref.py): matrices
    N(0, 1 / fan_in) -- the query and key rows 2 x that, so that the logits spread over a few units and the softmax is not flat; fc1
    1.5 x --, biases N(0, 0.1^2), LayerNorm gains 1 + N(0, 0.1^2), embeddings N(0, 0.5^2) (token_type_embedding too: a forgotten
    type-0 row must show)."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name, shape in tensor_shapes(arch).items():
        if name.endswith("ln_1.weight") or name.endswith("ln_2.weight") or name == "ln_embed.weight":
            t = 1.0 + 0.1 * torch.randn(shape, generator=g)
        elif name.endswith("bias"):
            t = 0.1 * torch.randn(shape, generator=g)
        elif name in ("token_embedding.weight", "positional_embedding", "token_type_embedding"):
            t = 0.5 * torch.randn(shape, generator=g)
        else:
            t = torch.randn(shape, generator=g) * shape[1] ** -0.5 * (1.5 if name.endswith("c_fc.weight") else 1.0)
            if name.endswith("in_proj_weight"):
                t[: 2 * arch.width] *= 2.0
        sd[name] = t
    return sd


def heavy_state_dict(arch=ARCH, seed=0):
    """``random_state_dict`` with the heavy tails of a trained tower, in the manner of oracle.clip_ref.add_outliers, for a post-LN
    model (every LayerNorm's output IS the residual stream, so its gains are the stream's channel scales): two massive channels of the
    embedding LayerNorm (gain x 20), in every block four channels of ln_1 and of ln_2 with their gain x U(3, 10), not compensated, and
    one sharp head (the query rows of head 0 x 4: near one-hot softmax rows)."""
    sd = {k: v.clone() for k, v in random_state_dict(arch, seed).items()}
    g = torch.Generator().manual_seed(seed * 7919 + 17)
    pick = lambda k: torch.randperm(arch.width, generator=g)[:k]           # noqa: E731
    sd["ln_embed.weight"][pick(2)] *= 20.0
    for i in range(arch.layers):
        b = f"transformer.resblocks.{i}"
        for nm in ("ln_1", "ln_2"):
            sd[f"{b}.{nm}.weight"][pick(4)] *= 3.0 + 7.0 * torch.rand(4, generator=g)
        sd[f"{b}.attn.in_proj_weight"][:64] *= 4.0
    return sd


def hf_model(sd, arch=ARCH, pooler=False):
    """``transformers.BertModel`` (eager attention, fp32, eval) holding the weights of `sd`."""
    from transformers import BertModel
    cfg = bert_config(arch)
    cfg._attn_implementation = "eager"
    model = BertModel(cfg, add_pooling_layer=pooler).eval()
    missing = model.load_state_dict(hf_checkpoint.to_bert_state_dict(sd, arch), strict=False)
    assert not missing.unexpected_keys and all(k.startswith("pooler.") or k.endswith("_ids") for k in missing.missing_keys), missing
    return model


def random_ids(lens, arch=ARCH, seed=1, pad_to=None):
    """[CLS] random ids [SEP] of the given lengths (a length-1 text is [CLS] alone), zero-padded to `pad_to` (default arch.ctx)."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.zeros(len(lens), pad_to or arch.ctx, dtype=torch.int32)
    for i, n in enumerate(lens):
        row = torch.randint(5, arch.vocab, (n,), generator=g, dtype=torch.int32)
        row[0] = CLS
        if n > 1:
            row[-1] = SEP
        ids[i, :n] = row
    return ids, torch.tensor(lens, dtype=torch.int32)


def _ln(x, sd, name, dtype):
    return F.layer_norm(x, (x.shape[-1],), sd[f"{name}.weight"].to(dtype), sd[f"{name}.bias"].to(dtype), EPS)


@torch.no_grad()
def hidden_states(sd, arch, ids_row, dtype=torch.float32):
    """The final rows [len, W] of ONE text given as its ids [len] (no padding exists here)."""
    p = lambda n: sd[n].to(dtype)                                      # noqa: E731
    n, w, heads = ids_row.numel(), arch.width, arch.heads
    x = p("token_embedding.weight")[ids_row.long()] + p("positional_embedding")[:n] + p("token_type_embedding")[0]
    x = _ln(x, sd, "ln_embed", dtype)
    for i in range(arch.layers):
        b = f"transformer.resblocks.{i}"
        q, k, v = (x @ p(f"{b}.attn.in_proj_weight").T + p(f"{b}.attn.in_proj_bias")).split(w, dim=-1)
        q, k, v = (t.view(n, heads, 64).transpose(0, 1) for t in (q, k, v))
        a = (torch.softmax(q @ k.transpose(-1, -2) / 8.0, dim=-1) @ v).transpose(0, 1).reshape(n, w)
        x = _ln(x + a @ p(f"{b}.attn.out_proj.weight").T + p(f"{b}.attn.out_proj.bias"), sd, f"{b}.ln_1", dtype)
        h = x @ p(f"{b}.mlp.c_fc.weight").T + p(f"{b}.mlp.c_fc.bias")
        h = 0.5 * h * (1.0 + torch.erf(h * 2.0 ** -0.5))
        x = _ln(x + h @ p(f"{b}.mlp.c_proj.weight").T + p(f"{b}.mlp.c_proj.bias"), sd, f"{b}.ln_2", dtype)
    return x


@torch.no_grad()
def encode(sd, arch, ids, lens, pooling="mean", normalize=False, dtype=torch.float32):
    """ids int [B, P] (P >= max(lens); what lies behind a text's length is never read), lens int [B] -> [B, W] in `dtype`."""
    out = []
    for row, n in zip(ids, torch.as_tensor(lens).tolist()):
        x = hidden_states(sd, arch, row[:n], dtype)
        e = x.sum(0) / n if pooling == "mean" else x[0]
        out.append(e / e.norm() if normalize else e)
    return torch.stack(out)


@torch.no_grad()
def hf_encode(model, ids, lens, pooling="mean"):
    """``BertModel`` on the padded batch with its attention mask, then sentence-transformers' pooling (mean: sum(h * mask) / sum(mask))."""
    p = ids.shape[1]
    mask = (torch.arange(p)[None, :] < torch.as_tensor(lens)[:, None]).long()
    h = model(input_ids=ids.long(), attention_mask=mask).last_hidden_state
    if pooling == "cls":
        return h[:, 0]
    m = mask[..., None].to(h.dtype)
    return (h * m).sum(1) / m.sum(1).clamp_min(1e-9)


def one_minus_cos(a, b):
    return 1.0 - F.cosine_similarity(a.double().cpu(), b.double().cpu(), dim=-1)


# ------------------------------------------------------------------------------------------------ checkpoint directory + tokenizer
_ONSETS, _VOWELS, _CODAS = "bdfgklmnprstvz", "aeiou", "lmnrstk"
WORDS = [o + v + c for o in _ONSETS for v in _VOWELS for c in _CODAS] + [o + v + c + "a" for o in _ONSETS[:7] for v in _VOWELS for c in _CODAS]
SUFFIXES = ["##s", "##ing", "##ed", "##er", "##ly"]


def vocabulary(arch=ARCH):
    """[PAD] [UNK] [CLS] [SEP] [MASK], then whole words and a few continuation pieces: fewer than arch.vocab entries."""
    vocab = {t: i for i, t in enumerate(["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"])}
    for w in WORDS + SUFFIXES:
        vocab[w] = len(vocab)
    assert len(vocab) <= arch.vocab and vocab["[CLS]"] == CLS and vocab["[SEP]"] == SEP
    return vocab


def write_tokenizer(directory, arch=ARCH):
    from tokenizers import Tokenizer, models, normalizers, pre_tokenizers, processors
    tok = Tokenizer(models.WordPiece(vocabulary(arch), unk_token="[UNK]"))
    tok.normalizer = normalizers.BertNormalizer(lowercase=True)
    tok.pre_tokenizer = pre_tokenizers.BertPreTokenizer()
    tok.post_processor = processors.TemplateProcessing(single="[CLS] $A [SEP]", pair="[CLS] $A [SEP] $B:1 [SEP]:1",
                                                       special_tokens=[("[CLS]", CLS), ("[SEP]", SEP)])
    tok.save(os.path.join(directory, "tokenizer.json"))


def save_directory(directory, sd, arch=ARCH, pooler=True, pooling=None, max_seq_length=None):
    """``BertModel.save_pretrained`` (with its pooler by default, as the published checkpoints have one) + tokenizer.json; `pooling`
    ("mean" / "cls") and `max_seq_length` add the sentence-transformers files."""
    directory = str(directory)
    hf_model(sd, arch, pooler=pooler).save_pretrained(directory)
    write_tokenizer(directory, arch)
    if pooling is not None:
        os.makedirs(os.path.join(directory, "1_Pooling"), exist_ok=True)
        with open(os.path.join(directory, "1_Pooling", "config.json"), "w") as f:
            json.dump({"word_embedding_dimension": arch.width, "pooling_mode_cls_token": pooling == "cls",
                       "pooling_mode_mean_tokens": pooling == "mean", "pooling_mode_max_tokens": False,
                       "pooling_mode_mean_sqrt_len_tokens": False}, f)
    if max_seq_length is not None:
        with open(os.path.join(directory, "sentence_bert_config.json"), "w") as f:
            json.dump({"max_seq_length": max_seq_length, "do_lower_case": True}, f)
    return directory


def sentences(n, seed=5, lo=3, hi=40):
    """n seeded sentences over WORDS (some words with a suffix, so that WordPiece continuation pieces occur), lo .. hi words each."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n):
        k = int(torch.randint(lo, hi + 1, (1,), generator=g))
        words = []
        for j in torch.randint(0, len(WORDS), (k,), generator=g).tolist():
            s = int(torch.randint(0, 12, (1,), generator=g))
            words.append(WORDS[j] + (SUFFIXES[s][2:] if s < len(SUFFIXES) else ""))
        out.append(" ".join(words).capitalize() + ".")
    return out


def toy_candidates(n=256, seed=9):
    """(queries, targets): target i repeats query i's words and adds a few, so that the diagonal is the intended match."""
    q = sentences(n, seed, 4, 10)
    extra = sentences(n, seed + 1, 2, 4)
    return q, [a.rstrip(".") + " " + b.lower() for a, b in zip(q, extra)]


def toy_set(sd, tokenize, n=64, margin=2e-3, arch=ARCH):
    """n (query, target) pairs picked from toy_candidates so that every oracle score keeps more than `margin` from its row's
    ground-truth score -- a rank comparison between the engine and the oracle then has no near-tie to trip over.  Greedy: a candidate
    joins when its scores against the members (both ways) respect the margin.  Returns (queries, targets, oracle query embeddings,
    oracle target embeddings), the embeddings L2-normalised fp32."""
    queries, targets = toy_candidates()
    qi, ql = tokenize(queries)
    ti, tl = tokenize(targets)
    q, t = encode(sd, arch, qi, ql, normalize=True), encode(sd, arch, ti, tl, normalize=True)
    s = q.double() @ t.double().T
    keep = []
    for c in range(len(queries)):
        ok = all(abs(float(s[i, c] - s[i, i])) > margin and abs(float(s[c, i] - s[c, c])) > margin for i in keep)
        if ok:
            keep.append(c)
        if len(keep) == n:
            break
    assert len(keep) == n, f"only {len(keep)} of {n} pairs with margin {margin}"
    return [queries[i] for i in keep], [targets[i] for i in keep], q[keep], t[keep]


def score_margin(query, target):
    """The smallest |s_ij - s_ii| over i and j != i of the cosine scores: what a rank comparison has to resolve."""
    s = F.normalize(query.double(), dim=-1) @ F.normalize(target.double(), dim=-1).T
    d = (s - s.diag()[:, None]).abs()
    d.fill_diagonal_(float("inf"))
    return float(d.min())


_cache = {}


def cached(key, fn):
    """Compute a reference once and share it among the tests that need it (left unchanged by every reader)."""
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]
