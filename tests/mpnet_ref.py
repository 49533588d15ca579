"""A CPU statement of the MPNet sentence encoders (model family 3: ``transformers.MPNetModel`` without its pooler, then mean or CLS
pooling) on the engine's tensor names, and the fixtures the MPNet tests share.  Not a test module; no GPU, no library.  Modelled on
tests/bert_ref.py, whose weights, sentences and toy set it reuses.

What differs from BERT: no token-type row, position j of a text reads row j + 2 of the checkpoint's positional table (the engine's
``positional_embedding`` holds rows 2 .. 2 + ctx - 1), every attention score gets ``bias[h][bucket(key - query)]`` from ONE
``relative_attention_bias`` [32, heads] for all layers, and the LayerNorm eps is the config's (1e-5 or 1e-12).

``encode`` computes every text on its own ``lens[i]`` positions.  It equals ``MPNetModel`` on a padded batch with its attention mask
whenever no ``<pad>`` id (1) occurs inside a text's length: Hugging Face builds position ids from the non-pad ids, the engine places
token j at position j.  ``random_ids`` never draws id 1.
"""
import json
import os

import torch
import torch.nn.functional as F

import bert_ref as B
from knowledge_enhanced_multimodal_retrieval_amd import hf_checkpoint
from knowledge_enhanced_multimodal_retrieval_amd.config import BertArch

EPS_PUBLISHED, EPS_DEFAULT = 1e-5, 1e-12
ARCH = BertArch(256, 2, vocab=1024, ctx=512, relative_bias=True, layer_norm_eps=EPS_PUBLISHED)
ARCH12 = BertArch(256, 2, vocab=1024, ctx=512, relative_bias=True, layer_norm_eps=EPS_DEFAULT)
# crosses every bucket threshold (8, 12, 16, 23, 32, 46, 64, 91), every 16-query tile, 64-key chunk and 128-query block edge, and
# reaches d = +-511: 2 418 rows in one packed call
LENGTHS = B.LENGTHS
SHUFFLED = B.SHUFFLED
BOS, PAD, EOS, UNK = 0, 1, 2, 3
BIAS_SEED, BIAS_SCALE = 3, 2.0
D = hf_checkpoint.MPNET_MAX_DISTANCE                              # 511


def bias_weight(heads, seed=BIAS_SEED):
    """``encoder.relative_attention_bias.weight`` [32, heads]: 2.0 N(0, 1), seeded -- a few units, like the logits."""
    return BIAS_SCALE * torch.randn(32, heads, generator=torch.Generator().manual_seed(seed))


def _with_bias(sd, arch):
    sd = {k: v for k, v in sd.items() if k != "token_type_embedding"}
    sd["relative_attention_bias"] = bias_weight(arch.heads)
    return sd


def random_state_dict(arch=ARCH, seed=0):
    """bert_ref's plain weights without the type row, plus the bias table."""
    return _with_bias(B.random_state_dict(arch, seed), arch)


def heavy_state_dict(arch=ARCH, seed=0):
    """bert_ref's heavy-tailed weights without the type row, plus the bias table."""
    return _with_bias(B.heavy_state_dict(arch, seed), arch)


def tensor_shapes(arch=ARCH):
    shapes = {k: v for k, v in B.tensor_shapes(arch).items() if k != "token_type_embedding"}
    shapes["relative_attention_bias"] = (32, arch.heads)
    return shapes


def mpnet_config(arch=ARCH, positions=None):
    from transformers import MPNetConfig
    return MPNetConfig(vocab_size=arch.vocab, hidden_size=arch.width, num_hidden_layers=arch.layers, num_attention_heads=arch.heads,
                       intermediate_size=4 * arch.width, max_position_embeddings=(positions or arch.ctx) + 2,
                       layer_norm_eps=arch.layer_norm_eps, relative_attention_num_buckets=32)


def hf_model(sd, arch=ARCH, pooler=False):
    """``transformers.MPNetModel`` (eager attention, fp32, eval) holding the weights of `sd`."""
    from transformers import MPNetModel
    cfg = mpnet_config(arch)
    cfg._attn_implementation = "eager"
    model = MPNetModel(cfg, add_pooling_layer=pooler).eval()
    missing = model.load_state_dict(hf_checkpoint.to_mpnet_state_dict(sd, arch), strict=False)
    assert not missing.unexpected_keys and all(k.startswith("pooler.") or k.endswith("_ids") for k in missing.missing_keys), missing
    return model


def random_ids(lens, arch=ARCH, seed=1, pad_to=None):
    """<s> random ids </s> of the given lengths (a length-1 text is <s> alone), padded with <pad> = 1 to `pad_to` (default arch.ctx);
    no id inside a text's length is <pad>."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.full((len(lens), pad_to or arch.ctx), PAD, dtype=torch.int32)
    for i, n in enumerate(lens):
        row = torch.randint(5, arch.vocab, (n,), generator=g, dtype=torch.int32)
        row[0] = BOS
        if n > 1:
            row[-1] = EOS
        ids[i, :n] = row
    return ids, torch.tensor(lens, dtype=torch.int32)


def position_bias(table, n):
    """[heads, n, n]: table[h][(key - query) + 511] for queries and keys 0 .. n - 1 of a [heads, 1023] table by distance."""
    idx = torch.arange(n)[None, :] - torch.arange(n)[:, None] + D
    return table[:, idx]


@torch.no_grad()
def hidden_states(sd, arch, ids_row, dtype=torch.float32, table=None):
    """The final rows [len, W] of ONE text given as its ids [len].  `table` (fp32 [heads, 1023], by distance) replaces the one expanded
    from the state dict's relative_attention_bias: the negative controls pass wrong ones."""
    p = lambda n: sd[n].to(dtype)                                      # noqa: E731
    n, w, heads, eps = ids_row.numel(), arch.width, arch.heads, arch.layer_norm_eps
    ln = lambda x, name: F.layer_norm(x, (w,), p(f"{name}.weight"), p(f"{name}.bias"), eps)      # noqa: E731
    table = hf_checkpoint.bias_by_distance(sd["relative_attention_bias"]) if table is None else table
    bias = position_bias(table.to(dtype), n)
    x = ln(p("token_embedding.weight")[ids_row.long()] + p("positional_embedding")[:n], "ln_embed")
    for i in range(arch.layers):
        b = f"transformer.resblocks.{i}"
        q, k, v = (x @ p(f"{b}.attn.in_proj_weight").T + p(f"{b}.attn.in_proj_bias")).split(w, dim=-1)
        q, k, v = (t.view(n, heads, 64).transpose(0, 1) for t in (q, k, v))
        a = (torch.softmax(q @ k.transpose(-1, -2) / 8.0 + bias, dim=-1) @ v).transpose(0, 1).reshape(n, w)
        x = ln(x + a @ p(f"{b}.attn.out_proj.weight").T + p(f"{b}.attn.out_proj.bias"), f"{b}.ln_1")
        h = x @ p(f"{b}.mlp.c_fc.weight").T + p(f"{b}.mlp.c_fc.bias")
        h = 0.5 * h * (1.0 + torch.erf(h * 2.0 ** -0.5))
        x = ln(x + h @ p(f"{b}.mlp.c_proj.weight").T + p(f"{b}.mlp.c_proj.bias"), f"{b}.ln_2")
    return x


@torch.no_grad()
def encode(sd, arch, ids, lens, pooling="mean", normalize=False, dtype=torch.float32, table=None):
    """ids int [B, P] (P >= max(lens); what lies behind a text's length is never read), lens int [B] -> [B, W] in `dtype`."""
    out = []
    for row, n in zip(ids, torch.as_tensor(lens).tolist()):
        x = hidden_states(sd, arch, row[:n], dtype, table)
        e = x.sum(0) / n if pooling == "mean" else x[0]
        out.append(e / e.norm() if normalize else e)
    return torch.stack(out)


@torch.no_grad()
def hf_encode(model, ids, lens, pooling="mean"):
    """``MPNetModel`` on the padded batch with its attention mask, then sentence-transformers' pooling."""
    p = ids.shape[1]
    mask = (torch.arange(p)[None, :] < torch.as_tensor(lens)[:, None]).long()
    h = model(input_ids=ids.long(), attention_mask=mask).last_hidden_state
    if pooling == "cls":
        return h[:, 0]
    m = mask[..., None].to(h.dtype)
    return (h * m).sum(1) / m.sum(1).clamp_min(1e-9)


one_minus_cos = B.one_minus_cos
cached = B.cached
sentences = B.sentences
score_margin = B.score_margin


def wrong_tables(table):
    """The negative controls' tables: what a kernel or a loader that gets the bias wrong would apply."""
    frozen = table.clone()
    frozen[:, : D - 63] = table[:, D - 63:D - 62]                   # beyond |d| = 63 the value at |d| = 63 (the far buckets never reached)
    frozen[:, D + 64:] = table[:, D + 63:D + 64]
    return {"no_bias": torch.zeros_like(table), "mirrored": table.flip(-1), "heads_rotated": table.roll(1, 0), "frozen_beyond_63": frozen}


# ------------------------------------------------------------------------------------------------ biased attention: the rounding statement
def attention_varlen_bias_emulation(qkv_bf16, row_start, width, table, kc=64):
    """fp64 statement of csrc/attention_stream.hip's BIAS instantiation, per packed item on its own rows: oracle.rounding
    attention_long_emulation (``_attention_chunked``) restated with s = q . k + bias[h][key - query].  The bias enters the kernel as the
    START VALUE of the fp32 accumulator of the score's first MFMA (the second MFMA continues from it), so the kernel's score is the fp32
    sum of bias and 64 bf16 products accumulated in the MFMAs' order; q carries the 1/8 and the bias is not scaled.  Everything after the
    score is the unbiased kernel's, applied to the biased s: running maximum per 64-key chunk, P = exp(s - m_c) rounded to bf16 for PV
    with the row sum from the unrounded P, one division.

    Budget (u = 2^-24, n = chunks): the terms of attention_long_emulation with two changes, both in eps, the relative error of a key's P.
    * The score: attention_long's bound 16 u sabs (sabs = sum |q||k|) covers two MFMAs over 64 exact products whose every partial sum
      is at most sabs in magnitude.  With the accumulator started at the bias every partial sum is at most |bias| + sabs, and the bias
      itself is an fp32 number taken exactly (no rounding on entry): 16 u (sabs + |bias|).
    * The fma s log2e - m' and exp2: unchanged in form, with |s| and |m_c| now those of the BIASED scores.
    flip, prop, chain and acc follow from eps, the chunk maxima and the sums exactly as derived there (the maxima and f_c are those of
    the biased scores).  A zero table gives attention_long_emulation's statement and budget back, term for term.
    Returns (O, extra), fp64 [rows, width]."""
    from oracle import rounding as R
    heads = width // 64
    u = 2.0 ** -24
    table = table.double().cpu()
    ref = torch.zeros(qkv_bf16.shape[0], width, dtype=torch.float64)
    extra = torch.zeros_like(ref)
    for a0, e0 in zip(row_start[:-1].tolist(), row_start[1:].tolist()):
        t = e0 - a0
        x = qkv_bf16[a0:e0].double().cpu().view(t, 3, heads, 64).permute(1, 2, 0, 3)
        q, k, v = x[0], x[1], x[2]                                   # [H, T, 64]
        bias = position_bias(table, t)                               # [H, T, T]
        n = (t + kc - 1) // kc
        chunks = [(c * kc, min(t, (c + 1) * kc)) for c in range(n)]
        scores = lambda a, b: q @ k[:, a:b].transpose(-1, -2) + bias[:, :, a:b]      # noqa: E731
        m_run, m = [], torch.full((heads, t, 1), float("-inf"), dtype=torch.float64)
        for a, b in chunks:
            m = torch.maximum(m, scores(a, b).amax(-1, keepdim=True))
            m_run.append(m)
        m_fin, m_0 = m_run[-1], m_run[0]
        zero = torch.zeros_like(q)
        o_sum, w_abs, flip = zero.clone(), zero.clone(), zero.clone()
        l, l_eps = torch.zeros_like(m_fin), torch.zeros_like(m_fin)
        for (a, b), m_c in zip(chunks, m_run):
            kk, vv = k[:, a:b], v[:, a:b]
            s = scores(a, b)
            sabs = q.abs() @ kk.abs().transpose(-1, -2) + bias[:, :, a:b].abs()
            f = torch.exp(m_c - m_fin)
            p = torch.exp(s - m_c)
            pb = R.rne_bf16(p)
            eps = u * (16 * sabs + 2 * (s.abs() + m_c.abs()) * 1.4427 + 4)
            move = torch.maximum((R.rne_bf16(p * (1 - eps)) - pb).abs(), (R.rne_bf16(p * (1 + eps)) - pb).abs())
            l = l + f * p.sum(-1, keepdim=True)
            l_eps = l_eps + f * (eps * p).sum(-1, keepdim=True)
            o_sum = o_sum + f * (pb @ vv)
            w_abs = w_abs + f * (pb @ vv.abs())
            flip = flip + f * (move @ vv.abs())
        o = o_sum / l
        rho = u * (6 * n + (m_fin - m_0) + 2 * torch.maximum(m_0.abs(), m_fin.abs()))
        ex = (flip + l_eps * o.abs() + rho * (w_abs + l * o.abs()) + (16 + n) * u * w_abs) / l + (16 + 2 * n) * u * o.abs()
        ref[a0:e0] = o.permute(1, 0, 2).reshape(t, width)
        extra[a0:e0] = ex.permute(1, 0, 2).reshape(t, width)
    return ref, extra


# ------------------------------------------------------------------------------------------------ checkpoint directory + tokenizer
def vocabulary(arch=ARCH):
    """<s> <pad> </s> <unk> <mask> at 0 .. 4, then bert_ref's words and continuation pieces."""
    vocab = {t: i for i, t in enumerate(["<s>", "<pad>", "</s>", "<unk>", "<mask>"])}
    for w in B.WORDS + B.SUFFIXES:
        vocab[w] = len(vocab)
    assert len(vocab) <= arch.vocab and (vocab["<s>"], vocab["<pad>"], vocab["</s>"], vocab["<unk>"]) == (BOS, PAD, EOS, UNK)
    return vocab


def write_tokenizer(directory, arch=ARCH):
    from tokenizers import Tokenizer, models, normalizers, pre_tokenizers, processors
    tok = Tokenizer(models.WordPiece(vocabulary(arch), unk_token="<unk>"))
    tok.normalizer = normalizers.BertNormalizer(lowercase=True)
    tok.pre_tokenizer = pre_tokenizers.BertPreTokenizer()
    tok.post_processor = processors.TemplateProcessing(single="<s> $A </s>", pair="<s> $A </s> </s> $B </s>",
                                                       special_tokens=[("<s>", BOS), ("</s>", EOS)])
    tok.save(os.path.join(directory, "tokenizer.json"))


def save_directory(directory, sd, arch=ARCH, pooler=True, pooling=None, max_seq_length=None):
    """``MPNetModel.save_pretrained`` (with its pooler by default, as the published checkpoint has one) + tokenizer.json; `pooling`
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
            json.dump({"max_seq_length": max_seq_length, "do_lower_case": False}, f)
    return directory


def toy_set(sd, tokenize, n=64, margin=2e-3, arch=ARCH):
    """bert_ref.toy_set with this module's statement: n (query, target) pairs whose oracle scores keep more than `margin` from their
    row's ground-truth score.  Returns (queries, targets, oracle query embeddings, oracle target embeddings), L2-normalised fp32."""
    queries, targets = B.toy_candidates()
    qi, ql = tokenize(queries)
    ti, tl = tokenize(targets)
    q, t = encode(sd, arch, qi, ql, normalize=True), encode(sd, arch, ti, tl, normalize=True)
    s = q.double() @ t.double().T
    keep = []
    for c in range(len(queries)):
        if all(abs(float(s[i, c] - s[i, i])) > margin and abs(float(s[c, i] - s[c, c])) > margin for i in keep):
            keep.append(c)
        if len(keep) == n:
            break
    assert len(keep) == n, f"only {len(keep)} of {n} pairs with margin {margin}"
    return [queries[i] for i in keep], [targets[i] for i in keep], q[keep], t[keep]
