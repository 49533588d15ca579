"""Two reference statements for towers whose heads are not 64 wide (ViT-H-14: vision heads of 80), for the tests of the head-dim-80
attention kernels (csrc/attention80.hip).  oracle/clip_ref.py and oracle/rounding.attention_emulation state `width // 64` heads; the
statements here take the head counts / the head dim as arguments and consume the same seeded weights (keyed by name) and the same
bf16 q | k | v.  Not a test module; no GPU, no library.

1. ``encode_image`` / ``encode_text``: the CLIP forward in torch fp64, OpenAI key names, head counts as arguments
   (tests/test_headdim_host.py checks it against ``transformers.CLIPModel`` with 16 vision heads at hidden 1280).
2. ``attention_statement``: oracle.rounding._attention_rows -- already head-dim-agnostic -- on [B, H, T, hd] views, with its score-error
   coefficient restated per MFMA of the chain."""
import torch
import torch.nn.functional as F

from oracle import rounding as R

U = 2.0 ** -24                     # fp32 unit roundoff
MFMA_U = 8                         # |fp32 accumulator of ONE v_mfma_f32_16x16x32_bf16 - exact| <= MFMA_U u sum|a||b| (see attention_statement)


# ------------------------------------------------------------------------------------------------ 1. CLIP forward, fp64
def _block64(x, sd, prefix, heads, causal, gelu):
    B, T, W = x.shape
    hd = W // heads
    p = lambda n: sd[f"{prefix}.{n}"].double()                                  # noqa: E731
    h = F.layer_norm(x, (W,), p("ln_1.weight"), p("ln_1.bias"), 1e-5)
    q, k, v = (h @ p("attn.in_proj_weight").T + p("attn.in_proj_bias")).split(W, dim=-1)
    q, k, v = (t.view(B, T, heads, hd).transpose(1, 2) for t in (q * hd ** -0.5, k, v))
    s = q @ k.transpose(-1, -2)
    if causal:
        s = s + torch.full((T, T), float("-inf"), dtype=torch.float64).triu_(1)
    a = (torch.softmax(s, dim=-1) @ v).transpose(1, 2).reshape(B, T, W)
    x = x + a @ p("attn.out_proj.weight").T + p("attn.out_proj.bias")
    h = F.layer_norm(x, (W,), p("ln_2.weight"), p("ln_2.bias"), 1e-5)
    h = h @ p("mlp.c_fc.weight").T + p("mlp.c_fc.bias")
    h = 0.5 * h * torch.erfc(-h * 2.0 ** -0.5) if gelu else h * torch.sigmoid(1.702 * h)
    return x + h @ p("mlp.c_proj.weight").T + p("mlp.c_proj.bias")


@torch.no_grad()
def encode_image(sd, arch, pixels, heads, activation="quick_gelu"):
    """pixels [B, 3, S, S] -> fp64 [B, embed_dim] (un-normalised); arch: the dict of oracle.clip_ref (or ClipArch.cfg_dict());
    heads: the vision tower's head count."""
    vw, p = arch["v_width"], arch["patch"]
    g = lambda n: sd[f"visual.{n}"].double()                                    # noqa: E731
    x = F.conv2d(pixels.double(), g("conv1.weight"), stride=p).flatten(2).transpose(1, 2)
    x = torch.cat([g("class_embedding").expand(x.shape[0], 1, vw), x], dim=1) + g("positional_embedding")
    x = F.layer_norm(x, (vw,), g("ln_pre.weight"), g("ln_pre.bias"), 1e-5)
    for i in range(arch["v_layers"]):
        x = _block64(x, sd, f"visual.transformer.resblocks.{i}", heads, False, activation == "gelu")
    x = F.layer_norm(x[:, 0, :], (vw,), g("ln_post.weight"), g("ln_post.bias"), 1e-5)
    return x @ g("proj")


@torch.no_grad()
def encode_text(sd, arch, ids, heads, activation="quick_gelu"):
    """ids [B, ctx] -> fp64 [B, embed_dim] (un-normalised), pooled at argmax(ids); heads: the text tower's head count."""
    tw = arch["t_width"]
    ids = ids.long()
    x = sd["token_embedding.weight"].double()[ids] + sd["positional_embedding"].double()[: ids.shape[1]]
    for i in range(arch["t_layers"]):
        x = _block64(x, sd, f"transformer.resblocks.{i}", heads, True, activation == "gelu")
    x = F.layer_norm(x, (tw,), sd["ln_final.weight"].double(), sd["ln_final.bias"].double(), 1e-5)
    return x[torch.arange(x.shape[0]), ids.argmax(dim=-1)] @ sd["text_projection"].double()


def one_minus_cos(a, b):
    return 1.0 - F.cosine_similarity(a.double().cpu(), b.double().cpu(), dim=-1)


# ------------------------------------------------------------------------------------------------ 2. attention, any head dim
def heads_view(qkv_bf16, batch, t, width, head_dim):
    """bf16 q | k | v rows [batch t, 3 width] -> fp64 q, k, v [B, H, T, hd]."""
    x = qkv_bf16.double().view(batch, t, 3, width // head_dim, head_dim).permute(2, 0, 3, 1, 4)
    return x[0], x[1], x[2]


def attention_rows(q, k, v, mask=None, mfmas=2):
    """oracle.rounding._attention_rows with the score-error coefficient a parameter.  _attention_rows bounds the fp32 error of a logit
    by 16 u sum|q||k| for the TWO v_mfma_f32_16x16x32_bf16 the head-dim-64 kernel chains over the head dim (K = 32 each): 8 u per
    MFMA of the chain.  A kernel that chains `mfmas` of them is given 8 mfmas u: 24 u for the three steps of head dim 80 (two full
    ones and the half step whose upper 16 k slots are zero).  The coefficient is DERIVED -- one MFMA sums 32 exact bf16 products
    and the incoming accumulator in fp32 in an order the ISA does not state, at most 33 roundings of partial sums no larger than
    sum|q||k|, of which the bar grants 8 u because the partial sums of products of either sign stay far below that bound; the
    16 u of oracle/rounding.py is that figure for two -- and not measured on the kernel under test.  Every other term is
    _attention_rows' own: with mfmas = 2 the result is _attention_rows', bit for bit (tests/test_headdim_host.py)."""
    o, extra = R._attention_rows(q, k, v, mask)
    if mfmas == 2:
        return o, extra
    # the additional (8 mfmas - 16) u sum|q||k| per logit moves P by that relative amount: _attention_rows' `prop` term for it
    s = q @ k.transpose(-1, -2)
    sabs = q.abs() @ k.abs().transpose(-1, -2)
    if mask is not None:
        s = s.masked_fill(mask, float("-inf"))
    p = torch.exp(s - s.amax(-1, keepdim=True))
    l = p.sum(-1, keepdim=True)
    eps = U * (MFMA_U * mfmas - 16) * sabs
    more = ((eps * p) @ v.abs() + (eps * p).sum(-1, keepdim=True) * o.abs()) / l
    return o, extra + more


def attention_statement(qkv_bf16, batch, t, width, head_dim):
    """fp64 statement of the non-causal tile kernel at any head dim (csrc/attention.hip at 64, csrc/attention80.hip at 80): (O, extra),
    both [batch t, width], as oracle.rounding.attention_emulation returns them; ceil(head_dim / 32) chained MFMAs per logit."""
    q, k, v = heads_view(qkv_bf16, batch, t, width, head_dim)
    o, extra = attention_rows(q, k, v, None, mfmas=(head_dim + 31) // 32)
    back = lambda y: y.permute(0, 2, 1, 3).reshape(batch * t, width)            # noqa: E731
    return back(o), back(extra)


def attention_pooled_statement(q_bf16, qkv_bf16, items, tokens, width, head_dim):
    """fp64 statement of the pooled-row kernel's vision form at any head dim: oracle.rounding.attention_pooled_emulation's rule -- ONE
    chunk of _attention_chunked holding every key -- on [items, H, K, hd] views.  Its score term, 16 u sum|q||k|, stands as it is: the
    pooled kernels take a logit as 8 fma per lane and the shuffle adds of the key's lanes (3 at head dim 64, 4 at 80: 12 roundings at
    most), not as MFMAs."""
    heads = width // head_dim
    kv = qkv_bf16.double().cpu().view(items, tokens, 3, heads, head_dim)
    k, v = kv[:, :, 1].transpose(1, 2), kv[:, :, 2].transpose(1, 2)             # [items, H, K, hd]
    qh = q_bf16.double().cpu().view(items, heads, 1, head_dim)
    o, extra = R._attention_chunked(qh, k, v, None, tokens)
    return o.reshape(items, width), extra.reshape(items, width)
