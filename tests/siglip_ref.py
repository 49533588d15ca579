"""An fp64 statement of both SigLIP towers on the engine's tensor names, for the tests of the SigLIP family (model option "family" = 1).
Not a test module; no GPU, no library.

``encode_image`` / ``encode_text`` state what ``transformers.SiglipModel`` computes (tests/test_siglip_host.py holds them to it); every
way in which that differs from the CLIP towers is a keyword switch whose default is SigLIP's, so that a test can state the WRONG model
-- the CLIP behaviour a kernel or a launch sequence would have if one difference were forgotten -- and show that the parity bar tells
the two apart:

    causal=True              the text tower behind CLIP's causal mask
    pool="argmax"            the text row of argmax(ids) instead of the last position
    eps=1e-5                 CLIP's LayerNorm epsilon
    act="gelu"|"quick_gelu"  the erf GELU / QuickGELU instead of the tanh GELU
    vision_pool="first_token"  ln_post of token 0 instead of the attention-pooling head
    conv_bias=False          the patch embedding without its bias
"""
import math

import torch
import torch.nn.functional as F

from knowledge_enhanced_multimodal_retrieval_amd.config import ClipArch

ACTS = ("gelu_pytorch_tanh", "gelu", "quick_gelu")


def act64(h, act="gelu_pytorch_tanh"):
    if act == "gelu_pytorch_tanh":
        return 0.5 * h * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (h + 0.044715 * h ** 3)))
    if act == "gelu":
        return 0.5 * h * torch.erfc(-h * 2.0 ** -0.5)
    if act == "quick_gelu":
        return h * torch.sigmoid(1.702 * h)
    raise ValueError(act)


def _mlp(x, p, prefix, act):
    return act64(x @ p(f"{prefix}.c_fc.weight").T + p(f"{prefix}.c_fc.bias"), act) @ p(f"{prefix}.c_proj.weight").T + p(f"{prefix}.c_proj.bias")


def _attention(q, k, v, heads, mask=None):
    """q [B, Tq, W] (unscaled), k / v [B, Tk, W] -> [B, Tq, W]; heads of W // heads, scale 1 / sqrt(head dim)."""
    B, Tq, W = q.shape
    hd = W // heads
    q, k, v = (t.view(B, t.shape[1], heads, hd).transpose(1, 2) for t in (q * hd ** -0.5, k, v))
    s = q @ k.transpose(-1, -2)
    if mask is not None:
        s = s + mask
    return (torch.softmax(s, dim=-1) @ v).transpose(1, 2).reshape(B, Tq, W)


def _block(x, sd, prefix, causal, eps, act):
    B, T, W = x.shape
    p = lambda n: sd[n].double()                                                   # noqa: E731
    h = F.layer_norm(x, (W,), p(f"{prefix}.ln_1.weight"), p(f"{prefix}.ln_1.bias"), eps)
    q, k, v = (h @ p(f"{prefix}.attn.in_proj_weight").T + p(f"{prefix}.attn.in_proj_bias")).split(W, dim=-1)
    mask = torch.full((T, T), float("-inf"), dtype=torch.float64).triu_(1) if causal else None
    a = _attention(q, k, v, W // 64, mask)
    x = x + a @ p(f"{prefix}.attn.out_proj.weight").T + p(f"{prefix}.attn.out_proj.bias")
    h = F.layer_norm(x, (W,), p(f"{prefix}.ln_2.weight"), p(f"{prefix}.ln_2.bias"), eps)
    return x + _mlp(h, p, f"{prefix}.mlp", act)


@torch.no_grad()
def vision_tokens(sd, arch: ClipArch, pixels, conv_bias=True):
    """The rows block 0 reads: patch embedding (+ bias) + positional embedding, fp64 [B, patches, W]; no class token, no ln_pre."""
    g = lambda n: sd[f"visual.{n}"].double()                                       # noqa: E731
    x = F.conv2d(pixels.double(), g("conv1.weight"), g("conv1.bias") if conv_bias else None, stride=arch.patch)
    return x.flatten(2).transpose(1, 2) + g("positional_embedding")


@torch.no_grad()
def map_head(sd, arch: ClipArch, h, eps=1e-6, act="gelu_pytorch_tanh", return_attention=False):
    """SiglipMultiheadAttentionPoolingHead on h = the post-LayerNorm tokens fp64 [B, T, W] -> [B, W]."""
    W = arch.v_width
    p = lambda n: sd[f"visual.attn_pool.{n}"].double()                             # noqa: E731
    wq, wk, wv = p("in_proj_weight").split(W, dim=0)
    bq, bk, bv = p("in_proj_bias").split(W, dim=0)
    q = (p("probe") @ wq.T + bq).expand(h.shape[0], 1, W)
    a = _attention(q, h @ wk.T + bk, h @ wv.T + bv, W // 64)
    r = (a @ p("out_proj.weight").T + p("out_proj.bias"))[:, 0]
    out = r + _mlp(F.layer_norm(r, (W,), p("ln.weight"), p("ln.bias"), eps), p, "mlp", act)
    return (out, a[:, 0]) if return_attention else out


@torch.no_grad()
def encode_image(sd, arch: ClipArch, pixels, eps=1e-6, act="gelu_pytorch_tanh", vision_pool="map", conv_bias=True):
    """pixels [B, 3, S, S] -> fp64 [B, v_width] (un-normalised)."""
    W = arch.v_width
    x = vision_tokens(sd, arch, pixels, conv_bias)
    for i in range(arch.v_layers):
        x = _block(x, sd, f"visual.transformer.resblocks.{i}", False, eps, act)
    g = lambda n: sd[f"visual.{n}"].double()                                       # noqa: E731
    if vision_pool == "first_token":
        return F.layer_norm(x[:, 0], (W,), g("ln_post.weight"), g("ln_post.bias"), eps)
    return map_head(sd, arch, F.layer_norm(x, (W,), g("ln_post.weight"), g("ln_post.bias"), eps), eps, act)


@torch.no_grad()
def encode_text(sd, arch: ClipArch, ids, eps=1e-6, act="gelu_pytorch_tanh", causal=False, pool="last"):
    """ids [B, ctx] -> fp64 [B, embed_dim] (un-normalised): no mask, the LAST position pooled, a head with bias."""
    W = arch.t_width
    ids = ids.long()
    x = sd["token_embedding.weight"].double()[ids] + sd["positional_embedding"].double()[: ids.shape[1]]
    for i in range(arch.t_layers):
        x = _block(x, sd, f"transformer.resblocks.{i}", causal, eps, act)
    x = F.layer_norm(x, (W,), sd["ln_final.weight"].double(), sd["ln_final.bias"].double(), eps)
    row = x[torch.arange(x.shape[0]), ids.argmax(dim=-1)] if pool == "argmax" else x[:, -1]
    return row @ sd["text_projection"].double() + sd["text_projection_bias"].double()


def one_minus_cos(a, b):
    return 1.0 - F.cosine_similarity(a.double().cpu(), b.double().cpu(), dim=-1)


# ------------------------------------------------------------------------------------------------ seeded weights and inputs
def tensor_shapes(arch: ClipArch):
    """name -> shape of every tensor the engine's SigLIP family loads (logit_scale / logit_bias besides)."""
    vw, tw, D, P = arch.v_width, arch.t_width, arch.embed_dim, arch.grid ** 2
    out = {"visual.conv1.weight": (vw, 3, arch.patch, arch.patch), "visual.conv1.bias": (vw,), "visual.positional_embedding": (P, vw),
           "visual.ln_post.weight": (vw,), "visual.ln_post.bias": (vw,),
           "token_embedding.weight": (arch.vocab, tw), "positional_embedding": (arch.ctx, tw), "ln_final.weight": (tw,), "ln_final.bias": (tw,),
           "text_projection": (tw, D), "text_projection_bias": (D,)}

    def mlp(prefix, w):
        out.update({f"{prefix}.c_fc.weight": (4 * w, w), f"{prefix}.c_fc.bias": (4 * w,), f"{prefix}.c_proj.weight": (w, 4 * w), f"{prefix}.c_proj.bias": (w,)})

    for prefix, w, layers in (("visual.transformer", vw, arch.v_layers), ("transformer", tw, arch.t_layers)):
        for i in range(layers):
            b = f"{prefix}.resblocks.{i}"
            out.update({f"{b}.ln_1.weight": (w,), f"{b}.ln_1.bias": (w,), f"{b}.attn.in_proj_weight": (3 * w, w), f"{b}.attn.in_proj_bias": (3 * w,),
                        f"{b}.attn.out_proj.weight": (w, w), f"{b}.attn.out_proj.bias": (w,), f"{b}.ln_2.weight": (w,), f"{b}.ln_2.bias": (w,)})
            mlp(f"{b}.mlp", w)
    h = "visual.attn_pool"
    out.update({f"{h}.probe": (vw,), f"{h}.in_proj_weight": (3 * vw, vw), f"{h}.in_proj_bias": (3 * vw,), f"{h}.out_proj.weight": (vw, vw),
                f"{h}.out_proj.bias": (vw,), f"{h}.ln.weight": (vw,), f"{h}.ln.bias": (vw,)})
    mlp(f"{h}.mlp", vw)
    return out


def random_state_dict(arch: ClipArch, seed=0):
    """Seeded fp32 weights under the engine's names, scaled so that activations stay O(1): matrices N(0, 1 / fan_in) (the MLP's fc1
    1.5 x that, so that pre-activations reach the range where the three activations differ), biases N(0, 0.1^2) (the patch
    embedding's N(0, 0.5^2): a forgotten conv bias must show), LayerNorm gains 1 + N(0, 0.1^2), embeddings N(0, 0.5^2)."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name, shape in tensor_shapes(arch).items():
        if name.endswith("ln_1.weight") or name.endswith("ln_2.weight") or name.endswith("ln.weight") or name.endswith("ln_post.weight") or name == "ln_final.weight":
            t = 1.0 + 0.1 * torch.randn(shape, generator=g)
        elif name == "visual.conv1.bias":
            t = 0.5 * torch.randn(shape, generator=g)
        elif name.endswith("bias"):
            t = 0.1 * torch.randn(shape, generator=g)
        elif name in ("token_embedding.weight", "positional_embedding", "visual.positional_embedding", "visual.attn_pool.probe"):
            t = 0.5 * torch.randn(shape, generator=g)
        elif name == "text_projection":
            t = torch.randn(shape, generator=g) * shape[0] ** -0.5
        else:
            fan_in = math.prod(shape[1:])
            t = torch.randn(shape, generator=g) * fan_in ** -0.5 * (1.5 if name.endswith("c_fc.weight") else 1.0)
        sd[name] = t
    sd["logit_scale"] = torch.tensor([math.log(10.0)])
    sd["logit_bias"] = torch.tensor([-10.0])
    return sd


def pixels(arch: ClipArch, n, seed=11):
    return torch.randn(n, 3, arch.image_size, arch.image_size, generator=torch.Generator().manual_seed(seed))


def text_ids(arch: ClipArch, n, seed=13):
    """Token rows as the SigLIP tokenizer leaves them: ids >= 2, the end-of-sequence id 1, pads of id 1 -- so argmax(ids) is never the
    last position (a text of full length apart), and a causal mask changes what the last row sees."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.ones(n, arch.ctx, dtype=torch.int32)
    for i in range(n):
        ln = int(torch.randint(2, arch.ctx - 2, (1,), generator=g))
        ids[i, :ln] = torch.randint(2, arch.vocab, (ln,), generator=g, dtype=torch.int32)
    return ids


# ------------------------------------------------------------------------------------------------ sharpened weights
# On the plain seeded weights three of the wrong statements sit too close to the right one for a 1e-2 bar (measured in fp64 on the
# shapes of the tests: eps 1e-5 at 1e-11, QuickGELU at 2e-5 .. 4e-5, the causal mask at 9e-3 at 64 positions).  Each gets weights that
# put the towers where the difference matters; the factors are fixed here, and tests/test_siglip_host.py asserts what they achieve.
#  * "eps": patch weights, patch bias, both positional tables and the token table times EPS_SHARPEN, so that the rows the first
#    LayerNorm sees have a variance near 1e-5 (unit-variance pixels, fan-in-normalised patch weights: about 1.5 EPS_SHARPEN^2 =
#    3.4e-6), where rsqrt(var + 1e-5) and rsqrt(var + 1e-6) differ by a factor near 2 and the first block's updates, which do not
#    scale with the rows, weigh differently against them.
#  * "act": fc1 bias shifted by ACT_SHIFT with fc1 weights times ACT_FC, so that pre-activations sit near -3 +- 0.5, where tanh GELU
#    gives -0.0036 and QuickGELU -0.018 (a factor of 5; the erf GELU -0.0040), and fc2 weights times ACT_PROJ so that the MLP updates
#    weigh as much as the stream.  (The tanh / erf pair stays below 1e-2 even so: it is separated at the op level.)
#  * "causal": the text tower's out_proj weights times CAUSAL_OUT: the last position sees every key under either mask, so the mask
#    reaches it only through the earlier rows' attention updates, which this makes larger.
EPS_SHARPEN = 1.5e-3
ACT_SHIFT, ACT_FC, ACT_PROJ = -3.0, 0.3, 32.0
CAUSAL_OUT = 4.0


def sharpen(sd, what):
    out = dict(sd)
    for n, t in sd.items():
        if what == "eps" and n in ("visual.conv1.weight", "visual.conv1.bias", "visual.positional_embedding", "token_embedding.weight", "positional_embedding"):
            out[n] = t * EPS_SHARPEN
        elif what == "act" and n.endswith("c_fc.bias"):
            out[n] = t + ACT_SHIFT
        elif what == "act" and n.endswith("c_fc.weight"):
            out[n] = t * ACT_FC
        elif what == "act" and n.endswith("c_proj.weight"):
            out[n] = t * ACT_PROJ
        elif what == "causal" and n.startswith("transformer.") and n.endswith("out_proj.weight"):
            out[n] = t * CAUSAL_OUT
    if what not in ("eps", "act", "causal"):
        raise ValueError(what)
    return out


# the wrong statements of each tower and the weights on which each must miss the right one by more than 1e-2: (switches, sharpening or None)
WRONG_IMAGE = [(dict(vision_pool="first_token"), None), (dict(conv_bias=False), None), (dict(eps=1e-5), "eps"), (dict(act="quick_gelu"), "act")]
WRONG_TEXT = [(dict(pool="argmax"), None), (dict(causal=True), "causal"), (dict(eps=1e-5), "eps"), (dict(act="quick_gelu"), "act")]
SEED = 3


# ------------------------------------------------------------------------------------------------ shared cases (host and GPU tests)
IMAGE_CASES = [("tiny-siglip", 3), ("tiny-siglip", 9), ("tiny-siglip-196", 3), ("tiny-siglip-196", 9), ("tiny-siglip-576", 3), ("tiny-siglip-576", 9)]
TEXT_CASES = [(16, 5), (64, 5)]            # (ctx, texts): tiny-siglip, and the same tower at SigLIP's 64 positions

_cache = {}


def text_arch(ctx):
    import dataclasses
    from knowledge_enhanced_multimodal_retrieval_amd.config import ARCHS
    return dataclasses.replace(ARCHS["tiny-siglip"], ctx=ctx)


def weights(arch: ClipArch, sharpening=None):
    key = ("w", arch, sharpening)
    if key not in _cache:
        sd = random_state_dict(arch, SEED)
        _cache[key] = sharpen(sd, sharpening) if sharpening else sd
    return _cache[key]


def image_reference(name, n, sharpening=None, **switches):
    """fp64 embeddings [n, W] of case (name, n) on the seeded (or sharpened) weights, computed once per process and never written to."""
    from knowledge_enhanced_multimodal_retrieval_amd.config import ARCHS
    key = ("i", name, n, sharpening, tuple(sorted(switches.items())))
    if key not in _cache:
        _cache[key] = encode_image(weights(ARCHS[name], sharpening), ARCHS[name], pixels(ARCHS[name], n), **switches)
    return _cache[key]


def text_reference(ctx, n, sharpening=None, **switches):
    key = ("t", ctx, n, sharpening, tuple(sorted(switches.items())))
    if key not in _cache:
        a = text_arch(ctx)
        _cache[key] = encode_text(weights(a, sharpening), a, text_ids(a, n), **switches)
    return _cache[key]


def hf_config_kwargs(arch: ClipArch):
    """kwargs of transformers.SiglipConfig for `arch`."""
    common = dict(hidden_act="gelu_pytorch_tanh", layer_norm_eps=1e-6)
    return {"text_config": dict(hidden_size=arch.t_width, intermediate_size=4 * arch.t_width, num_attention_heads=arch.t_width // 64,
                                num_hidden_layers=arch.t_layers, vocab_size=arch.vocab, max_position_embeddings=arch.ctx,
                                projection_size=arch.embed_dim, **common),
            "vision_config": dict(hidden_size=arch.v_width, intermediate_size=4 * arch.v_width, num_attention_heads=arch.v_width // 64,
                                  num_hidden_layers=arch.v_layers, image_size=arch.image_size, patch_size=arch.patch, **common)}
