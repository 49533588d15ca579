"""GPU: the kernels the SigLIP family adds, one by one -- the tanh-GELU fc1 epilogue of every GEMM kernel against fp64 under its
rounding budget (and the erf GELU / QuickGELU statements breaking that budget on the same outputs), the patch front without a class
token compared exactly, the attention-pooling head against the fp64 statement.  Every measured figure is printed (pytest -s)."""
import math

import pytest
import torch

import headdim_ref as H
import siglip_ref as S
from knowledge_enhanced_multimodal_retrieval_amd import _lib, debug, engine
from knowledge_enhanced_multimodal_retrieval_amd.config import ARCHS, ClipArch
from oracle import rounding as R

pytestmark = pytest.mark.gpu

COS_TOL = 1e-3             # the project's bar per embedding
MAX_BIAS = 0.02            # signed bias of a rounded output, bf16 ulp (tests/test_numerics_gpu.py)
KAPPA = 8                  # the accumulator bar of tests/test_numerics_gpu.py: |acc - fp64| <= KAPPA 2^-24 sum|a||w|
SLOPE = 1.13               # max |d gelu_tanh / dx| (1.129 near x = 1.4; asserted below)
EPI_T = _lib.EPI_BIAS_TGELU_BF16


def _note(name, value):
    print(f"NUMERICS {name} {value}")


def _bits(t):
    return t.contiguous().view(torch.int16)


# ------------------------------------------------------------------------------------------------ tanh-GELU epilogue
def _tgelu_extra(x64):
    """What csrc/common.h gelu_tanh may move the result by before the bf16 rounding, from its formula (units of 2^-24 relative; one
    fp32 rounding <= 1 unit, 1 ulp of a hardware transcendental <= 2 units):
      * the exponent t = K x (1 + 0.044715 x^2): x^2, the fma, the literal 0.044715f (2.5 units on the bracket), the product with x (1),
        K = the fp32 product of two fp32 literals (3), the product with K (1): 7.5 units of t, i.e. ln 2 |t| 7.5 = 5.2 |t| units of
        e = exp2(t), with |t| = 2 sqrt(2 / pi) log2(e) |x + 0.044715 x^3|;
      * v_exp_f32 (1 ulp = 2), the + 1 (1), v_rcp_f32 (1 ulp = 2), the product with x (1): 6 units; an error of e reaches 1 / (1 + e)
        damped by e / (1 + e) <= 1.
    2^-24 (6 + 5.2 |t|) |gelu_tanh(x)|: relative everywhere, the negative tail included (the sigmoid form has no cancellation)."""
    t = 2.0 * math.sqrt(2.0 / math.pi) * 1.4426950408889634 * (x64 + 0.044715 * x64 ** 3).abs()
    return 2.0 ** -24 * (6.0 + 5.2 * t) * S.act64(x64).abs()


def _operands(m, n, k, seed):
    """bf16 operands whose pre-activations are dense in (-3, -0.5): bias = linspace(-3, -0.5, n), sums of std 0.05."""
    g = torch.Generator().manual_seed(seed)
    ma = (m + 255) // 256 * 256
    a = torch.randn(ma, k, generator=g).to(torch.bfloat16)
    w = (torch.randn(n, k, generator=g) * k ** -0.5 * 0.05).to(torch.bfloat16)
    return a, w, torch.linspace(-3.0, -0.5, n)


def test_slope_constant():
    x = torch.linspace(-8, 8, 400001, dtype=torch.float64, requires_grad=True)
    (g,) = torch.autograd.grad(S.act64(x).sum(), x)
    assert float(g.abs().max()) <= SLOPE


@pytest.mark.parametrize("variant", [1, 2, 7, 8])          # 128 x 128, 256 x 256, persistent 256 x 256, skinny split-K
@pytest.mark.parametrize("k", [256, 768])
@pytest.mark.parametrize("n", [1024, 3072])
@pytest.mark.parametrize("m", [5, 300, 700])
def test_tanh_gelu_epilogue_against_fp64(device, variant, m, n, k):
    """bf16(gelu_tanh(A W^T + b)) of every kernel fc1 can take within half a bf16 ulp + the accumulator's budget carried through the
    slope + _tgelu_extra of the fp64 statement (ratio <= 1), twice with equal bits; the erf GELU and QuickGELU statements break the
    SAME budget on the same outputs (over the outputs of this range the erf statement is more than a bf16 ulp away at a third of the
    points, QuickGELU at 97 %)."""
    a, w, bias = _operands(m, n, k, 3 * m + n + k)
    a64, w64, b64 = a[:m].double(), w.double(), bias.double()
    x = a64 @ w64.T + b64
    assert -3.4 < float(x.min()) and float(x.max()) < -0.1
    extra = KAPPA * 2.0 ** -24 * (a64.abs() @ w64.abs().T + b64.abs()) * SLOPE + _tgelu_extra(x)
    ad, wd, bd = a.to(device), w.to(device), bias.to(device)
    with debug.override(gemm_variant=variant):
        og = engine.op_gemm(ad, wd, bd, m, EPI_T)[:m].cpu()
        again = engine.op_gemm(ad, wd, bd, m, EPI_T)[:m].cpu()
    assert torch.equal(_bits(og), _bits(again)), "two launches, two results"
    top, bias_u = R.check_budget(og, S.act64(x), extra, max_bias=MAX_BIAS, what=f"tgelu v{variant} {m}x{n}x{k}")
    wrong = {act: float(torch.nan_to_num(R.budget_ratio(og, S.act64(x, act), extra), nan=float("inf")).max()) for act in ("gelu", "quick_gelu")}
    _note(f"tgelu_v{variant}_{m}x{n}x{k}_ratio_bias_wrong", (round(top, 4), round(bias_u, 5), {k_: round(v, 2) for k_, v in wrong.items()}))
    assert wrong["gelu"] > 1.0 and wrong["quick_gelu"] > 1.0, wrong


def test_tanh_gelu_epilogue_tails(device):
    """Large |x|, the treatment the QuickGELU epilogue has: x >= 6 comes back as x itself rounded once, x <= -10 as a zero or a tiny
    negative number within the budget, nothing is NaN or inf."""
    m, n, k = 64, 1024, 256
    g = torch.Generator().manual_seed(5)
    a = torch.zeros(256, k).to(torch.bfloat16)
    w = torch.randn(n, k, generator=g).to(torch.bfloat16)
    bias = torch.cat([torch.linspace(-60, -10, n // 2), torch.linspace(6, 60, n // 2)])
    og = engine.op_gemm(a.to(device), w.to(device), bias.to(device), m, EPI_T)[:m].double().cpu()
    assert bool(torch.isfinite(og).all())
    want = R.rne_bf16(bias.double()).expand(m, n)
    assert torch.equal(og[:, n // 2:], want[:, n // 2:])
    assert bool((og[:, : n // 2] <= 0).all()) and float(og[:, : n // 2].abs().max()) <= 1e-30


# ------------------------------------------------------------------------------------------------ patch front
def _front_state(arch, seed):
    """Integer-valued patch weights, bias and positional table (exact in bf16 / fp32, sums far below 2^24) on the seeded weights."""
    g = torch.Generator().manual_seed(seed)
    sd = dict(S.weights(arch))
    sd["visual.conv1.weight"] = torch.randint(-2, 3, sd["visual.conv1.weight"].shape, generator=g).float()
    sd["visual.conv1.bias"] = torch.randint(-7, 8, sd["visual.conv1.bias"].shape, generator=g).float()
    sd["visual.positional_embedding"] = torch.randint(-50, 51, sd["visual.positional_embedding"].shape, generator=g).float()
    return sd


@pytest.mark.parametrize("variant", [0, 2])                 # the library's choice (128 x 128 tiles at these sizes), the 256 x 256 kernel forced
@pytest.mark.parametrize("name", ["tiny-siglip", "tiny-siglip-196"])
@pytest.mark.parametrize("batch", [3, 9])
def test_patch_front_without_class_token(device, name, batch, variant):
    """One non-zero patch per image, integers: row p of image b is exactly w . px + bias + pos[p] where the patch is, bias + pos[p]
    elsewhere; no row 0 is reserved for a class token (batch * patches rows, the first of them a patch row)."""
    arch = ARCHS[name]
    sd = _front_state(arch, 7)
    eng = engine.ClipEngine(arch, device, precision="bf16")
    eng.load_state_dict(sd)
    g = torch.Generator().manual_seed(batch)
    P, p, grid = arch.grid ** 2, arch.patch, arch.grid
    px = torch.zeros(batch, 3, arch.image_size, arch.image_size)
    where = [(b * 5 + (0 if b == 0 else 3)) % P for b in range(batch)]          # image 0: the FIRST patch (the row CLIP gives its class token)
    for b, pi in enumerate(where):
        y, x = divmod(pi, grid)
        px[b, :, y * p:(y + 1) * p, x * p:(x + 1) * p] = torch.randint(-4, 5, (3, p, p), generator=g).float()
    with debug.override(gemm_variant=variant):
        got = debug.image_tokens(eng, px.to(device))
    assert tuple(got.shape) == (batch * P, arch.v_width)
    want = S.vision_tokens(sd, arch, px).reshape(batch * P, arch.v_width)
    assert torch.equal(got.double().cpu(), want)
    with debug.override(gemm_variant=variant):
        again = debug.image_tokens(eng, px.to(device))
    assert torch.equal(got, again)
    base = (sd["visual.positional_embedding"] + sd["visual.conv1.bias"]).double()
    for b, pi in enumerate(where):
        rows = got[b * P:(b + 1) * P].double().cpu()
        other = torch.arange(P) != pi
        assert torch.equal(rows[other], base[other]) and not torch.equal(rows[pi], base[pi])


# ------------------------------------------------------------------------------------------------ the pooling head
def _head_state(arch, seed):
    """The seeded weights with the head's in_proj made exact: q, k and v weights are permutation matrices, the k / v biases multiples
    of 1/8, so that with token rows in eighths the k | v GEMM's bf16 outputs are exact and the attention kernel's operands are known."""
    g = torch.Generator().manual_seed(seed)
    W = arch.v_width
    sd = dict(S.weights(arch))
    eye = torch.eye(W)
    sd["visual.attn_pool.in_proj_weight"] = torch.cat([eye[torch.randperm(W, generator=g)] for _ in range(3)], dim=0)
    b = sd["visual.attn_pool.in_proj_bias"].clone()
    b[W:] = torch.randint(-8, 9, (2 * W,), generator=g).float() / 8
    sd["visual.attn_pool.in_proj_bias"] = b
    return sd


# the head at the widths and token counts of the registered models too: one-layer towers of ViT-B's 768 at 256 tokens and ViT-L's 1024 at 1024
HEAD_ARCHS = {**{n: ARCHS[n] for n in ("tiny-siglip", "tiny-siglip-196", "tiny-siglip-576")},
              "w768-t256": ClipArch(768, 256, 16, 768, 1, 256, 1, vocab=512, ctx=16, family="siglip"),
              "w1024-t1024": ClipArch(1024, 512, 16, 1024, 1, 256, 1, vocab=512, ctx=16, family="siglip")}


@pytest.mark.parametrize("name,batch", [("tiny-siglip", 5), ("tiny-siglip-196", 5), ("tiny-siglip-576", 3), ("w768-t256", 3), ("w1024-t1024", 2)])
def test_map_head_against_fp64(device, name, batch):
    """kemr_debug_map_head on token rows in eighths within +-4: the attention output within the pooled-row kernel's budget
    (R._attention_chunked, one chunk holding every key, as tests/test_headdim_ops_gpu.py::test_pooled_row_against_fp64) for the query
    finalize makes -- (probe . Wq^T + bq) / 8 in fp32, rounded to bf16 once -- and the head's output row within 1 - cos 1e-3 of the
    fp64 statement; two launches give the same bits."""
    arch = HEAD_ARCHS[name]
    W, T = arch.v_width, arch.v_tokens
    sd = _head_state(arch, 11)
    eng = engine.ClipEngine(arch, device)
    eng.load_state_dict(sd)
    g = torch.Generator().manual_seed(T)
    h = (torch.randint(-32, 33, (batch * T, W), generator=g).float() / 8).to(torch.bfloat16)
    out, attn = debug.map_head(eng, h.to(device), batch)
    out2, attn2 = debug.map_head(eng, h.to(device), batch)
    assert torch.equal(out, out2) and torch.equal(_bits(attn), _bits(attn2))
    wq, wk, wv = sd["visual.attn_pool.in_proj_weight"].split(W, dim=0)
    bq, bk, bv = sd["visual.attn_pool.in_proj_bias"].split(W, dim=0)
    q = (((sd["visual.attn_pool.probe"] @ wq.T) + bq) * 0.125).to(torch.bfloat16)          # a permutation: the fp32 sum is exact
    k, v = h.float() @ wk.T + bk, h.float() @ wv.T + bv
    assert torch.equal(k.to(torch.bfloat16).float(), k) and torch.equal(v.to(torch.bfloat16).float(), v)
    qkv = torch.cat([torch.zeros_like(k), k, v], dim=1).to(torch.bfloat16)
    ref, extra = H.attention_pooled_statement(q.expand(batch, W).contiguous(), qkv, batch, T, W, 64)
    top, bias = R.check_budget(attn.cpu(), ref, extra, max_bias=MAX_BIAS, what=f"map_head_attention_t{T}", bias_rounding_only=True)
    want, want_attn = S.map_head(sd, arch, h.double().view(batch, T, W), return_attention=True)
    assert float((want_attn - ref).abs().max()) <= 2.0 ** -6 * float(ref.abs().max())      # the two statements agree up to the rounding of q
    miss = float(S.one_minus_cos(out, want).max())
    _note(f"map_head_t{T}_attention_ratio_bias_row_1-cos", (round(top, 4), round(bias, 5), f"{miss:.3e}"))
    assert miss <= COS_TOL
    norm, _ = debug.map_head(eng, h.to(device), batch, normalize=True)
    assert float((norm.double().norm(dim=-1) - 1).abs().max()) <= 1e-6
    assert float(S.one_minus_cos(norm, want).max()) <= COS_TOL
