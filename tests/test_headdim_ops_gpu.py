"""GPU: the three head-dim-80 attention kernels (csrc/attention80.hip) through their op-level entry points -- kemr_op_attention_hd,
kemr_debug_op_attention_pooled_hd, kemr_op_attention_x3_hd -- against the fp64 statements of tests/headdim_ref.py, held to rounding
budgets (oracle/rounding.py; tests/test_headdim_host.py shows that the bars can fail).  Widths 240 (3 heads) and, once per kernel, 1280
(16 heads: ViT-H-14's vision tower); batches 3 and 9 (9 is no multiple of the 8 XCDs the tile kernel deals the images to).  Every
measured figure is printed as a NUMERICS line (pytest -s)."""
import pytest
import torch

import headdim_ref as H
from knowledge_enhanced_multimodal_retrieval_amd import debug, engine
from oracle import rounding as R

pytestmark = pytest.mark.gpu

HD = 80
MAX_BIAS = 0.02            # ulp: the |signed bias| bar of tests/test_numerics_paths_gpu.py
QSCALE = 2.0 / HD ** 0.5   # pre-scaled queries: logits of std 2, as 0.25 gives at head dim 64


def _note(name, value):
    print(f"NUMERICS {name} {value}")


def _bits(t):
    return t.contiguous().view(torch.int16)


def _qkv(rows, width, seed, qscale=QSCALE):
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(rows, 3 * width, generator=g)
    qkv[:, :width] *= qscale
    return qkv


# ------------------------------------------------------------------------------------------------ tile kernel
def _check_tile(device, qkv_bf, batch, t, width, what):
    got = engine.op_attention(qkv_bf.to(device), batch, t, width, False, head_dim=HD)
    again = engine.op_attention(qkv_bf.to(device), batch, t, width, False, head_dim=HD)
    assert torch.equal(_bits(got), _bits(again)), "two launches, two results"
    ref, extra = H.attention_statement(qkv_bf, batch, t, width, HD)
    top, bias = R.check_budget(got.cpu(), ref, extra, limit=1.0, what=what)
    _note(f"{what}_ratio_bias", (round(top, 4), round(bias, 5)))
    return got.cpu()


@pytest.mark.parametrize("batch", [3, 9])
@pytest.mark.parametrize("t", [1, 17, 50, 257, 288])
def test_tile_kernel_against_the_statement(device, t, batch):
    """Every length at which the kernel takes another path: one query, a ragged tile, T = 257 (the compile-time specialisation, eight
    waves), T = 288 (nine full key blocks, run-time T); two launches give the same bits."""
    width = 240
    _check_tile(device, _qkv(batch * t, width, 13 * t + batch).to(torch.bfloat16), batch, t, width, f"attn80_t{t}_b{batch}_w{width}")


def test_tile_kernel_at_the_width_of_vit_h_14(device):
    batch, t, width = 3, 257, 1280
    _check_tile(device, _qkv(batch * t, width, 5).to(torch.bfloat16), batch, t, width, f"attn80_t{t}_b{batch}_w{width}")


@pytest.mark.parametrize("waves", [4, 8])
def test_tile_kernel_wave_counts_give_the_same_bits(device, waves):
    """debug switch attn80_waves: four or eight waves per workgroup at T = 257 share the work differently, not the arithmetic."""
    batch, t, width = 9, 257, 240
    qkv = _qkv(batch * t, width, 77).to(torch.bfloat16).to(device)
    base = engine.op_attention(qkv, batch, t, width, False, head_dim=HD)
    with debug.override(attn80_waves=waves):
        assert torch.equal(_bits(engine.op_attention(qkv, batch, t, width, False, head_dim=HD)), _bits(base))


@pytest.mark.parametrize("t", [257, 288])
def test_tile_kernel_exact_structure(device, t):
    """Integer data.  Key j carries two ones, at column 40 + j % 18 and at column 64 + j // 18; query i has 40 at the two columns of its
    key c(i): that key scores 80, keys that share one column 40, the rest 0.  One key is 40 logits ahead, every other P is below
    e^-40 = 4e-18 of it, so the output is that key's V row -- integers of magnitude 1..8: what the other keys add, below 1e-15, is
    rounded away in fp32 -- in all 80 columns, exactly.  A contraction that ends at column 64 ties 16 keys per query instead."""
    batch, width = 3, 240
    heads = width // HD
    g = torch.Generator().manual_seed(t)
    q = torch.zeros(batch, t, heads, HD)
    k = torch.zeros(batch, t, heads, HD)
    v = torch.randint(1, 9, (batch, t, heads, HD), generator=g).float() * (torch.randint(0, 2, (batch, t, heads, HD), generator=g) * 2 - 1)
    j = torch.arange(t)
    k[:, j, :, 40 + j % 18] = 1.0
    k[:, j, :, 64 + j // 18] = 1.0
    c = (j * 7 + 3) % t                              # query i looks at key c(i)
    q[:, j, :, 40 + c % 18] = 40.0
    q[:, j, :, 64 + c // 18] = 40.0
    qkv = torch.cat([x.reshape(batch * t, width) for x in (q, k, v)], dim=1).to(torch.bfloat16)
    got = engine.op_attention(qkv.to(device), batch, t, width, False, head_dim=HD).cpu()
    want = v[:, c].reshape(batch * t, width).to(torch.bfloat16)
    assert torch.equal(_bits(got), _bits(want))


@pytest.mark.parametrize("head", [0, 1, 2])
def test_tile_kernel_one_hot_queries_and_loud_neighbours(device, head):
    """Query i of the head under test is the one-hot of column i, i = 0..79, so its logits are column i of K: columns 64..79 must count.
    The other heads' q, k and v are LARGE (64, 64, 256): the columns 80..95 of the head under test are the next head's first 16 (for the
    last head the next plane's), and a kernel that loaded them would add 64 x 64 to a logit and 256 to an output.  Against the statement,
    which splits the width into heads of 80."""
    batch, t, width = 2, 80, 240
    heads = width // HD
    g = torch.Generator().manual_seed(head)
    q = torch.full((batch, t, heads, HD), 64.0)
    k = torch.full((batch, t, heads, HD), 64.0)
    v = torch.full((batch, t, heads, HD), 256.0)
    q[:, :, head] = torch.eye(HD)[None] * 2.0
    k[:, :, head] = torch.randint(-2, 3, (batch, t, HD), generator=g).float()
    v[:, :, head] = torch.randint(-8, 9, (batch, t, HD), generator=g).float()
    qkv = torch.cat([x.reshape(batch * t, width) for x in (q, k, v)], dim=1).to(torch.bfloat16)
    got = _check_tile(device, qkv, batch, t, width, f"attn80_one_hot_head{head}")
    mine = got.view(batch, t, heads, HD)[:, :, head].float()
    assert float(mine.abs().max()) <= 8.0             # a convex mix of this head's V rows, nothing of a neighbour's 256
    # rows whose logits differ only in the columns 64..79 of K differ in their output
    assert not torch.equal(mine[:, 64:], mine[:, :16])


# ------------------------------------------------------------------------------------------------ pooled-row kernel
@pytest.mark.parametrize("tokens,width", [(50, 240), (257, 240), (257, 1280)])
def test_pooled_row_against_fp64(device, tokens, width):
    """The budget rule of tests/test_numerics_paths_gpu.py::test_pooled_row_vision_against_fp64 (one chunk of the chunked statement
    holding every key; the bias over the outputs the final rounding dominates), restated for heads of 80."""
    items = 5
    qkv = _qkv(items * tokens, width, tokens + width).to(torch.bfloat16)
    q = (torch.randn(items, width, generator=torch.Generator().manual_seed(tokens)) * QSCALE).to(torch.bfloat16)
    got = debug.op_attention_pooled(q.to(device), qkv.to(device), None, None, tokens, False, head_dim=HD)
    assert torch.equal(_bits(got), _bits(debug.op_attention_pooled(q.to(device), qkv.to(device), None, None, tokens, False, head_dim=HD)))
    ref, extra = H.attention_pooled_statement(q, qkv, items, tokens, width, HD)
    top, bias = R.check_budget(got.cpu(), ref, extra, max_bias=MAX_BIAS, what=f"pooled80_t{tokens}_w{width}", bias_rounding_only=True)
    _note(f"pooled80_t{tokens}_w{width}_ratio_bias", (round(top, 4), round(bias, 5)))


# ------------------------------------------------------------------------------------------------ fp32x3 attention
KAPPA = 8                  # the accumulator bar of tests/test_fp32x3_gpu.py
SPLIT = 2.0 ** -16         # what a pair (hi, lo) leaves of a value


def _attention64(qkv, r0, t, width, head_dim):
    """tests/test_fp32x3_gpu.py::_attention64 (non-causal) with the head dim a parameter: fp64 softmax attention of one item's fp32 rows
    and, per output, |d o| <= (expm1(2 max e_S) + c1 + EXP_ULPS 2^-23) sum_j p_j |v_j|, e_S = c1 sum|q||k|, c1 = 3 2^-16 + KAPPA 2^-24."""
    c1 = 3 * SPLIT + KAPPA * 2.0 ** -24
    x = qkv[r0:r0 + t].double()
    out, bound = torch.empty(t, width, dtype=torch.float64), torch.empty(t, width, dtype=torch.float64)
    for h in range(width // head_dim):
        q, k, v = (x[:, j * width + h * head_dim: j * width + (h + 1) * head_dim] for j in range(3))
        p = torch.softmax(q @ k.T, dim=-1)
        emax = (c1 * (q.abs() @ k.abs().T)).amax(-1, keepdim=True)
        out[:, h * head_dim:(h + 1) * head_dim] = p @ v
        bound[:, h * head_dim:(h + 1) * head_dim] = (torch.expm1(2 * emax) + c1 + R.EXP_ULPS * 2.0 ** -23) * (p @ v.abs())
    return out, bound


@pytest.mark.parametrize("t,batch,width", [(1, 3, 240), (17, 3, 240), (64, 9, 240), (257, 3, 240), (257, 2, 1280)])
def test_attention_x3_against_fp64_of_the_fp32_inputs(device, t, batch, width):
    """The bound of tests/test_fp32x3_gpu.py::_check_attention_x3: hi + lo within the statement's bound plus half an ulp of each stored
    term; the third block repeats hi; same bits on every launch."""
    _check_x3(device, _qkv(batch * t, width, 7 * t + batch), batch, t, width, f"attn80_x3_t{t}_b{batch}_w{width}")


def _check_x3(device, qkv, batch, t, width, what):
    tri = engine.op_attention_x3(qkv.to(device), batch, t, width, False, head_dim=HD)
    again = engine.op_attention_x3(qkv.to(device), batch, t, width, False, head_dim=HD)
    assert torch.equal(_bits(tri), _bits(again)), "two launches, two results"
    tri = tri.cpu()
    hi, lo, third = tri[:, :width], tri[:, width:2 * width], tri[:, 2 * width:]
    assert torch.equal(_bits(hi), _bits(third))
    val = hi.double() + lo.double()
    worst = 0.0
    for b in range(batch):
        ref, bound = _attention64(qkv, b * t, t, width, HD)
        got = val[b * t:(b + 1) * t]
        stored = 0.5 * R.ulp(lo[b * t:(b + 1) * t], "bf16") + 0.5 * R.ulp(got, "fp32")
        ratio = (got - ref).abs() / (bound + stored)
        top = float(torch.nan_to_num(ratio, nan=float("inf")).max())
        assert top <= 1.0, (t, b, R.worst(ratio, got, ref))
        worst = max(worst, top)
    _note(f"{what}_ratio", worst)
    return val


def test_attention_x3_one_hot_queries_and_loud_neighbours(device):
    """The fp32x3 form of the loud-neighbour case, middle head: logits are columns of K (64..79 included), nothing of columns 80..95.
    Held to the bound of the test above (its statement splits the width into heads of 80)."""
    batch, t, width, head = 2, 80, 240, 1
    g = torch.Generator().manual_seed(9)
    q = torch.full((batch, t, 3, HD), 64.0)
    k = torch.full((batch, t, 3, HD), 64.0)
    v = torch.full((batch, t, 3, HD), 256.0)
    q[:, :, head] = torch.eye(HD)[None] * 2.0
    k[:, :, head] = torch.randn(batch, t, HD, generator=g)
    v[:, :, head] = torch.randn(batch, t, HD, generator=g)
    qkv = torch.cat([x.reshape(batch * t, width) for x in (q, k, v)], dim=1)
    val = _check_x3(device, qkv, batch, t, width, "attn80_x3_one_hot").view(batch * t, 3, HD)[:, head]
    assert float(val.abs().max()) <= float(v[:, :, head].abs().max())      # a convex mix of this head's V rows, nothing of a neighbour's 256


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("width,head_dim,causal,msg", [(256, 80, False, "multiple of the head dim"),
                                                       (720, 72, False, "not served"), (1280, 128, False, "not served"),
                                                       (240, 80, True, "causal")])
def test_refusals_launch_nothing(device, width, head_dim, causal, msg):
    """KEMR_ERR_INVALID with a message; the output buffers keep their contents."""
    batch, t = 2, 16
    qkv = torch.zeros(batch * t, 3 * width, dtype=torch.bfloat16, device=device)
    with pytest.raises(RuntimeError, match=msg):
        engine.op_attention(qkv, batch, t, width, causal, head_dim=head_dim)
    with pytest.raises(RuntimeError, match=msg):
        engine.op_attention_x3(qkv.float(), batch, t, width, causal, head_dim=head_dim)
    with pytest.raises(RuntimeError, match=msg):
        debug.op_attention_pooled(qkv[:batch, :width].contiguous(), qkv, None, None, t, causal, head_dim=head_dim)
    import ctypes as C
    from knowledge_enhanced_multimodal_retrieval_amd import _lib
    out = torch.full((batch * t, width), 3.0, dtype=torch.bfloat16, device=device)
    rc = _lib.lib().kemr_op_attention_hd(C.c_void_p(qkv.data_ptr()), C.c_void_p(out.data_ptr()), batch, t, width, head_dim, 1 if causal else 0, None)
    torch.cuda.synchronize(device)
    assert rc == -1 and bool((out == 3.0).all())
