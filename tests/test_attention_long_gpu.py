"""GPU: non-causal attention beyond 288 tokens (csrc/attention_stream.hip, fixed length: K / V streamed through LDS with an online softmax) against
the fp32 softmax of the same bf16 inputs, with the bars of tests/test_ops_gpu.py::test_attention, and against the fp64 statement of
its chunked rounding (oracle/rounding.py attention_long_emulation: budget ratio <= 1, |signed bias| <= 0.02 ulp); and the pooled-row
attention of the last block at 577 tokens."""
import pytest
import torch

from knowledge_enhanced_multimodal_retrieval_amd import engine
from knowledge_enhanced_multimodal_retrieval_amd.config import ClipArch
from oracle import clip_ref
from oracle import rounding as R

pytestmark = pytest.mark.gpu
T_MAX = 1025                       # include/kemr.h KEMR_MAX_VISION_TOKENS


def _ref(qkv, batch, t, width):
    heads = width // 64
    q, k, v = qkv.float().view(batch, t, 3, heads, 64).permute(2, 0, 3, 1, 4)
    return (torch.softmax(q @ k.transpose(-1, -2), -1) @ v).transpose(1, 2).reshape(batch * t, width)


def _check(device, qkv_bf, batch, t, width, max_bias=0.02):
    ref = _ref(qkv_bf, batch, t, width)
    got = engine.op_attention(qkv_bf.to(device), batch, t, width, False).float().cpu()
    assert torch.isfinite(got).all()
    err = (got - ref).abs()
    assert float(err.max()) < 3e-2 and float(err.mean()) < 3e-3, (t, width, float(err.max()), float(err.mean()))
    ref64, extra = R.attention_long_emulation(qkv_bf, batch, t, width)
    top, bias = R.check_budget(got, ref64, extra, max_bias=max_bias, what=f"attn_long_t{t}_w{width}", bias_rounding_only=True)
    print(f"NUMERICS attn_long_fp32bands_t{t}_w{width}_ratio_bias {(round(top, 4), round(bias, 5))}")
    return got


@pytest.mark.parametrize("t,width,batch", [(289, 256, 3), (320, 256, 3), (577, 256, 3), (600, 256, 3), (T_MAX, 256, 3), (577, 1024, 2)])
def test_long_attention_matches_fp32(device, t, width, batch):
    g = torch.Generator().manual_seed(t + width)
    qkv = torch.randn(batch * t, 3 * width, generator=g)
    qkv[:, :width] *= 0.125 * 2.0                 # pre-scaled queries, logits of a few units
    _check(device, qkv.to(torch.bfloat16), batch, t, width)


@pytest.mark.parametrize("case", ["spike_first_chunk", "spike_last_ragged_chunk", "max_moves_every_chunk", "max_creeps"])
def test_online_rescale(device, case):
    """A key about 20 logits ahead of the rest in the FIRST 64-key chunk (every later chunk must leave it alone), in the last,
    one-key chunk of T = 577 (O and l of 576 keys are rescaled by ~e^-20 at the very end), and logits rising along the keys so
    that every chunk moves every row's maximum: by about 10 (log2 units), and by about 2.6 (rescale factors near 1, many times)."""
    t, batch, width = 577, 2, 256
    g = torch.Generator().manual_seed(11)
    qkv = torch.randn(batch * t, 3 * width, generator=g) * 0.1
    qkv[:, :width] *= 0.5
    for hd in range(width // 64):
        qkv[:, hd * 64] = 4.0                                     # q . k picks up 4 * k[d0] in every head
        if case == "max_moves_every_chunk":
            qkv[:, width + hd * 64] = torch.linspace(-8, 8, t).repeat(batch)      # logits -32 .. 32, rising
        elif case == "max_creeps":
            qkv[:, width + hd * 64] = torch.linspace(-2, 2, t).repeat(batch)      # logits -8 .. 8, rising
        else:
            spike = 5 if case == "spike_first_chunk" else t - 1
            for b in range(batch):
                qkv[b * t + spike, width + hd * 64] = 5.0         # logit 20 over ~0
    # spikes: most outputs sit just below a bf16 value (one key takes nearly all the weight), so the exact values do not spread over
    # their ulp intervals and the signed bias is not centred at 0 even for correct rounding -- the ratio bar only
    _check(device, qkv.to(torch.bfloat16), batch, t, width, max_bias=None if case.startswith("spike") else 0.02)


def test_deterministic_and_limits(device):
    t, batch, width = 577, 3, 512
    g = torch.Generator().manual_seed(2)
    qkv = torch.randn(batch * t, 3 * width, generator=g).to(torch.bfloat16).to(device)
    a = engine.op_attention(qkv, batch, t, width, False)
    b = engine.op_attention(qkv, batch, t, width, False)
    assert torch.equal(a, b)
    big = torch.zeros((T_MAX + 1) * 3 * 256, dtype=torch.bfloat16, device=device)
    with pytest.raises(RuntimeError, match="sequence length 1026"):
        engine.op_attention(big, 1, T_MAX + 1, 256, False)
    with pytest.raises(RuntimeError, match="288"):
        engine.op_attention(big, 1, 289, 256, True)


def test_pooled_row_path_at_577_tokens(device):
    """The last block's pooled-row attention beyond 320 keys: embeddings with and without it agree within the parity bar."""
    oa = dict(clip_ref.ARCHS["tiny"], image_size=192, patch=8, v_width=256, v_layers=2)      # 24 x 24 + 1 = 577 tokens
    arch = ClipArch(**oa)
    assert arch.v_tokens == 577
    sd = clip_ref.random_state_dict(oa, seed=4)
    eng = engine.ClipEngine(arch, device)
    eng.load_state_dict(sd)
    px = torch.randn(6, 3, 192, 192, generator=torch.Generator().manual_seed(5)).to(device)
    eng.set_last_block_pooled_row(True)
    assert eng.last_block_pooled_row()
    pooled = eng.encode_image(px).cpu()
    eng.set_last_block_pooled_row(False)
    assert not eng.last_block_pooled_row()
    full = eng.encode_image(px).cpu()
    # the pooled-row path (compact GEMMs, the pooled-row attention kernel) sums in another order than the full last block: if the
    # library skipped it at 577 tokens, both runs would give the same bits
    assert not torch.equal(pooled, full)
    cos = torch.nn.functional.cosine_similarity(pooled.double(), full.double(), dim=-1)
    assert float((1 - cos).max()) < 1e-3
    ref = clip_ref.encode_image(sd, oa, px.cpu())
    cos_ref = torch.nn.functional.cosine_similarity(pooled.double(), ref.double(), dim=-1)
    assert float((1 - cos_ref).max()) < 1e-3
