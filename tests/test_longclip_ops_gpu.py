"""GPU: the causal attention over packed items of 129 .. 288 rows alone (csrc/attention_stream.hip, PACKED CAUSAL instantiation; reached
through launch_attention_packed / kemr_debug_op_attention_packed), the kernel Long-CLIP's 248-position text towers run on.

The kernel is the streaming kernel of the BERT family with the chunk loop cut at the query block's diagonal, so the reference is the
same fp64 statement, ``oracle.rounding._attention_chunked`` in chunks of 64 keys, given the lower-triangular key mask per item
(tests/longclip_ref.py), with the bars of tests/test_bert_ops_gpu.py: budget ratio <= 1, |signed bias| <= 0.02 ulp over the outputs
the final rounding dominates."""
import ctypes as C

import pytest
import torch

import footprint as F
import longclip_ref as L
import stream_order as SO
from footprint import In, IntIn, Out
from knowledge_enhanced_multimodal_retrieval_amd import _lib, debug, engine
from oracle import rounding as R

pytestmark = pytest.mark.gpu

MAX_BIAS = 0.02
BF16 = torch.bfloat16


def _note(name, value):
    print(f"NUMERICS {name} {value}")


def _check(got, ref, extra, what, max_bias=MAX_BIAS):
    top, bias = R.check_budget(got.cpu(), ref, extra, fmt="bf16", max_bias=max_bias, what=what, bias_rounding_only=True)
    _note(f"{what}_ratio_bias", (round(top, 4), round(bias, 5)))


def _packed(device, qkv, rs, max_t, width):
    """kemr_debug_op_attention_packed on host tensors (rows no item owns stay 0)."""
    return debug.op_attention_packed(qkv.to(device), rs.to(device), max_t, width)


# ------------------------------------------------------------------------------------------------ lengths
@pytest.mark.parametrize("order,width", [("sorted", 128), ("shuffled", 128), ("sorted", 768)])
def test_packed_causal_attention_against_per_item_statement(device, order, width):
    """Lengths 1 .. 288 at the edges of a 16-query tile, a 64-key chunk and a 128-query block, 2 009 rows in one launch at max_t = 288."""
    qkv, rs, ref, extra = L.length_case(order, width)
    assert int(rs[-1]) == 2009
    got = _packed(device, qkv, rs, L.MAX_T, width).cpu()
    assert bool(torch.isfinite(got).all())
    _check(got, ref, extra, f"attn_packed_causal_{order}_w{width}")
    starts = rs[:-1].long()
    assert torch.equal(got[starts], qkv[starts, 2 * width:])          # row 0 of every item sees one key: its V row, exactly
    # against the fp32 causal softmax of the same bf16 inputs, with the bars of tests/test_attention_long_gpu.py
    worst, mean = 0.0, 0.0
    for a, e in zip(rs[:-1].tolist(), rs[1:].tolist()):
        q, k, v = qkv[a:e].float().view(e - a, 3, width // 64, 64).permute(1, 2, 0, 3)
        s = q @ k.transpose(-1, -2) + torch.full((e - a, e - a), float("-inf")).triu_(1)
        o = (torch.softmax(s, -1) @ v).transpose(0, 1).reshape(e - a, width)
        err = (got[a:e].float() - o).abs()
        worst, mean = max(worst, float(err.max())), mean + float(err.sum())
    assert worst < 3e-2 and mean / got.numel() < 3e-3, (worst, mean / got.numel())


# ------------------------------------------------------------------------------------------------ online rescale
@pytest.mark.parametrize("case", ["spike_first_chunk", "spike_diagonal_chunk", "max_moves_every_chunk", "max_creeps"])
def test_packed_causal_online_rescale(device, case):
    """tests/test_bert_ops_gpu.py::test_varlen_online_rescale under the causal mask.  A key ~20 logits ahead at position 5 (first chunk:
    rows 0 .. 4 of the first tile do not see it, every later row does and carries its maximum through every later chunk) or at
    position n - 8 (the diagonal chunk of the item's last rows: in the tile that holds it the rows before it are masked, the rows from
    it on meet their maximum in their LAST chunk and rescale everything before by ~e^-20); logits rising along the keys so that every
    chunk -- and inside the diagonal chunk every further visible key -- moves the maximum.  Items of 257, 65 and 288 rows."""
    width, lens = 256, [257, 65, 288]
    rs = L.row_start(lens)
    g = torch.Generator().manual_seed(11)
    qkv = torch.randn(int(rs[-1]), 3 * width, generator=g) * 0.1
    qkv[:, :width] *= 0.5
    for hd in range(width // 64):
        qkv[:, hd * 64] = 4.0                                      # q . k picks up 4 * k[d0] in every head
        for a, n in zip(rs[:-1].tolist(), lens):
            if case == "max_moves_every_chunk":
                qkv[a:a + n, width + hd * 64] = torch.linspace(-8, 8, n)          # logits -32 .. 32, rising
            elif case == "max_creeps":
                qkv[a:a + n, width + hd * 64] = torch.linspace(-2, 2, n)          # logits -8 .. 8, rising
            else:
                qkv[a + (5 if case == "spike_first_chunk" else n - 8), width + hd * 64] = 5.0      # logit 20 over ~0
    qkv = qkv.to(BF16)
    got = _packed(device, qkv, rs, L.MAX_T, width)
    ref, extra = L.causal_reference(qkv, rs, width)
    # spikes: most outputs sit just below a bf16 value, so the signed bias is not centred at 0 even for correct rounding -- ratio only
    _check(got, ref, extra, f"attn_packed_causal_{case}", max_bias=None if case.startswith("spike") else MAX_BIAS)


# ------------------------------------------------------------------------------------------------ isolation, repeatability, refusals
def test_items_are_isolated_runs_repeat_and_limits(device):
    """Overwriting every OTHER item's q | k | v rows with NaN leaves an item's output bit-identical; two launches give the same bits;
    rows no item owns are not written; a length beyond max_t is clamped to it (the item's first max_t rows are those of an item of
    that length, the rows behind stay unwritten); max_t = 289 and a width that is no multiple of 64 are refused."""
    width = 128
    qkv, rs, _, _ = L.length_case("shuffled", width)
    qd, rd = qkv.to(device), rs.to(device)
    base = debug.op_attention_packed(qd, rd, L.MAX_T, width)
    assert torch.equal(base, debug.op_attention_packed(qd, rd, L.MAX_T, width))
    for i in (0, 3, 7, len(L.SHUFFLED) - 1, L.SHUFFLED.index(288), L.SHUFFLED.index(129)):
        a, e = int(rs[i]), int(rs[i + 1])
        poisoned = torch.full_like(qd, float("nan"))
        poisoned[a:e] = qd[a:e]
        got = debug.op_attention_packed(poisoned, rd, L.MAX_T, width)
        assert torch.equal(got[a:e], base[a:e]), (i, a, e)
    # a launch over the middle items only: the rows in front of row_start[0] and behind row_start[batch] are not written
    a, e = int(rs[4]), int(rs[8])
    out = torch.full((qd.shape[0], width), 7.0, dtype=BF16, device=device)
    with torch.cuda.device(device):
        _lib.check(_lib.lib().kemr_debug_op_attention_packed(C.c_void_p(qd.data_ptr()), C.c_void_p(out.data_ptr()), C.c_void_p(rd[4:9].contiguous().data_ptr()),
                                                             4, L.MAX_T, width, C.c_void_p(torch.cuda.current_stream(device).cuda_stream)), "op_attention_packed")
    assert torch.equal(out[a:e], base[a:e]) and bool((out[:a] == 7.0).all()) and bool((out[e:] == 7.0).all())
    # lengths beyond max_t are clamped: one item of 288 rows at max_t = 200 computes its first 200 rows as an item of 200 rows
    i = L.SHUFFLED.index(288)
    a = int(rs[i])
    one = torch.tensor([0, 288], dtype=torch.int32, device=device)
    cut = torch.tensor([0, 200], dtype=torch.int32, device=device)
    item = qd[a:a + 288].contiguous()
    got = debug.op_attention_packed(item, one, 200, width)
    want = debug.op_attention_packed(item[:200].contiguous(), cut, 200, width)
    assert torch.equal(got[:200], want) and not bool(got[200:].any())
    assert torch.equal(want, base[a:a + 200])                        # causal: the first 200 rows of the 288-row item, whatever max_t
    with pytest.raises(RuntimeError, match="288"):
        debug.op_attention_packed(qd, rd, 289, width)
    with pytest.raises(RuntimeError, match="bad shape"):
        debug.op_attention_packed(qd, rd, L.MAX_T, 96)


# ------------------------------------------------------------------------------------------------ against the dense causal kernel
@pytest.mark.parametrize("t", [248, 288])
def test_against_dense_causal_kernel(device, t):
    """Equal-length items through the packed entry and through kemr_op_attention(causal): two kernels, two statements (P rounded
    against the running maximum of 64-key chunks / against the row's final maximum), each within its own budget, and the two outputs
    within the SUM of the two budgets of each other."""
    batch, width = 3, 128
    qkv = L.qkv(batch * t, width, 900 + t)
    rs = L.row_start([t] * batch)
    got = _packed(device, qkv, rs, t, width).cpu()
    dense = engine.op_attention(qkv.to(device), batch, t, width, True).cpu()
    ref, extra = L.causal_reference(qkv, rs, width)
    refd, extrad = R.attention_emulation(qkv, batch, t, width, True)
    _check(got, ref, extra, f"attn_packed_causal_equal_t{t}")
    top, _ = R.check_budget(dense, refd, extrad, fmt="bf16", what=f"attn_dense_causal_t{t}")
    budget = (0.5 * R.ulp(got) + extra) + (0.5 * R.ulp(dense) + extrad)
    ratio = float(((got.double() - dense.double()).abs() / budget).max())
    _note(f"attn_packed_vs_dense_t{t}_dense_ratio_and_mutual_ratio", (round(top, 4), round(ratio, 4)))
    assert ratio <= 1.0, (t, ratio)


# ------------------------------------------------------------------------------------------------ routing
def test_max_t_128_keeps_the_tile_kernels_bits(device):
    """max_t <= 128 stays on the tile kernels of csrc/attention.hip: the output bits are those of the commit before the streaming route
    existed (tests/golden/longclip_packed_t128.json holds their sha256, recorded there on an MI355X), per route of launch_nt<1..4>."""
    qkv, rs = L.routing_case()
    gold = L.routing_golden()
    assert gold["lens"] == L.ROUTING_LENS and gold["width"] == L.ROUTING_WIDTH
    for max_t in (32, 64, 96, 128):
        n = sum(1 for x in L.ROUTING_LENS if x <= max_t)          # the items that fit (sorted ascending)
        sub = rs[:n + 1]
        got = _packed(device, qkv, sub, max_t, L.ROUTING_WIDTH)[:int(sub[-1])]
        assert L.checksum(got) == gold["sha256"][str(max_t)], max_t


# ------------------------------------------------------------------------------------------------ contracts
def _lens_and_rows():
    lens = [1, 17, 129, 248, 200]
    rs = L.row_start(lens)
    return lens, rs, int(rs[-1])


def test_memory_contract(device):
    """tests/footprint.py: the same bits on windows whose margins hold NaN bytes (qkv), 0x7fffffff (row_start) and guard bytes (out);
    every margin intact; and of `out` exactly the launch's rows written (a launch over the middle items leaves the rest alone)."""
    width = 128
    lens, rs, rows = _lens_and_rows()
    fn = _lib.lib().kemr_debug_op_attention_packed

    def run(*args):
        with torch.cuda.device(device):
            _lib.check(fn(*args, C.c_void_p(torch.cuda.current_stream(device).cuda_stream)), "op_attention_packed")
    F.run_both(run, [In(L.qkv(rows, width, 5)), Out((rows, width), BF16), IntIn(rs), len(lens), 248, width], device, what="packed causal attention")
    a, e = int(rs[1]), int(rs[4])
    F.run_both(run, [In(L.qkv(rows, width, 5)), Out((rows, width), BF16, written=lambda v: v[a:e], keep=lambda v: [v[:a], v[e:]]), IntIn(rs[1:5]), 3, 248, width],
               device, what="packed causal attention, middle items")


def test_stream_contract(device):
    """tests/stream_order.py at max_t = 248: enqueued on a side stream while its inputs do not exist yet (row_start: the same lengths
    in reverse order), the call returns at once, gives the plain call's bits and leaves the default stream idle."""
    width = 128
    lens, rs, rows = _lens_and_rows()
    other = L.row_start(lens[::-1])
    fn = _lib.lib().kemr_debug_op_attention_packed

    def run(*args):
        with torch.cuda.device(device):
            _lib.check(fn(*args, C.c_void_p(torch.cuda.current_stream(device).cuda_stream)), "op_attention_packed")
    SO.run_late(run, [In(L.qkv(rows, width, 5)), Out((rows, width), BF16), IntIn(rs), len(lens), 248, width], device,
                what="packed causal attention", stale={2: other})
