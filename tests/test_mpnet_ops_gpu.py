"""GPU: the bias instantiation of the packed attention kernel (csrc/attention_stream.hip, model family 3: MPNet's relative position
bias) alone -- against its fp64 statement and rounding budget (tests/mpnet_ref.py attention_varlen_bias_emulation, the biased
restatement of oracle.rounding.attention_long_emulation) with the bars of tests/test_bert_ops_gpu.py (budget ratio <= 1, |signed bias|
<= 0.02 ulp); a zero table against the kernel without bias, bit for bit; isolation and repeatability; the memory and stream
contracts (tests/footprint.py, tests/stream_order.py)."""
import ctypes as C

import pytest
import torch

import footprint as F
import mpnet_ref as M
import stream_order as SO
from footprint import In, IntIn, Out
from knowledge_enhanced_multimodal_retrieval_amd import _lib, debug, hf_checkpoint
from oracle import rounding as R

pytestmark = pytest.mark.gpu

MAX_BIAS = 0.02
MAX_T = 512
BF16 = torch.bfloat16


def _note(name, value):
    print(f"NUMERICS {name} {value}")


def _qkv(rows, width, seed, qscale=0.25):
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(rows, 3 * width, generator=g)
    qkv[:, :width] *= qscale                    # pre-scaled queries: logits of a few units, like the bias
    return qkv.to(BF16)


def _row_start(lens):
    return torch.tensor([0] + list(lens)).cumsum(0).int()


def _table(width):
    """The table by distance of the fixture's bias (2.0 N(0, 1), seed 3) at width / 64 heads: fp32 [heads, 1023]."""
    return M.cached(("mpnet_table", width), lambda: hf_checkpoint.bias_by_distance(M.bias_weight(width // 64)))


def _reference(order, width):
    """(qkv, row_start, table, ref, extra) of the length set in the given order: computed once per (order, width), shared, never modified."""
    def make():
        rs = _row_start(M.LENGTHS if order == "sorted" else M.SHUFFLED)
        qkv = _qkv(int(rs[-1]), width, 700 + width)
        return (qkv, rs, _table(width)) + M.attention_varlen_bias_emulation(qkv, rs, width, _table(width))
    return M.cached(("mpnet_varlen", order, width), make)


@pytest.mark.parametrize("order,width", [("sorted", 256), ("shuffled", 256), ("sorted", 768), ("shuffled", 768)])
def test_biased_attention_against_per_item_emulation(device, order, width):
    """All sixteen lengths 1 .. 512 in one packed call of 2 418 rows: every bucket threshold, every tile, chunk and query-block edge and
    d = +-511 are crossed.  A length-1 item returns its V row exactly (one key: the softmax of one score, whatever its bias)."""
    qkv, rs, table, ref, extra = _reference(order, width)
    assert int(rs[-1]) == 2418
    got = debug.op_attention_varlen_bias(qkv.to(device), rs.to(device), table.to(device), MAX_T, width, fill=float("nan")).cpu()
    assert bool(torch.isfinite(got).all())                   # every row of every item was written
    top, bias = R.check_budget(got, ref, extra, max_bias=MAX_BIAS, what=f"attn_varlen_bias_{order}_w{width}", bias_rounding_only=True)
    _note(f"attn_varlen_bias_{order}_w{width}_ratio_bias", (round(top, 4), round(bias, 5)))
    ones = [int(a) for a, e in zip(rs[:-1], rs[1:]) if e - a == 1]
    assert ones and all(torch.equal(got[a], qkv[a, 2 * width:]) for a in ones)
    # the bias is seen: the same rows without it are far outside the budget
    plain = debug.op_attention_varlen(qkv.to(device), rs.to(device), MAX_T, width).cpu()
    assert float(R.budget_ratio(plain, ref, extra).max()) > 100.0


@pytest.mark.parametrize("width", [256, 768])
def test_zero_table_is_the_kernel_without_bias_bit_for_bit(device, width):
    qkv, rs, table, _, _ = _reference("shuffled", width)
    qd, rd = qkv.to(device), rs.to(device)
    base = debug.op_attention_varlen(qd, rd, MAX_T, width)
    zero = debug.op_attention_varlen_bias(qd, rd, torch.zeros_like(table).to(device), MAX_T, width)
    assert torch.equal(base, zero)
    assert not torch.equal(base, debug.op_attention_varlen_bias(qd, rd, table.to(device), MAX_T, width))


def test_biased_items_are_isolated_and_runs_repeat(device):
    """tests/test_bert_ops_gpu.py test_varlen_items_are_isolated_and_runs_repeat for the bias instantiation: every OTHER item's rows NaN
    leaves an item's output bit-identical; two runs give the same bits; rows no item owns are not written; the refusals hold."""
    width = 256
    qkv, rs, table, _, _ = _reference("shuffled", width)
    qd, rd, td = qkv.to(device), rs.to(device), table.to(device)
    base = debug.op_attention_varlen_bias(qd, rd, td, MAX_T, width)
    assert torch.equal(base, debug.op_attention_varlen_bias(qd, rd, td, MAX_T, width))
    for i in (0, 3, 7, len(M.SHUFFLED) - 1):
        a, e = int(rs[i]), int(rs[i + 1])
        poisoned = torch.full_like(qd, float("nan"))
        poisoned[a:e] = qd[a:e]
        got = debug.op_attention_varlen_bias(poisoned, rd, td, MAX_T, width)
        assert torch.equal(got[a:e], base[a:e]), (i, a, e)
    # a launch over the middle items only: the rows in front of row_start[0] and behind row_start[batch] keep their fill
    sub = rs[4:9].to(device)
    got = debug.op_attention_varlen_bias(qd, sub, td, MAX_T, width, fill=7.0)
    a, e = int(rs[4]), int(rs[8])
    assert torch.equal(got[a:e], base[a:e]) and bool((got[:a] == 7.0).all()) and bool((got[e:] == 7.0).all())
    # an item's output depends on its own positions only: the same rows as the first item of a launch and as a later one
    j = M.SHUFFLED.index(257)
    a, e = int(rs[j]), int(rs[j + 1])
    alone = debug.op_attention_varlen_bias(qd[a:e].contiguous(), torch.tensor([0, e - a], dtype=torch.int32, device=device), td, MAX_T, width)
    assert torch.equal(alone, base[a:e])
    with pytest.raises(RuntimeError, match="not in 1..512"):
        debug.op_attention_varlen_bias(qd, rd, td, 513, width)
    with pytest.raises(RuntimeError, match="multiple of the head dim 64"):
        _lib.check(_lib.lib().kemr_debug_op_attention_varlen_bias(C.c_void_p(qd.data_ptr()), C.c_void_p(base.data_ptr()), C.c_void_p(rd.data_ptr()),
                                                                  C.c_void_p(td.data_ptr()), len(M.SHUFFLED), MAX_T, 96, None), "debug_op_attention_varlen_bias")
    assert _lib.lib().kemr_debug_op_attention_varlen_bias(C.c_void_p(qd.data_ptr()), C.c_void_p(base.data_ptr()), C.c_void_p(rd.data_ptr()), None,
                                                          len(M.SHUFFLED), MAX_T, width, None) == -1
    assert b"null argument" in _lib.lib().kemr_last_error()


# ------------------------------------------------------------------------------------------------ memory and stream contracts
def _specs(width, lens, seed):
    rs = _row_start(lens)
    rows = int(rs[-1])
    return [In(_qkv(rows, width, seed, qscale=0.125)), Out((rows, width), BF16), IntIn(rs), In(_table(width)), len(lens), MAX_T, width], rs


def _run(device, name):
    fn = getattr(_lib.lib(), name)

    def run(*args):
        with torch.cuda.device(device):
            _lib.check(fn(*args, C.c_void_p(torch.cuda.current_stream(device).cuda_stream)), name)
    return run


@pytest.mark.parametrize("width,lens", [(256, [1, 17, 512]), (768, [65, 1, 129, 511])])
def test_biased_attention_memory_contract(device, width, lens):
    """Plain call against the call on windows (poisoned margins around qkv, row_start and the table; guarded output): the same bits,
    every margin intact -- the table is read inside its [heads, 1023] floats only, exactly the items' rows are written."""
    specs, _ = _specs(width, lens, 21)
    calls = F.run_both(_run(device, "kemr_debug_op_attention_varlen_bias"), specs, device, what=f"varlen attention with bias w={width}")
    assert bool(torch.isfinite(calls.win[1].view.float()).all())


def test_biased_attention_stream_contract(device):
    """On a side stream behind a device-side delay, the inputs still poison when the call returns: no host synchronisation, the same
    bits, the default stream idle (tests/stream_order.py S1 - S3)."""
    lens = [1, 17, 512]
    specs, rs = _specs(256, lens, 22)
    other = _row_start(lens[::-1])
    SO.run_late(_run(device, "kemr_debug_op_attention_varlen_bias"), specs, device, what="varlen attention with bias", stale={2: other})
