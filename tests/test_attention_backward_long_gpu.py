"""GPU: ``kemr_op_attention_backward_long`` (csrc/attention_bwd_stream.hip), the streaming non-causal attention backward, against the
fp64 statement and the rounding emulation of tests/attention_bwd_ref.py, its exact properties, its memory contract (tests/footprint.py),
its stream contract (tests/stream_order.py), and the route of ``engine.attention_backward``.

Shapes: width 128 (two heads), batch 3, t in {1, 16, 17, 63, 64, 65, 128, 129, 288, 289, 321, 577, 1025}: one key; exact and one-row
ragged 16-row tiles; one 64-row chunk exactly and one row either side of it; two chunks and one row more; both sides of the route
boundary; the forward's ragged cases 289 and 321; ViT-L/14@336px's length; the maximum.  The bar is that of
tests/test_attention_backward_gpu.py: per plane (dq, dk, dv) the relative L2 error against the fp64 statement on the same bf16 inputs
is at most 2 x the emulation's error at that shape.  The emulation rounds where the kernels round (P and dS to bf16 as MFMA operands,
the outputs to bf16; D from the unrounded fp32 P), so the factor covers the order of the fp32 sums -- here also the online rescaling
of the row sum and of D by exp(m - m') -- and the exponential's implementation, and nothing else."""
import ctypes as C
import functools

import pytest
import torch

import attention_bwd_ref as R
import footprint as F
import stream_order as SO
from footprint import In, Out, SizeOf, Work
from knowledge_enhanced_multimodal_retrieval_amd import _lib, engine

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
BATCH, WIDTH, ZERO_ITEM = 3, 128, 1
TS = [1, 16, 17, 63, 64, 65, 128, 129, 288, 289, 321, 577, 1025]
CONTRACT_TS = [17, 65, 289, 577]


@functools.lru_cache(maxsize=None)
def _case(t, width=WIDTH, batch=BATCH):
    """(qkv, dout, fp64 statement, emulation) of one shape: computed once, shared, never modified."""
    qkv, dout = R.make_inputs(batch, t, width, 3000 + 2 * t + width, zero_item=ZERO_ITEM)
    return qkv, dout, R.backward_fp64(qkv, dout, batch, t, width, 0), R.backward_emulated(qkv, dout, batch, t, width, 0)


def _need(batch, t, width):
    return int(_lib.lib().kemr_attention_backward_long_workspace_bytes(batch, t, width))


def _direct(device, qkv, dout, t, width=WIDTH, batch=BATCH):
    """One call of the op itself on tight torch tensors (whatever the engine's route is)."""
    q, d = qkv.to(device), dout.to(device)
    out = torch.empty_like(q)
    need = _need(batch, t, width)
    ws = torch.empty(max(need, 4), dtype=torch.uint8, device=device)
    with torch.cuda.device(device):
        _lib.check(_lib.lib().kemr_op_attention_backward_long(C.c_void_p(q.data_ptr()), C.c_void_p(d.data_ptr()), C.c_void_p(out.data_ptr()),
                                                              batch, t, width, C.c_void_p(ws.data_ptr()), need, R.stream(device)),
                   "op_attention_backward_long")
    return out


@pytest.mark.parametrize("t", TS)
def test_error_against_fp64_within_twice_the_emulation(device, t):
    qkv, dout, ref, emu = _case(t)
    got = _direct(device, qkv, dout, t).cpu()
    R.check_against_fp64(got, ref, emu, WIDTH, f"attention_backward_long t={t}")
    # the item whose dout rows are zero: exactly zero gradients
    assert not got[ZERO_ITEM * t:(ZERO_ITEM + 1) * t].float().any()
    if t == 1:          # one key: P = 1, dS = 0
        g = R.planes(got, WIDTH)
        assert not g["dq"].float().any() and not g["dk"].float().any()
        assert F.same_bits(g["dv"], dout)


def test_head_indexing_at_width_1024(device):
    """ViT-L/14@336px's own shape (16 heads, 577 tokens), batch 2 with item 1 zero: the same bar."""
    t, width, batch = 577, 1024, 2
    qkv, dout, ref, emu = _case(t, width, batch)
    got = _direct(device, qkv, dout, t, width, batch).cpu()
    R.check_against_fp64(got, ref, emu, width, f"attention_backward_long t={t} width={width}")
    assert not got[t:].float().any()


@pytest.mark.parametrize("t", CONTRACT_TS)
def test_two_launches_give_the_same_bits(device, t):
    qkv, dout, _, _ = _case(t)
    assert F.same_bits(_direct(device, qkv, dout, t), _direct(device, qkv, dout, t))


@pytest.mark.parametrize("t", CONTRACT_TS)
def test_an_item_depends_on_its_own_rows_only(device, t):
    """Item 1 of a call whose other items and whose surroundings (0xff margins in front of and behind every buffer) are different."""
    qkv, _, _, _ = _case(t)
    dout = R.make_inputs(BATCH, t, WIDTH, 77 + t)[1]                      # no zero item here
    base = _direct(device, qkv, dout, t).cpu()
    qkv2, dout2 = R.make_inputs(BATCH, t, WIDTH, 555 + t)
    own = slice(t, 2 * t)
    qkv2[own], dout2[own] = qkv[own], dout[own]
    need = _need(BATCH, t, WIDTH)
    wq = F.window(qkv2.shape, BF16, device, F.POISON, body=qkv2, what="qkv")
    wd = F.window(dout2.shape, BF16, device, F.POISON, body=dout2, what="dout")
    wo = F.window(qkv2.shape, BF16, device, F.GUARD, what="dqkv")
    ww = F.window((need,), torch.uint8, device, F.GUARD, body=F.POISON, what="workspace")
    with torch.cuda.device(device):
        _lib.check(_lib.lib().kemr_op_attention_backward_long(C.c_void_p(wq.ptr), C.c_void_p(wd.ptr), C.c_void_p(wo.ptr), BATCH, t, WIDTH,
                                                              C.c_void_p(ww.ptr), need, R.stream(device)), "op_attention_backward_long")
    torch.cuda.synchronize(device)
    assert wq.margins_intact() and wd.margins_intact() and wo.margins_intact() and ww.margins_intact()
    assert F.same_bits(wo.view[own], base[own])
    assert not torch.equal(wo.view[:t].cpu().float(), base[:t].float())       # (the other items did change)


def _specs(t, extra_rows):
    qkv, dout, _, _ = _case(t)
    rows = BATCH * t
    return [In(qkv), In(dout), Out((rows + extra_rows, 3 * WIDTH), BF16, written=lambda v: v[:rows], keep=lambda v: v[rows:]),
            BATCH, t, WIDTH, Work(_need(BATCH, t, WIDTH), row_bytes=12), SizeOf(6)]


def _run(device):
    fn = _lib.lib().kemr_op_attention_backward_long

    def run(*args):
        with torch.cuda.device(device):
            _lib.check(fn(*args, R.stream(device)), "op_attention_backward_long")
    return run


@pytest.mark.parametrize("t", CONTRACT_TS)
def test_memory_contract_exactly_batch_t_rows_written(device, t):
    """Exactly batch * t rows of dqkv, also when 7 spare rows follow; the workspace of exactly the stated size, poisoned, in guard margins."""
    F.run_both(_run(device), _specs(t, 7), device, what=f"attention_backward_long t={t}")


@pytest.mark.parametrize("t", CONTRACT_TS)
def test_stream_contract(device, t):
    SO.run_late(_run(device), _specs(t, 0), device, what=f"attention_backward_long t={t}")


def test_empty_batch_launches_nothing(device):
    out = torch.full((4, 3 * WIDTH), 7.0, dtype=BF16, device=device)
    keep = out.clone()
    assert _need(0, 4, WIDTH) == 0
    with torch.cuda.device(device):
        _lib.check(_lib.lib().kemr_op_attention_backward_long(C.c_void_p(out.data_ptr()), C.c_void_p(out.data_ptr()), C.c_void_p(out.data_ptr()),
                                                              0, 4, WIDTH, None, 0, R.stream(device)), "op_attention_backward_long")
    torch.cuda.synchronize(device)
    assert F.same_bits(out, keep)


# ------------------------------------------------------------------------------------------------ the route of engine.attention_backward
def test_route_at_288_is_the_lds_kernel(device):
    t = 288
    qkv, dout, _, _ = _case(t)
    q, d = qkv.to(device), dout.to(device)
    want = torch.empty_like(q)
    with torch.cuda.device(device):
        _lib.check(_lib.lib().kemr_op_attention_backward(C.c_void_p(q.data_ptr()), C.c_void_p(d.data_ptr()), C.c_void_p(want.data_ptr()), BATCH, t,
                                                         WIDTH, 0, R.stream(device)), "op_attention_backward")
    assert F.same_bits(engine.attention_backward(q, d, BATCH, t, WIDTH, False), want)


def test_route_at_289_is_the_streaming_kernel_and_causal_is_still_refused(device):
    t = 289
    qkv, dout, _, _ = _case(t)
    q, d = qkv.to(device), dout.to(device)
    assert F.same_bits(engine.attention_backward(q, d, BATCH, t, WIDTH, False), _direct(device, qkv, dout, t))
    with pytest.raises(RuntimeError, match=r"op_attention_backward: t = 289 is outside 1\.\.288"):
        engine.attention_backward(q, d, BATCH, t, WIDTH, True)
