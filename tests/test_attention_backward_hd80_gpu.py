"""GPU: ``kemr_op_attention_backward_hd`` at head dim 80 (csrc/attention_bwd80.hip), the streaming non-causal attention backward for heads
of 80, against the fp64 statement and the rounding emulation of tests/attention_bwd_hd_ref.py, its exact properties, its memory contract
(tests/footprint.py), its stream contract (tests/stream_order.py), the route of ``engine.attention_backward(head_dim=80)`` and what the
op is at head_dim = 64.

Shapes: width 160 (two heads of 80), batch 3, the dout rows of item 1 zero, t in {1, 5, 16, 17, 63, 64, 65, 128, 129, 257, 288, 289,
577, 1025}: one key; "tiny-h"'s length; exact and one-row-ragged 16-row tiles; one 64-row chunk exactly and one row either side of it;
two chunks and one row more; ViT-H-14's length; both sides of the forward's limit; the long lengths; the maximum.  The bar is the
project's standing one: per plane (dq, dk, dv) the relative L2 error against the fp64 statement on the same bf16 inputs is at most 2 x
the emulation's error at that shape.  The emulation rounds where the kernels round (P and dS to bf16 as MFMA operands, the outputs to
bf16; D from the unrounded fp32 P); on the CPU its error at head dim 80 is 2.25e-3 .. 2.40e-3 per plane at every one of these shapes,
and exactly 0 at t = 1, where the result must therefore be exact."""
import ctypes as C
import functools

import pytest
import torch

import attention_bwd_hd_ref as R
import footprint as F
import stream_order as SO
from footprint import In, Out, SizeOf, Work
from knowledge_enhanced_multimodal_retrieval_amd import _lib, engine

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
HD = 80
BATCH, WIDTH, ZERO_ITEM = 3, 160, 1
TS = [1, 5, 16, 17, 63, 64, 65, 128, 129, 257, 288, 289, 577, 1025]
CONTRACT_TS = [5, 17, 65, 257]


@functools.lru_cache(maxsize=None)
def _case(t, width=WIDTH, batch=BATCH):
    """(qkv, dout, fp64 statement, emulation) of one shape: computed once, shared, never modified."""
    qkv, dout = R.make_inputs(batch, t, width, 8000 + 2 * t + width, HD, zero_item=ZERO_ITEM)
    return qkv, dout, R.backward_fp64(qkv, dout, batch, t, width, HD), R.backward_emulated(qkv, dout, batch, t, width, HD)


def _need(batch, t, width, head_dim=HD):
    return int(_lib.lib().kemr_attention_backward_hd_workspace_bytes(batch, t, width, head_dim))


def _direct(device, qkv, dout, t, width=WIDTH, batch=BATCH, head_dim=HD, causal=0):
    """One call of the op itself on tight torch tensors (whatever the engine's route is)."""
    q, d = qkv.to(device), dout.to(device)
    out = torch.empty_like(q)
    need = _need(batch, t, width, head_dim)
    ws = torch.empty(max(need, 4), dtype=torch.uint8, device=device)
    with torch.cuda.device(device):
        _lib.check(_lib.lib().kemr_op_attention_backward_hd(C.c_void_p(q.data_ptr()), C.c_void_p(d.data_ptr()), C.c_void_p(out.data_ptr()),
                                                            batch, t, width, head_dim, causal, C.c_void_p(ws.data_ptr()), need,
                                                            R.stream(device)), "op_attention_backward_hd")
    return out


@pytest.mark.parametrize("t", TS)
def test_error_against_fp64_within_twice_the_emulation(device, t):
    qkv, dout, ref, emu = _case(t)
    got = _direct(device, qkv, dout, t).cpu()
    R.check_against_fp64(got, ref, emu, WIDTH, f"attention_backward_hd80 t={t}")
    # the item whose dout rows are zero: exactly zero gradients
    assert not got[ZERO_ITEM * t:(ZERO_ITEM + 1) * t].float().any()
    if t == 1:          # one key: P = 1, dS = 0
        g = R.planes(got, WIDTH)
        assert not g["dq"].float().any() and not g["dk"].float().any()
        assert F.same_bits(g["dv"], dout)


def test_head_indexing_at_width_1280(device):
    """ViT-H-14's own shape (16 heads of 80, 257 tokens), batch 2 with item 1 zero: the same bar."""
    t, width, batch = 257, 1280, 2
    qkv, dout, ref, emu = _case(t, width, batch)
    got = _direct(device, qkv, dout, t, width, batch).cpu()
    R.check_against_fp64(got, ref, emu, width, f"attention_backward_hd80 t={t} width={width}")
    assert not got[t:].float().any()


@pytest.mark.parametrize("t", [65, 257])
def test_heads_are_independent(device, t):
    """Only head 1's columns (80..159 of each plane and of dout) change: head 0's columns of dqkv keep their bits."""
    qkv, _, _, _ = _case(t)
    dout = R.make_inputs(BATCH, t, WIDTH, 91 + t, HD)[1]
    base = _direct(device, qkv, dout, t).cpu()
    qkv2, dout2 = R.make_inputs(BATCH, t, WIDTH, 191 + t, HD)
    for plane in range(3):
        qkv2[:, plane * WIDTH:plane * WIDTH + HD] = qkv[:, plane * WIDTH:plane * WIDTH + HD]
    dout2[:, :HD] = dout[:, :HD]
    got = _direct(device, qkv2, dout2, t).cpu()
    for plane in range(3):
        lo = plane * WIDTH
        assert F.same_bits(got[:, lo:lo + HD].contiguous(), base[:, lo:lo + HD].contiguous()), plane
        assert not torch.equal(got[:, lo + HD:lo + WIDTH].float(), base[:, lo + HD:lo + WIDTH].float())    # (head 1 did change)


@pytest.mark.parametrize("t", CONTRACT_TS)
def test_two_launches_give_the_same_bits(device, t):
    qkv, dout, _, _ = _case(t)
    assert F.same_bits(_direct(device, qkv, dout, t), _direct(device, qkv, dout, t))


@pytest.mark.parametrize("t", CONTRACT_TS)
def test_an_item_depends_on_its_own_rows_only(device, t):
    """Item 1 of a call whose other items and whose surroundings (0xff margins in front of and behind every buffer) are different."""
    qkv, _, _, _ = _case(t)
    dout = R.make_inputs(BATCH, t, WIDTH, 77 + t, HD)[1]                  # no zero item here
    base = _direct(device, qkv, dout, t).cpu()
    qkv2, dout2 = R.make_inputs(BATCH, t, WIDTH, 555 + t, HD)
    own = slice(t, 2 * t)
    qkv2[own], dout2[own] = qkv[own], dout[own]
    need = _need(BATCH, t, WIDTH)
    wq = F.window(qkv2.shape, BF16, device, F.POISON, body=qkv2, what="qkv")
    wd = F.window(dout2.shape, BF16, device, F.POISON, body=dout2, what="dout")
    wo = F.window(qkv2.shape, BF16, device, F.GUARD, what="dqkv")
    ww = F.window((need,), torch.uint8, device, F.GUARD, body=F.POISON, what="workspace")
    with torch.cuda.device(device):
        _lib.check(_lib.lib().kemr_op_attention_backward_hd(C.c_void_p(wq.ptr), C.c_void_p(wd.ptr), C.c_void_p(wo.ptr), BATCH, t, WIDTH, HD, 0,
                                                            C.c_void_p(ww.ptr), need, R.stream(device)), "op_attention_backward_hd")
    torch.cuda.synchronize(device)
    assert wq.margins_intact() and wd.margins_intact() and wo.margins_intact() and ww.margins_intact()
    assert F.same_bits(wo.view[own], base[own])
    assert not torch.equal(wo.view[:t].cpu().float(), base[:t].float())       # (the other items did change)


def _specs(t, extra_rows):
    qkv, dout, _, _ = _case(t)
    rows = BATCH * t
    return [In(qkv), In(dout), Out((rows + extra_rows, 3 * WIDTH), BF16, written=lambda v: v[:rows], keep=lambda v: v[rows:]),
            BATCH, t, WIDTH, HD, 0, Work(_need(BATCH, t, WIDTH), row_bytes=12), SizeOf(8)]


def _run(device):
    fn = _lib.lib().kemr_op_attention_backward_hd

    def run(*args):
        with torch.cuda.device(device):
            _lib.check(fn(*args, R.stream(device)), "op_attention_backward_hd")
    return run


@pytest.mark.parametrize("t", CONTRACT_TS)
def test_memory_contract_exactly_batch_t_rows_written(device, t):
    """Exactly batch * t rows of dqkv, also when 7 spare rows follow; the workspace of exactly the stated size, poisoned, in guard
    margins.  The poisoned margin behind qkv and dout is what a load past column 79 of the last head's last row would bring in."""
    F.run_both(_run(device), _specs(t, 7), device, what=f"attention_backward_hd80 t={t}")


@pytest.mark.parametrize("t", CONTRACT_TS)
def test_stream_contract(device, t):
    SO.run_late(_run(device), _specs(t, 0), device, what=f"attention_backward_hd80 t={t}")


def test_empty_batch_launches_nothing(device):
    out = torch.full((4, 3 * WIDTH), 7.0, dtype=BF16, device=device)
    keep = out.clone()
    assert _need(0, 4, WIDTH) == 0
    with torch.cuda.device(device):
        _lib.check(_lib.lib().kemr_op_attention_backward_hd(C.c_void_p(out.data_ptr()), C.c_void_p(out.data_ptr()), C.c_void_p(out.data_ptr()),
                                                            0, 4, WIDTH, HD, 0, None, 0, R.stream(device)), "op_attention_backward_hd")
    torch.cuda.synchronize(device)
    assert F.same_bits(out, keep)


# ------------------------------------------------------------------------------------------------ the routes
@pytest.mark.parametrize("t", [257, 289])
def test_engine_route_at_head_dim_80(device, t):
    qkv, dout, _, _ = _case(t)
    q, d = qkv.to(device), dout.to(device)
    assert F.same_bits(engine.attention_backward(q, d, BATCH, t, WIDTH, False, head_dim=HD), _direct(device, qkv, dout, t))
    with pytest.raises(RuntimeError, match=r"op_attention_backward_hd: causal = 1 is not served at head_dim = 80"):
        engine.attention_backward(q, d, BATCH, t, WIDTH, True, head_dim=HD)


def _inputs64(t, width=128):
    import attention_bwd_ref as R64
    return R64.make_inputs(BATCH, t, width, 4000 + t, zero_item=ZERO_ITEM)


@pytest.mark.parametrize("causal", [0, 1])
def test_head_dim_64_at_288_is_the_lds_op(device, causal):
    t, width = 288, 128
    qkv, dout = _inputs64(t)
    q, d = qkv.to(device), dout.to(device)
    want = torch.empty_like(q)
    with torch.cuda.device(device):
        _lib.check(_lib.lib().kemr_op_attention_backward(C.c_void_p(q.data_ptr()), C.c_void_p(d.data_ptr()), C.c_void_p(want.data_ptr()), BATCH, t,
                                                         width, causal, R.stream(device)), "op_attention_backward")
    assert F.same_bits(_direct(device, qkv, dout, t, width, BATCH, 64, causal), want)


def test_head_dim_64_at_289_is_the_long_op(device):
    t, width = 289, 128
    qkv, dout = _inputs64(t)
    q, d = qkv.to(device), dout.to(device)
    want = torch.empty_like(q)
    need = int(_lib.lib().kemr_attention_backward_long_workspace_bytes(BATCH, t, width))
    assert need == _need(BATCH, t, width, 64)
    ws = torch.empty(need, dtype=torch.uint8, device=device)
    with torch.cuda.device(device):
        _lib.check(_lib.lib().kemr_op_attention_backward_long(C.c_void_p(q.data_ptr()), C.c_void_p(d.data_ptr()), C.c_void_p(want.data_ptr()), BATCH,
                                                              t, width, C.c_void_p(ws.data_ptr()), need, R.stream(device)),
                   "op_attention_backward_long")
    assert F.same_bits(_direct(device, qkv, dout, t, width, BATCH, 64, 0), want)
