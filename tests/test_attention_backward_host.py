"""Host (no GPU): the ABI surface of ``kemr_op_attention_backward``, its refusals, and the reference statements of
tests/attention_bwd_ref.py against torch's fp64 autograd."""
import ctypes as C
import os
import re

import pytest
import torch

import attention_bwd_ref as R
from knowledge_enhanced_multimodal_retrieval_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEMR_ERR_INVALID = -1


def test_symbol_is_declared_and_abi_stays_4():
    assert _lib.SIGNATURES["kemr_op_attention_backward"] == (C.c_int, [C.c_void_p] * 3 + [C.c_int] * 4 + [C.c_void_p])
    header = open(os.path.join(ROOT, "include", "kemr.h")).read()
    assert re.search(r"\bint\s+kemr_op_attention_backward\s*\(\s*const void\* qkv_dev, const void\* dout_dev, void\* dqkv_dev, int batch, "
                     r"int t, int width, int causal,\s*void\* stream\);", header)
    assert "#define KEMR_ABI_VERSION 4" in header
    assert _lib.ABI_VERSION == 4 and _lib.lib().kemr_abi_version() == 4


# never dereferenced: every case is refused on the host, before any HIP call
P = C.c_void_p(0x1000)
NULL = C.c_void_p(None)


@pytest.mark.parametrize("args,names", [
    ((P, P, P, 2, 0, 128, 1), "t"),
    ((P, P, P, 2, 289, 128, 1), "t"),
    ((P, P, P, 2, 77, 96, 1), "width"),
    ((P, P, P, -1, 77, 128, 0), "batch"),
    ((NULL, P, P, 2, 77, 128, 1), "qkv"),
    ((P, NULL, P, 2, 77, 128, 1), "dout"),
    ((P, P, NULL, 2, 77, 128, 1), "dqkv"),
], ids=["t=0", "t=289", "width=96", "batch=-1", "qkv=NULL", "dout=NULL", "dqkv=NULL"])
def test_refused_on_the_host(args, names):
    L = _lib.lib()
    assert L.kemr_op_attention_backward(*args, None) == KEMR_ERR_INVALID
    msg = L.kemr_last_error().decode()
    assert msg.startswith("op_attention_backward:") and re.search(rf"\b{names}\b", msg), msg
    with pytest.raises(RuntimeError, match=names):
        _lib.check(L.kemr_op_attention_backward(*args, None), "op_attention_backward")


def test_engine_wrapper_has_no_cpu_fallback():
    from knowledge_enhanced_multimodal_retrieval_amd import engine
    qkv, dout = R.make_inputs(1, 4, 64, 0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        engine.attention_backward(qkv, dout, 1, 4, 64, True)


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("t", [1, 17, 77])
def test_statements_agree_with_autograd(t, causal):
    batch, width = 2, 128
    qkv, dout = R.make_inputs(batch, t, width, 100 + t, zero_item=None)
    x = qkv.double().requires_grad_(True)
    q, k, v = (R._heads(x[:, i * width:(i + 1) * width], batch, t, width) for i in range(3))
    out = R._rows(R.plain_attention(q, k, v, causal), batch, t, width)
    out.backward(dout.double())
    want = x.grad
    got = R.backward_fp64(qkv, dout, batch, t, width, causal)
    emu = R.backward_emulated(qkv, dout, batch, t, width, causal)
    assert emu.dtype == torch.bfloat16 and emu.shape == want.shape
    for name in ("dq", "dk", "dv"):
        w = R.planes(want, width)[name]
        # the statement is the same mathematics in the same precision: summation order only
        assert R.rel_l2(R.planes(got, width)[name], w) <= 1e-12, name
        # the emulation rounds P, dS and the output to bf16 (2^-9 relative each, independent; the fp32 sums add ~t 2^-24): an L2 error
        # above 4 x 2^-9 = 2^-7 would be a mistake in the emulation, not rounding
        e = R.rel_l2(R.planes(emu, width)[name], w)
        print(f"emulation vs autograd t={t} causal={causal} {name}: {e:.3e}")
        assert e <= 2.0 ** -7, (name, e)
        assert t > 1 or e == 0.0                # one key: P = 1 and dS = 0 exactly, dv = dout


def test_t1_is_exact_in_both_statements():
    qkv, dout = R.make_inputs(3, 1, 128, 5)
    for fn in (R.backward_fp64, R.backward_emulated):
        g = R.planes(fn(qkv, dout, 3, 1, 128, True), 128)
        assert not g["dq"].any() and not g["dk"].any()
        assert torch.equal(g["dv"].double(), dout.double())
