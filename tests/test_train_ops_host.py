"""Host (no GPU): the reference statements of tests/train_ops_ref.py against torch's fp64 autograd, four planted mistakes against the
same bar, the ABI surface of the training ops (csrc/train_ops.hip) and every refusal that needs no GPU."""
import ctypes as C
import os
import re

import pytest
import torch
import torch.nn.functional as F

import train_ops_ref as R
from knowledge_enhanced_multimodal_retrieval_amd import _lib, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEMR_OK, KEMR_ERR_INVALID = 0, -1
BAR = 1e-12                      # the statements are the same mathematics in the same precision as autograd: summation order only
NAMES = ("kemr_layernorm_backward_workspace_bytes", "kemr_op_layernorm_backward", "kemr_op_act_forward", "kemr_op_act_backward")


def _ln_case():
    x, gamma, dy = R.make_ln_inputs(37, 256, 5, torch.float32)
    beta = torch.randn(256, generator=torch.Generator().manual_seed(6), dtype=torch.float64)
    xd, gd, bd = x.double().requires_grad_(True), gamma.double().requires_grad_(True), beta.requires_grad_(True)
    F.layer_norm(xd, (256,), gd, bd, R.EPS).backward(dy.double())
    return x, gamma, dy, (xd.grad, gd.grad, bd.grad)


def _act_case(kind):
    pre, dout = R.make_act_inputs(8 * 500, 7)
    pre = pre[pre.float().abs() <= 12]                   # autograd of x sigmoid(1.702 x) forms 1 - s: keep to where that is still meaningful
    dout = dout[:pre.numel()]
    xd = pre.double().requires_grad_(True)
    (F.gelu(xd) if kind else xd * torch.sigmoid(1.702 * xd)).backward(dout.double())
    return pre, dout, xd.grad


def test_layernorm_statement_agrees_with_autograd():
    x, gamma, dy, want = _ln_case()
    for name, got, w in zip(("dx", "dgamma", "dbeta"), R.ln_backward_fp64(x, gamma, dy), want):
        e = R.rel_l2(got, w)
        print(f"layernorm backward statement vs autograd {name}: {e:.3e}")
        assert e <= BAR, (name, e)


@pytest.mark.parametrize("kind", [0, 1])
def test_activation_statements_agree_with_autograd(kind):
    pre, dout, want = _act_case(kind)
    e = R.rel_l2(R.act_backward_fp64(pre, dout, kind), want)
    print(f"activation backward statement vs autograd kind={kind}: {e:.3e}")
    assert e <= BAR
    xd = pre.double()
    assert R.rel_l2(R.ACT[kind][0](pre), F.gelu(xd) if kind else xd * torch.sigmoid(1.702 * xd)) <= BAR


@pytest.mark.parametrize("planted", ["var_w_minus_1", "drop_mean_gx"])
def test_planted_layernorm_mistakes_miss_the_bar(planted):
    x, gamma, dy, want = _ln_case()
    e = R.rel_l2(R.ln_backward_fp64(x, gamma, dy, planted)[0], want[0])
    print(f"planted {planted}: dx off by {e:.3e}")
    assert e >= 100 * BAR


@pytest.mark.parametrize("kind,planted", [(0, "no_1702"), (1, "phi_no_norm")])
def test_planted_activation_mistakes_miss_the_bar(kind, planted):
    pre, dout, want = _act_case(kind)
    e = R.rel_l2(R.act_backward_fp64(pre, dout, kind, planted), want)
    print(f"planted {planted}: dpre off by {e:.3e}")
    assert e >= 100 * BAR


def test_emulations_are_fp32_evaluations_of_the_statements():
    """Not a bar for the kernels: the emulations must be the statements in fp32 (2^-24 per operation; a few 1e-6 would be a mistake in
    them) and, for the activations, within bf16's half ulp of them."""
    for rows, dt in ((5, torch.bfloat16), (37, torch.float32), (2049, torch.bfloat16)):
        x, gamma, dy = R.make_ln_inputs(rows, 256, 11 + rows, dt)
        for name, e, w in zip(("dx", "dgamma", "dbeta"), R.ln_backward_emulated(x, gamma, dy), R.ln_backward_fp64(x, gamma, dy)):
            err = R.rel_l2(e, w)
            print(f"layernorm emulation rows={rows} {name}: {err:.3e}")
            assert e.dtype == torch.float32 and err <= 2e-6, (name, err)
    pre, dout = R.make_act_inputs(8 * 1027, 3)
    for kind in (0, 1):
        assert R.rel_l2(R.act_forward_emulated(pre, kind).double(), R.ACT[kind][0](pre)) <= 2.0 ** -8
        assert R.rel_l2(R.act_backward_emulated(pre, dout, kind).double(), R.act_backward_fp64(pre, dout, kind)) <= 2.0 ** -8


def test_symbols_are_declared_and_abi_stays_4():
    header = open(os.path.join(ROOT, "include", "kemr.h")).read()
    for name in NAMES:
        assert name in _lib.SIGNATURES and re.search(rf"\b{name}\s*\(", header), name
    assert _lib.SIGNATURES["kemr_op_layernorm_backward"] == (C.c_int, [C.c_void_p] * 3 + [C.c_int] + [C.c_void_p] * 3 + [C.c_int] * 2
                                                             + [C.c_void_p, C.c_size_t, C.c_void_p])
    assert "#define KEMR_ABI_VERSION 4" in header
    assert _lib.ABI_VERSION == 4 and _lib.lib().kemr_abi_version() == 4


# never dereferenced: every case is refused on the host, before any HIP call
P = C.c_void_p(0x1000)
NULL = C.c_void_p(None)
BIG = 1 << 30


@pytest.mark.parametrize("args,names", [
    ((NULL, P, P, 1, P, P, P, 8, 256, P, BIG), "x"),
    ((P, NULL, P, 1, P, P, P, 8, 256, P, BIG), "gamma"),
    ((P, P, NULL, 1, P, P, P, 8, 256, P, BIG), "dy"),
    ((P, P, P, 1, NULL, P, P, 8, 256, P, BIG), "dx"),
    ((P, P, P, 1, P, NULL, P, 8, 256, P, BIG), "dgamma"),
    ((P, P, P, 1, P, P, NULL, 8, 256, P, BIG), "dbeta"),
    ((P, P, P, 1, P, P, P, 8, 256, NULL, BIG), "workspace"),
    ((P, P, P, 1, P, P, P, 8, 320, P, BIG), "width"),
    ((P, P, P, 1, P, P, P, 8, 2048, P, BIG), "width"),
    ((P, P, P, 2, P, P, P, 8, 256, P, BIG), "dy_dtype"),
    ((P, P, P, 3, P, P, P, 8, 256, P, BIG), "dy_dtype"),
    ((P, P, P, 1, P, P, P, -1, 256, P, BIG), "rows"),
    ((C.c_void_p(0x1004), P, P, 1, P, P, P, 8, 256, P, BIG), "aligned"),
], ids=["x=NULL", "gamma=NULL", "dy=NULL", "dx=NULL", "dgamma=NULL", "dbeta=NULL", "workspace=NULL", "width=320", "width=2048", "dy=i32",
        "dy=fp8", "rows=-1", "x+4"])
def test_layernorm_backward_refused_on_the_host(args, names):
    L = _lib.lib()
    assert L.kemr_op_layernorm_backward(*args, None) == KEMR_ERR_INVALID
    msg = L.kemr_last_error().decode()
    assert msg.startswith("op_layernorm_backward:") and re.search(rf"\b{names}\b", msg), msg


@pytest.mark.parametrize("rows,width", [(1, 256), (5, 768), (3000, 1280)])
def test_a_workspace_one_byte_short_is_refused(rows, width):
    L = _lib.lib()
    need = L.kemr_layernorm_backward_workspace_bytes(rows, width)
    assert need > 0
    assert L.kemr_op_layernorm_backward(P, P, P, 1, P, P, P, rows, width, P, need - 1, None) == KEMR_ERR_INVALID
    msg = L.kemr_last_error().decode()
    assert re.search(r"\bworkspace_bytes\b", msg) and str(need) in msg, msg


def test_workspace_size_is_monotone_in_rows_and_a_function_of_its_arguments():
    L = _lib.lib()
    for width in (256, 512, 768, 1024, 1280):
        sizes = [L.kemr_layernorm_backward_workspace_bytes(r, width) for r in list(range(0, 2100)) + [16448, 1 << 20, (1 << 31) - 1]]
        assert sizes[0] == 0 and all(a <= b for a, b in zip(sizes, sizes[1:]))
        assert sizes[1] == 2 * width * 4                                         # one [2, width] fp32 slab
        assert sizes == [R.ln_groups(r) * 2 * width * 4 for r in list(range(0, 2100)) + [16448, 1 << 20, (1 << 31) - 1]]
        assert sizes[-1] == sizes[-2] == R.MAX_GROUPS * 2 * width * 4           # bounded: no size grows with the device or beyond G slabs


@pytest.mark.parametrize("fn,nptr", [("kemr_op_act_forward", 2), ("kemr_op_act_backward", 3)])
def test_activation_refused_on_the_host(fn, nptr):
    L = _lib.lib()
    f = getattr(L, fn)
    ptrs = [P] * nptr
    for args, names in [((*ptrs, 64, 2), "kind"), ((*ptrs, 64, -1), "kind"), ((*ptrs, 12, 0), "multiple of 8"), ((*ptrs, 7, 1), "multiple of 8"),
                        ((*ptrs, -8, 0), "negative"), ((*ptrs[:-1], C.c_void_p(0x1008), 64, 0), "aligned")] + \
                       [((*ptrs[:i], NULL, *ptrs[i + 1:], 64, 0), "NULL") for i in range(nptr)]:
        assert f(*args, None) == KEMR_ERR_INVALID, args
        msg = L.kemr_last_error().decode()
        assert msg.startswith(fn[len("kemr_"):] + ":") and names in msg, msg
    assert f(*ptrs, 0, 1, None) == KEMR_OK               # n == 0: nothing to launch, nothing dereferenced


def test_engine_wrappers_have_no_cpu_fallback_and_check_their_arguments():
    x, gamma, dy = R.make_ln_inputs(4, 256, 0)
    pre, dout = R.make_act_inputs(16, 0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        engine.layernorm_backward(x, gamma, dy)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        engine.act_forward(pre, "quick_gelu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        engine.act_backward(pre, dout, 1)
    with pytest.raises(RuntimeError, match="kind"):
        engine.act_forward(pre, "relu")
