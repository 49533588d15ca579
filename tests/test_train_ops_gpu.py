"""GPU: the training ops of csrc/train_ops.hip -- ``kemr_op_layernorm_backward``, ``kemr_op_act_forward``, ``kemr_op_act_backward`` --
against the statements of tests/train_ops_ref.py, their exact properties, their memory contract (tests/footprint.py) and their stream
contract (tests/stream_order.py).

LayerNorm backward.  Widths 256, 768, 1280; rows 1, 4, 5 (one row, an exact tile of four waves, a one-row ragged tile), 1031 (258
workgroups, the last tile three rows) and 2049: the grid is min(ceil(rows / 4), 512) workgroups, so 1031 rows are still one pass, and
2049 = 4 x 512 + 1 is the smallest count at which a wave walks a second row -- one wave does, with a ragged end.  dy in bf16 and fp32.
The bar: per output the relative L2 error against fp64 on the same inputs is at most 2 x the fp32 emulation's, which sums in the
kernel's stated order: the factor covers the order inside a row and the compiler's fused multiply-adds, nothing else.

Activations.  n = 8 (one lane) and 8 x 1027 (more than one workgroup, a ragged last one); pre covers [-12, 12] densely plus +-0,
+-large and the zero crossing of GELU's derivative.  Every element is held to ``oracle.rounding.check_budget``: half a bf16 ulp of the
result plus an fp32-evaluation allowance derived below from the accuracies of the instructions used, in units of 2^-24 (one rounding
<= 1 unit, one fp32 ulp <= 2 units)."""
import ctypes as C
import functools

import pytest
import torch

import footprint as FP
import stream_order as SO
import train_ops_ref as R
from footprint import In, Out, SizeOf, Work
from knowledge_enhanced_multimodal_retrieval_amd import _lib, engine
from oracle.rounding import check_budget

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
WIDTHS = [256, 768, 1280]
ROWS = [1, 4, 5, 1031, 2049]
NS = [8, 8 * 1027]
U = 2.0 ** -24


@functools.lru_cache(maxsize=None)
def _ln_case(rows, width, dt):
    """(x, gamma, dy, fp64 statement, emulation) of one shape: computed once, shared, never modified."""
    x, gamma, dy = R.make_ln_inputs(rows, width, 100 * rows + width + (dt == F32), dt)
    return x, gamma, dy, R.ln_backward_fp64(x, gamma, dy), R.ln_backward_emulated(x, gamma, dy)


@functools.lru_cache(maxsize=None)
def _act_case(n):
    return R.make_act_inputs(n, 40 + n)


def _stream(device):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


# ------------------------------------------------------------------------------------------------ LayerNorm backward
@pytest.mark.parametrize("dt", [BF16, F32], ids=["dy_bf16", "dy_f32"])
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("width", WIDTHS)
def test_layernorm_backward_within_twice_the_emulation(device, width, rows, dt):
    x, gamma, dy, ref, emu = _ln_case(rows, width, dt)
    got = [t.cpu() for t in engine.layernorm_backward(x.to(device), gamma.to(device), dy.to(device))]
    for name, g, r, e in zip(("dx", "dgamma", "dbeta"), got, ref, emu):
        assert g.dtype == F32 and g.shape == r.shape and bool(torch.isfinite(g).all()), name
        e_kernel, e_emu = R.rel_l2(g, r), R.rel_l2(e, r)
        print(f"layernorm_backward rows={rows} width={width} {dt}: {name} kernel {e_kernel:.4e} emulation {e_emu:.4e}")
        assert e_kernel <= 2.0 * e_emu, (name, e_kernel, e_emu)


@pytest.mark.parametrize("dt", [BF16, F32], ids=["dy_bf16", "dy_f32"])
def test_layernorm_backward_exact_properties(device, dt):
    x, gamma, dy, _, _ = _ln_case(2049, 768, dt)
    x, gamma, dy = x.to(device).clone(), gamma.to(device), dy.to(device)
    x[7] = 3.25                                            # a constant row: x^ = 0, rstd = 1 / sqrt(eps)
    a = engine.layernorm_backward(x, gamma, dy)
    b = engine.layernorm_backward(x, gamma, dy)
    for u, v in zip(a, b):                                 # two launches, the same bits
        assert FP.same_bits(u, v)
    assert bool(torch.isfinite(a[0][7]).all())
    for out in engine.layernorm_backward(x, gamma, torch.zeros_like(dy)):
        assert not out.any()                               # dy = 0: exactly zero


def test_layernorm_backward_rows_0(device):
    width = 512
    L = _lib.lib()
    assert L.kemr_layernorm_backward_workspace_bytes(0, width) == 0
    buf = torch.full((4, width), 7.0, dtype=F32, device=device)
    dg, db = torch.full((width,), 7.0, device=device), torch.full((width,), 7.0, device=device)
    keep = buf.clone()
    with torch.cuda.device(device):
        _lib.check(L.kemr_op_layernorm_backward(C.c_void_p(buf.data_ptr()), C.c_void_p(dg.data_ptr()), C.c_void_p(buf.data_ptr()), _lib.KEMR_F32,
                                                C.c_void_p(buf.data_ptr()), C.c_void_p(dg.data_ptr()), C.c_void_p(db.data_ptr()), 0, width,
                                                None, 0, _stream(device)), "op_layernorm_backward")
    torch.cuda.synchronize(device)
    assert FP.same_bits(buf, keep) and not dg.any() and not db.any()
    out = engine.layernorm_backward(torch.empty(0, width, device=device), torch.ones(width, device=device), torch.empty(0, width, dtype=BF16, device=device))
    assert out[0].shape == (0, width) and not out[1].any() and not out[2].any()


def _ln_specs(rows, width, dt, extra_rows):
    x, gamma, dy, _, _ = _ln_case(rows, width, dt)
    need = _lib.lib().kemr_layernorm_backward_workspace_bytes(rows, width)
    return [In(x), In(gamma), In(dy), _lib.KEMR_BF16 if dt == BF16 else _lib.KEMR_F32,
            Out((rows + extra_rows, width), F32, written=lambda v: v[:rows], keep=lambda v: v[rows:]), Out((width,), F32), Out((width,), F32),
            rows, width, Work(need, row_bytes=2 * width * 4), SizeOf(9)]


def _ln_run(device):
    fn = _lib.lib().kemr_op_layernorm_backward

    def run(*args):
        with torch.cuda.device(device):
            _lib.check(fn(*args, _stream(device)), "op_layernorm_backward")
    return run


@pytest.mark.parametrize("rows,width,dt", [(5, 768, BF16), (1031, 1280, BF16), (2049, 256, F32), (1, 1280, F32)])
def test_layernorm_backward_memory_contract(device, rows, width, dt):
    """Exactly rows x width elements of dx and width of dgamma / dbeta; the workspace of exactly the stated size, poisoned."""
    FP.run_both(_ln_run(device), _ln_specs(rows, width, dt, 7), device, what=f"layernorm_backward rows={rows} width={width}")


def test_layernorm_backward_stream_contract(device):
    SO.run_late(_ln_run(device), _ln_specs(2049, 768, BF16, 0), device, what="layernorm_backward")


# ------------------------------------------------------------------------------------------------ activations
def _qgelu_extra(x64):
    # (tests/test_numerics_gpu.py's formula) v_exp_f32 + v_rcp_f32 (1 ulp) of common.h quick_gelu on an fp32 argument: a few fp32 ulp,
    # growing with the exponent's argument
    return U * R.qgelu_fp64(x64).abs() * (8 + 4 * (1.702 * x64).abs())


def _gelu_extra(x64):
    # common.h gelu_erf, as tests/test_gelu_gpu.py derives it: erfcf of the device library budgeted at 13 ulp = 26 units, 1.5 units left
    # of its argument's rounding after the carried remainder, 3 roundings (the correction's fma, erfc x correction, the product with
    # 0.5 x, itself exact): 30.5 <= 32 units, relative everywhere.
    return U * 32 * R.gelu_fp64(x64).abs()


# The derivatives: extra = |dout| (|term 1| + |term 2|) 2^-24 K.  Every error below is RELATIVE to its own term, so the sum of the
# absolute terms bounds them where the terms cancel (GELU's derivative near -0.75).
#
# K_QGELU, from csrc/train_ops.hip quick_gelu_grad: f' = s + 1.702 x p q with e = exp(-1.702 |x|), q = 1 / (1 + e), p = e q and
# (s, 1 - s) = (q, p) or (p, q).  e: v_exp_f32 1 ulp = 2 units (its argument carries the product's remainder: nothing left of that
# rounding) + the correction's fma 1 = 3.  q: the sum's rounding 1 + what e's 3 units leave in 1 + e, at most 3 e / (1 + e) <= 1.5,
# + v_rcp_f32 1 ulp = 2: 4.5.  p = e q: 3 + 4.5 + 1 = 8.5.  Term 1 is p or q: <= 8.5.  Term 2 = ((x p) q) 1.702: p 8.5 + q 4.5 + two
# products 2 + the constant's own rounding 1 = 16.  The final fma rounds once (<= 1 unit of the result, which the absolute terms
# bound) and the product with dout once more: K = 16 + 1 + 1 = 18 units = 9 fp32 ulp.
K_QGELU = 18
# K_GELU, from gelu_erf_grad: f' = Phi + x phi.  Phi = 0.5 erfc(-x / sqrt 2) is gelu_erf's evaluation without the product with x:
# 26 (erfcf at 13 ulp) + 1.5 (argument) + 2 (the correction's fma, erfc x correction; 0.5 x is exact) = 29.5.  phi: expf of the device
# library (HIP's math reference: 1 ulp = 2 units) on an exact argument (x^2 carries its remainder), the correction's fma 1, two products 2
# and the constant's rounding 1: 6, and x phi is formed inside the final fma.  That fma rounds once and the product with dout once:
# K = 29.5 + 1 + 1 = 31.5 -> 32 units = 16 fp32 ulp, of which 26 are the device library's documented bound for erfcf.
K_GELU = 32


def _grad_extra(x64, dout64, kind):
    a, b = R.ACT[kind][1](x64)
    return dout64.abs() * (a.abs() + b.abs()) * U * (K_GELU if kind else K_QGELU)


@pytest.mark.parametrize("kind", [0, 1], ids=["quick_gelu", "gelu"])
@pytest.mark.parametrize("n", NS)
def test_activation_forward_and_backward_within_budget(device, n, kind):
    pre, dout = _act_case(n)
    x64, d64 = pre.double(), dout.double()
    out = engine.act_forward(pre.to(device), kind).cpu()
    dpre = engine.act_backward(pre.to(device), dout.to(device), kind).cpu()
    assert out.dtype == BF16 and dpre.dtype == BF16 and out.shape == pre.shape and dpre.shape == pre.shape
    top, _ = check_budget(out, R.ACT[kind][0](x64), (_gelu_extra if kind else _qgelu_extra)(x64), what=f"act_forward kind={kind} n={n}")
    print(f"act_forward kind={kind} n={n}: worst budget ratio {top:.3f}")
    top, _ = check_budget(dpre, R.act_backward_fp64(pre, dout, kind), _grad_extra(x64, d64, kind), what=f"act_backward kind={kind} n={n}")
    print(f"act_backward kind={kind} n={n}: worst budget ratio {top:.3f}")


@pytest.mark.parametrize("kind", [0, 1], ids=["quick_gelu", "gelu"])
def test_activation_exact_properties(device, kind):
    pre, dout = (t.to(device) for t in _act_case(NS[1]))
    assert not engine.act_backward(pre, torch.zeros_like(dout), kind).float().any()        # dout = 0: exactly zero
    assert FP.same_bits(engine.act_forward(pre, kind), engine.act_forward(pre, kind))
    assert FP.same_bits(engine.act_backward(pre, dout, kind), engine.act_backward(pre, dout, kind))
    two = pre.reshape(-1, 8)                               # any shape of n elements
    assert FP.same_bits(engine.act_forward(two, kind), engine.act_forward(pre, kind))


def _act_specs(n, backward, kind, extra_rows):
    pre, dout = _act_case(n)
    rows = n // 8
    ins = [In(pre.reshape(rows, 8))] + ([In(dout.reshape(rows, 8))] if backward else [])
    return ins + [Out((rows + extra_rows, 8), BF16, written=lambda v: v[:rows], keep=lambda v: v[rows:]), n, kind]


def _act_run(device, backward):
    fn = _lib.lib().kemr_op_act_backward if backward else _lib.lib().kemr_op_act_forward

    def run(*args):
        with torch.cuda.device(device):
            _lib.check(fn(*args, _stream(device)), "op_act")
    return run


@pytest.mark.parametrize("backward", [False, True], ids=["forward", "backward"])
@pytest.mark.parametrize("kind", [0, 1], ids=["quick_gelu", "gelu"])
@pytest.mark.parametrize("n", NS)
def test_activation_memory_contract_exactly_n_elements_written(device, n, kind, backward):
    FP.run_both(_act_run(device, backward), _act_specs(n, backward, kind, 7), device, what=f"act backward={backward} kind={kind} n={n}")


@pytest.mark.parametrize("backward,kind", [(False, 0), (True, 1)], ids=["forward", "backward"])
def test_activation_stream_contract(device, backward, kind):
    SO.run_late(_act_run(device, backward), _act_specs(NS[1], backward, kind, 0), device, what=f"act backward={backward}")
