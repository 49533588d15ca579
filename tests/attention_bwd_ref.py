"""Reference statements of the attention backward (``kemr_op_attention_backward``; csrc/attention_bwd.hip), CPU only.

Layout as the op has it: qkv bf16 [batch * t, 3 width] = q | k | v, heads of 64, q already scaled by 1/8; dout bf16 [batch * t, width];
dqkv [batch * t, 3 width] = the gradient with respect to the three planes as given.

  backward_fp64      the mathematical statement in fp64 on the given bf16 values: S = q k^T, P = softmax(S) (causal: keys <= query),
                     dP = dO v^T, D_i = sum_j P_ij dP_ij, dS = P o (dP - D), dq = dS k, dk = dS^T q, dv = P^T dO.  fp64 [.., 3 width].
  backward_emulated  the same with the kernel's rounding points: every product sum in fp32, P and dS rounded to bf16 where they are
                     MFMA operands (D from the unrounded fp32 P), the three outputs rounded to bf16.  What is left between it and the
                     kernel is the summation order of the fp32 sums and the exponential's implementation.
  rel_l2             the error measure of the tests; check_against_fp64 is the bar the three GPU test files hold their op to.
  plain_attention    softmax(q k^T) v in the dtype given, for torch autograd (the plain formulation the statement is checked against).
"""
import ctypes

import torch

HEAD = 64


def _heads(x, batch, t, width):
    """[batch * t, width] -> [batch, heads, t, 64]"""
    return x.reshape(batch, t, width // HEAD, HEAD).permute(0, 2, 1, 3)


def _rows(x, batch, t, width):
    """[batch, heads, t, 64] -> [batch * t, width]"""
    return x.permute(0, 2, 1, 3).reshape(batch * t, width)


def _mask(t, causal, dtype):
    m = torch.zeros(t, t, dtype=dtype)
    if causal:
        m.masked_fill_(torch.ones(t, t, dtype=torch.bool).triu(1), float("-inf"))
    return m


def plain_attention(q, k, v, causal):
    """q, k, v [batch, heads, t, 64] (q pre-scaled) -> [batch, heads, t, 64]; differentiable."""
    s = q @ k.transpose(-1, -2) + _mask(q.shape[-2], causal, q.dtype)
    return torch.softmax(s, dim=-1) @ v


def _backward(qkv, dout, batch, t, width, causal, dtype, round_operands):
    q, k, v = (_heads(qkv[:, i * width:(i + 1) * width].to(dtype), batch, t, width) for i in range(3))
    do = _heads(dout.to(dtype), batch, t, width)
    p = torch.softmax(q @ k.transpose(-1, -2) + _mask(t, causal, dtype), dim=-1)
    dp = do @ v.transpose(-1, -2)
    d = (p * dp).sum(-1, keepdim=True)
    ds = p * (dp - d)
    if round_operands:
        p, ds = p.to(torch.bfloat16).to(dtype), ds.to(torch.bfloat16).to(dtype)
    dq, dk, dv = ds @ k, ds.transpose(-1, -2) @ q, p.transpose(-1, -2) @ do
    return torch.cat([_rows(x, batch, t, width) for x in (dq, dk, dv)], dim=1)


def backward_fp64(qkv, dout, batch, t, width, causal):
    return _backward(qkv, dout, batch, t, width, causal, torch.float64, False)


def backward_emulated(qkv, dout, batch, t, width, causal):
    """bf16 [batch * t, 3 width]"""
    return _backward(qkv, dout, batch, t, width, causal, torch.float32, True).to(torch.bfloat16)


def rel_l2(x, ref):
    """||x - ref|| / ||ref|| in fp64; a zero reference asks for an exact zero (0.0) and gives inf otherwise."""
    x, ref = x.double(), ref.double()
    num, den = float((x - ref).norm()), float(ref.norm())
    if den == 0.0:
        return 0.0 if num == 0.0 else float("inf")
    return num / den


def planes(dqkv, width):
    return {"dq": dqkv[:, :width], "dk": dqkv[:, width:2 * width], "dv": dqkv[:, 2 * width:]}


def check_against_fp64(got, ref, emu, width, what):
    """The bar of the GPU tests: bf16, finite, and per plane (dq, dk, dv) the relative L2 error against the fp64 statement is at most
    2 x the emulation's.  `what` names the op and the shape in the printed figures."""
    assert got.dtype == torch.bfloat16 and got.shape == ref.shape
    assert bool(torch.isfinite(got.float()).all())
    for name in ("dq", "dk", "dv"):
        r = planes(ref, width)[name]
        e_kernel, e_emu = rel_l2(planes(got, width)[name], r), rel_l2(planes(emu, width)[name], r)
        print(f"{what} {name}: kernel {e_kernel:.4e} emulation {e_emu:.4e}")
        assert e_kernel <= 2.0 * e_emu, (name, e_kernel, e_emu)


def stream(device):
    """The current stream of `device` as the C ABI takes it."""
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def make_inputs(batch, t, width, seed, zero_item=None):
    """qkv randn with q pre-scaled by 1/8, dout randn with the rows of `zero_item` zero; both bf16."""
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(batch * t, 3 * width, generator=g)
    qkv[:, :width] *= 0.125
    dout = torch.randn(batch * t, width, generator=g)
    if zero_item is not None:
        dout[zero_item * t:(zero_item + 1) * t] = 0
    return qkv.to(torch.bfloat16), dout.to(torch.bfloat16)
