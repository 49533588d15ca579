"""Reference statements of the attention backward with the head dim as an argument (``kemr_op_attention_backward_hd``;
csrc/attention_bwd80.hip), CPU only: tests/attention_bwd_ref.py with ``HEAD`` a parameter.  Non-causal.

Layout as the op has it: qkv bf16 [batch * t, 3 width] = q | k | v, heads of ``head_dim``, q already scaled by ``head_dim ** -0.5``;
dout bf16 [batch * t, width]; dqkv [batch * t, 3 width] = the gradient with respect to the three planes as given.

  backward_fp64      the mathematical statement in fp64 on the given bf16 values (S = q k^T, P = softmax(S), dP = dO v^T,
                     D_i = sum_j P_ij dP_ij, dS = P o (dP - D), dq = dS k, dk = dS^T q, dv = P^T dO).
  backward_emulated  the same with the kernels' rounding points: fp32 sums, P and dS to bf16 as operands (D from the unrounded fp32 P),
                     the outputs to bf16.  At head_dim = 64 both are attention_bwd_ref's, bit for bit.
  make_inputs        attention_bwd_ref.make_inputs with q pre-scaled by head_dim ** -0.5.
``rel_l2``, ``planes``, ``check_against_fp64`` and ``stream`` are attention_bwd_ref's own.  Not a test module."""
import torch

from attention_bwd_ref import check_against_fp64, planes, rel_l2, stream  # noqa: F401  (re-exported)


def heads_of(x, batch, t, width, head_dim):
    """[batch * t, width] -> [batch, heads, t, head_dim]"""
    return x.reshape(batch, t, width // head_dim, head_dim).permute(0, 2, 1, 3)


def rows_of(x, batch, t, width):
    """[batch, heads, t, head_dim] -> [batch * t, width]"""
    return x.permute(0, 2, 1, 3).reshape(batch * t, width)


def plain_attention(q, k, v):
    """q, k, v [batch, heads, t, head_dim] (q pre-scaled) -> the same shape; differentiable."""
    return torch.softmax(q @ k.transpose(-1, -2), dim=-1) @ v


def _backward(qkv, dout, batch, t, width, head_dim, dtype, round_operands):
    q, k, v = (heads_of(qkv[:, i * width:(i + 1) * width].to(dtype), batch, t, width, head_dim) for i in range(3))
    do = heads_of(dout.to(dtype), batch, t, width, head_dim)
    p = torch.softmax(q @ k.transpose(-1, -2) + torch.zeros(t, t, dtype=dtype), dim=-1)
    dp = do @ v.transpose(-1, -2)
    d = (p * dp).sum(-1, keepdim=True)
    ds = p * (dp - d)
    if round_operands:
        p, ds = p.to(torch.bfloat16).to(dtype), ds.to(torch.bfloat16).to(dtype)
    dq, dk, dv = ds @ k, ds.transpose(-1, -2) @ q, p.transpose(-1, -2) @ do
    return torch.cat([rows_of(x, batch, t, width) for x in (dq, dk, dv)], dim=1)


def backward_fp64(qkv, dout, batch, t, width, head_dim):
    return _backward(qkv, dout, batch, t, width, head_dim, torch.float64, False)


def backward_emulated(qkv, dout, batch, t, width, head_dim):
    """bf16 [batch * t, 3 width]"""
    return _backward(qkv, dout, batch, t, width, head_dim, torch.float32, True).to(torch.bfloat16)


def make_inputs(batch, t, width, seed, head_dim, zero_item=None):
    """qkv randn with q pre-scaled by head_dim ** -0.5, dout randn with the rows of `zero_item` zero; both bf16."""
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(batch * t, 3 * width, generator=g)
    qkv[:, :width] *= 0.125 if head_dim == 64 else head_dim ** -0.5
    dout = torch.randn(batch * t, width, generator=g)
    if zero_item is not None:
        dout[zero_item * t:(zero_item + 1) * t] = 0
    return qkv.to(torch.bfloat16), dout.to(torch.bfloat16)
