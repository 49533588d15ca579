"""Rounding helpers for holding kernels to their rounding budgets.

TEST INFRASTRUCTURE ONLY (see ``oracle/__init__.py``).

A kernel that rounds its result once, to nearest even, lands within half an ulp of the exact value; what it computes in fp32
before that rounding moves the exact value by a little more (``extra``).  The helpers state both sides in fp64 on whatever
device the tensors live on:

* ``ulp(x, fmt)``: the unit in the last place of ``x`` in ``bf16``, ``e4m3`` (OCP e4m3fn) or ``fp32``, subnormals included.
* ``rne_bf16(x)`` / ``rne_e4m3(x)`` / ``rne_f32(x)``: one round-to-nearest-even of the fp64 values (no double rounding through
  fp32); ``rne_e4m3`` saturates at +-448 like ``kemr_op_e4m3_host``.
* ``budget_ratio(got, ref64, extra)``: ``|got - ref64| / (0.5 ulp(got) + extra)`` elementwise: <= 1 for a correctly rounded
  output of a value that the fp32 arithmetic moved by at most ``extra``.
* ``signed_bias_ulps(got, ref64)``: the mean of ``(got - ref64) sign(ref64) / ulp(ref64)``: ~0 for round-to-nearest-even,
  -0.5 for truncation, positive for an output that is systematically too large in magnitude.
"""
from __future__ import annotations

import torch

# significant bits (implicit one included) and the exponent of the smallest normal, as frexp reports it (x = m 2^e, m in [.5, 1))
_FORMATS = {"bf16": (8, -125), "e4m3": (4, -5), "fp32": (24, -125)}
E4M3_MAX = 448.0


def _fmt(fmt: str):
    if fmt not in _FORMATS:
        raise ValueError(f"unknown format {fmt!r} (one of {sorted(_FORMATS)})")
    return _FORMATS[fmt]


def _exp(x: torch.Tensor, emin: int) -> torch.Tensor:
    _, e = torch.frexp(x)
    return torch.where(x == 0, torch.full_like(e, emin), e).clamp_min(emin)


# The frexp / ldexp arithmetic runs on the CPU (results go back to the input's device): it is the statement of the rounding, and
# the CPU's fp64 is IEEE on every platform.
def ulp(x: torch.Tensor, fmt: str = "bf16") -> torch.Tensor:
    """fp64 ulp of every element of x in `fmt` (the subnormal spacing below the smallest normal)."""
    p, emin = _fmt(fmt)
    xc = x.double().cpu()
    return torch.ldexp(torch.ones_like(xc), _exp(xc, emin) - p).to(x.device)


def _rne(x: torch.Tensor, fmt: str) -> torch.Tensor:
    p, emin = _fmt(fmt)
    xc = x.double().cpu()
    e = _exp(xc, emin)
    return torch.ldexp(torch.round(torch.ldexp(xc, p - e)), e - p).to(x.device)    # torch.round: half to even


def rne_bf16(x: torch.Tensor) -> torch.Tensor:
    x64 = x.double()
    x32 = x64.float()
    if bool((x32.double() == x64).all()):                  # fp32 values: torch's fp32 -> bf16 cast is the one RNE rounding
        return x32.to(torch.bfloat16).double()
    return _rne(x64, "bf16")


def rne_f32(x: torch.Tensor) -> torch.Tensor:
    return _rne(x, "fp32")


def rne_e4m3(x: torch.Tensor) -> torch.Tensor:
    return _rne(x, "e4m3").clamp(-E4M3_MAX, E4M3_MAX)


def budget_ratio(got: torch.Tensor, ref64: torch.Tensor, extra=0.0, fmt: str = "bf16") -> torch.Tensor:
    got = got.double().cpu()
    extra = extra.double().cpu() if isinstance(extra, torch.Tensor) else extra
    return (got - ref64.double().cpu()).abs() / (0.5 * ulp(got, fmt) + extra)


def signed_bias_ulps(got: torch.Tensor, ref64: torch.Tensor, fmt: str = "bf16") -> float:
    ref64 = ref64.double().cpu()
    return float(((got.double().cpu() - ref64) * torch.sign(ref64) / ulp(ref64, fmt)).mean())


def worst(ratio: torch.Tensor, got: torch.Tensor, ref64: torch.Tensor) -> str:
    """The element with the largest ratio (NaN counts as the largest): its row, column, got, ref and ratio."""
    shape = (-1, ratio.shape[-1]) if ratio.dim() else (1, 1)
    r = ratio.double().reshape(shape)
    row, col = divmod(int(torch.argmax(torch.nan_to_num(r, nan=float("inf")))), r.shape[1])
    g, f = float(got.double().reshape(shape)[row, col]), float(ref64.double().reshape(shape)[row, col])
    return f"worst element row {row} col {col}: got {g!r} ref {f!r} ratio {float(r[row, col]):.4g}"


def check_budget(got: torch.Tensor, ref64: torch.Tensor, extra=0.0, fmt: str = "bf16", limit: float = 1.0,
                 max_bias: float | None = None, what: str = "") -> tuple[float, float]:
    """Asserts budget_ratio <= limit everywhere (and |signed bias| <= max_bias when given); returns (max ratio, bias)."""
    ratio = budget_ratio(got, ref64, extra, fmt)
    top = float(torch.nan_to_num(ratio, nan=float("inf")).max())
    assert top <= limit, f"{what}: budget ratio {top:.4g} > {limit} -- {worst(ratio, got, ref64)}"
    bias = signed_bias_ulps(got, ref64, fmt)
    if max_bias is not None:
        assert abs(bias) <= max_bias, f"{what}: signed bias {bias:+.4f} ulp beyond +-{max_bias}"
    return top, bias


def attention_emulation(qkv_bf16, batch, t, width, causal):
    """fp64 statement of what csrc/attention.hip computes (tests/test_numerics_gpu.py, tests/test_rounding_budget.py): q, k, v as the
    given bf16 values; scores and the row maximum; P = exp(s - max), whose row sum l is taken BEFORE P is rounded to bf16 for
    the PV product; O = (bf16(P) . V) / l.  Returns (O, extra): extra bounds how far the kernel's fp32 arithmetic may move
    each output before its final rounding -- up to two keys of a row whose bf16(P) lands on the other side of a rounding
    boundary, the fp32 error of the scores, of exp2 and of the two accumulations."""
    heads = width // 64
    x = qkv_bf16.double().view(batch, t, 3, heads, 64).permute(2, 0, 3, 1, 4)
    q, k, v = x[0], x[1], x[2]                                                   # [B, H, T, 64]
    s = q @ k.transpose(-1, -2)
    sabs = q.abs() @ k.abs().transpose(-1, -2)
    if causal:
        mask = torch.ones(t, t, dtype=torch.bool, device=s.device).triu_(1)
        s = s.masked_fill(mask, float("-inf"))
    mx = s.amax(-1, keepdim=True)
    p = torch.exp(s - mx)
    l = p.sum(-1, keepdim=True)
    pb = rne_bf16(p)
    o = (pb @ v) / l
    vabs = v.abs()
    flip = 2 * (ulp(pb) * (pb > 0) * vabs.amax(-1).unsqueeze(-2)).amax(-1, keepdim=True) / l
    eps = 2.0 ** -24 * (16 * sabs + 2 * (s.abs() + mx.abs()).nan_to_num(0.0, 0.0, 0.0) * 1.4427 + 4)
    prop = ((eps * p) @ vabs + (eps * p).sum(-1, keepdim=True) * o.abs()) / l
    acc = 2.0 ** -24 * (16 * (pb @ vabs) / l + 4 * o.abs())
    extra = flip.expand_as(o) + prop + acc
    back = lambda y: y.permute(0, 2, 1, 3).reshape(batch * t, width)            # noqa: E731
    return back(o), back(extra)
