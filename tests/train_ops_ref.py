"""Reference statements for csrc/train_ops.hip (tests/test_train_ops_host.py, tests/test_train_ops_gpu.py): the three backward formulas
in fp64, an fp32 emulation of each that rounds where the kernel rounds, and the input makers.

``planted`` switches one deliberate mistake on (the host test shows that each misses the bar the statements are held to):
  "var_w_minus_1"   LayerNorm: the variance divided by width - 1
  "drop_mean_gx"    LayerNorm: the mean(g x^) term of dx dropped
  "no_1702"         QuickGELU: the factor 1.702 missing from the second term of f'
  "phi_no_norm"     GELU: phi without its 1 / sqrt(2 pi)
"""
import math

import torch

EPS = 1e-5                     # kemr_op_layernorm's
BF16 = torch.bfloat16
MAX_GROUPS = 512               # csrc/train_ops.hip LNB_MAX_GROUPS


def rel_l2(x, ref):
    x, ref = x.double(), ref.double()
    den = float(ref.norm())
    return float((x - ref).norm()) / den if den else float((x - ref).norm())


# ------------------------------------------------------------------------------------------------ fp64 statements
def ln_backward_fp64(x, gamma, dy, planted=None):
    """(dx, dgamma, dbeta) of y = LayerNorm(x) gamma + beta for dy = d loss / d y, all fp64: g = dy gamma, x^ = (x - mean) rstd,
    dx = rstd (g - mean(g) - x^ mean(g x^)), dgamma = sum_rows dy x^, dbeta = sum_rows dy."""
    x, gamma, dy = x.double(), gamma.double(), dy.double()
    w = x.shape[-1]
    mean = x.mean(dim=-1, keepdim=True)
    var = ((x - mean) ** 2).sum(dim=-1, keepdim=True) / (w - 1 if planted == "var_w_minus_1" else w)
    rstd = 1.0 / torch.sqrt(var + EPS)
    xh = (x - mean) * rstd
    g = dy * gamma
    m2 = 0.0 if planted == "drop_mean_gx" else (g * xh).mean(dim=-1, keepdim=True)
    dx = rstd * (g - g.mean(dim=-1, keepdim=True) - xh * m2)
    return dx, (dy * xh).sum(dim=0), dy.sum(dim=0)


def qgelu_fp64(x):
    x = x.double()
    return x * torch.sigmoid(1.702 * x)


def qgelu_grad_terms_fp64(x, planted=None):
    """The two terms of f' = s + 1.702 x s (1 - s), s = sigmoid(1.702 x); s (1 - s) is formed without the cancellation of 1 - s."""
    x = x.double()
    s = torch.sigmoid(1.702 * x)
    c = torch.sigmoid(-1.702 * x)                        # 1 - s
    return s, (1.0 if planted == "no_1702" else 1.702) * x * s * c


def gelu_fp64(x):
    x = x.double()
    return 0.5 * x * torch.erfc(-x / math.sqrt(2.0))


def gelu_grad_terms_fp64(x, planted=None):
    """The two terms of f' = Phi(x) + x phi(x); Phi in its erfc form (relative accuracy in the negative tail)."""
    x = x.double()
    phi = torch.exp(-0.5 * x * x) * (1.0 if planted == "phi_no_norm" else 1.0 / math.sqrt(2.0 * math.pi))
    return 0.5 * torch.erfc(-x / math.sqrt(2.0)), x * phi


ACT = {0: (qgelu_fp64, qgelu_grad_terms_fp64), 1: (gelu_fp64, gelu_grad_terms_fp64)}


def act_backward_fp64(pre, dout, kind, planted=None):
    a, b = ACT[kind][1](pre, planted)
    return dout.double() * (a + b)


# ------------------------------------------------------------------------------------------------ fp32 emulations
def _fma(a, b, c):
    """fp32 fma(a, b, c): the product is exact in fp64 (one extra rounding of the sum to 53 bits, far below fp32's)."""
    return (a.double() * b.double() + c.double()).float()


def _wave_sum(s):
    """common.h wave_sum on [rows, 64] lane values: the xor butterfly 32, 16, ..., 1 (every lane ends with the same sum)."""
    o = 32
    while o:
        s = s[:, :o] + s[:, o:2 * o]
        o >>= 1
    return s                                             # [rows, 1]


def _lanes(t):
    """[rows, W] -> [rows, NV, 64, 4]: lane l of the row's wave holds elements 4 (64 i + l) .. + 3, i < NV."""
    return t.reshape(t.shape[0], -1, 64, 4)


def _lane_sum(t4):
    """sum over i of (e0 + e1) + (e2 + e3), i ascending, per lane; then the wave sum."""
    s = torch.zeros(t4.shape[0], 64, dtype=torch.float32)
    for i in range(t4.shape[1]):
        s = s + ((t4[:, i, :, 0] + t4[:, i, :, 1]) + (t4[:, i, :, 2] + t4[:, i, :, 3]))
    return _wave_sum(s)


def ln_groups(rows):
    return min((rows + 3) // 4, MAX_GROUPS)


def ln_backward_emulated(x, gamma, dy):
    """fp32 throughout, in the order include/kemr.h states for kemr_op_layernorm_backward: mean and rstd as the forward's (lane sums,
    wave butterfly, two passes); wave w of workgroup g walks rows 4 g + w, + 4 G, ... and accumulates dgamma (fma) and dbeta in that
    order; the four waves combine as ((w0 + w1) + w2) + w3; the second kernel's wave w sums slabs w, w + 4, ... and its waves combine
    the same way.  What is left between this and the kernel is the compiler's choice of fused multiply-adds inside a row."""
    x, gamma, dy = x.float(), gamma.float(), dy.float()
    rows, w = x.shape
    inv_w = torch.tensor(1.0 / w, dtype=torch.float32)
    mean = _lane_sum(_lanes(x)) * inv_w
    v = x - mean
    rstd = 1.0 / torch.sqrt(_lane_sum(_lanes(v * v)) * inv_w + torch.tensor(EPS, dtype=torch.float32))
    xh = v * rstd
    g = dy * gamma
    m1, m2 = _lane_sum(_lanes(g)) * inv_w, _lane_sum(_lanes(g * xh)) * inv_w
    dx = rstd * ((g - m1) - xh * m2)
    groups = ln_groups(rows)
    steps = (rows + 4 * groups - 1) // (4 * groups) if rows else 0
    pad = steps * 4 * groups - rows
    dyp = torch.cat([dy, torch.zeros(pad, w)]).reshape(steps, groups, 4, w)
    xhp = torch.cat([xh, torch.zeros(pad, w)]).reshape(steps, groups, 4, w)
    ag, ab = torch.zeros(groups, 4, w), torch.zeros(groups, 4, w)
    for k in range(steps):
        ab = ab + dyp[k]
        ag = _fma(dyp[k], xhp[k], ag)
    out = []
    for acc in (ag, ab):
        slab = ((acc[:, 0] + acc[:, 1]) + acc[:, 2]) + acc[:, 3]                      # [G, w]
        n4 = (groups + 3) // 4
        slab = torch.cat([slab, torch.zeros(4 * n4 - groups, w)]).reshape(n4, 4, w)
        part = torch.zeros(4, w)
        for j in range(n4):
            part = part + slab[j]
        out.append(((part[0] + part[1]) + part[2]) + part[3])
    return dx, out[0], out[1]


def act_forward_emulated(pre, kind):
    x = pre.float()
    y = x * torch.sigmoid(1.702 * x) if kind == 0 else 0.5 * x * torch.erfc(x * -0.70710677)
    return y.to(BF16)


def act_backward_emulated(pre, dout, kind):
    x = pre.float()
    if kind == 0:
        s, c = torch.sigmoid(1.702 * x), torch.sigmoid(-1.702 * x)
        d = s + 1.702 * x * s * c
    else:
        d = 0.5 * torch.erfc(x * -0.70710677) + x * (torch.exp(-0.5 * x * x) * 0.3989423)
    return (dout.float() * d).to(BF16)


# ------------------------------------------------------------------------------------------------ inputs
def make_ln_inputs(rows, width, seed, dy_dtype=BF16):
    """(x fp32, gamma fp32, dy): rows with a nonzero mean each (offsets of a few standard deviations), every 7th row heavy-tailed (cubed
    normals, a few entries of hundreds), a gamma with spread (0.05 .. 5, both signs), dy normal and rounded to dy_dtype."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, width, generator=g) * (0.5 + torch.rand(rows, 1, generator=g) * 4) + torch.randn(rows, 1, generator=g) * 3
    heavy = torch.arange(rows) % 7 == 3
    x[heavy] = x[heavy] + torch.randn(int(heavy.sum()), width, generator=g) ** 3 * 4
    gamma = torch.exp(torch.rand(width, generator=g) * 4.6 - 3.0) * torch.where(torch.rand(width, generator=g) < 0.2, -1.0, 1.0)
    dy = torch.randn(rows, width, generator=g).to(dy_dtype)
    return x.contiguous(), gamma.contiguous(), dy.contiguous()


def make_act_inputs(n, seed):
    """(pre bf16 [n], dout bf16 [n]): pre covers [-12, 12] densely (every bf16 value of the range when n allows, else an even spread),
    plus +-0, +-large (60, 1e4, 65536: far beyond where every term has saturated or underflowed) and the zero crossing of GELU's derivative near -0.75; dout normal."""
    g = torch.Generator().manual_seed(seed)
    special = torch.tensor([0.0, -0.0, 65536.0, -65536.0, 1.0e4, -1.0e4, 60.0, -60.0, -0.75, -0.7518, -0.7539, -0.7461, 5.9, -5.9, 12.0, -12.0])
    allb = torch.arange(0, 1 << 16, dtype=torch.int32).to(torch.int16).view(BF16)
    dense = allb[torch.isfinite(allb.float()) & (allb.float().abs() <= 12)]
    room = n - special.numel()
    if room >= dense.numel():
        fill = torch.cat([dense, (torch.rand(room - dense.numel(), generator=g) * 24 - 12).to(BF16)])
    else:
        fill = torch.linspace(-12, 12, max(room, 0)).to(BF16)
    pre = torch.cat([special.to(BF16), fill])[:n].contiguous()
    dout = torch.randn(n, generator=g).to(BF16)
    return pre, dout
