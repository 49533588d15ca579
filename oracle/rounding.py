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
  -0.5 for truncation, positive for an output that is systematically too large in magnitude.  ``relative_bias`` is the form for
  fp32 outputs that carry accumulated error.
* fp64 statements of the kernels: ``attention_emulation`` (csrc/attention.hip tile kernels), ``attention_long_emulation`` (the
  streaming kernel, P rounded against the running max of 64-key chunks), ``attention_pooled_emulation`` (one pooled query row),
  ``tail_emulation`` / ``l2norm_emulation`` (the pooling tail: LayerNorm @ proj, then the L2 step), ``patch_tokens_emulation``
  (the vision tower's token rows) and ``panel_scores_emulation`` (the similarity kernels' scores).  Each returns the exact value
  and ``extra``, derived in its docstring.
* exact statements, compared bit for bit: ``text_tokens_statement`` (the text tower's token rows and packed row starts) and
  ``panel_statement`` (the bf16 similarity panels); ``panel_representation_bound`` bounds what the panels' bf16 split costs
  against fp64 of the fp32 embeddings.
* fp64 statements of the learned-head kernels (csrc/rank.hip, csrc/rerank.hip): ``linear_head_statement``, ``gate_rows_emulation``,
  ``cross_attention_pairs_emulation`` and ``cross_attention_rerank_emulation``.  Their budgets use the square-root form of an fp32
  FMA chain's error (``FUSION_LAMBDA``), derived in ``_chain``.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

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


def signed_bias_ulps(got: torch.Tensor, ref64: torch.Tensor, fmt: str = "bf16", extra=None) -> float:
    """With `extra`: the mean over the elements whose extra is at most a quarter ulp, i.e. whose error the final rounding dominates.
    Where the fp32 arithmetic before the rounding is larger than an ulp -- outputs near 0, whose absolute error is their row's --
    the error in ulps is large and of either sign: one such element of a correct streaming-attention stand-in reads 8236 ulp and
    alone moves the mean over 300k outputs by 0.028 (tests/test_rounding_budget.py)."""
    ref64 = ref64.double().cpu()
    e = (got.double().cpu() - ref64) * torch.sign(ref64) / ulp(ref64, fmt)
    if extra is not None:
        extra = extra.double().cpu() if isinstance(extra, torch.Tensor) else torch.full_like(ref64, float(extra))
        e = e[(extra <= 0.25 * ulp(ref64, fmt)).expand_as(e)]
    return float(e.mean())


def worst(ratio: torch.Tensor, got: torch.Tensor, ref64: torch.Tensor) -> str:
    """The element with the largest ratio (NaN counts as the largest): its row, column, got, ref and ratio."""
    shape = (-1, ratio.shape[-1]) if ratio.dim() else (1, 1)
    r = ratio.double().reshape(shape)
    row, col = divmod(int(torch.argmax(torch.nan_to_num(r, nan=float("inf")))), r.shape[1])
    g, f = float(got.double().reshape(shape)[row, col]), float(ref64.double().reshape(shape)[row, col])
    return f"worst element row {row} col {col}: got {g!r} ref {f!r} ratio {float(r[row, col]):.4g}"


def check_budget(got: torch.Tensor, ref64: torch.Tensor, extra=0.0, fmt: str = "bf16", limit: float = 1.0,
                 max_bias: float | None = None, what: str = "", bias_rounding_only: bool = False) -> tuple[float, float]:
    """Asserts budget_ratio <= limit everywhere (and |signed bias| <= max_bias when given; bias_rounding_only: over the elements
    the final rounding dominates, signed_bias_ulps with extra); returns (max ratio, bias)."""
    ratio = budget_ratio(got, ref64, extra, fmt)
    top = float(torch.nan_to_num(ratio, nan=float("inf")).max())
    assert top <= limit, f"{what}: budget ratio {top:.4g} > {limit} -- {worst(ratio, got, ref64)}"
    bias = signed_bias_ulps(got, ref64, fmt, extra if bias_rounding_only else None)
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
    mask = torch.ones(t, t, dtype=torch.bool, device=q.device).triu_(1) if causal else None
    o, extra = _attention_rows(q, k, v, mask)
    back = lambda y: y.permute(0, 2, 1, 3).reshape(batch * t, width)            # noqa: E731
    return back(o), back(extra)


def _attention_rows(q, k, v, mask):
    """attention_emulation's statement for query rows q [..., Tq, 64] against keys k, v [..., Tk, 64] (fp64 holding bf16 values);
    mask (broadcast to [..., Tq, Tk], True = not a key of that row) or None.  Returns (O, extra), both [..., Tq, 64]."""
    s = q @ k.transpose(-1, -2)
    sabs = q.abs() @ k.abs().transpose(-1, -2)
    if mask is not None:
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
    return o, flip.expand_as(o) + prop + acc


def attention_long_emulation(qkv_bf16, batch, t, width, kc=64):
    """fp64 statement of what csrc/attention_stream.hip computes (non-causal, K / V streamed in chunks of kc keys; KEMR_ATTN_STREAM_KC,
    default 64).  The kernel rounds P to bf16 against the RUNNING maximum of the keys seen so far, not the final one, so
    attention_emulation (one pass, final maximum) does not state it.  Per query row, for chunk c (keys c kc .. min(T, (c + 1) kc) - 1;
    the pad keys of the ragged last chunk are -inf, i.e. absent):
        m_c = max of the scores of chunks 0 .. c,   P_c = exp(s - m_c),   f_c = exp(m_c - m_final)
        l   = sum_c f_c sum(P_c)               (the row sum from the UNROUNDED P, as in the tile kernel)
        O   = sum_c f_c (bf16(P_c) . V_c) / l  (the kernel's alpha = exp2(m_{c-1} - m_c) per chunk multiplies out to f_c)
    Returns (O, extra) as attention_emulation, [B T, width].  With u = 2^-24 (fp32 unit roundoff) and n = ceil(T / kc), extra is:
    * flip -- the bf16 rounding of a key's P is the one place where an fp32 error of relative size eps can move an output by a whole
      bf16 step.  The kernel's P differs from P_c by at most eps P_c (below), so a key can round to another value only if bf16(P_c (1 - eps))
      or bf16(P_c (1 + eps)) differs from bf16(P_c); its possible move is the larger of those two differences, and the term is
      sum_c f_c (move . |V_c|) / l -- every such key counted, per output column (a key no perturbation can flip contributes nothing).
      eps = u (16 sabs + 2 (|s| + |m_c|) log2 e + 4): the fp32 score (two bf16 MFMAs over 64 products, sabs = sum |q||k|, the bound
      attention_emulation uses), the fma s log2e - m' whose operands (|s|, the rounded running maximum |m_c| log2e) are rounded once
      each (< 2 u (|s| + |m_c|) log2 e in the exponent; its exp2 turns an error d of the exponent into ln 2 d of P) and exp2's own
      error (< 2 ulp = 4 u).
    * prop -- the same eps moves l (P enters l unrounded): sum_c f_c sum(eps P_c) |O| / l.
    * chain -- what multiplies chunk c's part of O and of l is a product of up to n fp32 factors instead of f_c: per chunk an exp2
      (< 4 u) and the roundings of O alpha and l alpha (u each), so < 6 n u; the exponent ml - m' of each alpha is an fp32
      difference (rounding < u |m' - ml| log2 e, i.e. < u |m' - ml| in the factor; summed over the chunks < u (m_final - m_0)); and
      the running maximum is kept as the rounded fp32 product m log2e (< 2 u |m| log2 e, ln 2 of it in the factor, at the chunk's and
      at the final maximum: < 2 u max(|m_0|, |m_final|)).  rho = u (6 n + (m_final - m_0) + 2 max(|m_0|, |m_final|)) relative on every
      term: rho (sum_c f_c bf16(P_c) . |V_c| + l |O|) / l.
    * acc -- the fp32 sums: O, per chunk two MFMAs of 32 products (16 u, attention_emulation's bound) added to the running O (one
      rounding per chunk), and the fp32 division: (16 + n) u sum_c f_c bf16(P_c) . |V_c| / l + 4 u |O|; l: positive terms, summed
      per lane in two accumulators of kc / 8 (8 roundings), added (1), rescaled and added to l (2 per chunk), then 2 shuffles:
      < (12 + 2 n) u relative, (12 + 2 n) u |O|."""
    heads = width // 64
    x = qkv_bf16.double().cpu().view(batch, t, 3, heads, 64).permute(2, 0, 3, 1, 4)
    o, extra = _attention_chunked(x[0], x[1], x[2], None, kc)                   # q, k, v [B, H, T, 64]
    back = lambda y: y.permute(0, 2, 1, 3).reshape(batch * t, width)            # noqa: E731
    return back(o), back(extra)


def _attention_chunked(q, k, v, key_ok, kc):
    """attention_long_emulation's statement for query rows q [..., Tq, 64] against keys k, v [..., Tk, 64] in chunks of kc keys;
    key_ok (broadcast to [..., 1, Tk], False = not a key of that item) or None.  Returns (O, extra), both [..., Tq, 64]."""
    u = 2.0 ** -24
    t = k.shape[-2]
    n = (t + kc - 1) // kc
    chunks = [(c * kc, min(t, (c + 1) * kc)) for c in range(n)]

    def scores(a, b):
        s = q @ k[..., a:b, :].transpose(-1, -2)
        return s if key_ok is None else s.masked_fill(~key_ok[..., a:b], float("-inf"))

    m_run, m = [], torch.full(q.shape[:-1] + (1,), float("-inf"), dtype=torch.float64)
    for a, b in chunks:
        m = torch.maximum(m, scores(a, b).amax(-1, keepdim=True))
        m_run.append(m)
    m_fin, m_0 = m_run[-1], m_run[0]
    zero = torch.zeros_like(q)
    o_sum, w_abs, flip = zero.clone(), zero.clone(), zero.clone()
    l, l_eps = torch.zeros_like(m_fin), torch.zeros_like(m_fin)
    for (a, b), m_c in zip(chunks, m_run):
        kk, vv = k[..., a:b, :], v[..., a:b, :]
        s = scores(a, b)
        sabs = q.abs() @ kk.abs().transpose(-1, -2)
        f = torch.exp(m_c - m_fin)
        p = torch.exp(s - m_c)                                                   # 0 where s = -inf
        pb = rne_bf16(p)
        eps = u * (16 * sabs + 2 * (s.nan_to_num(0.0, 0.0, 0.0).abs() + m_c.abs()) * 1.4427 + 4)
        move = torch.maximum((rne_bf16(p * (1 - eps)) - pb).abs(), (rne_bf16(p * (1 + eps)) - pb).abs())
        l = l + f * p.sum(-1, keepdim=True)
        l_eps = l_eps + f * (eps * p).sum(-1, keepdim=True)
        o_sum = o_sum + f * (pb @ vv)
        w_abs = w_abs + f * (pb @ vv.abs())
        flip = flip + f * (move @ vv.abs())
    o = o_sum / l
    rho = u * (6 * n + (m_fin - m_0) + 2 * torch.maximum(m_0.abs(), m_fin.abs()))
    extra = (flip + l_eps * o.abs() + rho * (w_abs + l * o.abs()) + (16 + n) * u * w_abs) / l + (16 + 2 * n) * u * o.abs()
    return o, extra


def pooled_keys(pool_idx, row_start, items, tokens, causal, maxk):
    """The key rows of each item as csrc/attention.hip attention_pooled_kernel takes them: r0 = row_start[b] (or b tokens), nk = tokens
    (vision) or pool_idx[b] - r0 + 1 (text), clamped into 1 .. maxk (the instantiation: 320 or 1088 keys).  Returns (r0, nk) as int64."""
    r0 = row_start[:items].long().cpu() if row_start is not None else torch.arange(items, dtype=torch.int64) * tokens
    nk = pool_idx[:items].long().cpu() - r0 + 1 if causal else torch.full((items,), tokens, dtype=torch.int64)
    return r0, nk.clamp(1, maxk)


def attention_pooled_emulation(q_bf16, qkv_bf16, pool_idx, row_start, items, tokens, width, causal, maxk):
    """fp64 statement of the pooled-row attention (csrc/attention.hip attention_pooled_kernel): one query row per item and head
    against the keys r0 .. r0 + nk - 1 of pooled_keys.  Its arithmetic is the tile kernel's for one row -- the global maximum
    of the row first, P = exp(s - max), the row sum from the unrounded P, bf16(P) into PV, one division at the end -- so
    attention_emulation restricted to that row states its O.  Its extra does not serve here: the flip term (two keys at the row's
    largest bf16(P) step) exceeds a quarter ulp of every output of a row of <= 77 keys, which leaves the signed-bias bar no element
    to measure.  The statement used is attention_long_emulation's with ONE chunk holding every key (m_c = the final max, f = 1: the
    single-pass O), whose flip term counts only the keys an fp32 error can flip.  Its fp32 sums are no longer than the bounds
    assume where it matters: the score of a key is 8 fma per lane + 3 shuffle adds (< 16 u sabs), and the PV sum runs sequentially
    over nk / 2 keys per lane, whose rounding errors are independent in sign, far below 17 u sum bf16(P)|V| in size at nk <= 1088
    (tests/test_numerics_paths_gpu.py prints the worst ratio).  Returns (O, extra) [items, width]."""
    heads = width // 64
    qkv = qkv_bf16.double().cpu()
    r0, nk = pooled_keys(pool_idx, row_start, items, tokens, causal, maxk)
    j = torch.arange(int(nk.max()))
    valid = j[None, :] < nk[:, None]
    rows = torch.where(valid, r0[:, None] + j[None, :], r0[:, None])                # [items, K]: masked keys read row r0 (P = 0)
    kv = qkv[rows]
    k = kv[..., width:2 * width].reshape(items, -1, heads, 64).transpose(1, 2)        # [items, H, K, 64]
    v = kv[..., 2 * width:].reshape(items, -1, heads, 64).transpose(1, 2)
    qh = q_bf16.double().cpu().view(items, heads, 1, 64)
    o, extra = _attention_chunked(qh, k, v, valid[:, None, None, :], max(1, int(nk.max())))
    return o.reshape(items, width), extra.reshape(items, width)


LN_EPS = 1e-5


def tail_emulation(xs, gamma, beta, proj, kappa, ln_factor):
    """fp64 statement of the pooling tail's first kernel (csrc/embed.hip tail_proj_kernel).  xs [batch, width]: the rows it normalises,
    EXACTLY -- the stored pooled row decoded from fp32 / 24-bit / bf16 and the pending updates added in fp32 in the kernel's order,
    (x + d1) + d2 (the caller builds them with torch fp32 adds, which round like the device's).  y = LayerNorm(xs) (eps LN_EPS,
    biased variance) * gamma + beta, out = y @ proj, in fp64.  Returns (out, extra):
        extra = kappa u sum_i |y_i| |P_ij|  +  ln_factor max_i |y_i| sum_i |P_ij|
    the first term the fp32 accumulation of the projection (width / 16 fma per lane, then 4 shuffle adds; kappa measured), the second
    the fp32 LayerNorm's error of y (< ln_factor max|y| per element: the bar tests/test_numerics_gpu.py holds the two-pass LayerNorm
    kernels to, the same arithmetic) carried through |P|."""
    x = xs.double().cpu()
    mean = x.mean(-1, keepdim=True)
    d = x - mean
    rstd = 1.0 / torch.sqrt((d * d).mean(-1, keepdim=True) + LN_EPS)
    y = d * rstd * gamma.double().cpu() + beta.double().cpu()
    p = proj.double().cpu()
    out = y @ p
    extra = kappa * 2.0 ** -24 * (y.abs() @ p.abs()) + ln_factor * y.abs().amax(-1, keepdim=True) * p.abs().sum(0)
    return out, extra


def l2norm_emulation(r):
    """fp64 statement of the pooling tail's L2 step (csrc/embed.hip l2norm_rows_kernel) applied to r, the kernel's own unnormalised
    fp32 output (a normalize = 0 run): r / ||r||.  Returns (ref, extra).  The kernel sums r_i^2 per lane over ceil(d / 64) columns
    (one rounding per product and per add: < (n + 1) u relative on positive terms), then over the wave in 6 butterfly adds (6 u):
    the sum S carries < (n + 7) u; sqrtf halves that and rounds once (u), 1.0f / x rounds once (u), and the product r_i * inv
    rounds once -- that last rounding is the half ulp of the budget ratio.  So extra = ((n + 7) / 2 + 2) u |ref|."""
    r64 = r.double().cpu()
    ref = r64 / r64.norm(dim=-1, keepdim=True)
    n = (r.shape[-1] + 63) // 64
    return ref, ((n + 7) / 2 + 2) * 2.0 ** -24 * ref.abs()


def relative_bias(got: torch.Tensor, ref64: torch.Tensor) -> float:
    """sum((got - ref64) sign(ref64)) / sum|ref64| in units of 2^-24: the signed bias of fp32 outputs that carry accumulated error
    (signed_bias_ulps divides by each element's own ulp, so outputs near 0 -- whose absolute error is that of their row -- would
    swamp it).  ~0 for unbiased arithmetic; 16 for outputs 2^-20 too large."""
    ref64 = ref64.double().cpu()
    return float(((got.double().cpu() - ref64) * torch.sign(ref64)).sum() / ref64.abs().sum()) * 2.0 ** 24


# ------------------------------------------------------------------------------------------------ token fronts
def patch_conv(px, conv_w, patch, with_abs=False):
    """The reference's patch embedding (OpenAI CLIP VisionTransformer: conv1, then reshape / permute to token rows) on the operands
    the kernels see: conv2d(rne_bf16(px), rne_bf16(conv_w), stride=patch) in fp64 on px's device, as [batch, patches, width] (patch
    py * grid + px).  with_abs: also the same of |px|, |w|.  Returns conv (or (conv, |conv|))."""
    x, w = rne_bf16(px.double()), rne_bf16(conv_w.double().to(px.device))
    tok = lambda y: y.flatten(2).transpose(1, 2)                                # noqa: E731
    conv = tok(F.conv2d(x, w, stride=patch))
    return (conv, tok(F.conv2d(x.abs(), w.abs(), stride=patch))) if with_abs else conv


def patch_tokens_emulation(px, conv_w, cls, pos, patch, kappa):
    """fp64 statement of the vision tower's token front: the fp32 rows [batch * tokens, width] ln_pre reads (csrc/embed.hip
    im2col_kernel and cls_rows_kernel, the EPI_PATCH_F32 epilogue of csrc/gemm.hip / gemm256.hip).  im2col rounds every pixel to bf16
    (RNE) and the host packs conv1.weight as bf16 (RNE), zero beyond its 3 p^2 columns; the GEMM sums the products in fp32 and its
    epilogue adds pos[1 + patch] to the sum in fp32 and stores the token row (image b, patch i: row b tokens + 1 + i).  So
        patch rows: ref = patch_conv + pos[1:],  extra = kappa u patch_conv(|px|, |w|)
        class rows: ref = fp32(cls + pos[0])     (cls_rows_kernel: one fp32 add; extra 0)
    A product of two bf16 values has at most 16 significant bits, exact in fp32, so the accumulation is the only error before the
    epilogue: at most kappa u sum|a||w| (u = 2^-24; the GEMM accumulator bar of tests/test_numerics_gpu.py).  The add of pos rounds
    once -- the half ulp of budget_ratio(fmt="fp32").  The K-pad columns add nothing (0 x 0).  Returns (ref, extra) on px's device."""
    conv, cabs = patch_conv(px, conv_w, patch, with_abs=True)
    b, _, width = conv.shape
    row0 = (cls.float().cpu() + pos.float().cpu()[0]).double().to(conv.device)
    ref = torch.cat([row0.expand(b, 1, width), conv + pos.double().to(conv.device)[1:]], 1)
    extra = torch.cat([torch.zeros_like(conv[:, :1]), kappa * 2.0 ** -24 * cabs], 1)
    return ref.reshape(-1, width), extra.reshape(-1, width)


def text_row_starts(lens, rows, ctx):
    """csrc/embed.hip row_starts_kernel: every length clamped into 1 .. ctx, the prefix sums capped so that every text keeps a row:
    row_start[0] = 0, row_start[i + 1] = min(l_0 + .. + l_i, rows - (batch - i - 1)).  int32 [batch + 1] on the CPU."""
    l = lens.long().cpu().reshape(-1).clamp(1, ctx)
    batch = l.numel()
    cap = rows - (batch - 1 - torch.arange(batch))
    return torch.cat([torch.zeros(1, dtype=torch.int64), torch.minimum(l.cumsum(0), cap)]).int()


def text_tokens_statement(ids, lens, rows, tok, pos, vocab, ctx):
    """Exact statement of the text tower's token front (csrc/embed.hip text_embed_kernel; row_starts_kernel for packed texts): the fp32
    rows tok[clamp(id, 0, vocab - 1)] + pos[t], ONE fp32 add each (torch's fp32 add on the CPU rounds like the device's).
    lens None: kemr_encode_text's batch * ctx rows, row b ctx + t = text b, position t.  Otherwise kemr_encode_text_packed's `rows`
    rows: text i owns the rows row_start[i] .. row_start[i + 1] - 1 (text_row_starts); row r belongs to the last text i with
    row_start[i] <= r, at position t = min(r - row_start[i], ctx - 1) -- so rows behind the last text (rows > the sum of the
    lengths) repeat its last position.  Returns (rows fp32 [n, width], row_start int32 [batch + 1] or None) on the CPU; the caller
    turns the rows into the storage type with .to(torch.bfloat16) (RNE) or engine.pack_f24_rows."""
    ids = ids.long().cpu()
    batch = ids.shape[0]
    if lens is None:
        r = torch.arange(batch * ctx)
        text, t, rs = r // ctx, r % ctx, None
    else:
        rs = text_row_starts(lens, rows, ctx)
        r = torch.arange(rows)
        text = torch.searchsorted(rs[:batch].long(), r, right=True) - 1
        t = (r - rs.long()[text]).clamp_max(ctx - 1)
    idx = ids[text, t].clamp(0, vocab - 1)
    return tok.float().cpu()[idx] + pos.float().cpu()[t], rs


# ------------------------------------------------------------------------------------------------ similarity panels and scores
def _f32_scale(s) -> float:
    return float(torch.tensor(float(s), dtype=torch.float32))             # the ABI passes part scales as fp32


def _bf16_bits(x64):
    """bf16 tensor of values that bf16 represents exactly (subnormals included): the upper halves of their fp32 bits."""
    return (x64.float().view(torch.int32) >> 16).to(torch.int16).view(torch.bfloat16)


def panel_statement(parts, part_scale, row_scale, terms, side):
    """Exact statement of csrc/sim.hip panel_build_kernel: the panel [round_up(rows, 256), nparts terms dpad] as bf16 bits (dpad =
    round_up(d, 64), kemr_panel_kdim).  Per part p and row: sc = fp32(part_scale[p] row_scale[p][row]) (the part scale alone without
    a row scale), v = fp32(src sc), hi = rne_bf16(v), lo = rne_bf16(v - hi).  v - hi is exact in fp32: hi is v rounded to 8
    significant bits, so v - hi is a multiple of v's fp32 ulp (>= 2^-149) below 2^-8 |v|, at most 16 significant bits.  Subnormal
    values are kept, not flushed, on the device as here (tests/test_numerics_sim_gpu.py pins a lo that is an fp32 subnormal).  Part
    p's columns start at p terms dpad: terms 1 [hi]; terms 3 [hi | lo | hi] on the query side (side 0, KEMR_SIDE_QUERY), [hi | hi | lo]
    on the gallery side, so that the contraction is hi.hi + lo.hi + hi.lo.  Columns d .. dpad of every segment and the rows rows ..
    round_up(rows, 256) are +0 (simk_select_kernel relies on zero pad rows).  fp64 on the CPU with this module's explicit roundings."""
    parts = [p.double().cpu() for p in parts]
    rows, d = parts[0].shape
    dpad = (d + 63) // 64 * 64
    out = torch.zeros((rows + 255) // 256 * 256, len(parts) * terms * dpad, dtype=torch.float64)
    for p, src in enumerate(parts):
        sc = torch.full((rows, 1), _f32_scale(part_scale[p]) if part_scale is not None else 1.0, dtype=torch.float64)
        if row_scale is not None and row_scale[p] is not None:
            sc = rne_f32(sc * row_scale[p].double().cpu().reshape(rows, 1))
        v = rne_f32(src * sc)
        hi = _rne(v, "bf16")
        lo = _rne(v - hi, "bf16")
        segs = [hi] if terms == 1 else ([hi, lo, hi] if side == 0 else [hi, hi, lo])
        for s, x in enumerate(segs):
            c0 = (p * terms + s) * dpad
            out[:rows, c0:c0 + d] = x
    return _bf16_bits(out)


def panel_scores_emulation(qpanel, gpanel, kappa, nq=None, ng=None):
    """fp64 statement of the scores csrc/sim.hip computes from two panels (sim_kernel, whose dense form kemr_scores_dense hands back
    the fp32 accumulators; pair_scores_kernel has the same operand roles and k order): S = Q[:nq] G[:ng]^T over the panels' own bf16
    values.  Every product of two bf16 values is exact in fp32 (16 significant bits), so only the fp32 accumulation of the MFMA K loop
    moves the result: extra = kappa u sum |Q||G| (u = 2^-24, the GEMM accumulator bar; kappa measured on the device).  The fp64 sum
    of <= 4608 exact products is exact to ~2^-40 relative, far below that.  Returns (ref, extra) [nq, ng], fp64 on the CPU."""
    q, g = qpanel[:nq].double().cpu(), gpanel[:ng].double().cpu()
    return q @ g.T, kappa * 2.0 ** -24 * (q.abs() @ g.abs().T)


def panel_representation_bound(q_parts, g_parts, terms, q_part_scale=None, q_row_scale=None, g_part_scale=None, g_row_scale=None):
    """What the panels cost against fp64 of the fp32 inputs: ref = sum_p X_p Y_p^T with X = src part_scale row_scale of the query
    parts and Y the same of the gallery parts (fp64: the product of three fp32 values carries < 2^-50, negligible here), and a bound
    on |S_panel - ref|, S_panel = the panels' exact dot products (panel_scores_emulation's ref; the kernel's accumulation comes on
    top).  u = 2^-24; per element v = the fp32 value the panel splits, v = X (1 + eta):
    * eta: sc = fp32(part_scale row_scale) and v = fp32(src sc) round once each -- |eta| <= u when one of them can round (a part
      scale != 1 alone, or a row scale alone: sc = row_scale exactly), 2 u + u^2 with both, 0 with neither;
    * terms 1: hi = v (1 + d), |d| <= 2^-8 (bf16's unit roundoff), so |hi_q hi_g - v_q v_g| <= (2 2^-8 + 2^-16) |v_q v_g|;
    * terms 3: v = hi + lo + e, |v - hi| <= 2^-8 |v|, |lo| <= (1 + 2^-8) 2^-8 |v|, |e| <= 2^-8 |v - hi| <= 2^-16 |v|.  Expanding
      (hi + lo + e)(hi + lo + e) with hi + lo = v - e:
          v_q v_g - (hi_q hi_g + lo_q hi_g + hi_q lo_g) = lo_q lo_g + e_q v_g + e_g v_q - e_q e_g,
      the dropped lo.lo term and both second-split residuals: <= (3 2^-16 + 2^-23 + 2^-31) |v_q v_g|.
    With c that factor: |S_panel - ref| <= sum_p sum_i (c (1 + eta_q)(1 + eta_g) + eta_q + eta_g + eta_q eta_g) |X_i| |Y_i|.  For
    values in bf16's normal range (|v| >= 2^-126; below it a rounding's error is absolute, <= 2^-134).  On unit vectors (sum |X||Y|
    <= 1) the worst case is 7.8e-3 (terms 1) / 4.6e-5 (terms 3); tests/test_sim_gpu.py::_fp64_slice_check's 2e-3 / 2e-6 are the
    measured, not the worst-case, errors of d = 768 (the roundings of the d terms are independent in sign).  Returns (ref, bound)
    [nq, ng], fp64 on the CPU."""
    u = 2.0 ** -24
    c = 2 * 2.0 ** -8 + 2.0 ** -16 if terms == 1 else 3 * 2.0 ** -16 + 2.0 ** -23 + 2.0 ** -31

    def side(parts, ps, rs):
        xs, etas = [], []
        for p, src in enumerate(parts):
            s = _f32_scale(ps[p]) if ps is not None else 1.0
            r = rs[p] if rs is not None else None
            x = src.double().cpu() * s
            if r is not None:
                x = x * r.double().cpu().reshape(-1, 1)
            n = int(s != 1.0) + int(r is not None)
            xs.append(x)
            etas.append((0.0, u, 2 * u + u * u)[n])
        return xs, etas

    xq, eq = side(q_parts, q_part_scale, q_row_scale)
    xg, eg = side(g_parts, g_part_scale, g_row_scale)
    ref = sum(x @ y.T for x, y in zip(xq, xg))
    bound = sum((c * (1 + a) * (1 + b) + a + b + a * b) * (x.abs() @ y.abs().T) for x, y, a, b in zip(xq, xg, eq, eg))
    return ref, bound


# ------------------------------------------------------------------------------------------------ learned fusion heads
U32 = 2.0 ** -24              # fp32 unit roundoff
FUSION_LAMBDA = 1.0           # lambda of _chain; measured in tests/test_rounding_budget.py (see cross_attention_pairs_emulation)
SHORT_CHAIN_LAMBDA = 4.0      # lambda of linear_head_statement and gate_rows_emulation (see linear_head_statement)
TANH_ULPS = 4.0               # c_tanh: what the device's tanhf may cost, fp32 ulp of the output (tests/test_numerics_heads_gpu.py)
EXP_ULPS = 4.0                # the same for expf in gate_rows_kernel, ulp of exp(-s)
_TINY = 2.0 ** -126           # absolute floor: a fast exp that underflows to 0 where exp(-200) = 1e-87


def _chain(n, abs_sum, lam=None):
    """What an n-term fp32 FMA chain may move its sum by: lam sqrt(n) u sum|terms|.  Every step rounds once, by at most u times the
    partial sum, itself at most sum|terms|; the worst case n u sum|terms| assumes n roundings of one sign and full size, and is
    useless for a three-layer head (about 5e4 fp32 ulp of the output at hid1 = 256, hid2 = 64, where correct fp32 arithmetic
    reads 3e-4 of it and a dropped unit passes).  Roundings are independent in sign, so they add in quadrature: sqrt(n) u
    sum|terms| is an n-step random walk with every step at its largest; lam is the safety factor on top."""
    return (FUSION_LAMBDA if lam is None else lam) * (float(n) ** 0.5) * U32 * abs_sum


def _fusion_mix(d, dd, p_i, p_t, c0, w2t, b2, w3, b3, lam, c_tanh):
    """The pair arithmetic shared by the dense and the gathered cross_attention kernels, in fp64.  d [B, R, H] = image score - target
    score per head, dd [B, R, H] what fp32 moved d by before the exponential (0 where the scores are given); p_x [B, H, hid1].
    Returns (out, extra) [B, R].  See cross_attention_pairs_emulation for the derivation."""
    heads = d.shape[-1]
    w_i = torch.sigmoid(d)
    w_t = torch.sigmoid(-d)                                                   # 1 - w_i without cancellation
    eps_e = U32 * (2 * d.abs() * 1.4427 + 4) + 3 * U32
    dw_i = w_i * eps_e + w_i * w_t * dd + _TINY
    dw_t = w_t * eps_e + w_i * w_t * dd + _TINY
    pre = c0 + w_i @ p_i + w_t @ p_t                                          # [B, R, hid1]
    pre_abs = c0.abs() + w_i @ p_i.abs() + w_t @ p_t.abs()
    dh = dw_i @ p_i.abs() + dw_t @ p_t.abs() + _chain(2 * heads, pre_abs, lam)
    h = pre.clamp_min(0)
    z = h @ w2t + b2
    dz = torch.sqrt((dh * dh) @ (w2t * w2t)) + _chain(w2t.shape[0] + 1, h @ w2t.abs() + b2.abs(), lam)
    z = z.clamp_min(0)
    o = z @ w3 + b3
    do = torch.sqrt((dz * dz) @ (w3 * w3)) + _chain(w3.shape[0], z @ w3.abs() + abs(b3), lam)
    out = 0.5 * torch.tanh(o)
    return out, 0.5 * do + c_tanh * ulp(out, "fp32")


def _head_consts(c0, w2t, b2, w3, b3):
    c0, w2t, b2, w3 = (t.double().cpu() for t in (c0, w2t, b2, w3))
    return c0.reshape(-1), w2t, b2.reshape(-1), w3.reshape(-1), _f32_scale(b3)


def cross_attention_pairs_emulation(st_i, st_t, p_i, p_t, c0, w2t, b2, w3, b3, lam=None, c_tanh=None):
    """fp64 statement of csrc/rank.hip cross_attn_pair_kernel on the fp32 tensors it is given: st_x [H, n_c, n_q] scaled scores, p_x
    [n_c, H, hid1], c0 [hid1], w2t [hid1, hid2], b2 / w3 [hid2], b3 (passed as fp32).  Per pair and head w_i = sigmoid(st_i - st_t),
    w_t = 1 - w_i (the kernel's two-way softmax); h = relu(c0 + sum_h w_i P_i + w_t P_t); z = relu(h W2^T + b2);
    out = 0.5 tanh(z . w3 + b3).  Returns (out, extra) [n_c, n_q], the kernel's transposed layout.  With u = 2^-24:
    * weights: the kernel takes exp(s_x - max) of both sides (one of them exp(0) = 1), adds, takes the reciprocal and multiplies.  The
      exponential gets attention_emulation's allowance, u (2 |d| log2 e + 4) relative (the fp32 subtraction and the fast exp), the
      add, reciprocal and multiply u each: dw_x = w_x (u (2 |d| log2 e + 4) + 3 u), plus 2^-126 for an exp that underflows to 0;
    * h: 2 H FMAs on c0, _chain(2 H, |c0| + sum w_i |P_i| + w_t |P_t|), plus sum dw_i |P_i| + dw_t |P_t|; ReLU does not grow an error;
    * z: hid1 FMAs and the add of b2, _chain(hid1 + 1, h |W2^T| + |b2|), plus the errors of h carried through |W2| IN QUADRATURE,
      sqrt(sum_j (dh_j W2_jk)^2): the roundings of different units are independent (the weights' share of dh is common to the units
      of a pair; it is small beside the allowance it is given, which the measured ratios below confirm);
    * o: hid2 FMAs on b3, _chain(hid2, |b3| + z |w3|), plus sqrt(sum_k (dz_k w3_k)^2);
    * out: tanh is 1-Lipschitz, 0.5 do, plus TANH_ULPS fp32 ulp of the output for the device's tanhf.
    The final rounding of 0.5 * tanhf is exact (a power of two); check_budget(fmt="fp32") grants its half ulp regardless.
    lambda (FUSION_LAMBDA) = 1: the CPU fp32 stand-in of tests/test_rounding_budget.py, which follows the kernel's order with a
    separate multiply and add per FMA, reads 0.032 .. 0.050 of the budget on the four named cases (hid1 x hid2 7x1, 260x17, 256x64, 500x64; bar 0.25; the rerank
    stand-in 0.017); W2 rounded
    to bf16 reads above 100.  The kernels on an MI355X read at most 0.19 (dense) and 0.15 (gathered) over the cases of
    tests/test_numerics_heads_gpu.py (bar 1); on exact arguments their 0.5 tanhf lies within 1.22 fp32 ulp of the fp64 value, so
    TANH_ULPS stays at 4."""
    sti, stt = st_i.double().cpu(), st_t.double().cpu()
    d = (sti - stt).permute(1, 2, 0)                                          # [n_c, n_q, H]
    c0, w2t, b2, w3, b3 = _head_consts(c0, w2t, b2, w3, b3)
    return _fusion_mix(d, torch.zeros_like(d), p_i.double().cpu(), p_t.double().cpu(), c0, w2t, b2, w3, b3, lam,
                       TANH_ULPS if c_tanh is None else c_tanh)


def rerank_dots(q, k_i, k_t, heads, cand, depth):
    """The gathered route's per-head dot products in fp64: (a_i, a_t, |q|.|k_i| + |q|.|k_t|, valid), each [nq, depth, heads]
    (valid [nq, depth]: the slots whose id lies in 0 .. ng - 1; the others read candidate 0 and are to be ignored)."""
    q, k_i, k_t = q.double().cpu(), k_i.double().cpu(), k_t.double().cpu()
    nq, dim = q.shape
    ng = k_i.shape[0]
    ids = cand.long().cpu()[:, :depth]
    valid = (ids >= 0) & (ids < ng)
    ids = torch.where(valid, ids, torch.zeros_like(ids))
    per_head = lambda x: x.view(nq, depth, heads, dim // heads).sum(-1)       # noqa: E731
    qq = q[:, None, :]
    ki, kt = k_i[ids], k_t[ids]                                               # [nq, depth, dim]
    return per_head(qq * ki), per_head(qq * kt), per_head(qq.abs() * ki.abs()) + per_head(qq.abs() * kt.abs()), valid


def cross_attention_rerank_emulation(q, k_i, k_t, p_i, p_t, c0, w2t, b2, w3, b3, cand, depth, lam=None, c_tanh=None):
    """fp64 statement of csrc/rerank.hip cross_attn_rerank_kernel: for every slot (row, j < depth) of cand [nq, ld] with an id c in
    0 .. ng - 1, the pair statement of cross_attention_pairs_emulation behind the per-head dot products s_x[h] = Q[row, head h] .
    K_x[c, head h] (q [nq, dim] already scaled, k_x [ng, dim], head h = columns h dim / H .. (h + 1) dim / H - 1, H = p_i.shape[1]).
    Every other slot (padding, an id outside the gallery) is -inf with extra 0.  Returns (out, extra) [nq, depth].
    The kernel sums a head's dim / H products per lane (an FMA chain of 4, or single products) and over the wave in 6 butterfly
    adds: _chain(dim / H + 6, |q| . |k|) per dot product.  The two errors of a head move d = s_i - s_t by at most their sum, and the
    softmax weight by w_i w_t (the sigmoid's slope) times that, on top of the pair statement's dw.  The rest is the pair statement:
    the kernel keeps the dense kernel's FMA order for h, one ascending-k accumulator chain per MFMA tile for z and the same tail."""
    heads = p_i.shape[1]
    a_i, a_t, ab, valid = rerank_dots(q, k_i, k_t, heads, cand, depth)
    nq = a_i.shape[0]
    ids = torch.where(valid, cand.long().cpu()[:, :depth], torch.zeros_like(valid, dtype=torch.int64)).reshape(-1)
    d = (a_i - a_t).reshape(nq * depth, 1, heads)
    dd = _chain(q.shape[1] // heads + 6, ab, lam).reshape(nq * depth, 1, heads)
    c0, w2t, b2, w3, b3 = _head_consts(c0, w2t, b2, w3, b3)
    out, extra = _fusion_mix(d, dd, p_i.double().cpu()[ids], p_t.double().cpu()[ids], c0, w2t, b2, w3, b3, lam,
                             TANH_ULPS if c_tanh is None else c_tanh)
    out, extra = out.reshape(nq, depth), extra.reshape(nq, depth)
    return out.masked_fill(~valid, float("-inf")), extra.masked_fill(~valid, 0.0)


def linear_head_statement(t2i, t2t, w0, b0, w1, b1, lam=None):
    """fp64 statement of csrc/rank.hip linear_head_kernel: out = b1 + sum_h w1[h] relu(w0[h, 0] t2i + w0[h, 1] t2t + b0[h]) for every
    element of the two equally shaped fp32 tensors (w0 [hidden, 2], b0 / w1 [hidden], b1 passed as fp32).  Returns (out, extra) in
    the inputs' shape.  A unit is two FMAs on b0[h]: at most 2 u (|w0 t2i| + |w0 t2t| + |b0|), the worst case (two terms need no
    statistics); ReLU does not grow it.  The output is a chain of `hidden` FMAs on b1 in ascending h: _chain(hidden, |b1| +
    sum |w1| relu(.)), plus the units' errors through |w1| in quadrature.  The last FMA's rounding is the half ulp of
    check_budget(fmt="fp32").  Evaluated in row blocks of at most 2^24 / hidden elements.
    lambda is SHORT_CHAIN_LAMBDA = 4 here and in gate_rows_emulation, not FUSION_LAMBDA: where the chain is a handful of steps the final
    rounding's half ulp is most of the error, and a stand-in can only stay at a quarter of (half an ulp + extra) if extra is at least
    1.5 ulp.  The FMA-exact CPU stand-ins of tests/test_rounding_budget.py read up to 0.35 (linear, hidden = 1) and 0.45 (gate, cols =
    1) at lambda = 1, 0.27 and 0.45 at 2, 0.17 and 0.15 at 4: the next power of two that meets 0.25 on every case.  The kernels on an MI355X read at
    most 0.24 (linear head) and 0.14 (gate); 1 / (1 + expf(-s)) on exact integer s lies within 0.92 fp32 ulp of the fp64 value."""
    shape = t2i.shape
    a, b = t2i.double().cpu().reshape(-1, 1), t2t.double().cpu().reshape(-1, 1)
    w0, b0, w1 = w0.double().cpu().reshape(-1, 2), b0.double().cpu().reshape(-1), w1.double().cpu().reshape(-1)
    b1 = _f32_scale(b1)
    hidden = w0.shape[0]
    step = max(1, (1 << 24) // hidden)
    outs, extras = [], []
    for s in range(0, a.shape[0], step):
        x, y = a[s:s + step] * w0[:, 0], b[s:s + step] * w0[:, 1]
        t = (x + y + b0).clamp_min(0)
        dt = 2 * U32 * (x.abs() + y.abs() + b0.abs())
        outs.append(t @ w1 + b1)
        extras.append(torch.sqrt((dt * dt) @ (w1 * w1)) + _chain(hidden, t @ w1.abs() + abs(b1), SHORT_CHAIN_LAMBDA if lam is None else lam))
    return torch.cat(outs).reshape(shape), torch.cat(extras).reshape(shape)


def gate_rows_emulation(x, pre, w, bias, relu, lam=None, c_exp=None):
    """fp64 statement of csrc/rank.hip gate_rows_kernel: out[r] = sigmoid(sum_c act(x[r, c] + pre[c]) w[c] + bias), act = ReLU when
    relu else the identity; x fp32 [rows, cols], pre [cols] or None, w [cols], bias passed as fp32.  Returns (out, extra) [rows].
    The kernel adds pre in fp32 (u |v|, nothing without pre), sums ceil(cols / 64) FMAs per lane, 6 butterfly adds over the wave
    and the add of the bias: _chain(ceil(cols / 64) + 7, sum |v w| + |bias|), plus the errors of v through |w| in quadrature; that
    is ds.  out = 1 / (1 + expf(-s)): the sigmoid's slope out (1 - out) carries ds and expf's EXP_ULPS ulp (2 u EXP_ULPS relative on
    exp(-s), i.e. out (1 - out) times that); the add and the division round once each, lambda 2 u out.  2^-126 absolute covers an
    exponential that overflows (s < -88: out is 0, never NaN) where the exact value is below every normal number.
    lambda is SHORT_CHAIN_LAMBDA (linear_head_statement), on the two output roundings as well: for out in [0.5, 1) one ulp IS u, so
    the add's u and the division's half ulp alone read 0.6 of a budget of half an ulp + 2 u (measured: 0.45 at cols = 1)."""
    x64, w64 = x.double().cpu(), w.double().cpu().reshape(-1)
    v = x64 if pre is None else x64 + pre.double().cpu().reshape(-1)
    dv = torch.zeros_like(v) if pre is None else U32 * v.abs()
    if relu:
        v = v.clamp_min(0)
    bias = _f32_scale(bias)
    s = v @ w64 + bias
    lam = SHORT_CHAIN_LAMBDA if lam is None else lam
    ds = torch.sqrt((dv * dv) @ (w64 * w64)) + _chain((x.shape[1] + 63) // 64 + 7, v.abs() @ w64.abs() + abs(bias), lam)
    out = torch.sigmoid(s)
    slope = out * torch.sigmoid(-s)
    c = EXP_ULPS if c_exp is None else c_exp
    return out, slope * (ds + 2 * U32 * c) + lam * 2 * U32 * out + _TINY
