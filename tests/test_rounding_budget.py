"""CPU: the rounding-budget bars of the GPU numerics tests can fail.  A stand-in "kernel" (torch fp32 on the CPU, rounded to
bf16 like the HIP epilogues) passes them; the same kernel with one planted defect -- truncation instead of round-to-nearest-even,
a scale a fraction of an ulp off, a dropped K-tile, the bias added twice, a wrong QuickGELU constant, a dropped key, a masked
causal diagonal -- fails the elementwise bar, the bias bar or both.  The bars and their `extra` terms are the ones
tests/test_numerics_gpu.py applies to the kernels.

The same for the kernels tests/test_numerics_paths_gpu.py holds to their budgets:
* streaming attention (T > 288, 64-key chunks): pad keys scored 0 instead of -inf, no rescale when the max moves, the one-key
  last chunk dropped, outputs x1.005, one chunk's P rounded against the stale max; and the chunked statement against the
  single-pass one (they differ by more than the budget in most outputs at T = 577);
* pooled-row attention: the pooled row's own key dropped, the first key row off by one;
* pooling tail: LayerNorm eps 1e-6, variance over width - 1, one projection row dropped, delta2 ignored, outputs x(1 + 2^-20);
  its L2 step: outputs x(1 + 2^-20), the norm of d - 1 columns."""
import pytest
import torch

from oracle import rounding as R

MAX_BIAS = 0.02           # ulp: |signed bias| bar of every bf16 output
KAPPA = 8                 # accumulator bar: |acc - ref64| <= KAPPA 2^-24 sum|a||w|, as in tests/test_numerics_gpu.py


def _trunc_bf16(x32):
    return (x32.contiguous().view(torch.int32) & ~0xffff).view(torch.float32)


def _passes(got, ref64, extra, rounding_only=False):
    ratio = R.budget_ratio(got, ref64, extra)
    top = float(torch.nan_to_num(ratio, nan=float("inf")).max())
    bias = R.signed_bias_ulps(got, ref64, extra=extra if rounding_only else None)
    return top <= 1.0 and abs(bias) <= MAX_BIAS, top, bias


# ------------------------------------------------------------------------------------------------ helpers themselves
def test_rne_matches_torch_casts_and_saturates():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(200000, generator=g, dtype=torch.float64) * 50
    x32 = x.float().double()                        # fp32 inputs: torch's fp32 -> bf16 / e4m3 casts are single roundings
    assert torch.equal(R.rne_bf16(x32), x32.float().to(torch.bfloat16).double())
    assert torch.equal(R.rne_e4m3(x32 / 8), (x32 / 8).float().to(torch.float8_e4m3fn).double())
    assert torch.equal(R.rne_e4m3(torch.tensor([500.0, -1e6, 449.0])), torch.tensor([448.0, -448.0, 448.0], dtype=torch.float64))
    # ties go to even; one rounding from fp64 (1 + 2^-8 + 2^-40 rounds up, not to the tie's even neighbour 1)
    t = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -40], dtype=torch.float64)
    assert torch.equal(R.rne_bf16(t), torch.tensor([1.0, 1 + 2 * 2.0 ** -7, 1 + 2.0 ** -7], dtype=torch.float64))
    assert R.rne_f32(torch.tensor([1 + 2.0 ** -24], dtype=torch.float64)).item() == 1.0


def test_ulp_formats():
    one = torch.tensor([1.0, -3.0, 0.0, 2.0 ** -130], dtype=torch.float64)
    assert R.ulp(one, "bf16").tolist() == [2.0 ** -7, 2.0 ** -6, 2.0 ** -133, 2.0 ** -133]
    assert R.ulp(one, "fp32").tolist() == [2.0 ** -23, 2.0 ** -22, 2.0 ** -149, 2.0 ** -149]
    assert R.ulp(torch.tensor([1.0, 448.0, 2.0 ** -8], dtype=torch.float64), "e4m3").tolist() == [2.0 ** -3, 32.0, 2.0 ** -9]


def test_check_budget_names_the_worst_element():
    ref = torch.tensor([[1.0, 2.0], [3.0, 4.0]], dtype=torch.float64)
    got = ref.clone()
    got[1, 0] = 3.0 + 2.0 ** -5
    with pytest.raises(AssertionError, match=r"row 1 col 0: got 3.03125 ref 3.0 ratio"):
        R.check_budget(got, ref, what="planted")


# ------------------------------------------------------------------------------------------------ GEMM epilogues
@pytest.fixture(scope="module")
def gemm_case():
    g = torch.Generator().manual_seed(1)
    m, n, k = 1024, 512, 1024
    a = torch.randn(m, k, generator=g).to(torch.bfloat16).float()
    w = (torch.randn(n, k, generator=g) * k ** -0.5).to(torch.bfloat16).float()
    bias = torch.randn(n, generator=g)
    ref64 = a.double() @ w.double().T + bias.double()
    absum = a.abs().double() @ w.abs().double().T + bias.abs().double()
    return a, w, bias, ref64, absum


def _acc(a, w, bias, k_used=None):
    k = a.shape[1] if k_used is None else k_used
    return a[:, :k] @ w[:, :k].T + bias                     # fp32, the "kernel" accumulator


def _gemm_extra(absum):
    return KAPPA * 2.0 ** -24 * absum


def test_gemm_bars_pass_correct_rne(gemm_case):
    a, w, bias, ref64, absum = gemm_case
    acc = _acc(a, w, bias)
    assert float(((acc.double() - ref64).abs() / (2.0 ** -24 * absum)).max()) <= KAPPA      # the accumulator bar itself
    ok, top, bias_u = _passes(acc.to(torch.bfloat16), ref64, _gemm_extra(absum))
    assert ok, (top, bias_u)


@pytest.mark.parametrize("defect", ["truncate", "scale_2^-9", "scale_1%", "drop_last_ktile", "bias_twice"])
def test_gemm_bars_catch_planted_defects(gemm_case, defect):
    a, w, bias, ref64, absum = gemm_case
    acc = _acc(a, w, bias)
    if defect == "truncate":
        got = _trunc_bf16(acc)
    elif defect == "scale_2^-9":
        got = (acc * (1 + 2.0 ** -9)).to(torch.bfloat16)
    elif defect == "scale_1%":
        got = (acc * 1.01).to(torch.bfloat16)
    elif defect == "drop_last_ktile":
        got = _acc(a, w, bias, a.shape[1] - 64).to(torch.bfloat16)
    else:
        got = (acc + bias).to(torch.bfloat16)
    ok, top, bias_u = _passes(got, ref64, _gemm_extra(absum))
    assert not ok, (defect, top, bias_u)


def _qgelu64(x):
    return x * torch.sigmoid(1.702 * x)


def _qgelu_extra(acc64):
    # the fp32 QuickGELU of the kernel (exp2 + a 1-ulp rcp) around an exact accumulator: a few fp32 ulp of the result,
    # growing with the exponent's argument
    return 2.0 ** -24 * _qgelu64(acc64).abs() * (8 + 4 * (1.702 * acc64).abs())


@pytest.mark.parametrize("const,ok_expected", [(1.702, True), (1.7, False)])
def test_qgelu_bars(gemm_case, const, ok_expected):
    a, w, bias, _, _ = gemm_case
    acc = _acc(a, w, bias)                                   # the reference starts from the kernel's own accumulator
    acc64 = acc.double()
    got = (acc * torch.sigmoid(const * acc)).to(torch.bfloat16)
    ok, top, bias_u = _passes(got, _qgelu64(acc64), _qgelu_extra(acc64))
    assert ok == ok_expected, (const, top, bias_u)


# ------------------------------------------------------------------------------------------------ attention
def _attention_kernel_cpu(qkv_bf16, batch, t, width, causal, defect=None):
    heads = width // 64
    x = qkv_bf16.float().view(batch, t, 3, heads, 64).permute(2, 0, 3, 1, 4)
    q, k, v = x[0], x[1], x[2]
    s = q @ k.transpose(-1, -2)
    mask = torch.zeros(t, t, dtype=torch.bool)
    if causal:
        mask |= torch.ones(t, t, dtype=torch.bool).triu_(1)
    if defect == "diag_masked":
        mask |= torch.eye(t, dtype=torch.bool)
    if defect == "drop_last_key":
        mask[:, t - 1] = True
    s = s.masked_fill(mask, float("-inf"))
    p = torch.exp(s - s.amax(-1, keepdim=True))
    l = p.sum(-1, keepdim=True)
    o = (p.to(torch.bfloat16).float() @ v) / l
    if defect == "scale_1.005":
        o = o * 1.005
    return o.permute(0, 2, 1, 3).reshape(batch * t, width).to(torch.bfloat16)


@pytest.mark.parametrize("defect,causal", [(None, False), (None, True), ("drop_last_key", False), ("diag_masked", True),
                                           ("scale_1.005", False)])
def test_attention_bars(defect, causal):
    batch, t, width = 3, 257, 256
    g = torch.Generator().manual_seed(7)
    qkv = torch.randn(batch * t, 3 * width, generator=g)
    qkv[:, :width] *= 0.25
    qkv_bf = qkv.to(torch.bfloat16)
    ref, extra = R.attention_emulation(qkv_bf, batch, t, width, causal)
    got = _attention_kernel_cpu(qkv_bf, batch, t, width, causal, defect)
    ok, top, bias_u = _passes(got, ref, extra)
    assert ok == (defect is None), (defect, causal, top, bias_u)


# ------------------------------------------------------------------------------------------------ streaming attention (T > 288)
def _long_case(t, batch=3, width=256, seed=17):
    g = torch.Generator().manual_seed(seed + t)
    qkv = torch.randn(batch * t, 3 * width, generator=g)
    qkv[:, :width] *= 0.25                        # pre-scaled queries: logits of a few units
    return qkv.to(torch.bfloat16)


def _long_kernel_cpu(qkv_bf16, batch, t, width, kc=64, defect=None):
    """csrc/attention_stream.hip in fp32 on the CPU: K / V in chunks of kc keys, running max m and sum l, O and l rescaled by
    exp(m - m') when the max moves, P rounded to bf16 against the running max, the sum from the unrounded P."""
    heads = width // 64
    x = qkv_bf16.float().view(batch, t, 3, heads, 64).permute(2, 0, 3, 1, 4)
    q, k, v = x[0], x[1], x[2]
    n = (t + kc - 1) // kc
    if defect == "pad_keys_scored_0":             # the ragged chunk's zero-filled pad keys left unmasked: score 0, V 0
        pad = torch.zeros(k.shape[:-2] + (n * kc - t, 64))
        k, v = torch.cat([k, pad], -2), torch.cat([v, pad], -2)
    m = torch.full(q.shape[:-1] + (1,), float("-inf"))
    l = torch.zeros_like(m)
    o = torch.zeros_like(q)
    for c in range(n):
        if defect == "drop_last_ragged_chunk" and c == n - 1:
            continue
        kk, vv = k[..., c * kc:(c + 1) * kc, :], v[..., c * kc:(c + 1) * kc, :]
        s = q @ kk.transpose(-1, -2)
        mnew = torch.maximum(m, s.amax(-1, keepdim=True))
        alpha = torch.ones_like(m) if defect == "no_rescale" else torch.exp(m - mnew)
        p = torch.exp(s - mnew)
        if defect == "stale_max_chunk1" and c == 1:        # chunk 1's P rounded against the max before it, then rescaled
            pb = torch.exp(s - m).to(torch.bfloat16).float() * torch.exp(m - mnew)
        else:
            pb = p.to(torch.bfloat16).float()
        l = l * alpha + p.sum(-1, keepdim=True)
        o = o * alpha + pb @ vv
        m = mnew
    o = o / l
    if defect == "scale_1.005":
        o = o * 1.005
    return o.permute(0, 2, 1, 3).reshape(batch * t, width).to(torch.bfloat16)


@pytest.mark.parametrize("t", [289, 385, 577, 1025])
def test_long_attention_bars_pass_the_streaming_kernel(t):
    batch, width = 3, 256
    qkv = _long_case(t, batch, width)
    ref, extra = R.attention_long_emulation(qkv, batch, t, width)
    ok, top, bias_u = _passes(_long_kernel_cpu(qkv, batch, t, width), ref, extra, rounding_only=True)
    assert ok, (t, top, bias_u)


@pytest.mark.parametrize("defect", ["pad_keys_scored_0", "no_rescale", "drop_last_ragged_chunk", "scale_1.005", "stale_max_chunk1"])
def test_long_attention_bars_catch_planted_defects(defect):
    batch, t, width = 3, 577, 256                 # 577 = 9 x 64 + 1: the last chunk holds one key and 63 pad keys
    qkv = _long_case(t, batch, width)
    ref, extra = R.attention_long_emulation(qkv, batch, t, width)
    ok, top, bias_u = _passes(_long_kernel_cpu(qkv, batch, t, width, defect=defect), ref, extra, rounding_only=True)
    assert not ok, (defect, top, bias_u)


def test_chunked_and_single_pass_statements_differ_at_577():
    """The streaming kernel rounds P against the running max, the tile kernel against the final one: at T = 577 the two fp64
    statements differ by more than the chunked statement's extra in most outputs (76 % here), so the correct streaming stand-in,
    held to the single-pass O with that extra, fails by two orders of magnitude -- the chunked statement is what makes the bar tight."""
    batch, t, width = 3, 577, 256
    qkv = _long_case(t, batch, width)
    got = _long_kernel_cpu(qkv, batch, t, width)
    ref1, _ = R.attention_emulation(qkv, batch, t, width, False)
    refc, extra = R.attention_long_emulation(qkv, batch, t, width)
    frac = float(((refc - ref1).abs() > extra).double().mean())
    assert frac > 0.5, frac
    top = float(R.budget_ratio(got, ref1, extra).max())
    assert top > 10.0, top


def test_long_emulation_kc_is_the_chunk_size():
    """One chunk holding every key is the single-pass statement: the same O as attention_emulation."""
    batch, t, width = 2, 289, 128
    qkv = _long_case(t, batch, width)
    o1, _ = R.attention_emulation(qkv, batch, t, width, False)
    oc, _ = R.attention_long_emulation(qkv, batch, t, width, kc=320)
    assert torch.allclose(o1, oc, rtol=1e-13, atol=0)


# ------------------------------------------------------------------------------------------------ pooled-row attention
def _pooled_kernel_cpu(q_bf16, qkv_bf16, r0, nk, width, defect=None):
    heads = width // 64
    out = torch.empty(len(r0), width)
    for b in range(len(r0)):
        a, n = int(r0[b]), int(nk[b])
        if defect == "r0_off_by_one" and a > 0:             # keys r0 - 1 .. r0 + nk - 2: the previous item's last row in, the pooled row out
            a -= 1
        if defect == "drop_pooled_key":
            n = max(n - 1, 1)
        kv = qkv_bf16[a:a + n].float()
        k = kv[:, width:2 * width].view(n, heads, 64).transpose(0, 1)
        v = kv[:, 2 * width:].view(n, heads, 64).transpose(0, 1)
        qh = q_bf16[b].float().view(heads, 1, 64)
        s = qh @ k.transpose(-1, -2)
        p = torch.exp(s - s.amax(-1, keepdim=True))
        out[b] = ((p.to(torch.bfloat16).float() @ v) / p.sum(-1, keepdim=True)).reshape(width)
    return out.to(torch.bfloat16)


def _pooled_case(width=256, lens=(9, 64, 65, 77, 40, 77, 33, 77)):
    """Text form: packed items, each pooled at its last row (the end-of-text token), q of the pooled rows."""
    g = torch.Generator().manual_seed(23)
    lens = torch.tensor(lens)
    row_start = torch.cat([torch.zeros(1, dtype=torch.int64), lens.cumsum(0)]).int()
    qkv = torch.randn(int(lens.sum()), 3 * width, generator=g).to(torch.bfloat16)
    q = (torch.randn(len(lens), width, generator=g) * 0.25).to(torch.bfloat16)
    pool_idx = (row_start[1:] - 1).int()
    return q, qkv, pool_idx, row_start


@pytest.mark.parametrize("defect", [None, "drop_pooled_key", "r0_off_by_one"])
def test_pooled_row_bars(defect):
    width = 256
    q, qkv, pool_idx, row_start = _pooled_case(width)
    items = len(pool_idx)
    ref, extra = R.attention_pooled_emulation(q, qkv, pool_idx, row_start, items, 77, width, True, 320)
    r0, nk = R.pooled_keys(pool_idx, row_start, items, 77, True, 320)
    got = _pooled_kernel_cpu(q, qkv, r0, nk, width, defect)
    ok, top, bias_u = _passes(got, ref, extra, rounding_only=True)
    assert ok == (defect is None), (defect, top, bias_u)


def test_pooled_keys_clamp():
    row_start = torch.tensor([0, 5, 300, 700], dtype=torch.int32)
    pool_idx = torch.tensor([-3, 5, 650], dtype=torch.int32)           # before its first row / its first row / 351 keys
    r0, nk = R.pooled_keys(pool_idx, row_start, 3, 77, True, 320)
    assert r0.tolist() == [0, 5, 300] and nk.tolist() == [1, 1, 320]
    r0, nk = R.pooled_keys(None, None, 3, 577, False, 1088)
    assert r0.tolist() == [0, 577, 1154] and nk.tolist() == [577] * 3


# ------------------------------------------------------------------------------------------------ pooling tail
TAIL_KAPPA = 1             # as tests/test_numerics_paths_gpu.py
LN_F32_FACTOR = 2.0 ** -21
TAIL_MAX_REL_BIAS = 4      # units of 2^-24 (rounding.relative_bias), as tests/test_numerics_paths_gpu.py


@pytest.fixture(scope="module")
def tail_case():
    g = torch.Generator().manual_seed(31)
    batch, width, d = 32, 768, 512
    x = torch.randn(batch, width, generator=g) + 0.5
    d1 = (torch.randn(batch, width, generator=g) * 0.5).to(torch.bfloat16).float()
    d2 = (torch.randn(batch, width, generator=g) * 0.5).to(torch.bfloat16).float()
    gamma = 1 + 0.1 * torch.randn(width, generator=g)
    beta = 0.1 * torch.randn(width, generator=g)
    proj = torch.randn(width, d, generator=g) * width ** -0.5
    return x, d1, d2, gamma, beta, proj


def _tail_kernel_cpu(xs, gamma, beta, proj, defect=None):
    width = xs.shape[1]
    mean = xs.sum(-1, keepdim=True) / width
    c = xs - mean
    var = (c * c).sum(-1, keepdim=True) / (width - 1 if defect == "var_over_w-1" else width)
    rstd = 1.0 / torch.sqrt(var + (1e-6 if defect == "eps_1e-6" else 1e-5))
    y = c * rstd * gamma + beta
    if defect == "drop_proj_row":
        y[:, 100] = 0.0
    out = y @ proj
    return out * (1 + 2.0 ** -20) if defect == "scale_2^-20" else out


def _tail_passes(got, ref, extra):
    top = float(torch.nan_to_num(R.budget_ratio(got, ref, extra, "fp32"), nan=float("inf")).max())
    bias = R.relative_bias(got, ref)
    return top <= 1.0 and abs(bias) <= TAIL_MAX_REL_BIAS, top, bias


@pytest.mark.parametrize("defect", [None, "eps_1e-6", "var_over_w-1", "drop_proj_row", "delta2_ignored", "scale_2^-20"])
def test_tail_bars(tail_case, defect):
    x, d1, d2, gamma, beta, proj = tail_case
    xs = (x + d1) + d2
    ref, extra = R.tail_emulation(xs, gamma, beta, proj, TAIL_KAPPA, LN_F32_FACTOR)
    got = _tail_kernel_cpu(x + d1 if defect == "delta2_ignored" else xs, gamma, beta, proj, defect)
    ok, top, bias = _tail_passes(got, ref, extra)
    assert ok == (defect is None), (defect, top, bias)


@pytest.mark.parametrize("defect", [None, "scale_2^-20", "norm_of_d-1_columns"])
def test_l2norm_bars(tail_case, defect):
    x, d1, d2, gamma, beta, proj = tail_case
    r = _tail_kernel_cpu((x + d1) + d2, gamma, beta, proj)
    ref, extra = R.l2norm_emulation(r)
    s = (r[:, :-1] * r[:, :-1]).sum(-1, keepdim=True) if defect == "norm_of_d-1_columns" else (r * r).sum(-1, keepdim=True)
    got = r * (1.0 / torch.sqrt(s))
    if defect == "scale_2^-20":
        got = got * (1 + 2.0 ** -20)
    ok, top, bias = _tail_passes(got, ref, extra)
    assert ok == (defect is None), (defect, top, bias)


# ------------------------------------------------------------------------------------------------ vision token front
FRONT_KAPPA = 8                # as tests/test_numerics_front_gpu.py: the GEMM accumulator bar
FRONT_MAX_REL_BIAS = 4         # units of 2^-24 (rounding.relative_bias), the tail's bar


@pytest.fixture(scope="module")
def patch_case():
    g = torch.Generator().manual_seed(41)
    b, s, p, width = 3, 56, 14, 256            # kv = 588: 52 K-pad columns, as ViT-L/14
    px = torch.randn(b, 3, s, s, generator=g)
    w = torch.randn(width, 3, p, p, generator=g) * (3 * p * p) ** -0.5
    cls = torch.randn(width, generator=g) * 0.1
    pos = torch.randn((s // p) ** 2 + 1, width, generator=g) * 0.1
    return px, w, cls, pos, p


def _patch_kernel_cpu(px, w, cls, pos, patch, defect=None):
    """The token front in fp32 on the CPU: im2col (pixels rounded to bf16, k = c p^2 + dy p + dx, zero up to kpad) times the bf16
    weights, + pos[1 + patch] in fp32 (the EPI_PATCH_F32 epilogue); class rows cls + pos[0]."""
    b, _, s, _ = px.shape
    width, gr = w.shape[0], s // patch
    kv = 3 * patch * patch
    kpad = (kv + 63) // 64 * 64
    x = _trunc_bf16(px) if defect == "truncate_pixels" else px.to(torch.bfloat16).float()
    x = x.view(b, 3, gr, patch, gr, patch)                                   # b c py dy px dx
    x = x.permute(0, 2, 4, 1, 5, 3) if defect == "dy_dx_swapped" else x.permute(0, 2, 4, 1, 3, 5)
    pad = float("nan") if defect == "kpad_not_zero" else 0.0                 # what an unwritten pad of a NaN-filled workspace holds
    a = torch.nn.functional.pad(x.reshape(b * gr * gr, kv), (0, kpad - kv), value=pad)
    wk = torch.nn.functional.pad(w.to(torch.bfloat16).float().reshape(width, kv), (0, kpad - kv))
    pi = torch.arange(gr * gr).repeat(b)
    tokens = (a @ wk.T + pos[pi if defect == "pos_pi" else pi + 1]).view(b, gr * gr, width)
    row0 = cls if defect == "cls_without_pos0" else cls + pos[0]
    return torch.cat([row0.expand(b, 1, width), tokens], 1).reshape(-1, width)


def _front_failures(got, ref, extra, tokens):
    """The checks tests/test_numerics_front_gpu.py applies to the vision rows, by name: class_rows (bit for bit), ratio (budget ratio
    <= 1 in fp32 ulps), bias (|relative bias| <= FRONT_MAX_REL_BIAS)."""
    failed = []
    cls_rows = torch.arange(0, got.shape[0], tokens)
    if not torch.equal(got[cls_rows].double(), ref[cls_rows].double()):
        failed.append("class_rows")
    if float(torch.nan_to_num(R.budget_ratio(got, ref, extra, "fp32"), nan=float("inf")).max()) > 1.0:
        failed.append("ratio")
    if not abs(R.relative_bias(got, ref)) <= FRONT_MAX_REL_BIAS:
        failed.append("bias")
    return failed


def test_patch_front_bars_pass_the_stand_in(patch_case):
    px, w, cls, pos, p = patch_case
    ref, extra = R.patch_tokens_emulation(px, w, cls, pos, p, FRONT_KAPPA)
    got = _patch_kernel_cpu(px, w, cls, pos, p)
    assert _front_failures(got, ref, extra, pos.shape[0]) == []
    kappa = float(((got - ref).abs() / (extra / FRONT_KAPPA)).nan_to_num(0.0, 0.0, 0.0).max())     # the accumulator bar itself
    assert kappa <= FRONT_KAPPA, kappa


@pytest.mark.parametrize("defect,check", [("truncate_pixels", "ratio"), ("dy_dx_swapped", "ratio"), ("pos_pi", "ratio"),
                                          ("cls_without_pos0", "class_rows"), ("kpad_not_zero", "ratio")])
def test_patch_front_bars_catch_planted_defects(patch_case, defect, check):
    px, w, cls, pos, p = patch_case
    ref, extra = R.patch_tokens_emulation(px, w, cls, pos, p, FRONT_KAPPA)
    failed = _front_failures(_patch_kernel_cpu(px, w, cls, pos, p, defect), ref, extra, pos.shape[0])
    assert check in failed, (defect, failed)


# ------------------------------------------------------------------------------------------------ text token front
@pytest.fixture(scope="module")
def text_case():
    """Ids outside 0 .. vocab - 1, lengths 0, negative, > ctx and exact; the first 8 columns of tok / pos hold bf16 ties of both
    parities (tok = (m + 1/2) 2^-7 in [1, 2), pos = 0): the RNE bar."""
    g = torch.Generator().manual_seed(43)
    vocab, ctx, width, batch = 64, 16, 32, 40
    tok = torch.randn(vocab, width, generator=g)
    pos = torch.randn(ctx, width, generator=g) * 0.1
    tok[:, :8] = (torch.randint(128, 256, (vocab, 8), generator=g).float() + 0.5) * 2.0 ** -7
    pos[:, :8] = 0.0
    ids = torch.randint(-5, vocab + 5, (batch, ctx), generator=g, dtype=torch.int32)
    lens = torch.randint(-3, ctx + 4, (batch,), generator=g, dtype=torch.int32)
    lens[:4] = torch.tensor([0, -2, ctx + 3, ctx])
    return ids, lens, tok, pos, vocab, ctx


def _text_kernel_cpu(ids, lens, rows, tok, pos, vocab, ctx, defect=None):
    """row_starts_kernel and text_embed_kernel sequentially on the CPU (fp32 rows)."""
    batch = ids.shape[0]
    if lens is None:
        r = torch.arange(batch * ctx)
        text, t, rs = r // ctx, r % ctx, None
    else:
        lo = 0 if defect == "len_clamp_0" else 1
        run, starts = 0, [0]
        for i in range(batch):
            run += min(max(int(lens[i]), lo), ctx)
            cap = rows - (batch - (i + 1)) - (1 if defect == "cap_off_by_one" else 0)
            starts.append(min(run, cap))
        rs = torch.tensor(starts, dtype=torch.int32)
        r = torch.arange(rows)
        text = torch.searchsorted(rs[:batch].long(), r, right=True) - 1
        t = (r - rs.long()[text]).clamp_max(ctx - 1)
    idx = ids.long()[text, t]
    idx = idx % vocab if defect == "unclamped_ids" else idx.clamp(0, vocab - 1)      # an unclamped id reads some other row
    tp = (t + 1).clamp_max(ctx - 1) if defect == "pos_t+1" else t
    return tok[idx] + pos[tp], rs


def _half_up_bf16(x32):
    return ((x32.contiguous().view(torch.int32) + 0x8000) & ~0xffff).view(torch.float32)


def _text_failures(got_rows, got_rs, want_rows, want_rs):
    """The checks of tests/test_numerics_front_gpu.py, by name: row_start and rows, both bit for bit."""
    failed = []
    if want_rs is not None and not torch.equal(got_rs, want_rs):
        failed.append("row_start")
    if got_rows.shape != want_rows.shape or not torch.equal(got_rows.view(torch.int16), want_rows.view(torch.int16)):
        failed.append("rows")
    return failed


@pytest.mark.parametrize("layout", ["unpacked", "packed_exact", "packed_more_rows", "packed_capped"])
def test_text_front_statement_passes_the_stand_in(text_case, layout):
    ids, lens, tok, pos, vocab, ctx = text_case
    total = int(lens.clamp(1, ctx).sum())
    rows = {"unpacked": 0, "packed_exact": total, "packed_more_rows": total + 37, "packed_capped": total - 29}[layout]
    ln = None if layout == "unpacked" else lens
    want, want_rs = R.text_tokens_statement(ids, ln, rows, tok, pos, vocab, ctx)
    got, got_rs = _text_kernel_cpu(ids, ln, rows, tok, pos, vocab, ctx)
    assert _text_failures(got, got_rs, want, want_rs) == []
    assert _text_failures(got.to(torch.bfloat16), got_rs, want.to(torch.bfloat16), want_rs) == []
    if ln is not None:
        assert int(want_rs[-1]) == min(rows, total) and bool((want_rs[1:] > want_rs[:-1]).all())     # every text keeps a row


@pytest.mark.parametrize("defect,check", [("pos_t+1", "rows"), ("unclamped_ids", "rows"), ("bf16_half_up", "rows"),
                                          ("len_clamp_0", "row_start"), ("cap_off_by_one", "row_start")])
def test_text_front_statement_catches_planted_defects(text_case, defect, check):
    ids, lens, tok, pos, vocab, ctx = text_case
    rows = int(lens.clamp(1, ctx).sum()) - 29                  # the caps bind for the last texts
    want, want_rs = R.text_tokens_statement(ids, lens, rows, tok, pos, vocab, ctx)
    got, got_rs = _text_kernel_cpu(ids, lens, rows, tok, pos, vocab, ctx, defect)
    want = want.to(torch.bfloat16)
    got = _half_up_bf16(got).to(torch.bfloat16) if defect == "bf16_half_up" else got.to(torch.bfloat16)
    failed = _text_failures(got, got_rs, want, want_rs)
    assert check in failed, (defect, failed)


# ------------------------------------------------------------------------------------------------ similarity panels
def _panel_kernel_cpu(parts, part_scale, row_scale, terms, side, defect=None):
    """panel_build_kernel in fp32 on the CPU (torch's fp32 -> bf16 cast is RNE)."""
    rows, d = parts[0].shape
    dpad = (d + 63) // 64 * 64
    out = torch.zeros((rows + 255) // 256 * 256, len(parts) * terms * dpad, dtype=torch.bfloat16)
    if defect == "nonzero_pad_rows":
        out[rows:] = 1.0
    for p, src in enumerate(parts):
        ps = torch.tensor(part_scale[p], dtype=torch.float32)
        sc = torch.full((rows, 1), 1.0 if defect == "part_scale_after_rounding" else float(ps))
        if row_scale[p] is not None and defect != "row_scale_ignored":
            sc = sc * row_scale[p].reshape(rows, 1)
        v = src * sc
        hi = _trunc_bf16(v).to(torch.bfloat16) if defect == "truncate_hi" else v.to(torch.bfloat16)
        lo = (v - hi.float()).to(torch.bfloat16)
        if defect == "part_scale_after_rounding":
            hi, lo = (hi.float() * ps).to(torch.bfloat16), (lo.float() * ps).to(torch.bfloat16)
        if defect == "lo_dropped" and side == 0:
            lo = torch.zeros_like(lo)
        query = (side == 0) != (defect == "layouts_swapped")
        segs = [hi] if terms == 1 else ([hi, lo, hi] if query else [hi, hi, lo])
        for s, x in enumerate(segs):
            c0 = (p * terms + s) * dpad
            out[:rows, c0:c0 + d] = x
    return out


def _panel_diff(got, want, rows, d, terms, nparts):
    """Names of the regions whose bits differ: 'p{part}s{segment}' (valid rows and columns), 'pad_cols', 'pad_rows'."""
    gb, wb = got.view(torch.int16), want.view(torch.int16)
    dpad = (d + 63) // 64 * 64
    names = [] if torch.equal(gb[rows:], wb[rows:]) else ["pad_rows"]
    for p in range(nparts):
        for s in range(terms):
            c0 = (p * terms + s) * dpad
            if not torch.equal(gb[:rows, c0:c0 + d], wb[:rows, c0:c0 + d]):
                names.append(f"p{p}s{s}")
            if not torch.equal(gb[:rows, c0 + d:c0 + dpad], wb[:rows, c0 + d:c0 + dpad]) and "pad_cols" not in names:
                names.append("pad_cols")
    return names


@pytest.fixture(scope="module")
def panel_case():
    """Two parts of [100, 65]: part 0 scaled by 0.7 (not a power of two), part 1 by a row scale."""
    g = torch.Generator().manual_seed(47)
    rows, d = 100, 65
    parts = [torch.randn(rows, d, generator=g), torch.randn(rows, d, generator=g) * 3]
    return parts, [0.7, 1.0], [None, torch.rand(rows, generator=g) + 0.5], rows, d


@pytest.mark.parametrize("terms,side", [(1, 0), (3, 0), (3, 1)])
def test_panel_statement_is_the_stand_in(panel_case, terms, side):
    parts, ps, rs, rows, d = panel_case
    want = R.panel_statement(parts, ps, rs, terms, side)
    assert want.shape == (256, 2 * terms * 128) and want.dtype == torch.bfloat16
    assert _panel_diff(_panel_kernel_cpu(parts, ps, rs, terms, side), want, rows, d, terms, 2) == []


@pytest.mark.parametrize("defect,side,check", [("truncate_hi", 1, "p0s0"), ("lo_dropped", 0, "p0s1"), ("layouts_swapped", 0, "p0s1"),
                                               ("layouts_swapped", 1, "p1s2"), ("part_scale_after_rounding", 0, "p0s0"),
                                               ("row_scale_ignored", 1, "p1s0"), ("nonzero_pad_rows", 0, "pad_rows")])
def test_panel_statement_catches_planted_defects(panel_case, defect, side, check):
    parts, ps, rs, rows, d = panel_case
    want = R.panel_statement(parts, ps, rs, 3, side)
    names = _panel_diff(_panel_kernel_cpu(parts, ps, rs, 3, side, defect), want, rows, d, 3, 2)
    assert check in names, (defect, names)


def test_panel_statement_keeps_subnormals():
    """v = 1 + 2^-9 + 2^-17 scaled by 2^-120: hi = 2^-120, lo = 2^-129 + 2^-137 -- an fp32 subnormal, rounded to bf16's subnormal
    grid (2^-133) = 2^-129 exactly; and v = 3 2^-132 (itself an fp32 subnormal, on bf16's grid): hi = v, lo = 0."""
    src = torch.tensor([[1 + 2.0 ** -9 + 2.0 ** -17, 3 * 2.0 ** -12]], dtype=torch.float32)
    panel = R.panel_statement([src], [2.0 ** -120], None, 3, 1).double()
    assert panel[0, [0, 64, 128]].tolist() == [2.0 ** -120, 2.0 ** -120, 2.0 ** -129]
    assert panel[0, [1, 65, 129]].tolist() == [3 * 2.0 ** -132, 3 * 2.0 ** -132, 0.0]


# ------------------------------------------------------------------------------------------------ similarity scores
SIM_KAPPA = 10                 # as tests/test_numerics_sim_gpu.py
SIM_MAX_REL_BIAS = 4


@pytest.fixture(scope="module")
def scores_case():
    """Two parts x 3 terms (kdim 4608, the fused T2I + T2T width) of unit rows, the second part weighted 0.4."""
    g = torch.Generator().manual_seed(53)
    nq, ng, d = 200, 300, 768
    unit = lambda n: torch.nn.functional.normalize(torch.randn(n, d, generator=g), dim=-1)     # noqa: E731
    q, gi, gt = unit(nq), unit(ng), unit(ng)
    qp = R.panel_statement([q, q], [0.6, 0.4], None, 3, 0)
    gp = R.panel_statement([gi, gt], None, None, 3, 1)
    return q, gi, gt, qp, gp, nq, ng


def _score_failures(got, ref, extra):
    failed = []
    if float(torch.nan_to_num(R.budget_ratio(got, ref, extra, "fp32"), nan=float("inf")).max()) > 1.0:
        failed.append("ratio")
    if not abs(R.relative_bias(got, ref)) <= SIM_MAX_REL_BIAS:
        failed.append("bias")
    return failed


def _scores_cpu(qp, gp, nq, ng, defect=None):
    q, g = qp[:nq].float(), gp[:ng].float()
    if defect == "drop_last_ktile":
        q, g = q[:, :-64], g[:, :-64]
    if defect == "lo_hi_missing":                  # the query panel's lo segments zeroed: hi.hi + hi.lo only
        q = q.clone()
        q[:, 768:1536] = 0.0
        q[:, 3 * 768 + 768:3 * 768 + 1536] = 0.0
    s = q @ g.T
    return s * (1 + 2.0 ** -20) if defect == "scale_2^-20" else s


def test_scores_bars_pass_the_stand_in(scores_case):
    q, gi, gt, qp, gp, nq, ng = scores_case
    ref, extra = R.panel_scores_emulation(qp, gp, SIM_KAPPA, nq, ng)
    got = _scores_cpu(qp, gp, nq, ng)
    assert _score_failures(got, ref, extra) == []
    rep, bound = R.panel_representation_bound([q, q], [gi, gt], 3, q_part_scale=[0.6, 0.4])
    assert float(((got.double() - rep).abs() / (bound + extra)).max()) <= 1.0


@pytest.mark.parametrize("defect,check", [("scale_2^-20", "bias"), ("drop_last_ktile", "ratio"), ("lo_hi_missing", "ratio")])
def test_scores_bars_catch_planted_defects(scores_case, defect, check):
    q, gi, gt, qp, gp, nq, ng = scores_case
    ref, extra = R.panel_scores_emulation(qp, gp, SIM_KAPPA, nq, ng)
    failed = _score_failures(_scores_cpu(qp, gp, nq, ng, defect), ref, extra)
    assert check in failed, (defect, failed)


def test_representation_bound_is_tight_enough_to_matter(scores_case):
    """The bf16 panels (terms 1) of the same rows sit within their bound and break the terms-3 bound (worst 9.7 x it here): the
    terms-3 bound catches a panel whose lo terms are lost on both sides."""
    q, gi, gt, qp, gp, nq, ng = scores_case
    qp1 = R.panel_statement([q, q], [0.6, 0.4], None, 1, 0)
    gp1 = R.panel_statement([gi, gt], None, None, 1, 1)
    s1, extra1 = R.panel_scores_emulation(qp1, gp1, SIM_KAPPA, nq, ng)
    rep, b1 = R.panel_representation_bound([q, q], [gi, gt], 1, q_part_scale=[0.6, 0.4])
    _, b3 = R.panel_representation_bound([q, q], [gi, gt], 3, q_part_scale=[0.6, 0.4])
    err = (s1 - rep).abs()
    assert float((err / (b1 + extra1)).max()) <= 1.0
    assert float((err / (b3 + extra1)).max()) > 4.0


# ------------------------------------------------------------------------------------------------ learned fusion heads
HEAD_STAND_IN_BAR = 0.25       # the CPU stand-ins must leave a factor of four to the GPU's FMA contraction, exp, tanh and division
HEAD_DEFECT_SHARE = 0.02       # a planted defect must break the budget on at least this share of the outputs


def _head_ratio(got, ref, extra):
    """Budget ratio over the finite slots of the statement; padded slots (-inf) must be -inf in `got`."""
    pad = torch.isinf(ref)
    assert bool(torch.isinf(got.double()[pad]).all())
    return torch.nan_to_num(R.budget_ratio(got, ref, extra, "fp32")[~pad], nan=float("inf"))


def _head_check(name, defect, got, ref, extra):
    ratio = _head_ratio(got, ref, extra)
    top, share = float(ratio.max()), float((ratio > 1).double().mean())
    print(f"{name} defect={defect}: worst ratio {top:.4g}, share above 1: {share:.3f}")
    if defect is None:
        assert top <= HEAD_STAND_IN_BAR, (name, top)
    else:
        assert share >= HEAD_DEFECT_SHARE, (name, defect, top, share)
    return top


def _fma(a, b, c):
    """fmaf: the product of two fp32 values is exact in fp64, so one fp64 add and one rounding to fp32 is the fused result (up to
    a double rounding 2^-29 of an ulp away from a tie)."""
    return (a.double() * b.double() + c.double()).float()


def _mix_cpu(a, b, p_i, p_t, c0, w2t, b2, w3, b3, defect=None):
    """fp32 stand-in of the pair arithmetic in the kernels' order, FMA for FMA (torch's exp, tanh and division in place of the
    device's): a, b [B, R, H] scores, p_x [B, H, hid1] -> [B, R]."""
    heads, hid1, hid2 = a.shape[-1], w2t.shape[0], w2t.shape[1]
    mx = torch.maximum(a, b)
    ea, eb = torch.exp(a - mx), torch.exp(b - mx)
    inv = 1.0 / (ea + eb)
    wi, wt = ea * inv, eb * inv
    if defect == "weights_swapped_in_one_head":
        wi, wt = wi.clone(), wt.clone()
        wi[..., 3], wt[..., 3] = wt[..., 3].clone(), wi[..., 3].clone()
    hs = (torch.zeros_like(c0) if defect == "c0_dropped" else c0).expand(a.shape[0], a.shape[1], hid1)
    for h in range(heads):
        hs = _fma(wi[..., h, None], p_i[:, None, h, :], _fma(wt[..., h, None], p_t[:, None, h, :], hs))
    hs = hs.clamp_min(0)
    if defect == "last_hid1_unit_dropped":
        hs = hs.clone()
        hs[..., -1] = 0
    w2 = w2t.to(torch.bfloat16).float() if defect == "w2_bf16" else w2t
    acc = torch.zeros(a.shape[0], a.shape[1], hid2)
    for j in range(hid1):
        acc = _fma(hs[..., j, None], w2[j], acc)
    z = acc.clamp_min(0) + b2 if defect == "b2_after_relu" else (acc + b2).clamp_min(0)
    o = torch.full(a.shape[:2], b3, dtype=torch.float32)
    for k in range(hid2 - 1 if defect == "chain_stops_at_hid2-1" else hid2):
        o = _fma(z[..., k], w3[k], o)
    return torch.tanh(o) if defect == "tanh_without_half" else 0.5 * torch.tanh(o)


def _pairs_cpu(st_i, st_t, p_i, p_t, c0, w2t, b2, w3, b3, defect=None):
    return _mix_cpu(st_i.permute(1, 2, 0), st_t.permute(1, 2, 0), p_i, p_t, c0, w2t, b2, w3, b3, defect)


def _head_params(g, heads, n_c, hid1, hid2, scale):
    r = lambda *s: torch.randn(*s, generator=g) * scale                       # noqa: E731
    return dict(p_i=r(n_c, heads, hid1), p_t=r(n_c, heads, hid1), c0=r(hid1), w2t=r(hid1, hid2), b2=r(hid2), w3=r(hid2),
                b3=float(r(1)[0]))


PAIR_CASES = {"7x1": (7, 1, 1.0), "260x17": (260, 17, 0.3), "256x64": (256, 64, 0.1), "500x64": (500, 64, 0.05)}


@pytest.fixture(scope="module")
def pair_cases():
    out = {}
    for i, (name, (hid1, hid2, scale)) in enumerate(PAIR_CASES.items()):
        g = torch.Generator().manual_seed(100 + i)
        prm = _head_params(g, 8, 3, hid1, hid2, scale)
        st_i, st_t = torch.randn(8, 3, 200, generator=g) * 2, torch.randn(8, 3, 200, generator=g) * 2
        out[name] = (st_i, st_t, prm, R.cross_attention_pairs_emulation(st_i, st_t, **prm))
    return out


PAIR_DEFECTS = ["weights_swapped_in_one_head", "c0_dropped", "b2_after_relu", "chain_stops_at_hid2-1", "last_hid1_unit_dropped", "w2_bf16",
                "tanh_without_half"]


@pytest.mark.parametrize("case", list(PAIR_CASES))
@pytest.mark.parametrize("defect", [None] + PAIR_DEFECTS)
def test_cross_attention_pair_budget(pair_cases, case, defect):
    st_i, st_t, prm, (ref, extra) = pair_cases[case]
    _head_check(f"pairs {case}", defect, _pairs_cpu(st_i, st_t, defect=defect, **prm), ref, extra)


def _rerank_cpu(q, k_i, k_t, cand, depth, prm, defect=None):
    """fp32 stand-in of the gathered route: per-head dot products of the gathered rows, then the pair arithmetic."""
    heads = prm["p_i"].shape[1]
    nq, dim = q.shape
    ng, hd = k_i.shape[0], dim // heads
    ids = cand[:, :depth].long()
    valid = (ids >= 0) & (ids < ng)
    ids = torch.where(valid, ids, torch.zeros_like(ids))
    used = dim // 4 * 4 if defect == "last_dim%4_elements_dropped" else dim
    keep = (torch.arange(dim) < used).float()

    def dots(k):
        prod = (q[:, None, :] * k[ids] * keep).view(nq, depth, heads, hd)
        if defect == "neighbouring_heads_columns":
            prod = prod.clone()
            prod[:, :, 0] = prod[:, :, 1]
        return prod.sum(-1)

    flat = lambda x: x.reshape(nq * depth, 1, heads)                         # noqa: E731
    p = {n: (v[ids.reshape(-1)] if n in ("p_i", "p_t") else v) for n, v in prm.items()}
    out = _mix_cpu(flat(dots(k_i)), flat(dots(k_t)), **p).reshape(nq, depth)
    return out.masked_fill(~valid, float("-inf"))


def _rerank_case(seed, heads, dim, hid1, hid2, scale, ng=40, nq=3, depth=100):
    g = torch.Generator().manual_seed(seed)
    prm = _head_params(g, heads, ng, hid1, hid2, scale)
    amp = (2.0 / (dim // heads) ** 0.5) ** 0.5                               # per-head dot products ~ randn * 2
    q, k_i, k_t = (torch.randn(n, dim, generator=g) * amp for n in (nq, ng, ng))
    cand = torch.randint(0, ng, (nq, depth + 3), generator=g, dtype=torch.int32)
    cand[0, 5], cand[1, 0], cand[2, depth - 1] = -1, ng, 2 ** 31 - 1
    return q, k_i, k_t, cand, depth, prm


@pytest.mark.parametrize("defect", [None, "neighbouring_heads_columns"])
def test_cross_attention_rerank_budget(defect):
    q, k_i, k_t, cand, depth, prm = _rerank_case(7, 8, 72, 260, 17, 0.3)
    ref, extra = R.cross_attention_rerank_emulation(q, k_i, k_t, cand=cand, depth=depth, **prm)
    assert tuple(ref.shape) == (3, depth) and int(torch.isinf(ref).sum()) == 3          # the three slots outside the gallery
    _head_check("rerank dim 72", defect, _rerank_cpu(q, k_i, k_t, cand, depth, prm, defect), ref, extra)


@pytest.mark.parametrize("defect", [None, "last_dim%4_elements_dropped"])
def test_cross_attention_rerank_budget_catches_a_dropped_vector_tail(defect):
    """dim % 4 != 0 needs a head count that does not divide by four: the statement takes the heads from p_i (the kernel serves
    8 heads, where dim % 8 == 0 leaves no such tail -- its scalar instance is for dim % 32 != 0)."""
    q, k_i, k_t, cand, depth, prm = _rerank_case(8, 2, 6, 8, 4, 1.0)
    ref, extra = R.cross_attention_rerank_emulation(q, k_i, k_t, cand=cand, depth=depth, **prm)
    _head_check("rerank dim 6", defect, _rerank_cpu(q, k_i, k_t, cand, depth, prm, defect), ref, extra)


def _linear_cpu(t2i, t2t, w0, b0, w1, b1, defect=None):
    a, b = (t2t, t2i) if defect == "inputs_swapped" else (t2i, t2t)
    acc = torch.full_like(a, b1)
    for h in range(w0.shape[0]):
        t = _fma(w0[h, 0], a, _fma(w0[h, 1], b, b0[h]))
        acc = _fma(w1[h], t if defect == "relu_dropped" else t.clamp_min(0), acc)
    if defect == "last_element_not_written":
        acc[-1] = -7.0                                                       # the test's sentinel
    return acc


@pytest.mark.parametrize("hidden", [1, 128, 2048])
@pytest.mark.parametrize("defect", [None, "relu_dropped", "inputs_swapped", "last_element_not_written"])
def test_linear_head_budget(hidden, defect):
    g = torch.Generator().manual_seed(200 + hidden)
    n = 33 if defect == "last_element_not_written" else 2000                 # one unwritten element of 33 is 3 % of the outputs
    t2i, t2t = torch.randn(n, generator=g) * 0.3, torch.randn(n, generator=g) * 0.3
    w0, b0, w1 = torch.randn(hidden, 2, generator=g), torch.randn(hidden, generator=g) * 0.3, torch.randn(hidden, generator=g) * hidden ** -0.5
    b1 = float(torch.randn(1, generator=g)[0])
    ref, extra = R.linear_head_statement(t2i, t2t, w0, b0, w1, b1)
    _head_check(f"linear hidden {hidden}", defect, _linear_cpu(t2i, t2t, w0, b0, w1, b1, defect), ref, extra)


def _gate_cpu(x, pre, w, bias, relu, defect=None):
    rows, cols = x.shape
    used = cols // 64 * 64 if defect == "last_cols%64_dropped" else cols
    v = x if pre is None or defect == "pre_ignored" else x + pre
    if relu or defect == "relu_when_off":
        v = v.clamp_min(0)
    pad = (cols + 63) // 64 * 64
    s = torch.zeros(rows, 64)
    vp, wp = torch.zeros(rows, pad), torch.zeros(pad)
    vp[:, :used], wp[:used] = v[:, :used], w[:used]
    for c in range(0, pad, 64):                                              # lane l sums columns l, l + 64, ...
        s = _fma(vp[:, c:c + 64], wp[c:c + 64], s)
    return 1.0 / (1.0 + torch.exp(-(s.sum(-1) + bias)))


def _gate_case(cols, with_pre):
    g = torch.Generator().manual_seed(300 + cols)
    x = torch.randn(400, cols, generator=g)
    pre = torch.randn(cols, generator=g) * 0.5 if with_pre else None
    return x, pre, torch.randn(cols, generator=g) * cols ** -0.5


@pytest.mark.parametrize("cols", [1, 64, 65, 1000])
@pytest.mark.parametrize("relu,with_pre", [(0, True), (1, True), (0, False)])
def test_gate_rows_budget_passes_the_stand_in(cols, relu, with_pre):
    x, pre, w = _gate_case(cols, with_pre)
    ref, extra = R.gate_rows_emulation(x, pre, w, 0.25, relu)
    _head_check(f"gate cols {cols} relu {relu} pre {with_pre}", None, _gate_cpu(x, pre, w, 0.25, relu), ref, extra)


@pytest.mark.parametrize("cols", [65, 1000])
@pytest.mark.parametrize("relu,with_pre,defect", [(0, True, "relu_when_off"), (1, True, "pre_ignored"), (0, True, "pre_ignored"),
                                                  (1, True, "last_cols%64_dropped"), (0, False, "last_cols%64_dropped")])
def test_gate_rows_budget_catches_planted_defects(cols, relu, with_pre, defect):
    x, pre, w = _gate_case(cols, with_pre)
    ref, extra = R.gate_rows_emulation(x, pre, w, 0.25, relu)
    _head_check(f"gate cols {cols} relu {relu} pre {with_pre}", defect, _gate_cpu(x, pre, w, 0.25, relu, defect), ref, extra)
