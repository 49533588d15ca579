"""CPU: the rounding-budget bars of the GPU numerics tests can fail.  A stand-in "kernel" (torch fp32 on the CPU, rounded to
bf16 like the HIP epilogues) passes them; the same kernel with one planted defect -- truncation instead of round-to-nearest-even,
a scale a fraction of an ulp off, a dropped K-tile, the bias added twice, a wrong QuickGELU constant, a dropped key, a masked
causal diagonal -- fails the elementwise bar, the bias bar or both.  The bars and their `extra` terms are the ones
tests/test_numerics_gpu.py applies to the kernels."""
import pytest
import torch

from oracle import rounding as R

MAX_BIAS = 0.02           # ulp: |signed bias| bar of every bf16 output
KAPPA = 8                 # accumulator bar: |acc - ref64| <= KAPPA 2^-24 sum|a||w|, as in tests/test_numerics_gpu.py


def _trunc_bf16(x32):
    return (x32.contiguous().view(torch.int32) & ~0xffff).view(torch.float32)


def _passes(got, ref64, extra):
    ratio = R.budget_ratio(got, ref64, extra)
    top = float(torch.nan_to_num(ratio, nan=float("inf")).max())
    return top <= 1.0 and abs(R.signed_bias_ulps(got, ref64)) <= MAX_BIAS, top, R.signed_bias_ulps(got, ref64)


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
