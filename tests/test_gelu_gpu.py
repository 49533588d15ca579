"""GPU: the exact-GELU route -- the EPI_BIAS_GELU_BF16 epilogue of every GEMM kernel fc1 can take, held to its rounding budget
against fp64 (oracle/rounding.py), and the towers with option "activation" = gelu against Hugging Face `hidden_act: gelu`
fixtures (tests/golden/make_golden_gelu.py).  Every measured worst ratio / bias / 1 - cos is printed (pytest -s).

Measured on the MI355X (this file's NUMERICS lines; DESIGN.md section 2 quotes them): see the docstrings below."""
import importlib.util
import json
import math
import os

import numpy as np
import pytest
import torch

from knowledge_enhanced_multimodal_retrieval_amd import _lib, clip_api, debug, engine
from knowledge_enhanced_multimodal_retrieval_amd.config import ARCHS
from oracle import clip_ref
from oracle import rounding as R

pytestmark = pytest.mark.gpu

COS_TOL = 1e-3             # the project's bar per embedding (tests/test_encoder_gpu.py)
MAX_BIAS = 0.02            # signed bias of a rounded output, bf16 ulp (tests/test_numerics_gpu.py)
KAPPA = 8                  # the accumulator bar of tests/test_numerics_gpu.py: |acc - fp64| <= KAPPA 2^-24 sum|a||w|
GELU_SLOPE = 1.13          # max |d gelu / dx| (1.129 at x = 1.41)
ACC_MAX = 12.0             # every pre-activation of these tests: the results stay normal bf16 numbers (gelu(-12) = -2e-32)
EPI_G, EPI_F32 = _lib.EPI_BIAS_GELU_BF16, _lib.EPI_BIAS_RESID_F32


def _note(name, value):
    print(f"NUMERICS {name} {value}")


def _gelu64(x):
    """0.5 x erfc(-x / sqrt 2) in fp64: exact GELU in the form that keeps relative accuracy in the negative tail."""
    x = x.double().cpu()
    return 0.5 * x * torch.special.erfc(-x * math.sqrt(0.5))


def _gelu_extra(acc64):
    """What csrc/common.h gelu_erf may move the result by before the bf16 rounding: 2^-24 (c_rel |gelu64(acc)| + c_abs |acc|) with
    c_abs = 0 -- the kernel evaluates the erfc form, whose error is relative everywhere, the negative tail included -- and
    c_rel = 32, independent of acc, from the formula (units of 2^-24 relative, 1 fp32 ulp <= 2 units):
      * erfcf of the device library: HIP's math reference lists it at 2 ulp; the library is built to OpenCL's bound for erfc, 16
        ulp, which that figure is measured under but does not guarantee -- budgeted at 13 ulp = 26 units;
      * its argument z = -x / sqrt 2: the tail of erfc amplifies an argument error by erfc'/erfc ~ 2 z, a plain fp32 product
        (1.28 units of z) would cost up to 1.28 acc^2 + |acc| units.  The kernel carries the product's remainder e and applies
        erfc(z + e) = erfc(z) (1 - 2 max(z, 0) e): what is left is (erfc'/erfc - 2 z) z 1.28 <= 1.5 units for z > 0 and
        1.13 |z| exp(-z^2) 1.28 <= 0.7 units for z <= 0;
      * the correction's fma, erfc x correction, and the product with 0.5 x (exact): 3 roundings = 3 units.
    26 + 1.5 + 3 = 30.5 <= 32.  (The issue's cap is 32 + acc^2; the acc^2 share is not used.)"""
    return 2.0 ** -24 * 32 * _gelu64(acc64).abs()


def _sample_rows(m):
    """Rows for the CPU fp64 reference: both ends of every 256-row tile boundary region and an even spread (at most ~600)."""
    edge = [r for t in range(0, m, 256) for r in (t, t + 1, t + 127, t + 128, t + 254, t + 255) if r < m]
    return torch.tensor(sorted(set(edge[:300] + list(range(0, m, max(1, m // 300))))), dtype=torch.long)


def _operands(m, n, k, kind, seed):
    """bf16 operands from a CPU generator (the same numbers on every machine).  kind "random": unit-variance sums and a N(0, 1)
    bias; "linspace": bias = linspace(-10, 10, n) and sums of std 0.25, so that the pre-activations cover the negative tail and the
    saturated side and stay inside +-ACC_MAX."""
    g = torch.Generator().manual_seed(seed)
    ma = (m + 255) // 256 * 256
    a = torch.randn(ma, k, generator=g).to(torch.bfloat16)
    w = (torch.randn(n, k, generator=g) * k ** -0.5 * (1.0 if kind == "random" else 0.25)).to(torch.bfloat16)
    bias = torch.randn(n, generator=g) if kind == "random" else torch.linspace(-10, 10, n)
    return a, w, bias


def _check_tail_and_saturation(og, acc64, what):
    """The linspace case: outputs of pre-activations >= 6 are the pre-activation itself (erfc = 2 in fp32), rounded once; a zero of
    either sign appears only where fp64 GELU rounds to it."""
    og, ref = og.double().cpu(), _gelu64(acc64)
    sat = acc64 >= 6.0
    assert int(sat.sum()) > 0 and int((acc64 <= -6.0).sum()) > 0, what
    assert torch.equal(og[sat], R.rne_bf16(acc64[sat])), what
    want = R.rne_bf16(ref)
    assert torch.equal(og == 0, want == 0) and torch.equal(torch.signbit(og[og == 0]), torch.signbit(want[want == 0])), what
    assert float(ref[ref != 0].abs().min()) >= 2.0 ** -126, what            # normal bf16 numbers throughout


# ------------------------------------------------------------------------------------------------ the epilogue, kernel by kernel
@pytest.mark.parametrize("kind", ["random", "linspace"])
@pytest.mark.parametrize("variant,m,n,k", [(1, 300, 768, 256), (2, 514, 256, 1024), (7, 256 * 70 + 19, 1024, 256), (7, 1000, 1024, 1024)])
def test_gelu_epilogue_against_fp64_of_the_kernels_accumulator(device, variant, m, n, k, kind):
    """EPI_BIAS_RESID_F32 onto C = 0 hands back the kernel's own fp32 accumulator (+ bias); the GELU output of the same kernel within
    half a bf16 ulp + _gelu_extra of gelu64(accumulator).  Variant 1 = 128x128, 2 = 256x256, 7 = persistent (284 tiles, several per
    workgroup, on the pre-staged first K-tile; 16 tiles at K = 1024), each twice for state leaked between launches."""
    a, w, bias = (t.to(device) for t in _operands(m, n, k, kind, 5 * m + n + k))
    ma = a.shape[0]
    with debug.override(gemm_variant=variant):
        acc = engine.op_gemm(a, w, bias, m, EPI_F32, c=torch.zeros(ma, n, device=device))[:m]
        og = engine.op_gemm(a, w, bias, m, EPI_G)[:m]
        again = engine.op_gemm(a, w, bias, m, EPI_G)[:m]
    assert torch.equal(og, again), "two launches, two results"
    assert float(acc.abs().max()) <= ACC_MAX
    rows = _sample_rows(m)
    acc64, got = acc[rows.to(device)].double().cpu(), og[rows.to(device)].cpu()
    top, bias_u = R.check_budget(got, _gelu64(acc64), _gelu_extra(acc64), max_bias=MAX_BIAS, what=f"gelu v{variant} {kind}")
    _note(f"gelu_v{variant}_{m}x{n}x{k}_{kind}_ratio_bias", (top, bias_u))
    if kind == "linspace":
        _check_tail_and_saturation(got, acc64, f"gelu v{variant}")


@pytest.mark.parametrize("kind", ["random", "linspace"])
@pytest.mark.parametrize("variant", [7, 8])
@pytest.mark.parametrize("m,n,k", [(129, 512, 192), (77, 2304, 768)])
def test_gelu_epilogue_small_m_against_fp64_sum(device, variant, m, n, k, kind):
    """At m <= 512 the forced persistent kernel (7) and the skinny split-K kernel (8) have no fp32 epilogue of the same summation
    order: their GELU outputs against gelu64 of the fp64 sum, the accumulator's budget carried through |d gelu / dx| <= 1.13."""
    a, w, bias = _operands(m, n, k, kind, 7 * m + n + k)
    a64, w64, b64 = a[:m].double(), w.double(), bias.double()
    ref = a64 @ w64.T + b64
    assert float(ref.abs().max()) <= ACC_MAX
    extra = KAPPA * 2.0 ** -24 * (a64.abs() @ w64.abs().T + b64.abs()) * GELU_SLOPE + _gelu_extra(ref)
    with debug.override(gemm_variant=variant):
        og = engine.op_gemm(a.to(device), w.to(device), bias.to(device), m, EPI_G)[:m].cpu()
        again = engine.op_gemm(a.to(device), w.to(device), bias.to(device), m, EPI_G)[:m].cpu()
    assert torch.equal(og, again)
    top, bias_u = R.check_budget(og, _gelu64(ref), extra, max_bias=MAX_BIAS, what=f"gelu v{variant} small m {kind}")
    _note(f"gelu_v{variant}_{m}x{n}x{k}_{kind}_ratio_bias", (top, bias_u))


@pytest.mark.parametrize("kind", ["random", "linspace"])
@pytest.mark.parametrize("m,n,k", [(300, 768, 256), (256 * 70 + 19, 1024, 256)])
def test_gelu_epilogue_fp8_exact_integers(device, m, n, k, kind):
    """e4m3 integers {-2..2} and power-of-two column scales: the pre-activation exact * wscale + bias is a multiple of 2^-8 below 16,
    exact in fp32, so the output is the GELU epilogue's arithmetic alone: within the same budget of gelu64 of that number."""
    g = torch.Generator().manual_seed(m + n + k)
    ma = (m + 255) // 256 * 256
    a = torch.randint(-2, 3, (ma, k), generator=g).float()
    w = torch.randint(-2, 3, (n, k), generator=g).float()
    if kind == "random":                                   # sums of std 32: scaled to std 0.25 .. 1, bias in eighths within +-6
        wscale = torch.ldexp(torch.ones(n), torch.randint(-7, -4, (n,), generator=g))
        bias = torch.randint(-48, 49, (n,), generator=g).float() / 8
    else:
        wscale = torch.ldexp(torch.ones(n), torch.randint(-8, -6, (n,), generator=g))
        bias = torch.round(torch.linspace(-10, 10, n) * 64) / 64
    rows = _sample_rows(m)
    x = (a[rows].double() @ w.double().T) * wscale.double() + bias.double()
    assert float(x.abs().max()) <= ACC_MAX and torch.equal(x.float().double(), x)
    a8, w8 = a.to(device).to(torch.float8_e4m3fn), w.to(device).to(torch.float8_e4m3fn)
    og = engine.op_gemm_fp8(a8, w8, wscale.to(device), bias.to(device), m, EPI_G)[:m]
    again = engine.op_gemm_fp8(a8, w8, wscale.to(device), bias.to(device), m, EPI_G)[:m]
    assert torch.equal(og, again)
    got = og[rows.to(device)].cpu()
    ref = _gelu64(x)
    top, bias_u = R.check_budget(got, ref, _gelu_extra(x), max_bias=None, what=f"gelu fp8 {kind}")
    # x lives on a grid (about 2 000 distinct values among 230 000): gelu64(x) does not spread over the bf16 ulp intervals, and one
    # correct rounding of it already has a signed bias of -0.026 .. -0.033 ulp.  The kernel's bias is held to that of the ideal rounding.
    ideal_u = R.signed_bias_ulps(R.rne_bf16(ref), ref)
    _note(f"gelu_fp8_{m}x{n}x{k}_{kind}_ratio_bias_idealbias", (top, bias_u, ideal_u))
    assert abs(bias_u - ideal_u) <= MAX_BIAS, (bias_u, ideal_u)
    if kind == "linspace":
        _check_tail_and_saturation(got, x, "gelu fp8")


def test_gelu_epilogue_is_refused_by_the_experiment_kernels(device):
    """The A/B experiment kernels (gemm_variant 4, 5, 6, 9; `build.py --ab-variants` only) did not get the epilogue: they return
    KEMR_ERR_INVALID instead of computing something else."""
    if not debug.ab_variants():
        pytest.skip("the product library holds no experiment kernels (build.py --ab-variants)")
    a, w, bias = (t.to(device) for t in _operands(1000, 1024, 256, "random", 1))
    for variant in (4, 5, 6, 9):
        with debug.override(gemm_variant=variant):
            with pytest.raises(RuntimeError, match="not a bf16-store epilogue"):
                engine.op_gemm(a, w, bias, 1000, EPI_G)


def test_bad_epilogue_values_are_still_refused(device):
    a, w, bias = (t.to(device) for t in _operands(300, 256, 128, "random", 2))
    for epi in (3, 6, -1):
        with pytest.raises(RuntimeError, match="bad epilogue"):
            engine.op_gemm(a, w, bias, 300, epi)
    a8 = torch.zeros(512, 256, device=device).to(torch.float8_e4m3fn)
    with pytest.raises(RuntimeError, match="not a bf16-store epilogue"):
        engine.op_gemm_fp8(a8, a8[:256], torch.ones(256, device=device), None, 300, EPI_F32)


# ------------------------------------------------------------------------------------------------ the towers
_GEN, _FIX = [], {}


def _gen():
    if not _GEN:
        spec = importlib.util.spec_from_file_location("make_golden_gelu", os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "make_golden_gelu.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        _GEN.append(mod)
    return _GEN[0]


def _fixture(name):
    """(weights, pixels, ids, fixture arrays) of a case, built once per session and left unchanged."""
    if name not in _FIX:
        gen = _gen()
        z = np.load(gen.fixture_path(name))
        meta = json.loads(bytes(z["meta_json"]).decode())
        sd = gen.gelu_fixture_state_dict(clip_ref.ARCHS[name], meta["weight_seed"])
        # (an fp64 sum of a large tensor depends on how many threads share it: to 1e-12, as tests/test_oracle_golden.py holds its own)
        assert sorted(sd) == sorted(meta["weight_abs_sums"]), "the fixture's weights changed"
        for k, v in meta["weight_abs_sums"].items():
            assert float(sd[k].double().abs().sum()) == pytest.approx(v, rel=1e-12), k
        px, ids = gen.fixture_inputs(clip_ref.ARCHS[name], meta["n_images"], meta["n_texts"])
        assert float(px.double().abs().sum()) == pytest.approx(meta["pixel_abs_sum"], rel=1e-12) and np.array_equal(ids.numpy(), z["ids"])
        _FIX[name] = (sd, px, ids, {k: torch.from_numpy(z[k]) for k in z.files if k.endswith("features") or k.endswith("quick_gelu")})
    return _FIX[name]


def _miss(a, b):
    return 1.0 - torch.nn.functional.cosine_similarity(a.double().cpu(), b.double(), dim=-1)


def _engine(name, device, precision, activation, sd):
    eng = engine.ClipEngine(ARCHS[name], device, precision=precision, activation=activation)
    eng.load_state_dict(sd)
    return eng


def _encode_all(eng, px, ids, device, image_batches):
    """Image embeddings per batch size, text embeddings through kemr_encode_text and through the packed route."""
    imgs = {nb: eng.encode_image(px[:nb].to(device)) for nb in image_batches}
    eng.pack_text = False
    full = eng.encode_text(ids.to(device))
    eng.pack_text = True
    packed = eng.encode_text(ids)                          # host ids: the lengths come from them
    return imgs, full, packed


# image batches: tiny 4 x 17 = 68 token rows; tiny-long 2 x 197 = 394 (below 512) and 4 x 197 = 788 (the persistent kernel, and the
# residual-add epilogues where the precision has them)
TOWER_CASES = [("tiny", (4,)), ("tiny-long", (2, 4))]


@pytest.mark.parametrize("pooled", [True, False])
@pytest.mark.parametrize("precision", ["bf16-x24", "bf16", "bf16-res16", "fp8", "fp8-mlp"])
@pytest.mark.parametrize("name,image_batches", TOWER_CASES)
def test_towers_match_the_hf_gelu_fixtures(device, name, image_batches, precision, pooled):
    """Option "activation" = gelu against transformers.CLIPModel with hidden_act "gelu" on the same weights and inputs: 1 - cos <=
    COS_TOL per embedding.  "fp8-mlp" (fc1 on e4m3 operands) is held to its QuickGELU twin instead: at most twice the 1 - cos the
    same precision shows, in this run, with activation quick_gelu against the fixture's quick_gelu outputs of the same weights."""
    sd, px, ids, fix = _fixture(name)
    eng = _engine(name, device, precision, "gelu", sd)
    eng.set_last_block_pooled_row(pooled)
    imgs, full, packed = _encode_all(eng, px, ids, device, image_batches)
    worst_t = max(float(_miss(full, fix["text_features"]).max()), float(_miss(packed, fix["text_features"]).max()))
    worst_i = max(float(_miss(imgs[nb], fix["image_features"][:nb]).max()) for nb in image_batches)
    _note(f"towers_gelu_{name}_{precision}_pooled{int(pooled)}_1-cos_image_text", (worst_i, worst_t))
    assert worst_t <= COS_TOL                               # (the text tower never runs on fp8 operands)
    if precision != "fp8-mlp":
        assert worst_i <= COS_TOL
        return
    twin = _engine(name, device, precision, "quick_gelu", sd)
    twin.set_last_block_pooled_row(pooled)
    timgs = {nb: twin.encode_image(px[:nb].to(device)) for nb in image_batches}
    twin_i = max(float(_miss(timgs[nb], fix["image_features_quick_gelu"][:nb]).max()) for nb in image_batches)
    _note(f"towers_fp8-mlp_{name}_pooled{int(pooled)}_1-cos_gelu_vs_quick_gelu_twin", (worst_i, twin_i))
    assert worst_i <= 2 * twin_i


def test_hf_directory_end_to_end_at_vit_b32(device, tmp_path):
    """A save_pretrained directory (hidden_act "gelu", ViT-B/32's shape) through clip_api.load -- the key map, the model's
    activation, option "activation", the kernels -- and the two calls the reference's evaluator_hf.py makes, at the default precision."""
    from safetensors.torch import save_file
    name = "ViT-B/32"
    sd, px, ids, fix = _fixture(name)
    cfg = clip_ref.hf_config_kwargs(clip_ref.ARCHS[name])
    cfg["text_config"]["hidden_act"] = cfg["vision_config"]["hidden_act"] = "gelu"
    d = str(tmp_path / "hf")
    os.makedirs(d)
    with open(os.path.join(d, "config.json"), "w") as f:
        json.dump({"model_type": "clip", **cfg}, f)
    save_file({k: v.contiguous() for k, v in clip_ref.to_hf_state_dict(sd, clip_ref.ARCHS[name]).items()}, os.path.join(d, "model.safetensors"))
    model, _ = clip_api.load(d, device=device)
    assert model.activation == "gelu" and model.arch == ARCHS[name]
    got_i = model.get_image_features(pixel_values=px.to(device))
    longest = int((ids.argmax(-1) + 1).max())                                   # a processor pads to the batch's longest text
    got_t = model.get_text_features(input_ids=ids[:, :longest].long().to(device), attention_mask=torch.ones(len(ids), longest, device=device))
    assert model.engine().activation == "gelu" and model.engine().precision == _lib.DEFAULT_PRECISION
    mi, mt = float(_miss(got_i, fix["image_features"]).max()), float(_miss(got_t, fix["text_features"]).max())
    _note("hf_directory_ViT-B-32_gelu_1-cos_image_text", (mi, mt))
    assert mi <= COS_TOL and mt <= COS_TOL
    assert float(_miss(got_i, fix["image_features_quick_gelu"]).min()) > COS_TOL


def test_the_switch_does_something_and_the_default_does_nothing(device):
    name = "tiny-long"
    sd, px, ids, fix = _fixture(name)
    pxd = px.to(device)
    never = engine.ClipEngine(ARCHS[name], device)                               # the option is never touched
    never.load_state_dict(sd)
    explicit = _engine(name, device, _lib.DEFAULT_PRECISION, "quick_gelu", sd)
    explicit.set_activation("quick_gelu")
    qi, qt = never.encode_image(pxd), never.encode_text(ids)
    assert torch.equal(qi, explicit.encode_image(pxd)) and torch.equal(qt, explicit.encode_text(ids))
    assert float(_miss(qi, fix["image_features_quick_gelu"]).max()) <= COS_TOL and float(_miss(qt, fix["text_features_quick_gelu"]).max()) <= COS_TOL
    # the same weights, the other activation: off the QuickGELU fixture, on the GELU one
    explicit.set_activation("gelu")
    gi, gt = explicit.encode_image(pxd), explicit.encode_text(ids)
    assert float(_miss(gi, fix["image_features_quick_gelu"]).min()) > COS_TOL and float(_miss(gt, fix["text_features_quick_gelu"]).min()) > COS_TOL
    assert float(_miss(gi, fix["image_features"]).max()) <= COS_TOL and float(_miss(gt, fix["text_features"]).max()) <= COS_TOL
    # back and forth on the live model: the first results, bit for bit; the other model never moved
    explicit.set_activation("quick_gelu")
    assert torch.equal(qi, explicit.encode_image(pxd)) and torch.equal(qt, explicit.encode_text(ids))
    explicit.set_activation("gelu")
    assert torch.equal(gi, explicit.encode_image(pxd)) and torch.equal(gt, explicit.encode_text(ids))
    assert torch.equal(qi, never.encode_image(pxd)) and never.activation == "quick_gelu"
    with pytest.raises(ValueError, match="quick_gelu.*gelu"):
        explicit.set_activation("tanh")
