"""GPU: the ViT-L/14@336px vision tower (577 tokens: the streaming attention kernel in every block, the pooled-row attention in
the last) against the fp32 CPU oracle, at a tiny width with the real sequence length, at the longest supported sequence, and at
full size; and clip.load("ViT-L/14@336px") end to end.  Parity bar: cosine >= 1 - 1e-3 per embedding (tests/test_encoder_gpu.py)."""
import numpy as np
import pytest
import torch

from knowledge_enhanced_multimodal_retrieval_amd import clip_api, engine
from knowledge_enhanced_multimodal_retrieval_amd.config import ARCHS, ClipArch
from oracle import clip_ref

pytestmark = pytest.mark.gpu
COS_TOL = 1e-3
NAME = "ViT-L/14@336px"
# the oracle's architecture dict of the 336 px model (oracle/clip_ref.ARCHS has the 224 px one only)
ORACLE_336 = dict(clip_ref.ARCHS["ViT-L/14"], image_size=336)
TINY_577 = dict(clip_ref.ARCHS["tiny"], image_size=192, patch=8, v_width=256, v_layers=2)      # 24 x 24 + 1 = 577 tokens
TINY_1025 = dict(clip_ref.ARCHS["tiny"], image_size=256, patch=8, v_width=256, v_layers=2)     # 32 x 32 + 1 = 1025 (the limit)


def _cos(a, b):
    return torch.nn.functional.cosine_similarity(a.double(), b.double(), dim=-1)


def _engine(oa, device, precision="bf16-x24", outliers=False, seed=0):
    sd = clip_ref.random_state_dict(oa, seed=seed, outliers=outliers)
    eng = engine.ClipEngine(ClipArch(**oa), device, precision=precision)
    eng.load_state_dict(sd)
    return sd, eng


def test_tiny_577_tokens_match_oracle(device):
    sd, eng = _engine(TINY_577, device)
    assert eng.arch.v_tokens == 577
    n_call = eng.image_batch
    assert n_call < engine.MAX_IMAGE_BATCH
    g = torch.Generator().manual_seed(21)
    px = torch.randn(n_call + 2, 3, 192, 192, generator=g)                  # crosses an encoder call boundary
    ref = clip_ref.encode_image(sd, TINY_577, px)
    for n in (1, 5, n_call + 2):
        got = eng.encode_image(px[:n].to(device)).cpu()
        c = _cos(got, ref[:n])
        print(f"tiny-577 batch {n}: 1 - cos max {float((1 - c).max()):.2e}")
        assert float((1 - c).max()) < COS_TOL, n
    # slices are independent: the last two images alone give the same bits as inside the two-call batch
    assert torch.equal(eng.encode_image(px[-2:].to(device)).cpu(), got[-2:])


def test_tiny_1025_tokens_match_oracle(device):
    sd, eng = _engine(TINY_1025, device)
    assert eng.arch.v_tokens == 1025
    px = torch.randn(2, 3, 256, 256, generator=torch.Generator().manual_seed(22))
    got = eng.encode_image(px.to(device)).cpu()
    assert float((1 - _cos(got, clip_ref.encode_image(sd, TINY_1025, px))).max()) < COS_TOL


_ORACLE = {}


def _full_oracle(outliers):
    if outliers not in _ORACLE:
        sd = clip_ref.random_state_dict(ORACLE_336, seed=0, outliers=outliers)
        px = torch.randn(2, 3, 336, 336, generator=torch.Generator().manual_seed(1234))
        _ORACLE[outliers] = (sd, px, clip_ref.encode_image(sd, ORACLE_336, px))
    return _ORACLE[outliers]


@pytest.mark.parametrize("precision,outliers", [("bf16-x24", False), ("bf16", False), ("bf16-x24", True), ("fp8", False)])
def test_full_size_336_matches_oracle(device, precision, outliers):
    sd, px, ref = _full_oracle(outliers)
    eng = engine.ClipEngine(ARCHS[NAME], device, precision=precision)
    eng.load_state_dict(sd)
    got = eng.encode_image(px.to(device)).cpu()
    c = _cos(got, ref)
    print(f"ViT-L/14@336px {precision} outliers={outliers}: 1 - cos max {float((1 - c).max()):.2e}")
    assert float((1 - c).max()) < COS_TOL
    del eng
    torch.cuda.empty_cache()


def test_clip_load_336_end_to_end(device, monkeypatch):
    from PIL import Image
    monkeypatch.setattr(clip_api, "_allow_random", True)
    model, preprocess = clip_api.load(NAME, device=str(device))
    assert model.arch == ARCHS[NAME] and preprocess.n_px == 336
    rng = np.random.default_rng(3)
    img = Image.fromarray(rng.integers(0, 256, (400, 520, 3), dtype=np.uint8))
    x = preprocess(img)
    assert x.shape == (3, 336, 336)
    with torch.no_grad():
        got = model.encode_image(x[None].to(device))
    eng = engine.ClipEngine(ARCHS[NAME], device)
    eng.load_state_dict({k: v for k, v in model.state_dict().items() if k != "logit_scale"})
    want = eng.encode_image(x[None].to(device))
    assert torch.equal(got, want)
