"""ViT-L/14@336px without a GPU: the model name through clip.load / the evaluator CLI, the checkpoint file name, the C ABI's
sequence limits, and the fp32 oracle against transformers at a sequence longer than 288 tokens."""
import argparse
import ctypes as C

import pytest
import torch

from knowledge_enhanced_multimodal_retrieval_amd import _lib, clip_api, engine, evaluators
from knowledge_enhanced_multimodal_retrieval_amd.config import ARCHS
from oracle import clip_ref

NAME = "ViT-L/14@336px"
MAX_VISION_TOKENS = 1025          # include/kemr.h KEMR_MAX_VISION_TOKENS


def test_registered_and_public():
    assert NAME in clip_api.available_models()
    a = ARCHS[NAME]
    assert (a.embed_dim, a.image_size, a.patch, a.v_width, a.v_layers, a.t_width, a.t_layers) == (768, 336, 14, 1024, 24, 768, 12)
    assert a.v_tokens == 577
    for old in ("ViT-B/32", "ViT-B/16", "ViT-L/14"):
        assert old in clip_api.available_models()


def test_image_call_size():
    assert engine.image_call_items(ARCHS["ViT-L/14"]) == engine.MAX_IMAGE_BATCH == 255
    assert engine.image_call_items(ARCHS["ViT-B/32"]) == 255
    n = engine.image_call_items(ARCHS[NAME])
    assert 1 <= n <= 255 * 257 // 577
    assert n == engine.tile_friendly_batch(577, 1024, (255 * 257 // 577) // 2, 255 * 257 // 577)


def _tiny_sd(tmp_path, arch_name, monkeypatch):
    """A real (tiny) checkpoint cannot stand in for ViT-L/14: the strict load checks shapes.  So the checkpoint is the seeded model
    itself with one tensor changed, and the test checks that the change arrives."""
    monkeypatch.setattr(clip_api, "_allow_random", True)
    model, _ = clip_api.load(arch_name, device="cpu")
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    sd["visual.class_embedding"].fill_(0.25)
    p = tmp_path / (arch_name.replace("/", "-").replace("@", "-") + ".pt")
    torch.save(sd, p)
    return p


def test_load_name_parsing(tmp_path, monkeypatch):
    monkeypatch.setattr(clip_api, "_allow_random", True)
    model, pre = clip_api.load(NAME, device="cpu")
    assert model.arch == ARCHS[NAME]
    assert pre.n_px == 336
    assert model.visual.positional_embedding.shape == (577, 1024)
    assert model.weights_source == "random(seed 0)"
    # "<arch>@<file>" keeps its meaning for the 224 px model ...
    p224 = _tiny_sd(tmp_path, "ViT-L/14", monkeypatch)
    m224, pre224 = clip_api.load(f"ViT-L/14@{p224}", device="cpu")
    assert m224.arch == ARCHS["ViT-L/14"] and pre224.n_px == 224
    assert m224.weights_source == str(p224.resolve())
    assert torch.all(m224.visual.class_embedding == 0.25)
    # ... and the 336 px name takes a checkpoint behind a second '@'
    p336 = _tiny_sd(tmp_path, NAME, monkeypatch)
    m336, pre336 = clip_api.load(f"{NAME}@{p336}", device="cpu")
    assert m336.arch == ARCHS[NAME] and pre336.n_px == 336
    assert m336.weights_source == str(p336.resolve())
    assert torch.all(m336.visual.class_embedding == 0.25)
    with pytest.raises(FileNotFoundError):
        clip_api.load(f"{NAME}@{tmp_path / 'missing.pt'}", device="cpu")
    with pytest.raises(RuntimeError, match="not found"):
        clip_api.load("ViT-H/14", device="cpu")


def test_weights_for_upstream_file_name(tmp_path, monkeypatch):
    (tmp_path / "ViT-L-14-336px.pt").write_bytes(b"")
    (tmp_path / "ViT-L-14.pt").write_bytes(b"")
    monkeypatch.setenv("KEMR_CLIP_WEIGHTS", str(tmp_path))
    assert clip_api._weights_for(NAME) == str(tmp_path / "ViT-L-14-336px.pt")
    assert clip_api._weights_for("ViT-L/14") == str(tmp_path / "ViT-L-14.pt")


def test_load_clip_model_with_checkpoint(tmp_path, monkeypatch):
    from src.clip.model import clip_model as ref_path
    p = _tiny_sd(tmp_path, NAME, monkeypatch)
    monkeypatch.setattr(clip_api, "_allow_random", False)
    model, pre = ref_path.load_clip_model(model_name=NAME, checkpoint_path=str(p), device="cpu")
    assert model.arch == ARCHS[NAME] and pre.n_px == 336
    assert torch.all(model.visual.class_embedding == 0.25)


def test_evaluator_cli_accepts_the_name():
    for baseline in (False, True):
        parser = argparse.ArgumentParser()
        evaluators._common_args(parser, baseline)
        args = parser.parse_args(["--model_name", NAME, "--output_file", "r.json"])
        assert args.model_name == NAME
    parser = argparse.ArgumentParser()
    evaluators._common_args(parser, False)
    with pytest.raises(SystemExit):
        parser.parse_args(["--model_name", "ViT-L/14@448px", "--output_file", "r.json"])


def _create(**kw):
    cfg = dict(ARCHS["ViT-L/14"].as_dict())
    cfg.update(kw)
    L = _lib.lib()
    h = C.c_void_p()
    rc = L.kemr_model_create(C.byref(_lib.KemrCfg(**cfg)), C.byref(h))
    if rc == 0:
        L.kemr_model_destroy(h)
    return rc, L.kemr_last_error().decode()


def test_model_create_sequence_limits():
    assert _create(image_size=336, patch=14)[0] == 0                   # 24 x 24 + 1 = 577 tokens
    assert _create(image_size=448, patch=14)[0] == 0                   # 32 x 32 + 1 = 1025 = the limit
    rc, msg = _create(image_size=33 * 14, patch=14)                    # 33 x 33 + 1 = 1090 tokens
    assert rc != 0 and "1090" in msg and str(MAX_VISION_TOKENS) in msg
    rc, msg = _create(ctx=289)
    assert rc != 0 and "sequence length > 288 not supported" in msg
    assert _create(ctx=288)[0] == 0


def test_oracle_matches_transformers_beyond_288_tokens():
    transformers = pytest.importorskip("transformers")
    oa = dict(clip_ref.ARCHS["tiny"], image_size=144, patch=8, v_layers=1, t_layers=1)     # 18 x 18 + 1 = 325 tokens
    sd = clip_ref.random_state_dict(oa, seed=3)
    cfg = transformers.CLIPConfig(**clip_ref.hf_config_kwargs(oa))
    hf = transformers.CLIPModel(cfg).eval()
    missing, unexpected = hf.load_state_dict(clip_ref.to_hf_state_dict(sd, oa), strict=False)
    assert not [k for k in missing if "position_ids" not in k] and not unexpected
    px = torch.randn(2, 3, 144, 144, generator=torch.Generator().manual_seed(9))
    with torch.no_grad():
        ref = hf.get_image_features(pixel_values=px)
    if not isinstance(ref, torch.Tensor):
        ref = ref.pooler_output if getattr(ref, "pooler_output", None) is not None else ref[0]
    got = clip_ref.encode_image(sd, oa, px)
    assert float((got - ref).abs().max()) < 1e-5 * max(1.0, float(ref.abs().max()))
