"""Host side of the "fp32x3" encoder precision (KEMR_PREC_FP32X3 = 6, include/kemr.h): the names, the argument order of finalize's
checks, the workspace the mode asks for, and the fixture of tests/test_fp32x3_gpu.py.  No GPU."""
import ctypes as C
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

from knowledge_enhanced_multimodal_retrieval_amd import _lib, engine
from knowledge_enhanced_multimodal_retrieval_amd.config import ARCHS
from oracle import clip_ref

HERE = os.path.dirname(os.path.abspath(__file__))


def _model(name="tiny"):
    h = C.c_void_p()
    cfg = _lib.KemrCfg(**ARCHS[name].as_dict())
    assert _lib.lib().kemr_model_create(C.byref(cfg), C.byref(h)) == 0
    return h


def test_the_names():
    assert _lib.PREC_FP32X3 == 6 and _lib.PRECISIONS["fp32x3"] == 6
    assert sorted(set(_lib.PRECISIONS.values())) == [1, 2, 3, 4, 5, 6]
    for name in ("kemr_op_layernorm_x3", "kemr_op_gemm_x3", "kemr_op_attention_x3"):
        assert name in _lib.SIGNATURES and hasattr(_lib.lib(), name)
    assert _lib.lib().kemr_abi_version() == 4


def test_finalize_checks_the_precision_before_the_keys():
    """Precision 6 is a precision: a model with missing keys is KEMR_ERR_STATE (-2), refused before any GPU work; 7 and above,
    and 0, stay KEMR_ERR_INVALID (-1) -- the precision check comes first."""
    lib = _lib.lib()
    h = _model()
    try:
        assert lib.kemr_model_finalize(h, 6) == -2 and b"missing key" in lib.kemr_last_error()
        for bad in (7, 8, 0, -1):
            assert lib.kemr_model_finalize(h, bad) == -1 and b"unsupported precision" in lib.kemr_last_error(), bad
        assert lib.kemr_model_finalize(h, _lib.PREC_BF16) == -2
    finally:
        lib.kemr_model_destroy(h)


def test_the_environment_and_the_engine_accept_the_name(monkeypatch):
    """KEMR_PRECISION is read in one place (what clip.load / load_clip_model pack with and what the evaluator CLIs record)."""
    monkeypatch.setenv("KEMR_PRECISION", "fp32x3")
    assert _lib.env_precision() == "fp32x3"
    monkeypatch.setenv("KEMR_PRECISION", "fp32")
    with pytest.raises(ValueError, match="fp32x3"):
        _lib.env_precision()
    monkeypatch.delenv("KEMR_PRECISION")
    assert _lib.env_precision() == _lib.DEFAULT_PRECISION
    assert _lib.env_precision({"KEMR_PRECISION": "fp32x3"}) == "fp32x3" and _lib.env_precision({"KEMR_PRECISION": ""}) == _lib.DEFAULT_PRECISION
    # the engine's own check runs before it touches a device
    with pytest.raises(ValueError, match="fp32x3"):
        engine.ClipEngine(ARCHS["tiny"], "cuda:0", precision="fp32x4")
    with pytest.raises(RuntimeError, match="GPU"):
        engine.ClipEngine(ARCHS["tiny"], "cpu", precision="fp32x3")


def x3_workspace_bytes(width, rows):
    """include/kemr.h / csrc/encode.hip ws_layout_x3: per row of the ceil256(rows) allocated, x fp32 [W], h bf16 [3W], qkv fp32 [3W], hidden bf16 [12W]."""
    mp = (rows + 255) // 256 * 256
    return mp * width * (4 + 3 * 2 + 3 * 4 + 12 * 2)


@pytest.mark.parametrize("name", ["tiny", "tiny-long", "ViT-B/32", "ViT-L/14", "ViT-L/14@336px"])
def test_the_modes_workspace_is_at_least_the_defaults(name):
    """A model that is not finalized reports the default layout's size (what precision 1 needs); the size precision 6 needs, from the
    documented layout, is never smaller -- a caller that sizes for "fp32x3" can run every mode (the GPU test holds the library to
    this formula on a finalized model)."""
    lib = _lib.lib()
    a = ARCHS[name]
    h = _model(name)
    try:
        for batch in (1, 3, 64, 255):
            assert x3_workspace_bytes(a.v_width, batch * a.v_tokens) >= lib.kemr_workspace_bytes(h, _lib.TOWER_VISION, batch) > 0
            assert x3_workspace_bytes(a.t_width, batch * a.ctx) >= lib.kemr_workspace_bytes(h, _lib.TOWER_TEXT, batch) > 0
            rows = batch * 9
            assert x3_workspace_bytes(a.t_width, rows) + 256 * (((batch + 1) * 4 + 255) // 256) >= lib.kemr_text_packed_workspace_bytes(h, rows, batch) > 0
    finally:
        lib.kemr_model_destroy(h)


def test_the_heavy_fixture_holds_what_its_generator_says():
    """tests/golden/fp32x3_heavy_ViT-B-32.npz: the weights rebuilt from the seeds have the stored abs-sums, and the preconditions
    of the regime test hold on the stored numbers: bf16 operands outside 1e-3, the two-term split inside."""
    spec = importlib.util.spec_from_file_location("make_golden_fp32x3", os.path.join(HERE, "golden", "make_golden_fp32x3.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    z = np.load(gen.fixture_path())
    meta = json.loads(bytes(z["meta_json"]).decode())
    arch = clip_ref.ARCHS[gen.NAME]
    sd = gen.heavy_state_dict(arch, tuple(meta["gains"]), meta["weight_seed"])
    assert sorted(sd) == sorted(meta["weight_abs_sums"])
    for k, v in meta["weight_abs_sums"].items():
        assert float(sd[k].double().abs().sum()) == pytest.approx(v, rel=1e-12), k
    px, ids = gen.fixture_inputs(arch, meta["n_images"], meta["n_texts"])
    assert float(px.double().abs().sum()) == pytest.approx(meta["pixel_abs_sum"], rel=1e-12) and np.array_equal(ids.numpy(), z["ids"])
    assert z["image_features"].shape == (4, 512) and z["text_features"].shape == (8, 512)
    assert float(z["bf16_image"].max()) > 1e-3 and float(z["bf16_text"].max()) > 1e-3
    assert float(z["split2_image"].max()) < 1e-7 and float(z["split2_text"].max()) < 1e-3
    # the two-term rounding keeps 16 bits: |split2(t) - t| <= 2^-16 |t|
    t = torch.randn(4096, generator=torch.Generator().manual_seed(3)) * 100
    assert float(((gen.split2(t) - t).abs() / t.abs()).max()) <= 2.0 ** -16
