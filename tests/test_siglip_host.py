"""CPU: the SigLIP family -- architectures and names, the fp64 statement of tests/siglip_ref.py against transformers.SiglipModel, the
Hugging Face directory route both ways round, every refusal (config fields, model option "family", finalize, the packed text entry
point), the tokenizer callable and the image transform, and the proof that the parity bar of tests/test_siglip_tower_gpu.py can fail:
every CLIP behaviour the family must not have misses the right statement by more than 1e-2 on the weights and inputs those tests use."""
import ctypes as C
import json
import os
import types

import numpy as np
import pytest
import torch
import transformers

import siglip_ref as S
from knowledge_enhanced_multimodal_retrieval_amd import _lib, clip_api, config, hf_checkpoint, preprocess, tokenizer
from knowledge_enhanced_multimodal_retrieval_amd.clip_module import CLIP, SigLIP
from knowledge_enhanced_multimodal_retrieval_amd.config import ARCHS, ClipArch

WRONG_BAR = 1e-2           # ten times the parity bar of the GPU tests (1e-3)
TINY = ARCHS["tiny-siglip"]


# ------------------------------------------------------------------------------------------------ architectures
def test_siglip_archs_are_registered():
    want = {"ViT-B-16-SigLIP": (224, 768, 12, 196), "ViT-B-16-SigLIP-256": (256, 768, 12, 256), "ViT-B-16-SigLIP-384": (384, 768, 12, 576),
            "ViT-B-16-SigLIP-512": (512, 768, 12, 1024), "ViT-L-16-SigLIP-256": (256, 1024, 24, 256), "ViT-L-16-SigLIP-384": (384, 1024, 24, 576)}
    for name, (size, width, layers, tokens) in want.items():
        a = config.get_arch(name)
        assert (a.family, a.image_size, a.patch, a.v_width, a.t_width, a.v_layers, a.t_layers) == ("siglip", size, 16, width, width, layers, layers)
        assert (a.embed_dim, a.vocab, a.ctx, a.v_tokens, a.v_head_dim) == (width, 32000, 64, tokens, 64)
        assert name in clip_api.available_models()
        assert a.as_dict()["family"] == "siglip" and sorted(a.cfg_dict()) == sorted(n for n, _ in _lib.KemrCfg._fields_)
    for name, size, tokens in (("tiny-siglip", 64, 16), ("tiny-siglip-196", 224, 196), ("tiny-siglip-576", 384, 576)):
        a = ARCHS[name]
        assert (a.family, a.image_size, a.patch, a.v_tokens, a.v_width, a.t_width, a.v_layers, a.t_layers, a.vocab, a.ctx) == \
            ("siglip", size, 16, tokens, 256, 256, 2, 2, 512, 16)
    with pytest.raises(ValueError, match="family"):
        ClipArch(256, 64, 16, 256, 2, 256, 2, family="siglip2")
    with pytest.raises(ValueError, match="embed_dim"):
        ClipArch(128, 64, 16, 256, 2, 256, 2, family="siglip")


def test_clip_archs_did_not_grow():
    for name, a in ARCHS.items():
        if a.family == "clip":
            assert "family" not in a.as_dict() and "family" not in a.cfg_dict()
            assert a.v_tokens == a.grid ** 2 + 1
    assert list(ARCHS["ViT-L/14"].as_dict()) == ["embed_dim", "image_size", "patch", "v_width", "v_layers", "t_width", "t_layers", "vocab", "ctx"]
    assert clip_api.available_models()[:5] == ["ViT-B/32", "ViT-B/16", "ViT-L/14", "ViT-L/14@336px", "ViT-H-14"]


# ------------------------------------------------------------------------------------------------ the statement against transformers
def _hf_model(arch, sd):
    model = transformers.SiglipModel(transformers.SiglipConfig(**S.hf_config_kwargs(arch), attn_implementation="eager")).eval()
    missing, unexpected = model.load_state_dict(hf_checkpoint.to_siglip_state_dict(sd, arch), strict=False)
    assert not [k for k in missing if "position_ids" not in k] and not unexpected
    return model


def _features(model, px, ids):
    with torch.no_grad():
        i = model.get_image_features(pixel_values=px)
        t = model.get_text_features(input_ids=ids.long())
    return (i if torch.is_tensor(i) else i.pooler_output), (t if torch.is_tensor(t) else t.pooler_output)


def test_fp64_statement_against_transformers():
    """transformers.SiglipModel built from a config, the weights through the key map: image and text embeddings to 1e-5 of their
    largest element (the tolerance of tests/test_headdim_host.py for the CLIP statement against CLIPModel)."""
    sd = S.weights(TINY)
    px, ids = S.pixels(TINY, 3), S.text_ids(TINY, 5)
    hf_i, hf_t = _features(_hf_model(TINY, sd), px, ids)
    for got, ref in ((hf_i, S.encode_image(sd, TINY, px)), (hf_t, S.encode_text(sd, TINY, ids))):
        assert float((got.double() - ref).abs().max() / ref.abs().max()) <= 1e-5


def test_tanh_gelu_is_the_sigmoid_form():
    x = torch.linspace(-12, 12, 100001, dtype=torch.float64)
    sig = x * torch.sigmoid(2.0 * (2.0 / torch.pi) ** 0.5 * (x + 0.044715 * x ** 3))
    assert float((S.act64(x) - sig).abs().max()) <= 4e-15
    assert float((S.act64(x) - torch.nn.functional.gelu(x, approximate="tanh")).abs().max()) <= 4e-15


# ------------------------------------------------------------------------------------------------ Hugging Face directories
@pytest.mark.parametrize("fmt", ["safetensors", "bin"])
def test_hf_directory_round_trip(tmp_path, fmt):
    sd = S.weights(TINY)
    model = _hf_model(TINY, sd)
    d = str(tmp_path / fmt)
    if fmt == "safetensors":
        model.save_pretrained(d, safe_serialization=True)
        assert os.path.isfile(os.path.join(d, "model.safetensors"))
    else:
        os.makedirs(d)
        torch.save(model.state_dict(), os.path.join(d, "pytorch_model.bin"))
        with open(os.path.join(d, "config.json"), "w") as f:
            f.write(model.config.to_json_string())
    arch, act, got = hf_checkpoint.read_hf_directory(d)
    assert arch == TINY and act == "gelu_pytorch_tanh"
    assert set(got) == set(sd) and all(torch.equal(got[k], sd[k]) for k in sd)
    back = hf_checkpoint.to_siglip_state_dict(got, arch)
    hf_sd = {k: v for k, v in model.state_dict().items() if not k.endswith("position_ids")}
    assert set(back) == set(hf_sd) and all(torch.equal(back[k], hf_sd[k]) for k in hf_sd)
    m, pre = clip_api.load(d, device="cpu")
    assert isinstance(m, SigLIP) and isinstance(pre, preprocess.SiglipPreprocess) and pre.n_px == TINY.image_size
    assert m.arch == TINY and m.model_name == "tiny-siglip" and m.weights_source == os.path.abspath(d)
    mine = m.state_dict()
    assert set(mine) == set(sd) and all(torch.equal(mine[k], sd[k]) for k in sd)
    m2, pre2 = SigLIP.from_pretrained(d, device="cpu")
    assert isinstance(m2, SigLIP) and pre2.n_px == pre.n_px
    with pytest.raises(ValueError, match="activation"):
        clip_api.load(d, device="cpu", activation="gelu")
    with pytest.raises(RuntimeError, match="GPU"):
        m.encode_text(S.text_ids(TINY, 1))


def test_module_is_strict_and_copies_get_their_own_handle():
    import copy
    import pickle
    m = SigLIP(TINY, "tiny-siglip").eval().float()
    assert set(m.state_dict()) == set(S.tensor_shapes(TINY)) | {"logit_scale", "logit_bias"}
    assert {k: tuple(v.shape) for k, v in m.state_dict().items() if k in S.tensor_shapes(TINY)} == S.tensor_shapes(TINY)
    sd = S.weights(TINY)
    m.load_state_dict(sd, strict=True)
    with pytest.raises(RuntimeError, match="Unexpected key"):
        m.load_state_dict({**sd, "visual.class_embedding": torch.zeros(256)}, strict=True)
    with pytest.raises(RuntimeError, match="Missing key"):
        m.load_state_dict({k: v for k, v in sd.items() if k != "visual.conv1.bias"}, strict=True)
    for c in (copy.deepcopy(m), pickle.loads(pickle.dumps(m))):
        assert c._engine is None and c._dirty and all(torch.equal(a, b) for a, b in zip(c.state_dict().values(), m.state_dict().values()))
    with pytest.raises(ValueError, match="family"):
        SigLIP(ARCHS["tiny"])
    with pytest.raises(ValueError, match="quick_gelu.*gelu"):
        CLIP(ARCHS["tiny"], activation="gelu_pytorch_tanh")          # not an option of the CLIP module


def _cfg(**edits):
    kw = S.hf_config_kwargs(ARCHS["ViT-B-16-SigLIP"])
    kw["model_type"] = "siglip"
    for path, v in edits.items():
        side, field = path.split("__")
        kw[side][field] = v
    return kw


def test_config_refusals_name_their_field():
    assert hf_checkpoint.arch_from_siglip_config(_cfg()) == ARCHS["ViT-B-16-SigLIP"]
    assert hf_checkpoint.arch_from_siglip_config(_cfg(vision_config__image_size=384)) == ARCHS["ViT-B-16-SigLIP-384"]
    assert hf_checkpoint.arch_from_siglip_config({"text_config": {}, "vision_config": {}}) == ARCHS["ViT-B-16-SigLIP"]      # transformers' defaults
    so400m = dict(vision_config__hidden_size=1152, vision_config__num_attention_heads=16, vision_config__intermediate_size=4304)
    cases = [(so400m, "vision_config.hidden_size"),
             (dict(vision_config__hidden_size=1024, vision_config__intermediate_size=4096, vision_config__num_attention_heads=12), "vision_config.num_attention_heads"),
             (dict(text_config__num_attention_heads=16), "text_config.num_attention_heads"),
             (dict(text_config__intermediate_size=3000), "text_config.intermediate_size"),
             (dict(vision_config__hidden_act="gelu"), "vision_config.hidden_act"),
             (dict(text_config__hidden_act="quick_gelu"), "text_config.hidden_act"),
             (dict(text_config__layer_norm_eps=1e-5), "text_config.layer_norm_eps"),
             (dict(vision_config__layer_norm_eps=1e-12), "vision_config.layer_norm_eps"),
             (dict(vision_config__vision_use_head=False), "vision_config.vision_use_head"),
             (dict(text_config__projection_size=512), "text_config.projection_size"),
             (dict(vision_config__image_size=230), "vision_config.image_size")]
    for edits, field in cases:
        with pytest.raises(ValueError) as e:
            hf_checkpoint.arch_from_siglip_config(_cfg(**edits))
        assert field in str(e.value), (field, str(e.value))
    heads72 = dict(vision_config__hidden_size=1152 + 128, vision_config__num_attention_heads=16, vision_config__intermediate_size=4 * 1280)
    with pytest.raises(ValueError, match="num_attention_heads.*head dim of 80"):
        hf_checkpoint.arch_from_siglip_config(_cfg(**heads72))
    # the CLIP route and its refusals are untouched: a CLIPModel config with SigLIP's activation, or gelu_new, is still refused there
    from oracle import clip_ref
    kw = clip_ref.hf_config_kwargs(ARCHS["tiny"].cfg_dict())
    for act in ("gelu_new", "gelu_pytorch_tanh"):
        kw["text_config"]["hidden_act"] = kw["vision_config"]["hidden_act"] = act
        with pytest.raises(ValueError, match="hidden_act"):
            hf_checkpoint.arch_and_activation_from_hf_config(kw)


# ------------------------------------------------------------------------------------------------ the C ABI on the host
def _create(name="tiny-siglip", family=None):
    lib = _lib.lib()
    h = C.c_void_p()
    assert lib.kemr_model_create(C.byref(_lib.KemrCfg(**ARCHS[name].cfg_dict())), C.byref(h)) == 0
    if family is not None:
        assert lib.kemr_model_set_option(h, b"family", family) == 0, lib.kemr_last_error()
    return lib, h


def _names(lib, h):
    return [lib.kemr_model_tensor_name(h, i).decode() for i in range(lib.kemr_model_num_tensors(h))]


def _load(lib, h, name, shape):
    t = torch.zeros(shape)
    dims = (C.c_int64 * len(shape))(*shape)
    return lib.kemr_model_load_tensor(h, name.encode(), C.c_void_p(t.data_ptr()), _lib.KEMR_F32, dims, len(shape))


def test_family_option_rebuilds_the_name_list():
    lib, h = _create()
    v = C.c_int(-1)
    assert lib.kemr_abi_version() == 4
    assert lib.kemr_model_get_option(h, b"family", C.byref(v)) == 0 and v.value == 0
    clip_names = _names(lib, h)
    assert "visual.class_embedding" in clip_names and "visual.conv1.bias" not in clip_names
    assert set(clip_names) == set(CLIP(TINY.__class__(**{**TINY.cfg_dict()})).state_dict()) - {"logit_scale"}
    for bad in (-1, 2):
        assert lib.kemr_model_set_option(h, b"family", bad) == -1 and b"0 (CLIP) or 1 (SigLIP)" in lib.kemr_last_error()
    assert lib.kemr_model_set_option(h, b"family", 1) == 0
    assert lib.kemr_model_get_option(h, b"family", C.byref(v)) == 0 and v.value == 1
    names = _names(lib, h)
    assert set(names) == set(S.tensor_shapes(TINY)) and len(names) == len(set(names))
    for gone in ("visual.class_embedding", "visual.ln_pre.weight", "visual.ln_pre.bias", "visual.proj"):
        assert gone not in names
    # shapes: the positional table has one row per patch; logit_bias is ignored like logit_scale; strictness otherwise
    assert _load(lib, h, "visual.positional_embedding", (17, 256)) == -1 and b"size mismatch" in lib.kemr_last_error()
    assert _load(lib, h, "logit_bias", (1,)) == 0 and _load(lib, h, "logit_scale", (1,)) == 0
    assert lib.kemr_model_set_option(h, b"family", 0) == 0 and lib.kemr_model_set_option(h, b"family", 1) == 0      # nothing stored yet
    assert _load(lib, h, "visual.class_embedding", (256,)) == -1 and b"unexpected key" in lib.kemr_last_error()
    assert _load(lib, h, "visual.positional_embedding", (16, 256)) == 0
    for value in (0, 1):
        assert lib.kemr_model_set_option(h, b"family", value) == -2 and b"before the first kemr_model_load_tensor" in lib.kemr_last_error()
    assert _names(lib, h) == names
    lib.kemr_model_destroy(h)
    lib, h = _create()                                      # a CLIP model: a stray logit_bias is still an unexpected key
    assert _load(lib, h, "logit_bias", (1,)) == -1 and b"unexpected key" in lib.kemr_last_error()
    lib.kemr_model_destroy(h)


def test_family_refusals_before_any_gpu_work():
    lib, h = _create(family=1)
    for prec in (_lib.PREC_FP8, _lib.PREC_FP8_MLP, _lib.PREC_FP8_RES16):
        assert lib.kemr_model_finalize(h, prec) == -1 and b"fp8" in lib.kemr_last_error() and b"family 1" in lib.kemr_last_error()
    assert lib.kemr_model_finalize(h, _lib.PREC_FP32X3) == -1 and b"KEMR_PREC_FP32X3" in lib.kemr_last_error() and b"family 1" in lib.kemr_last_error()
    assert lib.kemr_model_finalize(h, _lib.PREC_BF16) == -2 and b"missing key 'visual.conv1.weight'" in lib.kemr_last_error()
    assert lib.kemr_model_set_option(h, b"vision_head_dim", 80) == -1 and b"vision_head_dim 64 only" in lib.kemr_last_error()
    assert lib.kemr_model_set_option(h, b"vision_head_dim", 64) == 0
    # option "activation": its range and message are what they were; in this family it is not consulted
    assert lib.kemr_model_set_option(h, b"activation", 2) == -1 and b"0 (QuickGELU) or 1 (GELU)" in lib.kemr_last_error()
    assert lib.kemr_model_set_option(h, b"activation", 1) == 0
    buf = (C.c_char * 256)()
    p = C.cast(buf, C.c_void_p)
    assert lib.kemr_encode_text_packed(h, p, p, 1, 1, p, 0, p, 256, None) == -1
    msg = lib.kemr_last_error()
    assert b"encode_text_packed" in msg and b"family 1" in msg and b"pad position is a key" in msg
    lib.kemr_model_destroy(h)
    lib, h = _create("tiny", family=1)                      # embed_dim 128 at v_width 256: the family has no vision projection
    assert lib.kemr_model_finalize(h, _lib.PREC_BF16) == -1 and b"embed_dim 128 must equal v_width 256" in lib.kemr_last_error()
    lib.kemr_model_destroy(h)
    lib, h = _create("tiny-h")
    assert lib.kemr_model_set_option(h, b"vision_head_dim", 80) == 0
    assert lib.kemr_model_set_option(h, b"family", 1) == -1 and b"vision_head_dim 64 only" in lib.kemr_last_error()
    lib.kemr_model_destroy(h)
    assert lib.kemr_op_gemm(p, p, None, p, 1, 100, 64, _lib.EPI_BIAS_TGELU_BF16, None) == -1 and b"N % 128" in lib.kemr_last_error()   # known epilogue: the shape is what is refused
    for bad in (3, 6, 7, 9):                                # 3 and 7 are internal to the library, 6 and 9 are no values
        assert lib.kemr_op_gemm(p, p, None, p, 1, 128, 64, bad, None) == -1 and b"bad epilogue" in lib.kemr_last_error()


# ------------------------------------------------------------------------------------------------ tokenizer and image transform
def _write_unigram(directory):
    from tokenizers import Tokenizer, decoders, models, pre_tokenizers
    words = ["a", "photo", "of", "cat", "dog", "the", "s"]
    vocab = [("<pad>", 0.0), ("</s>", 0.0), ("<unk>", 0.0), ("▁", -6.0)] + [("▁" + w, -2.0) for w in words] + \
        [(c, -5.0) for c in "abcdefghijklmnopqrstuvwxyz0123456789"]
    tok = Tokenizer(models.Unigram(vocab, unk_id=2))
    tok.pre_tokenizer = pre_tokenizers.Metaspace()
    tok.decoder = decoders.Metaspace()
    os.makedirs(directory, exist_ok=True)
    tok.save(os.path.join(directory, "tokenizer.json"))
    return {t: i for i, (t, _) in enumerate(vocab)}


def test_tokenize_callable(tmp_path):
    import pickle
    d = str(tmp_path / "tok")
    v = _write_unigram(d)
    fn = tokenizer.siglip_tokenizer(d)
    ids = fn(["A photo, of a CAT!!", "  the   dog's  ", ""])
    assert ids.dtype == torch.int32 and tuple(ids.shape) == (3, 64)
    w = lambda s: v["▁" + s]                                                  # noqa: E731
    assert ids[0, :6].tolist() == [w("a"), w("photo"), w("of"), w("a"), w("cat"), 1] and bool((ids[0, 6:] == 1).all())
    assert ids[1, :3].tolist()[:1] == [w("the")] and 1 in ids[1].tolist() and v["<unk>"] not in ids[1].tolist()      # "dogs": the apostrophe is stripped
    assert bool((ids[2] == 1).all())
    long = fn("a photo of a cat " * 40, )
    assert tuple(long.shape) == (1, 64) and int(long[0, -1]) == 1 and 1 not in long[0, :-1].tolist()                # cut to 64 keeping the EOS
    short = tokenizer.SiglipTokenize(d, context_length=16)("a cat")
    assert tuple(short.shape) == (1, 16) and short[0, :3].tolist() == [w("a"), w("cat"), 1]
    assert torch.equal(pickle.loads(pickle.dumps(fn))(["a dog"]), fn(["a dog"]))
    # canonicalisation is SiglipTokenizer.canonicalize_text's
    from transformers.models.siglip.tokenization_siglip import SiglipTokenizer
    fake = types.SimpleNamespace(do_lower_case=True)
    fake.remove_punctuation = lambda t: SiglipTokenizer.remove_punctuation(fake, t)
    for text in ("A photo, of a CAT!!", "  the   dog's\tbowl\n", "It's {} -- 50% off: [now]", "plain"):
        assert tokenizer.siglip_canonicalize(text) == SiglipTokenizer.canonicalize_text(fake, text)
    only_spm = tmp_path / "spm"
    only_spm.mkdir()
    (only_spm / "spiece.model").write_bytes(b"\x00")
    with pytest.raises(FileNotFoundError, match="sentencepiece"):
        tokenizer.siglip_tokenizer(str(only_spm))
    with pytest.raises(FileNotFoundError, match="tokenizer.json"):
        tokenizer.siglip_tokenizer(str(tmp_path / "nothing"))


def test_image_transform_against_siglip_image_processor():
    from PIL import Image
    img = Image.fromarray(np.random.default_rng(0).integers(0, 256, (150, 291, 3), dtype=np.uint8))      # not square: squashed, not cropped
    for n in (64, 224):
        proc = transformers.SiglipImageProcessor(size={"height": n, "width": n})
        want = proc(images=img, return_tensors="pt")["pixel_values"][0]
        got = preprocess.SiglipPreprocess(n)(img)
        assert got.dtype == torch.float32 and tuple(got.shape) == (3, n, n)
        assert float((got - want).abs().max()) <= 1e-6
        assert float(got.min()) >= -1.0 and float(got.max()) <= 1.0
    assert not preprocess.SiglipPreprocess(64).defer_to_gpu
    clip_api.allow_random_weights(True)
    try:
        with pytest.warns(RuntimeWarning, match="RANDOM weights"):
            model, pre = clip_api.load("tiny-siglip", device="cpu")
    finally:
        clip_api.allow_random_weights(False)
    assert isinstance(model, SigLIP)
    assert isinstance(pre, preprocess.SiglipPreprocess) and pre.n_px == 64


def test_a_models_default_tokenizer(tmp_path):
    """What encode_dataset / EmbeddingStore.build / CLIPRetriever / the CLIs tokenise with when no tokenize_fn is given: CLIP's BPE for a
    CLIP model; for a SigLIP model the tokenizer.json its tokenizer_dir names, and an error up front when it names none."""
    from knowledge_enhanced_multimodal_retrieval_amd import evaluators
    assert evaluators.model_tokenize(CLIP(ARCHS["tiny"])) is evaluators.default_tokenize
    assert evaluators.model_tokenize(object()) is evaluators.default_tokenize
    m = SigLIP(TINY, "tiny-siglip")
    with pytest.raises(RuntimeError, match="tokenizer.json.*--tokenizer_dir"):
        evaluators.model_tokenize(m)
    with pytest.raises(RuntimeError, match="tokenizer.json"):
        evaluators.model_tokenizer_name(m)
    d = str(tmp_path / "tok")
    v = _write_unigram(d)
    m.tokenizer_dir = d
    fn = evaluators.model_tokenize(m)
    ids = fn(["a photo of the cat"])
    assert tuple(ids.shape) == (1, TINY.ctx) and ids.dtype == torch.int32                      # the MODEL's context, not 64 or 77
    assert ids[0, :6].tolist() == [v["▁a"], v["▁photo"], v["▁of"], v["▁the"], v["▁cat"], 1]
    assert evaluators.model_tokenizer_name(m) == f"siglip tokenizers ({os.path.join(d, 'tokenizer.json')})"
    # a save_pretrained directory that ships its tokenizer.json binds it at load; one without leaves the attribute empty
    model = _hf_model(TINY, S.weights(TINY))
    for sub_dir, with_tok in (("with", True), ("without", False)):
        dd = str(tmp_path / sub_dir)
        model.save_pretrained(dd, safe_serialization=True)
        if with_tok:
            _write_unigram(dd)
        loaded, _ = clip_api.load(dd, device="cpu")
        assert loaded.tokenizer_dir == (os.path.abspath(dd) if with_tok else None)
    args = types.SimpleNamespace(tokenizer_dir=d, model_name="tiny")
    with pytest.raises(ValueError, match="--tokenizer_dir is for SigLIP models"):
        evaluators._bind_tokenizer(CLIP(ARCHS["tiny"]), args)
    evaluators._bind_tokenizer(loaded, args)
    assert loaded.tokenizer_dir == d
    with pytest.raises(RuntimeError, match="tokenizer.json"):
        evaluators._bind_tokenizer(SigLIP(TINY), types.SimpleNamespace(tokenizer_dir=None, model_name="tiny-siglip"))


# ------------------------------------------------------------------------------------------------ the bars can fail
@pytest.mark.parametrize("name,n", S.IMAGE_CASES)
def test_wrong_image_statements_miss_by_more_than_the_bar(name, n):
    """On the GPU tests' weights and pixels each CLIP behaviour is more than 1e-2 from the right statement; eps and the activation on
    their sharpened weights (siglip_ref.EPS_SHARPEN = 1.5e-3; ACT_SHIFT, ACT_FC, ACT_PROJ = -3, 0.3, 32)."""
    for switches, sharpening in S.WRONG_IMAGE:
        right = S.image_reference(name, n, sharpening)
        miss = float(S.one_minus_cos(right, S.image_reference(name, n, sharpening, **switches)).min())
        print(f"NUMERICS wrong_image {name} n{n} {switches} sharpened={sharpening} min 1-cos {miss:.3e}")
        assert miss > WRONG_BAR, (switches, sharpening, miss)


@pytest.mark.parametrize("ctx,n", S.TEXT_CASES)
def test_wrong_text_statements_miss_by_more_than_the_bar(ctx, n):
    """The same for the text tower (the causal mask on siglip_ref.CAUSAL_OUT = 4)."""
    for switches, sharpening in S.WRONG_TEXT:
        right = S.text_reference(ctx, n, sharpening)
        miss = float(S.one_minus_cos(right, S.text_reference(ctx, n, sharpening, **switches)).min())
        print(f"NUMERICS wrong_text ctx{ctx} n{n} {switches} sharpened={sharpening} min 1-cos {miss:.3e}")
        assert miss > WRONG_BAR, (switches, sharpening, miss)


def test_plain_weights_do_not_separate_eps_and_activation():
    """Why the sharpened cases exist: on the plain seeded weights eps 1e-5 and QuickGELU are below the PARITY bar, so a tower test on
    plain weights alone could not tell them from the right model."""
    right = S.image_reference("tiny-siglip", 3)
    for switches in (dict(eps=1e-5), dict(act="quick_gelu"), dict(act="gelu")):
        assert float(S.one_minus_cos(right, S.image_reference("tiny-siglip", 3, None, **switches)).max()) < 1e-3
