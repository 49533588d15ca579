"""Host: Long-CLIP above the library -- the model names, the fold of its two positional tables, Hugging Face directories with 248 text
positions, the context-length tokenizer, and the packed call's refusals for the other model families.  No GPU."""
import ctypes as C
import gzip
import pickle

import pytest
import torch

import longclip_ref as L
from knowledge_enhanced_multimodal_retrieval_amd import _lib, clip_api, config, evaluators, hf_checkpoint, tokenizer
from knowledge_enhanced_multimodal_retrieval_amd.clip_module import CLIP
from oracle import clip_ref


# ------------------------------------------------------------------------------------------------ names
def test_model_names_and_architectures():
    names = clip_api.available_models()
    assert "LongCLIP-B" in names and "LongCLIP-L" in names
    assert names[:5] == ["ViT-B/32", "ViT-B/16", "ViT-L/14", "ViT-L/14@336px", "ViT-H-14"]
    for long_name, base in (("LongCLIP-B", "ViT-B/16"), ("LongCLIP-L", "ViT-L/14")):
        a, b = config.get_arch(long_name), config.get_arch(base)
        assert a.ctx == 248 and b.ctx == 77
        assert {k: v for k, v in a.cfg_dict().items() if k != "ctx"} == {k: v for k, v in b.cfg_dict().items() if k != "ctx"}
        assert a.family == "clip" and a.v_head_dim == 64
    tiny, t0 = config.get_arch("tiny-ctx248"), config.get_arch("tiny")
    assert tiny.ctx == 248 and tiny.ctx <= 288 and {**t0.cfg_dict(), "ctx": 248} == tiny.cfg_dict()


def test_name_at_path_loads_a_released_state_dict(tmp_path):
    """clip.load("<name>@<path>") on a file with both positional tables (the released form) and on an already folded one."""
    sd = _released(seed=4)
    p = tmp_path / "longclip-tiny.pt"
    torch.save(sd, p)
    model, _ = clip_api.load(f"tiny-ctx248@{p}", device="cpu")
    assert model.arch.ctx == 248 and model.context_length == 248 and tuple(model.positional_embedding.shape) == (248, 256)
    want = torch.cat([sd["positional_embedding"][:20], sd["positional_embedding_res"][20:]])
    assert torch.equal(model.positional_embedding.detach(), want)
    torch.save(hf_checkpoint.fold_longclip_positions(sd), p)
    again, _ = clip_api.load(f"tiny-ctx248@{p}", device="cpu")
    assert torch.equal(again.positional_embedding.detach(), want)


# ------------------------------------------------------------------------------------------------ the positional tables
def _released(seed=4):
    """A state dict in the form of Long-CLIP's released files: OpenAI names, two positional tables [248, W]."""
    sd = {k: v.clone() for k, v in clip_ref.random_state_dict(L.ORACLE_ARCH, seed=seed).items()}
    sd["positional_embedding_res"] = torch.randn(248, 256, generator=torch.Generator().manual_seed(seed + 1)) * 0.01
    return sd


def test_fold_is_the_masked_sum_of_the_two_tables():
    sd = _released()
    out = hf_checkpoint.fold_longclip_positions(sd)
    pos, res = sd["positional_embedding"], sd["positional_embedding_res"]
    assert "positional_embedding_res" not in out and "positional_embedding_res" in sd           # the input is left as it was
    assert torch.equal(out["positional_embedding"], torch.cat([pos[:20], res[20:]]))
    # the published forward: pos * mask1 + pos_res * mask2, mask1 = 1 on 0 .. 19, mask2 = 1 on 20 .. 247
    m1 = (torch.arange(248) < 20).float()[:, None]
    assert torch.equal(out["positional_embedding"], pos * m1 + res * (1 - m1))
    assert torch.equal(hf_checkpoint.fold_longclip_positions(sd, keep=0)["positional_embedding"], res)
    assert torch.equal(hf_checkpoint.fold_longclip_positions(sd, keep=248)["positional_embedding"], pos)
    assert all(torch.equal(out[k], v) for k, v in sd.items() if not k.startswith("positional_embedding"))
    # without the second table: any CLIP dict, a folded one included, comes back unchanged
    again = hf_checkpoint.fold_longclip_positions(out)
    assert set(again) == set(out) and all(again[k] is out[k] for k in out)


def test_fold_refusals_name_both_shapes():
    sd = _released()
    sd["positional_embedding_res"] = sd["positional_embedding_res"][:77]
    with pytest.raises(ValueError, match=r"\(248, 256\).*\(77, 256\)"):
        hf_checkpoint.fold_longclip_positions(sd)
    sd = _released()
    with pytest.raises(ValueError, match=r"\(248, 256\).*\(248, 256\).*77"):                 # both tables 248 long, the architecture 77
        hf_checkpoint.fold_longclip_positions(sd, ctx=77)
    with pytest.raises((KeyError, ValueError), match=r"\(248, 256\)"):                       # a strict load into a 77-position model says the same
        CLIP(config.ClipArch(128, 32, 8, 256, 2, 256, 2, vocab=512, ctx=77)).load_state_dict(sd, strict=True)
    del sd["positional_embedding"]
    with pytest.raises(KeyError, match="positional_embedding"):
        hf_checkpoint.fold_longclip_positions(sd)


def test_folded_dict_loads_strictly():
    sd = _released()
    model = CLIP(L.ARCH)
    with pytest.raises(RuntimeError, match="positional_embedding_res"):                      # what torch's strict load says of the raw dict
        torch.nn.Module.load_state_dict(model, sd, strict=True)
    res = model.load_state_dict(hf_checkpoint.fold_longclip_positions(sd), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert tuple(model.positional_embedding.shape) == (248, 256)
    other = CLIP(L.ARCH)
    other.load_state_dict(sd, strict=True)                                                   # the model folds a released dict by itself
    assert torch.equal(other.positional_embedding, model.positional_embedding)


# ------------------------------------------------------------------------------------------------ Hugging Face directories
def test_hf_directory_with_248_positions_round_trips(tmp_path):
    transformers = pytest.importorskip("transformers")
    sd = clip_ref.random_state_dict(L.ORACLE_ARCH, seed=6)
    hf = transformers.CLIPModel(transformers.CLIPConfig(**clip_ref.hf_config_kwargs(L.ORACLE_ARCH))).eval()
    missing, unexpected = hf.load_state_dict(clip_ref.to_hf_state_dict(sd, L.ORACLE_ARCH), strict=False)
    assert not [k for k in missing if "position_ids" not in k] and not unexpected
    d = str(tmp_path / "longclip-hf")
    hf.save_pretrained(d)
    arch, act, got = hf_checkpoint.read_hf_directory(d)
    assert arch.ctx == 248 and arch == L.ARCH and act == "quick_gelu"
    assert tuple(got["positional_embedding"].shape) == (248, 256) and torch.equal(got["positional_embedding"], sd["positional_embedding"])
    model, _ = clip_api.load(d, device="cpu")
    assert model.arch.ctx == 248 and model.model_name == "tiny-ctx248" and tuple(model.positional_embedding.shape) == (248, 256)
    assert CLIP.from_pretrained(d, device="cpu").context_length == 248


# ------------------------------------------------------------------------------------------------ tokenizer
@pytest.fixture()
def small_bpe(tmp_path, monkeypatch):
    """The synthetic merge table of tests/test_host_logic.py as the process's BPE vocabulary."""
    merges = ["#version: test"] + ["a b", "ab c</w>", "d e</w>"] + [f"x{i} y{i}" for i in range(49152 - 256 - 2 - 3)]
    p = tmp_path / "bpe.txt.gz"
    with gzip.open(p, "wt", encoding="utf-8") as f:
        f.write("\n".join(merges))
    monkeypatch.setenv("KEMR_BPE_VOCAB", str(p))
    monkeypatch.setattr(tokenizer, "_tokenizer", None)
    yield str(p)
    tokenizer._tokenizer = None


def test_tokenizer_follows_the_context_length(small_bpe):
    model = CLIP(L.ARCH)
    fn = evaluators.model_tokenize(model)
    assert fn is not evaluators.default_tokenize and fn.context_length == 248
    ids = fn(["abc de", "abc " * 400, "de"])
    assert ids.dtype == torch.int32 and tuple(ids.shape) == (3, 248)
    assert ids[0, 0] == tokenizer.SOT and ids[0, 3] == tokenizer.EOT and not bool(ids[0, 4:].any())
    assert ids[1, 247] == tokenizer.EOT and int((ids[1] == tokenizer.EOT).sum()) == 1        # cut: ends in EOT, no padding
    assert torch.equal(ids, tokenizer.tokenize(["abc de", "abc " * 400, "de"], context_length=248, truncate=True))
    assert torch.equal(fn("abc de"), ids[:1])
    back = pickle.loads(pickle.dumps(fn))
    assert back == fn and torch.equal(back(["abc de", "abc " * 400, "de"]), ids)
    name = evaluators.model_tokenizer_name(model)
    assert "248" in name and small_bpe in name
    # 77 positions: default_tokenize ITSELF (model_tokenizer_name compares by identity), [B, 77] as ever
    m77 = CLIP(config.get_arch("tiny-long"))
    assert evaluators.model_tokenize(m77) is evaluators.default_tokenize
    assert tuple(evaluators.model_tokenize(m77)(["abc"]).shape) == (1, 77)
    assert evaluators.model_tokenizer_name(m77) == tokenizer.tokenizer_name()
    for public in ("LongCLIP-B", "LongCLIP-L"):
        assert evaluators.model_tokenize(type("M", (), {"arch": config.get_arch(public)})()).context_length == 248


# ------------------------------------------------------------------------------------------------ the other families
def _model(cfg, family=None, option=None):
    lib = _lib.lib()
    h = C.c_void_p()
    c = _lib.KemrCfg(**cfg)
    if family is None:
        assert lib.kemr_model_create(C.byref(c), C.byref(h)) == 0
    else:
        assert lib.kemr_model_create_family(C.byref(c), family, C.byref(h)) == 0
    if option is not None:
        assert lib.kemr_model_set_option(h, b"family", option) == 0
    return h


def test_packed_call_refusals_of_the_other_families_are_unchanged():
    """Families 1 to 3: the packed call (and its pooled form) answers what it answered before, before any argument is looked at beyond
    the model -- no GPU is touched.  Family 2 / 3 are served packed: what they refuse is the pooled form and the dense call."""
    lib = _lib.lib()
    ids = (C.c_int32 * 512)()
    out = (C.c_float * 1024)()
    p = lambda x: C.cast(x, C.c_void_p)                   # noqa: E731

    def packed(h, pooled=False):
        if pooled:
            rc = lib.kemr_encode_text_packed_pooled(h, p(ids), p(ids), 1, 1, p(out), None, 0, None)
        else:
            rc = lib.kemr_encode_text_packed(h, p(ids), p(ids), 1, 1, p(out), 0, None, 0, None)
        return rc, (lib.kemr_last_error() or b"").decode()

    siglip = _model(config.get_arch("tiny-siglip").cfg_dict(), option=1)
    rc, msg = packed(siglip)
    assert rc == -1 and msg == ("encode_text_packed: not available for family 1 (SigLIP): its text tower is unmasked and pools the last "
                                "position, so a pad position is a key and no row can be left out")
    rc, msg = packed(siglip, pooled=True)
    assert rc == -1 and msg.startswith("encode_text_packed_pooled: not available for family 1 (SigLIP)")
    for option in (None, _lib.FAMILY_MPNET):
        bert = _model(config.BERT_ARCHS["tiny-bert"].cfg_dict(), family=_lib.FAMILY_BERT, option=option)
        rc, msg = packed(bert, pooled=True)
        assert rc == -1 and msg == "encode_text_packed_pooled: not available for family 2 (BERT): a sentence encoder has no projection head"
        rc = lib.kemr_encode_text(bert, p(ids), 1, p(out), 0, None, 0, None)
        assert rc == -1 and (lib.kemr_last_error() or b"").decode().startswith("encode_text: not available for family 2 (BERT)")
        rc, msg = packed(bert)                                            # served: the refusal left is the state, not the family
        assert rc != 0 and "not finalized" in msg
        lib.kemr_model_destroy(bert)
    lib.kemr_model_destroy(siglip)
    # family 0 at ctx 248: the packed call's own refusal is gone (an unfinalized model is what is left to say)
    clip248 = _model(L.ARCH.cfg_dict())
    rc, msg = packed(clip248)
    assert rc != 0 and "not finalized" in msg and "128" not in msg
    lib.kemr_model_destroy(clip248)
