"""CPU: the BERT sentence encoders (model family 2) up to the device -- the CPU statement against ``transformers.BertModel``, the
checkpoint mapping and its refusals, the sentence-transformers files, the tokenizer, ``SentenceEncoder.encode``'s ordering, the
evaluator shims' arguments, and the library's host-side checks of ``kemr_model_create_family``.  No GPU call is made here."""
import ctypes as C
import json
import os
import re

import pytest
import torch

import bert_ref as B
from knowledge_enhanced_multimodal_retrieval_amd import _lib, hf_checkpoint, sentence_model, tokenizer
from knowledge_enhanced_multimodal_retrieval_amd.config import BERT_ARCHS, BertArch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sd():
    return B.cached("sd0", lambda: B.random_state_dict(B.ARCH, 0))


# ------------------------------------------------------------------------------------------------ the CPU statement
@pytest.mark.parametrize("pooling", ["mean", "cls"])
def test_bert_ref_equals_transformers(pooling):
    """bert_ref.encode (every text on its own length) against BertModel (eager attention, fp32) on the padded batch with its attention
    mask + sentence-transformers' pooling, on the length set of the GPU tests: <= 1e-5 absolute."""
    sd = _sd()
    ids, lens = B.random_ids(B.LENGTHS)
    ref = B.encode(sd, B.ARCH, ids, lens, pooling)
    hf = B.cached(("hf", pooling), lambda: B.hf_encode(B.hf_model(sd), ids, lens, pooling))
    err = float((ref - hf).abs().max())
    print(f"BERT bert_ref_vs_transformers_{pooling}_max_abs {err:.3g}")
    assert err <= 1e-5, err
    assert float(ref.abs().max()) > 0.5          # not a comparison of zeros


def test_bert_ref_does_not_depend_on_the_padding():
    sd = _sd()
    lens = [1, 5, 17, 64]
    ids, l = B.random_ids(lens, pad_to=64)
    wide = torch.full((len(lens), 512), 777, dtype=torch.int32)           # other ids behind every text
    wide[:, :64] = ids
    for i, n in enumerate(lens):
        wide[i, n:] = 777
    assert torch.equal(B.encode(sd, B.ARCH, ids, l), B.encode(sd, B.ARCH, wide, l))
    # and stock BertModel agrees: its output for a text is the same bits however far the batch is padded
    model = B.hf_model(sd)
    a, b = B.hf_encode(model, ids, l), B.hf_encode(model, torch.cat([ids, torch.zeros(4, 100, dtype=torch.int32)], 1), l)
    assert float((a - b).abs().max()) == 0.0


def test_the_wrong_models_miss_the_bar():
    """What the parity bar (1 - cos <= 1e-3) must tell apart: a pre-LN reading of the same weights, a forgotten token-type row, CLS
    instead of mean pooling -- each is beyond 1e-2 on the fixture's weights."""
    sd = _sd()
    ids, lens = B.random_ids([5, 17, 64, 129])
    ref = B.encode(sd, B.ARCH, ids, lens)
    no_type = dict(sd, token_type_embedding=torch.zeros_like(sd["token_type_embedding"]))
    assert float(B.one_minus_cos(B.encode(no_type, B.ARCH, ids, lens), ref).min()) > 1e-2
    assert float(B.one_minus_cos(B.encode(sd, B.ARCH, ids, lens, "cls"), ref).min()) > 1e-2


# ------------------------------------------------------------------------------------------------ checkpoint mapping
def test_state_dict_round_trip(tmp_path):
    sd = _sd()
    hf = hf_checkpoint.to_bert_state_dict(sd, B.ARCH)
    back = hf_checkpoint.from_bert_state_dict(hf, B.ARCH)
    assert sorted(back) == sorted(sd) == sorted(B.tensor_shapes())
    assert all(torch.equal(back[k], sd[k]) for k in sd)
    # `bert.`-prefixed keys, a pooler, a task head and the buffers are accepted / ignored
    pre = {f"bert.{k}": v for k, v in hf.items()}
    pre.update({"bert.pooler.dense.weight": torch.zeros(2, 2), "bert.embeddings.position_ids": torch.zeros(1, 512),
                "cls.predictions.bias": torch.zeros(3)})
    back = hf_checkpoint.from_bert_state_dict(pre, B.ARCH)
    assert all(torch.equal(back[k], sd[k]) for k in sd)
    with pytest.raises(KeyError, match="missing key 'encoder.layer.1.output.LayerNorm.bias'"):
        hf_checkpoint.from_bert_state_dict({k: v for k, v in hf.items() if k != "encoder.layer.1.output.LayerNorm.bias"}, B.ARCH)
    with pytest.raises(KeyError, match="unexpected key 'encoder.layer.2.x'"):
        hf_checkpoint.from_bert_state_dict(dict(hf, **{"encoder.layer.2.x": torch.zeros(1)}), B.ARCH)
    # a save_pretrained directory (with pooler) reads back to the same tensors and the architecture
    d = B.save_directory(tmp_path, sd)
    arch, act, got = hf_checkpoint.read_hf_directory(d)
    assert arch == B.ARCH and act == "gelu" and isinstance(arch, BertArch)
    assert sorted(got) == sorted(sd) and all(torch.equal(got[k], sd[k]) for k in sd)


def _cfg(**kw):
    cfg = json.loads(B.bert_config().to_json_string())
    cfg.update(kw)
    return cfg


@pytest.mark.parametrize("change,message", [
    (dict(model_type="mpnet"), "relative position bias"),
    (dict(position_embedding_type="relative_key"), "position_embedding_type = 'relative_key'"),
    (dict(hidden_size=384, num_attention_heads=6, intermediate_size=1536), "hidden_size = 384 is not a multiple of 256"),
    (dict(num_attention_heads=8), "head dim of 32"),
    (dict(intermediate_size=768), "intermediate_size = 768 is not 4 x hidden_size"),
    (dict(hidden_act="gelu_new"), "hidden_act = 'gelu_new'"),
    (dict(hidden_act="relu"), "hidden_act = 'relu'"),
    (dict(layer_norm_eps=1e-5), "layer_norm_eps"),
    (dict(max_position_embeddings=1024), "served up to 512"),
])
def test_config_refusals(change, message):
    with pytest.raises(ValueError, match=re.escape(message)):
        hf_checkpoint.arch_from_bert_config(_cfg(**change))


def test_named_checkpoints_are_plain_bert():
    """E5-base-v2 and GTE-large by their published config numbers."""
    e5 = hf_checkpoint.arch_from_bert_config(dict(model_type="bert", hidden_size=768, num_hidden_layers=12, num_attention_heads=12,
                                                  intermediate_size=3072, vocab_size=30522, max_position_embeddings=512, hidden_act="gelu"))
    gte = hf_checkpoint.arch_from_bert_config(dict(model_type="bert", hidden_size=1024, num_hidden_layers=24, num_attention_heads=16,
                                                   intermediate_size=4096, vocab_size=30522, max_position_embeddings=512, hidden_act="gelu"))
    assert e5 == BERT_ARCHS["e5-base-v2"] and gte == BERT_ARCHS["gte-large"]
    assert e5.cfg_dict() == dict(embed_dim=768, image_size=0, patch=0, v_width=0, v_layers=0, t_width=768, t_layers=12, vocab=30522, ctx=512)


def test_mpnet_directory_is_refused_with_the_reason(tmp_path):
    (tmp_path / "config.json").write_text(json.dumps(dict(model_type="mpnet", hidden_size=768)))
    (tmp_path / "model.safetensors").write_bytes(b"")
    with pytest.raises(ValueError, match="relative position bias"):
        hf_checkpoint.read_hf_directory(str(tmp_path))


def test_sentence_transformers_files_are_honoured(tmp_path):
    sd = _sd()
    plain = B.save_directory(tmp_path / "plain", sd)
    arch, _, _ = hf_checkpoint.read_hf_directory(plain)
    assert (arch.pooling, arch.ctx, arch.positions) == ("mean", 512, 0)
    st = B.save_directory(tmp_path / "st", sd, pooling="cls", max_seq_length=128)
    arch, _, got = hf_checkpoint.read_hf_directory(st)
    assert (arch.pooling, arch.ctx, arch.positions) == ("cls", 128, 512)
    assert got["positional_embedding"].shape == (128, 256) and torch.equal(got["positional_embedding"], sd["positional_embedding"][:128])
    assert hf_checkpoint.sentence_transformers_settings(B.save_directory(tmp_path / "mean", sd, pooling="mean")) == ("mean", 0)
    os.makedirs(tmp_path / "max" / "1_Pooling")
    (tmp_path / "max" / "1_Pooling" / "config.json").write_text(json.dumps({"pooling_mode_max_tokens": True}))
    with pytest.raises(ValueError, match="pooling_mode_max_tokens"):
        hf_checkpoint.sentence_transformers_settings(str(tmp_path / "max"))


# ------------------------------------------------------------------------------------------------ tokenizer
def test_tokenizer_equals_tokenizers_own(tmp_path):
    from tokenizers import Tokenizer
    B.write_tokenizer(str(tmp_path))
    texts = B.sentences(12, seed=3, lo=1, hi=60) + ["", "Bak baks BAKING zzz!"]
    for max_length in (512, 16):
        own = Tokenizer.from_file(str(tmp_path / "tokenizer.json"))
        own.enable_truncation(max_length=max_length)
        want = [own.encode(t).ids for t in texts]
        tok = tokenizer.bert_tokenizer(str(tmp_path), max_length)
        ids, lens = tok(texts)
        assert ids.shape == (len(texts), max_length) and ids.dtype == torch.int32 and lens.dtype == torch.int32
        assert lens.tolist() == [len(w) for w in want]
        for row, w in zip(ids, want):
            assert row[: len(w)].tolist() == w and not row[len(w):].any()
            assert w[0] == B.CLS and w[-1] == B.SEP and len(w) <= max_length
        assert tok.encode_lists(texts) == want
    assert max(lens.tolist()) == 16 and lens.tolist()[-2] == 2               # truncated at max_length; "" is [CLS] [SEP]
    v = B.vocabulary()
    assert want[-1] == [B.CLS, v["bak"], v["bak"], v["##s"], v["bak"], v["##ing"], 1, 1, B.SEP]          # lower-cased, pieces, [UNK] [UNK] for "zzz" "!"
    import pickle
    ids2, _ = pickle.loads(pickle.dumps(tok))(texts)
    assert torch.equal(ids2, ids)
    with pytest.raises(FileNotFoundError, match="tokenizer.json"):
        tokenizer.bert_tokenizer(str(tmp_path / "nowhere"))


# ------------------------------------------------------------------------------------------------ SentenceEncoder.encode
class _FakeEngine:
    """Stands in for BertEngine on the CPU: the 'embedding' of a text is (its length, the sum of its ids, its second id), and the calls
    are recorded."""

    def __init__(self):
        self.calls = []

    def encode_ids(self, ids, lens, normalize=False):
        self.calls.append((ids.clone(), torch.as_tensor(lens).clone(), normalize))
        return torch.stack([torch.as_tensor(lens).float(), ids.sum(1).float(), ids[:, 1].float()], 1)


def _fake_encoder(tmp_path):
    B.write_tokenizer(str(tmp_path))
    enc = sentence_model.SentenceEncoder.__new__(sentence_model.SentenceEncoder)
    enc.arch, enc.engine, enc.device = B.ARCH, _FakeEngine(), torch.device("cuda:0")
    enc.tokenize = tokenizer.bert_tokenizer(str(tmp_path), B.ARCH.ctx)
    return enc


def test_encode_sorts_by_length_and_returns_input_order(tmp_path):
    enc = _fake_encoder(tmp_path)
    texts = B.sentences(9, seed=4, lo=1, hi=30)
    want = [enc.tokenize.encode_lists([t])[0] for t in texts]
    out = enc.encode(texts, normalize_embeddings=True)
    assert out.shape == (9, 3) and out.dtype.name == "float32"
    assert out[:, 0].tolist() == [len(w) for w in want] and out[:, 1].tolist() == [sum(w) for w in want]
    ids, lens, normalize = enc.engine.calls[0]
    assert normalize is True and ids.shape == (9, B.ARCH.ctx)
    assert lens.tolist() == sorted(lens.tolist(), reverse=True) and lens.tolist() != [len(w) for w in want]      # longest first inside
    assert sentence_model.length_sorted_order([3, 9, 3, 7]) == [1, 3, 0, 2]                                       # stable
    t = enc.encode(texts, convert_to_tensor=True)
    assert torch.is_tensor(t) and torch.equal(t, torch.from_numpy(out))
    one = enc.encode(texts[2], convert_to_tensor=True)
    assert one.shape == (3,) and one.tolist() == t[2].tolist()
    assert len(enc.encode(texts, convert_to_numpy=False)) == 9
    assert enc.encode([]).shape == (0, 3)
    assert enc.to("cuda") is enc and enc.eval() is enc
    with pytest.raises(RuntimeError, match="GPU only"):
        enc.to("cpu")


# ------------------------------------------------------------------------------------------------ evaluator shims
def test_evaluator_shims_import_and_parse_the_references_arguments():
    import baselines.evaluate_text_models as legacy
    import src.clip.eval.evaluator_lm as lm
    from knowledge_enhanced_multimodal_retrieval_amd import evaluators as E
    assert lm.evaluate_text_model is E.evaluate_text_model and lm.evaluate_text_model_for_training is E.evaluate_text_model_for_training
    assert lm.main is E.main_text_lm and legacy.main is E.main_text_variants and legacy.evaluate_text_model is E.evaluate_text_model_variants
    import inspect
    assert list(inspect.signature(lm.evaluate_text_model).parameters)[:7] == ["model", "dataset", "batch_size", "device", "seed", "compute_recall", "compute_mrr"]
    assert list(inspect.signature(legacy.evaluate_text_model).parameters)[:6] == ["model", "dataset", "batch_size", "device", "mode", "seed"]
    a = E.text_lm_parser().parse_args("--model_name /m --texts_dir t --images_dir i --split val --mrr_only --batch_size 8 --device cuda "
                                      "--output_file o.json --seed 7".split())
    assert (a.model_name, a.split, a.mrr_only, a.batch_size, a.seed) == ("/m", "val", True, 8, 7)
    b = E.text_variants_parser().parse_args("--model_name /m --texts_dir t --description_type hybrid_o1 --images_dir i --splits_file s.json "
                                            "--split test --eval_mode single --batch_size 8 --device cuda --output_file o.json --seed 7".split())
    assert (b.description_type, b.eval_mode, b.splits_file) == ("hybrid_o1", "single", "s.json")
    with pytest.raises(SystemExit):
        E.text_variants_parser().parse_args("--model_name /m --texts_dir t --images_dir i --output_file o".split())      # description_type is required
    with pytest.raises(RuntimeError, match="not a directory"):
        E._load_sentence_encoder("intfloat/e5-base-v2", "cuda")


def test_variant_dataset_reads_five_variants(tmp_path):
    from knowledge_enhanced_multimodal_retrieval_amd.evaluators import TextVariantsDataset
    (tmp_path / "a.json").write_text(json.dumps({"hybrid_descriptions": ["one", " ", "three"], "content_descriptions": list("abcdefg")}))
    ds = TextVariantsDataset(["a", "missing"], str(tmp_path), "hybrid_o2")
    assert ds[0] == ["one", "", "three", "", ""] and ds[1] == [""] * 5
    assert TextVariantsDataset(["a"], str(tmp_path), "content")[0] == list("abcde")


def test_toy_set_has_the_margins_the_rank_test_needs(tmp_path):
    """tests/test_bert_encoder_gpu.py compares the engine's T2T metrics with the oracle's on bert_ref.toy_set: every oracle score is
    more than 2e-3 from its row's ground-truth score (checked here on the CPU), and the set is not trivial (not every rank is 1)."""
    from oracle import metrics_ref
    B.write_tokenizer(str(tmp_path))
    queries, targets, q, t = B.toy_set(_sd(), tokenizer.bert_tokenizer(str(tmp_path), B.ARCH.ctx))
    assert len(queries) == len(targets) == 64 and q.shape == t.shape == (64, 256)
    margin = B.score_margin(q, t)
    print(f"BERT toy_set_margin {margin:.4g}")
    assert margin > 2e-3, margin
    m = metrics_ref.retrieval_metrics(q.numpy(), t.numpy(), prefix="T2T")
    print(f"BERT toy_set_oracle_metrics {m}")
    assert sorted(m) == ["T2T_MRR", "T2T_Mean_Rank", "T2T_R@1", "T2T_R@10", "T2T_R@20", "T2T_R@5"]


# ------------------------------------------------------------------------------------------------ the library, host side
def _kcfg(**kw):
    base = dict(embed_dim=256, image_size=0, patch=0, v_width=0, v_layers=0, t_width=256, t_layers=2, vocab=1024, ctx=512)
    base.update(kw)
    return _lib.KemrCfg(**base)


def test_abi_additions():
    """New symbols exist; the ABI version stays 4 with a 'Still 4' note, as the header's rule for additions asks."""
    lib = _lib.lib()
    for name in ("kemr_model_create_family", "kemr_debug_op_attention_varlen", "kemr_debug_op_layernorm_post", "kemr_debug_op_pool_rows",
                 "kemr_debug_bert_front"):
        assert hasattr(lib, name), name
    text = open(os.path.join(ROOT, "include", "kemr.h")).read()
    assert re.search(r"#define\s+KEMR_ABI_VERSION\s+4\b", text) and re.search(r"#define\s+KEMR_MAX_BERT_CTX\s+512\b", text)
    assert re.search(r"#define\s+KEMR_MAX_TEXT_CTX\s+288\b", text)
    assert "Still 4: kemr_model_create_family" in text
    assert lib.kemr_abi_version() == 4 and _lib.MAX_BERT_CTX == 512


def test_create_family_checks_the_configuration():
    lib = _lib.lib()
    err = lambda: lib.kemr_last_error().decode()          # noqa: E731
    h = C.c_void_p()
    assert lib.kemr_model_create_family(C.byref(_kcfg()), 2, C.byref(h)) == 0
    names = [lib.kemr_model_tensor_name(h, i).decode() for i in range(lib.kemr_model_num_tensors(h))]
    assert sorted(names) == sorted(B.tensor_shapes()) and names[:5] == ["token_embedding.weight", "positional_embedding",
                                                                          "token_type_embedding", "ln_embed.weight", "ln_embed.bias"]
    v = C.c_int(-1)
    assert lib.kemr_model_get_option(h, b"family", C.byref(v)) == 0 and v.value == 2
    assert lib.kemr_model_get_option(h, b"pooling", C.byref(v)) == 0 and v.value == 0
    assert lib.kemr_model_set_option(h, b"pooling", 1) == 0 and lib.kemr_model_set_option(h, b"pooling", 2) == -1
    assert lib.kemr_model_set_option(h, b"family", 0) == -1 and "kemr_model_create_family" in err()
    assert lib.kemr_model_set_option(h, b"vision_head_dim", 64) == -1 and "no vision tower" in err()
    # the only encode call of the family is the packed one; the others name it
    assert lib.kemr_encode_text(h, None, 1, None, 0, None, 0, None) == -1 and "kemr_encode_text_packed" in err() and "length" in err()
    assert lib.kemr_encode_image(h, None, 1, None, 0, None, 0, None) == -1 and "family 2" in err()
    assert lib.kemr_encode_text_packed(h, None, None, 1, 1, None, 0, None, 0, None) == -1 and "null argument" in err()
    assert lib.kemr_workspace_bytes(h, _lib.TOWER_TEXT, 3) == 0 and lib.kemr_workspace_bytes(h, _lib.TOWER_VISION, 3) == 0
    # 2 418 rows -> 2 560 allocated: x 4 B (before finalize the stream counts as fp32; 3 B / 2 B once a precision is packed) + h, delta,
    # delta2 2 B each + big 8 B = 18 B per element; + the row starts; no pooled-row area
    assert lib.kemr_text_packed_workspace_bytes(h, 2418, 16) == 2560 * 256 * 18 + 256
    assert lib.kemr_text_packed_workspace_bytes(h, 3, 16) == 0
    # finalize: the precisions the family does not serve, worded like family 1's (before the strict-load check, no GPU touched)
    for prec in (_lib.PREC_FP8, _lib.PREC_FP8_MLP, _lib.PREC_FP8_RES16):
        assert lib.kemr_model_finalize(h, prec) == -1 and "the fp8 precisions are not served for family 2 (BERT)" in err()
    assert lib.kemr_model_finalize(h, _lib.PREC_FP32X3) == -1 and "KEMR_PREC_FP32X3 is not served for family 2 (BERT)" in err()
    assert lib.kemr_model_finalize(h, _lib.PREC_BF16) == -2 and "missing key" in err()
    lib.kemr_model_destroy(h)
    for bad, msg in ((dict(ctx=513), "512"), (dict(image_size=32, patch=8), "text-only"), (dict(v_width=256, v_layers=2), "text-only"),
                     (dict(embed_dim=128), "embed_dim 128 must equal t_width 256"), (dict(t_width=384, embed_dim=384), "t_width in"),
                     (dict(t_layers=0), "non-positive")):
        h2 = C.c_void_p()
        assert lib.kemr_model_create_family(C.byref(_kcfg(**bad)), 2, C.byref(h2)) == -1, bad
        assert msg in err(), (bad, err())
    h3 = C.c_void_p()
    assert lib.kemr_model_create_family(C.byref(_kcfg()), 3, C.byref(h3)) == -1 and "family" in err()
    assert lib.kemr_model_create(C.byref(_kcfg()), C.byref(h3)) == -1            # the CLIP entry point still demands vision fields


def test_create_family_0_and_1_are_create_plus_option():
    """Families 0 and 1 through the new entry point: the tensor lists of kemr_model_create + set_option("family"), and a CLIP model
    still refuses family 2 by option with a message naming the entry point."""
    lib = _lib.lib()
    cfg = _lib.KemrCfg(embed_dim=256, image_size=64, patch=16, v_width=256, v_layers=2, t_width=256, t_layers=2, vocab=512, ctx=16)
    for fam in (0, 1):
        a, b = C.c_void_p(), C.c_void_p()
        assert lib.kemr_model_create_family(C.byref(cfg), fam, C.byref(a)) == 0 and lib.kemr_model_create(C.byref(cfg), C.byref(b)) == 0
        assert lib.kemr_model_set_option(b, b"family", fam) == 0
        na = [lib.kemr_model_tensor_name(a, i) for i in range(lib.kemr_model_num_tensors(a))]
        nb = [lib.kemr_model_tensor_name(b, i) for i in range(lib.kemr_model_num_tensors(b))]
        assert na == nb and len(na) > 20
        assert lib.kemr_workspace_bytes(a, 0, 3) == lib.kemr_workspace_bytes(b, 0, 3) > 0
        assert lib.kemr_model_set_option(b, b"family", 2) == -1 and b"kemr_model_create_family" in lib.kemr_last_error()
        assert lib.kemr_model_set_option(b, b"pooling", 1) == -1 and b"family 2" in lib.kemr_last_error()
        lib.kemr_model_destroy(a)
        lib.kemr_model_destroy(b)
    bad = _lib.KemrCfg(embed_dim=256, image_size=64, patch=16, v_width=256, v_layers=2, t_width=256, t_layers=2, vocab=512, ctx=512)
    h = C.c_void_p()
    assert lib.kemr_model_create_family(C.byref(bad), 0, C.byref(h)) == -1 and b"288" in lib.kemr_last_error()
