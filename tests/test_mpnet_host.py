"""CPU: the MPNet sentence encoder (model family 3, all-mpnet-base-v2) up to the device -- the bucket rule and the table by distance
against ``transformers``' own, the checkpoint mapping and its refusals, the CPU statement tests/mpnet_ref.py against
``transformers.MPNetModel``, negative controls that show the GPU bar can see a wrong bias, and the library's host-side checks of
family 3.  No GPU call is made here."""
import ctypes as C
import json
import re

import numpy as np
import pytest
import torch

import mpnet_ref as M
from knowledge_enhanced_multimodal_retrieval_amd import _lib, hf_checkpoint, tokenizer
from knowledge_enhanced_multimodal_retrieval_amd.config import BERT_ARCHS, BertArch

D = 511


def _sd():
    return M.cached("mpnet_sd0", lambda: M.random_state_dict(M.ARCH, 0))


# ------------------------------------------------------------------------------------------------ the bucket rule and the table
def test_bucket_rule_equals_transformers_for_all_1023_distances():
    from transformers.models.mpnet.modeling_mpnet import MPNetEncoder
    d = torch.arange(-D, D + 1)                                     # key - query, what compute_position_bias passes
    want = MPNetEncoder.relative_position_bucket(d, num_buckets=32)
    got = torch.tensor([hf_checkpoint.relative_position_bucket(int(x)) for x in d])
    assert torch.equal(got, want)
    # every bucket is reached within 512 positions, except 16 (a key behind the query at distance 0 does not exist)
    assert sorted(set(got.tolist())) == [b for b in range(32) if b != 16]
    # the thresholds as the rule states them: keys behind the query (d > 0) take 16 .. 31
    first = {8: 8, 12: 9, 16: 10, 23: 11, 32: 12, 46: 13, 64: 14, 91: 15}
    for a, b in first.items():
        assert hf_checkpoint.relative_position_bucket(-a) == b and hf_checkpoint.relative_position_bucket(-(a - 1)) == b - 1
        assert hf_checkpoint.relative_position_bucket(a) == b + 16
    assert hf_checkpoint.relative_position_bucket(0) == 0 and hf_checkpoint.relative_position_bucket(-D) == 15


def test_table_by_distance_reproduces_compute_position_bias():
    """table[h][(k - q) + 511] is MPNetEncoder.compute_position_bias at T = 512, for the python expansion and for the library's
    (the packed arena of a family-3 model, read back on the host)."""
    model = M.hf_model(_sd())
    x = torch.zeros(1, 512, M.ARCH.width)
    with torch.no_grad():
        want = model.encoder.compute_position_bias(x)[0]           # [heads, 512, 512]
    table = hf_checkpoint.bias_by_distance(_sd()["relative_attention_bias"])
    assert table.shape == (M.ARCH.heads, 1023) and table.dtype == torch.float32
    assert torch.equal(M.position_bias(table, 512), want)
    with pytest.raises(ValueError, match="expected \\[32, heads\\]"):
        hf_checkpoint.bias_by_distance(torch.zeros(16, 4))
    # the library's expansion at finalize: the arena entry of relative_attention_bias
    lib = _lib.lib()
    h = _create()
    for name, t in _sd().items():
        host = t.detach().float().contiguous()
        shape = (C.c_int64 * max(host.dim(), 1))(*host.shape)
        assert lib.kemr_model_load_tensor(h, name.encode(), C.c_void_p(host.data_ptr()), _lib.KEMR_F32, shape, host.dim()) == 0, lib.kemr_last_error()
    n = C.c_size_t(0)
    assert lib.kemr_debug_pack_weights(h, _lib.PREC_BF16, None, 0, C.byref(n)) == 0, lib.kemr_last_error()
    buf = np.empty(n.value, dtype=np.uint8)
    assert lib.kemr_debug_pack_weights(h, _lib.PREC_BF16, C.c_void_p(buf.ctypes.data), n.value, C.byref(n)) == 0
    names = [lib.kemr_model_tensor_name(h, i).decode() for i in range(lib.kemr_model_num_tensors(h))]
    w = M.ARCH.width
    off = 0
    for nm in names[:names.index("relative_attention_bias")]:        # entries in name order, each on a multiple of 256 bytes
        off += -(-int(np.prod(M.tensor_shapes()[nm])) * 4 // 256) * 256
    assert names[:3] == ["token_embedding.weight", "positional_embedding", "relative_attention_bias"]
    got = torch.from_numpy(buf[off:off + M.ARCH.heads * 1023 * 4].view(np.float32).reshape(M.ARCH.heads, 1023).copy())
    assert torch.equal(got, table)
    pos = torch.from_numpy(buf[1024 * w * 4:1024 * w * 4 + 512 * w * 4].view(np.float32).reshape(512, w).copy())
    assert torch.equal(pos, _sd()["positional_embedding"])            # verbatim: no type row is added for this family
    lib.kemr_model_destroy(h)


# ------------------------------------------------------------------------------------------------ checkpoint mapping
def test_state_dict_round_trip_through_mpnet_model(tmp_path):
    sd = _sd()
    model = M.hf_model(sd, pooler=True)
    hf = model.state_dict()
    back = hf_checkpoint.from_mpnet_state_dict(hf, M.ARCH)
    assert sorted(back) == sorted(sd) == sorted(M.tensor_shapes())
    assert all(torch.equal(back[k], sd[k]) for k in sd)
    assert all(tuple(back[k].shape) == M.tensor_shapes()[k] for k in sd)
    assert hf["embeddings.position_embeddings.weight"].shape == (514, 256)
    b0 = "transformer.resblocks.0.attn.in_proj_weight"
    assert torch.equal(back[b0][256:512], hf["encoder.layer.0.attention.attn.k.weight"])          # q | k | v
    # `mpnet.`-prefixed keys, a pooler, a task head and the buffers are accepted / ignored
    pre = {f"mpnet.{k}": v for k, v in hf.items()}
    pre.update({"mpnet.embeddings.position_ids": torch.zeros(1, 514), "lm_head.bias": torch.zeros(3)})
    back = hf_checkpoint.from_mpnet_state_dict(pre, M.ARCH)
    assert all(torch.equal(back[k], sd[k]) for k in sd)
    with pytest.raises(KeyError, match="missing key 'encoder.relative_attention_bias.weight'"):
        hf_checkpoint.from_mpnet_state_dict({k: v for k, v in hf.items() if k != "encoder.relative_attention_bias.weight"}, M.ARCH)
    with pytest.raises(KeyError, match="unexpected key 'embeddings.token_type_embeddings.weight'"):
        hf_checkpoint.from_mpnet_state_dict(dict(hf, **{"embeddings.token_type_embeddings.weight": torch.zeros(1)}), M.ARCH)


def test_read_sentence_directory(tmp_path):
    sd = _sd()
    plain = M.save_directory(tmp_path / "plain", sd)
    arch, got = hf_checkpoint.read_sentence_directory(plain)
    assert arch == M.ARCH and isinstance(arch, BertArch) and arch.relative_bias and arch.layer_norm_eps == 1e-5 and arch.library_family == 3
    assert sorted(got) == sorted(sd) and all(torch.equal(got[k], sd[k]) for k in sd)
    st = M.save_directory(tmp_path / "st", sd, pooling="cls", max_seq_length=384)
    arch, got = hf_checkpoint.read_sentence_directory(st)
    assert (arch.pooling, arch.ctx, arch.positions) == ("cls", 384, 512)
    assert got["positional_embedding"].shape == (384, 256) and torch.equal(got["positional_embedding"], sd["positional_embedding"][:384])
    arch12, _ = hf_checkpoint.read_sentence_directory(M.save_directory(tmp_path / "eps12", sd, M.ARCH12))
    assert arch12 == M.ARCH12 and arch12 != M.ARCH
    # the other route keeps refusing MPNet, with its words; the sentence route serves BERT exactly as read_hf_directory does
    with pytest.raises(ValueError, match="relative position bias"):
        hf_checkpoint.read_hf_directory(plain)
    import bert_ref as B
    bsd = B.cached("sd0", lambda: B.random_state_dict(B.ARCH, 0))
    bdir = B.save_directory(tmp_path / "bert", bsd, pooling="cls", max_seq_length=128)
    a1, _, s1 = hf_checkpoint.read_hf_directory(bdir)
    a2, s2 = hf_checkpoint.read_sentence_directory(bdir)
    assert a1 == a2 and not a2.relative_bias and a2.library_family == 2 and sorted(s1) == sorted(s2) and all(torch.equal(s1[k], s2[k]) for k in s1)
    (tmp_path / "clip").mkdir()
    (tmp_path / "clip" / "config.json").write_text(json.dumps(dict(model_type="clip")))
    with pytest.raises(ValueError, match="not a sentence encoder"):
        hf_checkpoint.read_sentence_directory(str(tmp_path / "clip"))


def test_published_config_numbers_give_the_registered_arch():
    """sentence-transformers/all-mpnet-base-v2 by its published config.json numbers."""
    cfg = dict(model_type="mpnet", hidden_size=768, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072, vocab_size=30527,
               max_position_embeddings=514, hidden_act="gelu", layer_norm_eps=1e-05, relative_attention_num_buckets=32, pad_token_id=1,
               bos_token_id=0, eos_token_id=2)
    arch = hf_checkpoint.arch_from_mpnet_config(cfg)
    assert arch == BERT_ARCHS["all-mpnet-base-v2"]
    assert arch.cfg_dict() == dict(embed_dim=768, image_size=0, patch=0, v_width=0, v_layers=0, t_width=768, t_layers=12, vocab=30527, ctx=512)
    assert arch.library_family == 3 and BERT_ARCHS["e5-base-v2"].library_family == 2
    assert BertArch(768, 12) == BERT_ARCHS["e5-base-v2"]             # the new fields' defaults leave every existing arch equal to itself


def _cfg(**kw):
    cfg = json.loads(M.mpnet_config().to_json_string())
    cfg.update(kw)
    return cfg


@pytest.mark.parametrize("change,message", [
    (dict(relative_attention_num_buckets=64), "relative_attention_num_buckets = 64; served: 32"),
    (dict(layer_norm_eps=1e-6), "layer_norm_eps = 1e-06"),
    (dict(num_attention_heads=8), "head dim of 32"),
    (dict(hidden_size=384, num_attention_heads=6, intermediate_size=1536), "hidden_size = 384 is not a multiple of 256"),
    (dict(max_position_embeddings=516), "served up to 514"),
    (dict(model_type="bert"), "is not an MPNetModel"),
    (dict(hidden_act="relu"), "hidden_act = 'relu'"),
])
def test_config_refusals(change, message):
    with pytest.raises(ValueError, match=re.escape(message)):
        hf_checkpoint.arch_from_mpnet_config(_cfg(**change))


def test_arch_refuses_another_eps():
    with pytest.raises(ValueError, match="MPNet encoders are served with"):
        BertArch(256, 2, relative_bias=True, layer_norm_eps=1e-6)
    with pytest.raises(ValueError, match="1e-12 only"):
        BertArch(256, 2, layer_norm_eps=1e-5)


# ------------------------------------------------------------------------------------------------ the CPU statement
@pytest.mark.parametrize("pooling", ["mean", "cls"])
def test_mpnet_ref_equals_transformers(pooling):
    """mpnet_ref.encode (every text on its own length) against MPNetModel (eager attention, fp32) on the padded batch with its attention
    mask + sentence-transformers' pooling, on the length set of the GPU tests: <= 1e-5 absolute, the closeness tests/test_bert_host.py
    asks of the BERT statement."""
    sd = _sd()
    ids, lens = M.random_ids(M.LENGTHS)
    ref = M.encode(sd, M.ARCH, ids, lens, pooling)
    hf = M.hf_encode(M.cached("mpnet_hf", lambda: M.hf_model(sd)), ids, lens, pooling)
    err = float((ref - hf).abs().max())
    print(f"MPNET mpnet_ref_vs_transformers_{pooling}_max_abs {err:.3g}")
    assert err <= 1e-5, err
    assert float(ref.abs().max()) > 0.5          # not a comparison of zeros


def test_eps_is_the_configs():
    """The two eps values are two models: HF at 1e-12 equals the statement at 1e-12 (<= 1e-5) on a fixture where a LayerNorm row has a
    small variance, so that the eps shows."""
    sd = {k: v.clone() for k, v in _sd().items()}
    ids, lens = M.random_ids([5, 64, 129], seed=4)
    ref12 = M.encode(sd, M.ARCH12, ids, lens)
    hf12 = M.hf_encode(M.hf_model(sd, M.ARCH12), ids, lens)
    assert float((ref12 - hf12).abs().max()) <= 1e-5


def test_negative_controls_the_bar_sees_a_wrong_bias():
    """On the plain fixture the statement run with each of four wrong tables differs from the right one by 1 - cos >= 2e-3 at every
    length >= 2 (the frozen table: at lengths >= 127) -- twice the GPU bar, so an engine applying any of them cannot pass."""
    sd = _sd()
    ids, lens = M.random_ids(M.LENGTHS)
    right = M.cached("mpnet_oracle_plain_sorted_raw", lambda: M.encode(sd, M.ARCH, ids, lens))
    table = hf_checkpoint.bias_by_distance(sd["relative_attention_bias"])
    for name, wrong in M.wrong_tables(table).items():
        assert not torch.equal(wrong, table), name
        gap = M.one_minus_cos(M.encode(sd, M.ARCH, ids, lens, table=wrong), right)
        applies = lens >= (127 if name == "frozen_beyond_63" else 2)
        print(f"MPNET negative_control_{name}_min_1_minus_cos {float(gap[applies].min()):.3g} (bias seed {M.BIAS_SEED})")
        assert float(gap[applies].min()) >= 2e-3, (name, gap.tolist())
        assert float(gap[lens == 1].max()) == 0.0                    # one token: the softmax of one score, whatever the bias
    frozen = M.wrong_tables(table)["frozen_beyond_63"]
    assert torch.equal(frozen[:, D - 63:D + 64], table[:, D - 63:D + 64])


# ------------------------------------------------------------------------------------------------ tokenizer
def test_tokenizer_with_mpnet_special_tokens(tmp_path):
    """BertTokenize runs the directory's tokenizer.json whatever its special tokens: <s> = 0 first, </s> = 2 last also after truncation,
    <unk> = 3; nothing assumes [CLS] / [SEP] ids or pad id 0 (positions behind a text's length are never read by the engine)."""
    M.write_tokenizer(str(tmp_path))
    tok = tokenizer.bert_tokenizer(str(tmp_path), 16)
    texts = M.sentences(6, seed=3, lo=1, hi=60) + ["", "Bak zzz"]
    lists = tok.encode_lists(texts)
    assert all(w[0] == M.BOS and w[-1] == M.EOS and len(w) <= 16 and M.PAD not in w for w in lists)
    assert max(len(w) for w in lists) == 16 and lists[-2] == [M.BOS, M.EOS]
    assert lists[-1] == [M.BOS, M.vocabulary()["bak"], M.UNK, M.EOS]
    ids, lens = tok(texts)
    assert lens.tolist() == [len(w) for w in lists] and ids.shape == (8, 16)


# ------------------------------------------------------------------------------------------------ the library, host side
def _kcfg(**kw):
    base = dict(embed_dim=256, image_size=0, patch=0, v_width=0, v_layers=0, t_width=256, t_layers=2, vocab=1024, ctx=512)
    base.update(kw)
    return _lib.KemrCfg(**base)


def _create(**kw):
    """A family-3 model: created as family 2, switched before its first tensor (include/kemr.h)."""
    h = C.c_void_p()
    assert _lib.lib().kemr_model_create_family(C.byref(_kcfg(**kw)), 2, C.byref(h)) == 0, _lib.lib().kemr_last_error()
    assert _lib.lib().kemr_model_set_option(h, b"family", 3) == 0, _lib.lib().kemr_last_error()
    return h


def test_family_3_is_created_with_strict_names():
    lib = _lib.lib()
    err = lambda: lib.kemr_last_error().decode()          # noqa: E731
    assert hasattr(lib, "kemr_debug_op_attention_varlen_bias") and lib.kemr_abi_version() == 4
    h = _create()
    names = [lib.kemr_model_tensor_name(h, i).decode() for i in range(lib.kemr_model_num_tensors(h))]
    assert sorted(names) == sorted(M.tensor_shapes()) and "token_type_embedding" not in names
    v = C.c_int(-1)
    assert lib.kemr_model_get_option(h, b"family", C.byref(v)) == 0 and v.value == 3
    x = torch.zeros(2, 256)
    shape = (C.c_int64 * 2)(2, 256)
    assert lib.kemr_model_load_tensor(h, b"token_type_embedding", C.c_void_p(x.data_ptr()), _lib.KEMR_F32, shape, 2) == -1
    assert "unexpected key 'token_type_embedding'" in err()
    bad = (C.c_int64 * 2)(32, 12)
    assert lib.kemr_model_load_tensor(h, b"relative_attention_bias", C.c_void_p(x.data_ptr()), _lib.KEMR_F32, bad, 2) == -1 and "expected [32,4,]" in err()
    for name, t in _sd().items():                                   # everything but the bias: finalize names it
        if name == "relative_attention_bias":
            continue
        host = t.detach().float().contiguous()
        shp = (C.c_int64 * max(host.dim(), 1))(*host.shape)
        assert lib.kemr_model_load_tensor(h, name.encode(), C.c_void_p(host.data_ptr()), _lib.KEMR_F32, shp, host.dim()) == 0, err()
    assert lib.kemr_model_finalize(h, _lib.PREC_BF16) == -2 and "missing key 'relative_attention_bias'" in err()
    # what family 2 refuses, family 3 refuses with the same wording
    for prec in (_lib.PREC_FP8, _lib.PREC_FP8_MLP, _lib.PREC_FP8_RES16):
        assert lib.kemr_model_finalize(h, prec) == -1 and "the fp8 precisions are not served for family 2 (BERT)" in err()
    assert lib.kemr_model_finalize(h, _lib.PREC_FP32X3) == -1 and "KEMR_PREC_FP32X3 is not served for family 2 (BERT)" in err()
    assert lib.kemr_encode_text(h, None, 1, None, 0, None, 0, None) == -1 and "kemr_encode_text_packed" in err()
    assert lib.kemr_encode_image(h, None, 1, None, 0, None, 0, None) == -1 and "no vision tower" in err()
    assert lib.kemr_model_set_option(h, b"family", 0) == -1 and "kemr_model_create_family" in err()
    assert lib.kemr_model_set_option(h, b"family", 3) == -2 and "before the first kemr_model_load_tensor" in err()      # tensors are loaded
    assert lib.kemr_model_set_option(h, b"vision_head_dim", 64) == -1 and "no vision tower" in err()
    assert lib.kemr_model_set_option(h, b"pooling", 1) == 0 and lib.kemr_model_set_option(h, b"pooling", 2) == -1
    assert lib.kemr_workspace_bytes(h, _lib.TOWER_TEXT, 3) == 0
    assert lib.kemr_text_packed_workspace_bytes(h, 2418, 16) == 2560 * 256 * 18 + 256          # family 2's layout
    lib.kemr_model_destroy(h)
    # the switch goes both ways before the first load, and rebuilds the tensor list each time
    h = _create()
    assert lib.kemr_model_set_option(h, b"family", 2) == 0 and lib.kemr_model_get_option(h, b"family", C.byref(v)) == 0 and v.value == 2
    back = [lib.kemr_model_tensor_name(h, i).decode() for i in range(lib.kemr_model_num_tensors(h))]
    assert "token_type_embedding" in back and "relative_attention_bias" not in back
    assert lib.kemr_model_set_option(h, b"family", 3) == 0 and lib.kemr_model_set_option(h, b"family", 4) == -1
    assert [lib.kemr_model_tensor_name(h, i).decode() for i in range(lib.kemr_model_num_tensors(h))] == names
    lib.kemr_model_destroy(h)
    # the create call itself keeps refusing 3 and says where family 3 is
    h3 = C.c_void_p()
    assert lib.kemr_model_create_family(C.byref(_kcfg()), 3, C.byref(h3)) == -1 and 'kemr_model_set_option(m, "family", 3)' in err()


def test_layer_norm_eps_option():
    """5 and 12 only, family 3 only."""
    lib = _lib.lib()
    err = lambda: lib.kemr_last_error().decode()          # noqa: E731
    h = _create()
    v = C.c_int(-1)
    assert lib.kemr_model_get_option(h, b"layer_norm_eps", C.byref(v)) == 0 and v.value == 5            # the published checkpoint's
    assert lib.kemr_model_set_option(h, b"layer_norm_eps", 12) == 0
    assert lib.kemr_model_get_option(h, b"layer_norm_eps", C.byref(v)) == 0 and v.value == 12
    assert lib.kemr_model_set_option(h, b"layer_norm_eps", 5) == 0
    for bad in (0, 6, 1, -5, 13):
        assert lib.kemr_model_set_option(h, b"layer_norm_eps", bad) == -1 and "5 (1e-5) or 12 (1e-12)" in err(), bad
    assert lib.kemr_model_get_option(h, b"layer_norm_eps", C.byref(v)) == 0 and v.value == 5
    lib.kemr_model_destroy(h)
    clip = _lib.KemrCfg(embed_dim=256, image_size=64, patch=16, v_width=256, v_layers=2, t_width=256, t_layers=2, vocab=512, ctx=16)
    for fam in (0, 1, 2):
        g = C.c_void_p()
        assert lib.kemr_model_create_family(C.byref(clip if fam < 2 else _kcfg()), fam, C.byref(g)) == 0
        assert lib.kemr_model_set_option(g, b"layer_norm_eps", 5) == -1 and "family 3 (MPNet) only" in err(), fam
        assert lib.kemr_model_get_option(g, b"layer_norm_eps", C.byref(v)) == -1
        if fam < 2:
            assert lib.kemr_model_set_option(g, b"family", 3) == -1 and "kemr_model_create_family(cfg, 2)" in err()
        lib.kemr_model_destroy(g)
