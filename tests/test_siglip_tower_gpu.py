"""GPU: the SigLIP towers end to end against the fp64 statement of tests/siglip_ref.py -- at the 4-byte-stream precision "bf16" and at
the default precision, on plain and on sharpened weights (1 - cos <= 1e-3 from the right statement, more than 1e-2 from every CLIP
behaviour the family must not have: tests/test_siglip_host.py shows the fp64 side of that) --, the text tower's pad positions, the
refusals, the Hugging Face directory route, and a CLIP model's bits beside a SigLIP model in the same process."""
import json
import os

import pytest
import torch
import transformers

import siglip_ref as S
from knowledge_enhanced_multimodal_retrieval_amd import _lib, clip_api, engine, hf_checkpoint
from knowledge_enhanced_multimodal_retrieval_amd.config import ARCHS
from oracle import clip_ref

pytestmark = pytest.mark.gpu

COS_TOL = 1e-3
WRONG_BAR = 1e-2
PRECISIONS = ["bf16", _lib.DEFAULT_PRECISION]


def _note(name, value):
    print(f"NUMERICS {name} {value}")


def _engine(arch, device, sd, precision=_lib.DEFAULT_PRECISION):
    eng = engine.ClipEngine(arch, device, precision=precision)
    eng.load_state_dict(sd)
    return eng


def _check(got, right, wrongs, what):
    miss = float(S.one_minus_cos(got, right).max())
    far = {str(k): float(S.one_minus_cos(got, w).min()) for k, w in wrongs}
    _note(what, (f"{miss:.3e}", {k: f"{v:.3e}" for k, v in far.items()}))
    assert miss <= COS_TOL, (what, miss)
    for k, v in far.items():
        assert v > WRONG_BAR, (what, k, v)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", ["tiny-siglip", "tiny-siglip-196", "tiny-siglip-576"])
def test_vision_tower_against_fp64(device, name, precision):
    arch = ARCHS[name]
    for sharpening in (None, "eps", "act"):
        eng = _engine(arch, device, S.weights(arch, sharpening), precision)
        for n in (3, 9):
            got = eng.encode_image(S.pixels(arch, n).to(device))
            wrongs = [(sw, S.image_reference(name, n, sharpening, **sw)) for sw, sh in S.WRONG_IMAGE if sh == sharpening]
            _check(got, S.image_reference(name, n, sharpening), wrongs, f"image_{name}_n{n}_{precision}_{sharpening}")
        if sharpening is None:
            # every token of the last block feeds the pooling head: option "last_block_pooled_row" is ignored by this tower
            eng.set_last_block_pooled_row(False)
            assert torch.equal(eng.encode_image(S.pixels(arch, 9).to(device)), got)
            norm = eng.encode_image(S.pixels(arch, 9).to(device), normalize=True)
            assert float((norm.double().norm(dim=-1) - 1).abs().max()) <= 1e-6 and float(S.one_minus_cos(norm, got).max()) <= 1e-12


def test_vision_tower_with_fused_residual_adds(device):
    """"bf16-res16" at 1728 token rows: the out-proj / fc2 epilogues add into the bf16 stream, nothing is pending for ln_post."""
    name, n = "tiny-siglip-576", 3
    eng = _engine(ARCHS[name], device, S.weights(ARCHS[name]), "bf16-res16")
    assert eng.residual_fusion_active()
    _check(eng.encode_image(S.pixels(ARCHS[name], n).to(device)), S.image_reference(name, n), [], f"image_{name}_n{n}_bf16-res16")


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("ctx,n", S.TEXT_CASES)
def test_text_tower_against_fp64(device, ctx, n, precision):
    arch = S.text_arch(ctx)
    ids = S.text_ids(arch, n)
    for sharpening in (None, "causal", "eps", "act"):
        eng = _engine(arch, device, S.weights(arch, sharpening), precision)
        wrongs = [(sw, S.text_reference(ctx, n, sharpening, **sw)) for sw, sh in S.WRONG_TEXT if sh == sharpening]
        for pooled in (True, False):                  # the pooled-row last block (pool index ctx - 1) and the full block
            eng.set_last_block_pooled_row(pooled)
            _check(eng.encode_text(ids), S.text_reference(ctx, n, sharpening), wrongs, f"text_ctx{ctx}_n{n}_{precision}_{sharpening}_pooled{int(pooled)}")
            _check(eng.encode_text(ids.to(device)), S.text_reference(ctx, n, sharpening), [], f"text_ctx{ctx}_devids_{precision}_{sharpening}")


def test_pad_positions_are_keys_and_the_last_position_is_pooled(device):
    arch = ARCHS["tiny-siglip"]
    eng = _engine(arch, device, S.weights(arch))
    base = S.text_ids(arch, 1)[0]
    ln = int((base != 1).sum())
    assert ln + 2 < arch.ctx
    rows = base.repeat(4, 1)
    rows[1, ln + 1] = 7                               # differs from row 0 only in the pad region, BEHIND the end-of-sequence id
    rows[2, arch.ctx - 1] = 9                         # ... only at the last position
    out = eng.encode_text(rows)                       # row 3 == row 0
    assert torch.equal(out[0], out[3])
    for i in (1, 2):
        assert float(S.one_minus_cos(out[0:1], out[i:i + 1])) > 1e-4
    ref = S.encode_text(S.weights(arch), arch, rows)
    assert float(S.one_minus_cos(out, ref).max()) <= COS_TOL
    # argmax(ids) is nowhere near the pooled row: rows whose largest id sits at position 0 pool the last position all the same
    assert int(rows[0].argmax()) != arch.ctx - 1


class _NoPacked:
    """The library handle of one engine with the packed text entry point made fatal."""

    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        if name == "kemr_encode_text_packed":
            raise AssertionError("encode_text reached kemr_encode_text_packed")
        return getattr(self._lib, name)


def test_encode_text_never_takes_the_packed_route(device):
    import ctypes as C
    arch = ARCHS["tiny-siglip"]
    eng = _engine(arch, device, S.weights(arch))
    assert eng.pack_text is False
    real, eng._L = eng._L, _NoPacked(eng._L)
    ids = S.text_ids(arch, 5)
    eng.pack_text = True                              # even when asked to
    a = eng.encode_text(ids)
    b = eng.encode_text(ids.to(device), lens=torch.full((5,), 3))
    eng._L = real
    assert torch.equal(a, b)
    out, lens = torch.zeros(5, arch.embed_dim, device=device), torch.full((5,), arch.ctx, dtype=torch.int32, device=device)
    ws = torch.zeros(int(real.kemr_workspace_bytes(eng._h, _lib.TOWER_TEXT, 5)) + 4096, dtype=torch.uint8, device=device)
    dev_ids = ids.to(device)
    rc = real.kemr_encode_text_packed(eng._h, C.c_void_p(dev_ids.data_ptr()), C.c_void_p(lens.data_ptr()), 5 * arch.ctx, 5,
                                      C.c_void_p(out.data_ptr()), 0, C.c_void_p(ws.data_ptr()), ws.numel(), None)
    assert rc == -1 and b"not available for family 1" in real.kemr_last_error()
    assert float(out.abs().max()) == 0.0


def test_precisions_that_are_not_served_raise(device):
    arch = ARCHS["tiny-siglip"]
    sd = S.weights(arch)
    for prec in ("fp8", "fp8-x24", "fp8-mlp", "fp8-res16"):
        with pytest.raises(RuntimeError, match="fp8 precisions are not served for family 1"):
            _engine(arch, device, sd, prec)
    with pytest.raises(RuntimeError, match="KEMR_PREC_FP32X3 is not served for family 1"):
        _engine(arch, device, sd, "fp32x3")
    eng = _engine(arch, device, sd)
    with pytest.raises(ValueError, match="quick_gelu.*gelu"):
        eng.set_activation("gelu_pytorch_tanh")
    got = eng.encode_image(S.pixels(arch, 3).to(device))
    eng.set_activation("gelu")                        # the option is not consulted in this family
    assert torch.equal(eng.encode_image(S.pixels(arch, 3).to(device)), got)


def _hf_features(model, px, ids):
    with torch.no_grad():
        i = model.get_image_features(pixel_values=px)
        t = model.get_text_features(input_ids=ids.long())
    return (i if torch.is_tensor(i) else i.pooler_output), (t if torch.is_tensor(t) else t.pooler_output)


def test_hf_directory_end_to_end(device, tmp_path):
    """save_pretrained directory -> clip.load -> encode_* within 1e-3 of transformers' own fp32 features."""
    arch = ARCHS["tiny-siglip"]
    torch.manual_seed(0)
    hf = transformers.SiglipModel(transformers.SiglipConfig(**S.hf_config_kwargs(arch), attn_implementation="eager")).eval()
    hf.load_state_dict(hf_checkpoint.to_siglip_state_dict(S.weights(arch), arch), strict=False)
    hf.save_pretrained(str(tmp_path), safe_serialization=True)
    model, pre = clip_api.load(str(tmp_path), device=device)
    assert type(model).__name__ == "SigLIP" and pre.n_px == arch.image_size
    px, ids = S.pixels(arch, 3), S.text_ids(arch, 5)
    want_i, want_t = _hf_features(hf, px, ids)
    assert float(S.one_minus_cos(model.encode_image(px.to(device)), want_i).max()) <= COS_TOL
    assert float(S.one_minus_cos(model.encode_text(ids), want_t).max()) <= COS_TOL
    assert float(S.one_minus_cos(model.get_image_features(pixel_values=px.to(device)), want_i).max()) <= COS_TOL
    # a processor's shorter rows are padded with the pad id 1, as padding="max_length" does
    short = ids[:, : arch.ctx - 4].clone()
    full = torch.nn.functional.pad(short, (0, 4), value=1)
    assert torch.equal(model.get_text_features(input_ids=short), model.encode_text(full))
    li, lt = model(px.to(device), ids[:3])
    cos = torch.nn.functional.normalize(want_i.double(), dim=-1) @ torch.nn.functional.normalize(want_t[:3].double(), dim=-1).T
    want = cos * float(hf.logit_scale.exp()) + float(hf.logit_bias)
    assert float((li.double().cpu() - want).abs().max()) <= 2e-2 and torch.equal(lt, li.t())


def _write_unigram(directory):
    from tokenizers import Tokenizer, models, pre_tokenizers
    vocab = [("<pad>", 0.0), ("</s>", 0.0), ("<unk>", 0.0), ("▁", -6.0)] + [(c, -3.0) for c in "abcdefghijklmnopqrstuvwxyz0123456789"]
    tok = Tokenizer(models.Unigram(vocab, unk_id=2))
    tok.pre_tokenizer = pre_tokenizers.Metaspace()
    tok.save(os.path.join(directory, "tokenizer.json"))


def test_evaluators_run_a_siglip_directory_with_its_own_tokenizer(device, tmp_path):
    """encode_dataset, EmbeddingStore.build and the evaluator CLI on a SigLIP directory with NO tokenize_fn given: the texts go through
    the directory's tokenizer.json ([B, ctx] ids of its vocabulary), the embeddings are the ones encode_text gives for those ids, and the
    results JSON names that tokenizer.  (A SigLIP model without a tokenizer.json fails up front: tests/test_siglip_host.py.)"""
    from knowledge_enhanced_multimodal_retrieval_amd import evaluators, retriever, tokenizer
    from knowledge_enhanced_multimodal_retrieval_amd.datasets import SyntheticRetrievalDataset
    arch = ARCHS["tiny-siglip"]
    d = str(tmp_path / "ckpt")
    hf = transformers.SiglipModel(transformers.SiglipConfig(**S.hf_config_kwargs(arch), attn_implementation="eager")).eval()
    hf.load_state_dict(hf_checkpoint.to_siglip_state_dict(S.weights(arch), arch), strict=False)
    hf.save_pretrained(d, safe_serialization=True)
    _write_unigram(d)
    model, _ = clip_api.load(d, device=device)
    ds = SyntheticRetrievalDataset(12, arch.image_size, seed=1)
    image, query, target, uuids = evaluators.encode_dataset(model, ds, batch_size=5)
    assert tuple(image.shape) == tuple(query.shape) == tuple(target.shape) == (12, arch.embed_dim) and len(uuids) == 12
    fn = tokenizer.siglip_tokenizer(d, arch.ctx)
    want_q = model.encode_text(fn([ds[i][1] for i in range(12)]), normalize=True)
    want_t = model.encode_text(fn([ds[i][2] for i in range(12)]), normalize=True)
    assert float(S.one_minus_cos(query, want_q).max()) <= 1e-6 and float(S.one_minus_cos(target, want_t).max()) <= 1e-6
    store = retriever.EmbeddingStore.build(model, ds, batch_size=5)
    assert len(store.uuids) == 12
    assert isinstance(retriever.CLIPRetriever(model, store).tokenize_fn, tokenizer.SiglipTokenize)
    out = str(tmp_path / "res" / "metrics.json")
    res = evaluators.main_evaluator(["--model_name", d, "--synthetic", "12", "--output_file", out, "--num_workers", "0", "--mrr_only"])
    assert res["tokenizer"] == f"siglip tokenizers ({os.path.join(d, 'tokenizer.json')})" and res["num_samples"] == 12
    with open(out) as f:
        assert json.load(f)["tokenizer"] == res["tokenizer"]


def test_clip_bits_beside_a_siglip_model(device):
    """A CLIP model encodes the same bits before, while and after a SigLIP model lives in the process."""
    oa = clip_ref.ARCHS["tiny"]
    sd = clip_ref.random_state_dict(oa, seed=2)
    px = torch.randn(5, 3, 32, 32, generator=torch.Generator().manual_seed(3)).to(device)
    ids = clip_ref.synthetic_ids(oa, 5)
    clip = engine.ClipEngine(ARCHS["tiny"], device)
    clip.load_state_dict(sd)
    before = (clip.encode_image(px), clip.encode_text(ids))
    arch = ARCHS["tiny-siglip"]
    sig = _engine(arch, device, S.weights(arch))
    s_before = (sig.encode_image(S.pixels(arch, 3).to(device)), sig.encode_text(S.text_ids(arch, 5)))
    during = (clip.encode_image(px), clip.encode_text(ids))
    s_after = (sig.encode_image(S.pixels(arch, 3).to(device)), sig.encode_text(S.text_ids(arch, 5)))
    del sig
    clip2 = engine.ClipEngine(ARCHS["tiny"], device)
    clip2.load_state_dict(sd)
    after = (clip2.encode_image(px), clip2.encode_text(ids))
    for a, b, c in zip(before, during, after):
        assert torch.equal(a, b) and torch.equal(a, c)
    for a, b in zip(s_before, s_after):
        assert torch.equal(a, b)
    assert float(clip_ref_cos(before[0], clip_ref.encode_image(sd, oa, px.cpu()))) <= COS_TOL


def clip_ref_cos(a, b):
    return S.one_minus_cos(a, b).max()
