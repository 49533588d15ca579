"""GPU: the BERT sentence encoder (model family 2) end to end -- kemr_encode_text_packed against the CPU statement tests/bert_ref.py
(fp32) at the project's embedding bar 1 - cos <= 1e-3, packed against alone, the memory contract (tests/footprint.py, modelled on
tests/test_footprint_towers_gpu.py), and the Python surface: SentenceEncoder.encode and evaluate_text_model."""
import ctypes as C

import pytest
import torch

import bert_ref as B
import footprint as F
from footprint import IntIn, Out, SizeOf, Work
from knowledge_enhanced_multimodal_retrieval_amd import _lib, debug, engine
from knowledge_enhanced_multimodal_retrieval_amd.sentence_model import SentenceEncoder

pytestmark = pytest.mark.gpu

BAR = 1e-3                     # the project's embedding bar: 1 - cos against the fp32 statement
ERR_WORKSPACE = -4             # include/kemr.h KEMR_ERR_WORKSPACE
F32 = torch.float32


def _weights(kind):
    return B.cached(("sd", kind), lambda: (B.heavy_state_dict if kind == "heavy" else B.random_state_dict)(B.ARCH, 0))


def _engine(device, precision=_lib.DEFAULT_PRECISION, kind="plain", pooling="mean"):
    eng = engine.BertEngine(B.BertArch(256, 2, vocab=1024, ctx=512, pooling=pooling), device, precision)
    eng.load_state_dict(_weights(kind))
    return eng


def _inputs(order="sorted"):
    return B.random_ids(B.LENGTHS if order == "sorted" else B.SHUFFLED, seed=1 if order == "sorted" else 2)


def _oracle(kind, order, pooling="mean"):
    ids, lens = _inputs(order)
    return B.cached(("oracle", kind, order, pooling), lambda: B.encode(_weights(kind), B.ARCH, ids, lens, pooling, normalize=True))


@pytest.mark.parametrize("precision", [_lib.DEFAULT_PRECISION, "bf16"])
@pytest.mark.parametrize("kind", ["plain", "heavy"])
def test_encoder_matches_the_cpu_statement(device, precision, kind):
    """All sixteen lengths 1 .. 512 in one packed call of 2 418 rows, then in shuffled order: every item within 1 - cos <= 1e-3 of
    bert_ref (fp32), on plain and on heavy-tailed weights, at the default precision (24-bit stream) and at "bf16" (fp32 stream)."""
    eng = _engine(device, precision, kind)
    for order in ("sorted", "shuffled"):
        ids, lens = _inputs(order)
        got = eng.encode_ids(ids, lens, normalize=True).cpu()
        assert bool(torch.isfinite(got).all())
        gap = B.one_minus_cos(got, _oracle(kind, order))
        print(f"BERT encoder_{kind}_{precision}_{order}_max_1_minus_cos {float(gap.max()):.3g} (at length {int(lens[int(gap.argmax())])})")
        assert float(gap.max()) <= BAR, (kind, precision, order, gap.tolist())
        assert float((got.norm(dim=-1) - 1).abs().max()) < 1e-5


def test_cls_pooling_and_option(device):
    eng = _engine(device, pooling="cls")
    ids, lens = _inputs("shuffled")
    got = eng.encode_ids(ids, lens, normalize=True).cpu()
    assert float(B.one_minus_cos(got, _oracle("plain", "shuffled", "cls")).max()) <= BAR
    long = lens >= 15                                               # (a one-token text's mean IS its first row)
    assert float(B.one_minus_cos(got, _oracle("plain", "shuffled"))[long].min()) > 1e-2      # not the mean
    eng.set_pooling("mean")                                         # the option may be flipped between calls
    assert float(B.one_minus_cos(eng.encode_ids(ids, lens, normalize=True).cpu(), _oracle("plain", "shuffled")).max()) <= BAR


def test_packed_equals_alone(device):
    """A text's embedding inside the packed batch against the same text encoded alone.  Which statement applies: with the GEMM routing
    held the same (debug switch gemm_variant = 1, the 128 x 128 tile kernel for every launch; its rows do not depend on the other rows)
    the two are BIT-IDENTICAL -- every other kernel of the path works per row or per item.  With the automatic routing a launch of
    2 418 rows and one of <= 512 rows go to different GEMM kernels (persistent 256 x 256 against skinny split-K), whose fp32 sums run
    in another order: held to 1 - cos <= 1e-6."""
    eng = _engine(device)
    ids, lens = _inputs("shuffled")
    picks = [0, 5, 9, len(B.SHUFFLED) - 1] + [B.SHUFFLED.index(1), B.SHUFFLED.index(512)]
    with debug.override(gemm_variant=1):
        packed = eng.encode_ids(ids, lens).clone()
        for i in picks:
            alone = eng.encode_ids(ids[i:i + 1], lens[i:i + 1])
            assert F.same_bits(alone[0], packed[i]), (i, int(lens[i]))
    packed = eng.encode_ids(ids, lens).clone()
    worst = 0.0
    for i in picks:
        alone = eng.encode_ids(ids[i:i + 1], lens[i:i + 1])
        worst = max(worst, float(B.one_minus_cos(alone, packed[i:i + 1])))
    print(f"BERT packed_vs_alone_auto_routing_max_1_minus_cos {worst:.3g}")
    assert worst <= 1e-6, worst
    # two calls of the same batch: the same bits
    assert F.same_bits(eng.encode_ids(ids, lens), packed)


# ------------------------------------------------------------------------------------------------ memory contract
def _stream(device):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _both(device, fn, specs, what):
    def run(*args):
        with torch.cuda.device(device):
            _lib.check(fn(*args, _stream(device)), what)
    return F.run_both(run, specs, device, what=what)


def _refusals(device, fn, calls, i_ws, i_out, what):
    """256 bytes too few, then the pointer moved by 128 bytes: KEMR_ERR_WORKSPACE both times, `out` still all 0xa5 and the workspace
    still all 0xff -- nothing was launched (tests/test_footprint_towers_gpu.py _refusals)."""
    ws, out = calls.win[i_ws], calls.win[i_out]
    as_ptr = lambda t: C.c_void_p(t.data_ptr())          # noqa: E731
    for shift, less in ((0, 256), (128, 0)):
        ws.refill_body(F.POISON)
        out.refill_body(F.GUARD)
        args = calls.args(True, as_ptr)
        args[i_ws] = C.c_void_p(ws.ptr + shift)
        args[i_ws + 1] = ws.nbytes - less
        with torch.cuda.device(device):
            rc = fn(*args, _stream(device))
        torch.cuda.synchronize(device)
        assert rc == ERR_WORKSPACE, (what, shift, less, rc, _lib.lib().kemr_last_error())
        assert F.all_bytes(out.view, F.GUARD) and F.all_bytes(ws.view, F.POISON), (what, shift, less)
        assert ws.margins_intact() and out.margins_intact()


@pytest.mark.parametrize("precision", ["bf16-x24", "bf16", "bf16-res16"])
def test_encoder_inside_its_workspace(device, precision):
    """kemr_encode_text_packed of a family-2 model twice -- a roomy zeroed workspace, and one of EXACTLY
    kemr_text_packed_workspace_bytes with every byte 0xff (NaN in every slot) inside guard margins, ids and lens inside margins --
    gives the same bits with every margin intact; then the refusals.  Batches: three ragged texts (the shortest 1), and the sixteen
    lengths (2 418 rows: the persistent GEMM's whole-tile stores land in the pad rows)."""
    L = _lib.lib()
    eng = _engine(device, precision)
    for lens_list in ([1, 512, 5], B.SHUFFLED):
        ids, lens = B.random_ids(lens_list, seed=3)
        batch, rows = len(lens_list), int(sum(lens_list))
        need = int(L.kemr_text_packed_workspace_bytes(eng._h, rows, batch))
        calls = _both(device, L.kemr_encode_text_packed,
                      [eng._h, IntIn(ids), IntIn(lens), rows, batch, Out((batch, 256), F32), int(batch == 3), Work(need, need + (1 << 20), 8 * 256),
                       SizeOf(7)], f"bert encode_text_packed {precision} batch={batch}")
        assert bool(torch.isfinite(calls.win[5].view).all())
        _refusals(device, L.kemr_encode_text_packed, calls, 7, 5, f"bert encode_text_packed {precision} batch={batch}")


def test_front_inside_its_workspace_and_refusals(device):
    L = _lib.lib()
    eng = _engine(device)
    ids, lens = B.random_ids([1, 512, 5], seed=3)
    rows, batch = 518, 3
    need = int(L.kemr_text_packed_workspace_bytes(eng._h, rows, batch))
    calls = _both(device, L.kemr_debug_bert_front,
                  [eng._h, IntIn(ids), IntIn(lens), rows, batch, Out((rows, 3 * 256), torch.uint8), Out((rows, 256), torch.bfloat16),
                   Out((batch + 1,), torch.int32), Work(need, need + (1 << 20), 8 * 256), SizeOf(8)], "debug_bert_front")
    assert calls.win[7].view.tolist() == [0, 1, 513, 518]
    _refusals(device, L.kemr_debug_bert_front, calls, 8, 5, "debug_bert_front")
    # the calls a family-2 model does not serve, and a row count outside batch .. batch * ctx: refused before anything is launched
    dev = lambda t: C.c_void_p(t.to(device).data_ptr())          # noqa: E731
    out = torch.zeros(3, 256, device=device)
    ws = torch.zeros(need, dtype=torch.uint8, device=device)
    idd, ld = ids.to(device), lens.to(device)
    p = lambda t: C.c_void_p(t.data_ptr())                       # noqa: E731
    assert L.kemr_encode_text(eng._h, p(idd), 3, p(out), 0, p(ws), need, None) == -1 and b"kemr_encode_text_packed" in L.kemr_last_error()
    assert L.kemr_encode_image(eng._h, p(idd), 3, p(out), 0, p(ws), need, None) == -1 and b"family 2" in L.kemr_last_error()
    assert L.kemr_encode_text_packed(eng._h, p(idd), p(ld), 2, 3, p(out), 0, p(ws), need, None) == -1 and b"2 rows for 3 texts" in L.kemr_last_error()
    assert L.kemr_encode_text_packed(eng._h, p(idd), p(ld), 3 * 512 + 1, 3, p(out), 0, p(ws), 1 << 40, None) == -1
    with pytest.raises(ValueError, match="not served for this family"):
        engine.BertEngine(B.ARCH, device, "fp32x3")


# ------------------------------------------------------------------------------------------------ Python surface
@pytest.fixture(scope="module")
def checkpoint(tmp_path_factory):
    return B.save_directory(tmp_path_factory.mktemp("bert"), _weights("plain"))


def test_sentence_encoder_matches_the_cpu_statement(device, checkpoint):
    """SentenceEncoder.from_pretrained(dir).encode(texts, normalize_embeddings=True): rows in input order, each within the bar of
    bert_ref on the tokenizer's own ids."""
    enc = SentenceEncoder.from_pretrained(checkpoint, device=device)
    assert enc.arch == B.ARCH and enc.get_sentence_embedding_dimension() == 256
    texts = B.sentences(24, seed=6, lo=1, hi=120) + ["", B.sentences(1, seed=8, lo=600, hi=600)[0]]          # the last one is truncated at 512
    got = enc.encode(texts, normalize_embeddings=True)
    assert got.shape == (26, 256) and got.dtype.name == "float32"
    ids, lens = enc.tokenize(texts)
    assert int(lens.max()) == 512 and int(lens.min()) == 2
    ref = B.encode(_weights("plain"), B.ARCH, ids, lens, normalize=True)
    gap = B.one_minus_cos(torch.from_numpy(got), ref)
    print(f"BERT sentence_encoder_max_1_minus_cos {float(gap.max()):.3g}")
    assert float(gap.max()) <= BAR, gap.tolist()
    one = enc.encode(texts[3], convert_to_tensor=True, normalize_embeddings=True)
    assert one.is_cuda and one.shape == (256,) and float(B.one_minus_cos(one[None], ref[3:4])) <= BAR


def test_evaluate_text_model_on_the_toy_set(device, checkpoint):
    """evaluate_text_model (the reference's signature and T2T_* keys) on 64 (query, target) pairs whose oracle score margins exceed
    2e-3: the metrics are the ones oracle.metrics_ref gives on the oracle embeddings; likewise the MRR-only form."""
    from knowledge_enhanced_multimodal_retrieval_amd import evaluators as E
    from oracle import metrics_ref
    enc = SentenceEncoder.from_pretrained(checkpoint, device=device)
    queries, targets, q, t = B.toy_set(_weights("plain"), enc.tokenize)
    assert B.score_margin(q, t) > 2e-3
    dataset = list(zip(queries, targets))
    want = metrics_ref.retrieval_metrics(q.numpy(), t.numpy(), prefix="T2T")
    got = E.evaluate_text_model(enc, dataset, batch_size=24, device="cuda", seed=42)
    print(f"BERT evaluate_text_model {got}")
    assert sorted(got) == sorted(want) == ["T2T_MRR", "T2T_Mean_Rank", "T2T_R@1", "T2T_R@10", "T2T_R@20", "T2T_R@5"]
    for k in want:
        assert got[k] == pytest.approx(want[k], rel=1e-9, abs=1e-9), (k, got[k], want[k])
    mrr = E.evaluate_text_model_for_training(enc, dataset, batch_size=64)
    assert sorted(mrr) == ["T2T_MRR", "T2T_Mean_Rank"] and mrr["T2T_MRR"] == pytest.approx(want["T2T_MRR"], rel=1e-9)


def test_variant_metrics_equal_the_references_numpy_form(device):
    """The legacy script's single and multi modes through ranking.ranks_of_groups (pair scores + one rank-only sim_topk pass with
    text_to_artifact as the group) against the reference's statement in numpy: argsort of -S, the position of the first candidate of
    the query's own artifact."""
    import numpy as np
    from knowledge_enhanced_multimodal_retrieval_amd import evaluators as E
    g = torch.Generator().manual_seed(12)
    n, d = 40, 256
    base = torch.randn(n, d, generator=g)
    var = [torch.nn.functional.normalize(base + 4.0 * torch.randn(n, d, generator=g), dim=-1) for _ in range(5)]

    def numpy_form(mode):
        ranks = []
        for qv in ([0] if mode == "single" else range(5)):
            others = [v for v in range(5) if v != qv]
            cand = np.stack([var[v][a].double().numpy() for a in range(n) for v in others])
            owner = np.array([a for a in range(n) for _ in others])
            s = var[qv].double().numpy() @ cand.T
            for i in range(n):
                order = np.argsort(-s[i], kind="stable")
                ranks.append(int(np.where(owner[order] == i)[0][0]) + 1)
        r = np.array(ranks)
        out = {f"T2T_R@{k}": float(np.mean(r <= k) * 100) for k in (1, 5, 10, 20)}
        out.update(T2T_MRR=float(np.mean(1.0 / r) * 100), T2T_Mean_Rank=float(np.mean(r)))
        return out

    for mode in ("single", "multi"):
        got, want = E.variant_metrics([v.to(device) for v in var], mode), numpy_form(mode)
        assert sorted(got) == sorted(want)
        for k in want:
            assert got[k] == pytest.approx(want[k], rel=1e-9), (mode, k, got[k], want[k])
        assert 1.0 < want["T2T_Mean_Rank"]                          # not a trivial case
