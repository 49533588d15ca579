"""GPU: the MPNet sentence encoder (model family 3) end to end -- kemr_encode_text_packed against the CPU statement tests/mpnet_ref.py
(fp32) at the project's embedding bar 1 - cos <= 1e-3 (tests/test_mpnet_host.py shows that the bar sees a wrong bias: each of four
wrong tables is >= 2e-3 away), packed against alone, the memory contract (tests/footprint.py), the Python surface
(SentenceEncoder.from_pretrained on a saved MPNet directory, evaluate_text_model), and a family-2 model in the same process."""
import ctypes as C

import pytest
import torch

import bert_ref as B
import footprint as F
import mpnet_ref as M
from footprint import IntIn, Out, SizeOf, Work
from knowledge_enhanced_multimodal_retrieval_amd import _lib, debug, engine
from knowledge_enhanced_multimodal_retrieval_amd.sentence_model import SentenceEncoder

pytestmark = pytest.mark.gpu

BAR = 1e-3                     # the project's embedding bar: 1 - cos against the fp32 statement
ERR_WORKSPACE = -4             # include/kemr.h KEMR_ERR_WORKSPACE
F32 = torch.float32
ARCHS = {"1e-5": M.ARCH, "1e-12": M.ARCH12}


def _weights(kind):
    return M.cached(("mpnet_sd", kind), lambda: (M.heavy_state_dict if kind == "heavy" else M.random_state_dict)(M.ARCH, 0))


def _engine(device, precision=_lib.DEFAULT_PRECISION, kind="plain", eps="1e-5"):
    eng = engine.BertEngine(ARCHS[eps], device, precision)
    eng.load_state_dict(_weights(kind))
    return eng


def _inputs(order="sorted"):
    return M.random_ids(M.LENGTHS if order == "sorted" else M.SHUFFLED, seed=1 if order == "sorted" else 2)


def _oracle(kind, order, eps="1e-5"):
    ids, lens = _inputs(order)
    return M.cached(("mpnet_oracle", kind, order, eps), lambda: M.encode(_weights(kind), ARCHS[eps], ids, lens, normalize=True))


@pytest.mark.parametrize("eps", ["1e-5", "1e-12"])
@pytest.mark.parametrize("kind", ["plain", "heavy"])
def test_encoder_matches_the_cpu_statement(device, kind, eps):
    """All sixteen lengths 1 .. 512 in one packed call of 2 418 rows, then in shuffled order: every item within 1 - cos <= 1e-3 of
    mpnet_ref (fp32), on plain and on heavy-tailed weights, at both LayerNorm eps values; unit norms."""
    eng = _engine(device, kind=kind, eps=eps)
    v = C.c_int(0)
    _lib.check(_lib.lib().kemr_model_get_option(eng._h, b"family", C.byref(v)))
    assert v.value == 3
    _lib.check(_lib.lib().kemr_model_get_option(eng._h, b"layer_norm_eps", C.byref(v)))
    assert v.value == (5 if eps == "1e-5" else 12)
    for order in ("sorted", "shuffled"):
        ids, lens = _inputs(order)
        got = eng.encode_ids(ids, lens, normalize=True).cpu()
        assert bool(torch.isfinite(got).all())
        gap = M.one_minus_cos(got, _oracle(kind, order, eps))
        print(f"MPNET encoder_{kind}_eps{eps}_{order}_max_1_minus_cos {float(gap.max()):.3g} (at length {int(lens[int(gap.argmax())])})")
        assert float(gap.max()) <= BAR, (kind, eps, order, gap.tolist())
        assert float((got.norm(dim=-1) - 1).abs().max()) < 1e-5


def test_fp32_stream_precision(device):
    eng = _engine(device, "bf16")
    ids, lens = _inputs("shuffled")
    gap = M.one_minus_cos(eng.encode_ids(ids, lens, normalize=True).cpu(), _oracle("plain", "shuffled"))
    assert float(gap.max()) <= BAR, gap.tolist()


def test_packed_equals_alone(device):
    """tests/test_bert_encoder_gpu.py test_packed_equals_alone for family 3: with the GEMM routing held the same (gemm_variant = 1) a
    text inside the packed batch and the same text alone are BIT-IDENTICAL -- the biased attention works per item, a text's positions
    start at 0 wherever it is packed --; with the automatic routing 1 - cos <= 1e-6; two calls of a batch give the same bits."""
    eng = _engine(device)
    ids, lens = _inputs("shuffled")
    picks = [0, 5, 9, len(M.SHUFFLED) - 1] + [M.SHUFFLED.index(1), M.SHUFFLED.index(512)]
    with debug.override(gemm_variant=1):
        packed = eng.encode_ids(ids, lens).clone()
        for i in picks:
            alone = eng.encode_ids(ids[i:i + 1], lens[i:i + 1])
            assert F.same_bits(alone[0], packed[i]), (i, int(lens[i]))
    packed = eng.encode_ids(ids, lens).clone()
    worst = 0.0
    for i in picks:
        alone = eng.encode_ids(ids[i:i + 1], lens[i:i + 1])
        worst = max(worst, float(M.one_minus_cos(alone, packed[i:i + 1])))
    print(f"MPNET packed_vs_alone_auto_routing_max_1_minus_cos {worst:.3g}")
    assert worst <= 1e-6, worst
    assert F.same_bits(eng.encode_ids(ids, lens), packed)


# ------------------------------------------------------------------------------------------------ memory contract
def _stream(device):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


@pytest.mark.parametrize("precision", ["bf16-x24", "bf16-res16"])
def test_encoder_inside_its_workspace(device, precision):
    """kemr_encode_text_packed of a family-3 model twice -- a roomy zeroed workspace, and one of EXACTLY
    kemr_text_packed_workspace_bytes with every byte 0xff inside guard margins, ids and lens inside margins -- gives the same bits with
    every margin intact; then a workspace 256 bytes short is refused with nothing launched."""
    L = _lib.lib()
    eng = _engine(device, precision)
    fn = L.kemr_encode_text_packed

    def run(*args):
        with torch.cuda.device(device):
            _lib.check(fn(*args, _stream(device)), "encode_text_packed")
    for lens_list in ([1, 512, 5], M.SHUFFLED):
        ids, lens = M.random_ids(lens_list, seed=3)
        batch, rows = len(lens_list), int(sum(lens_list))
        need = int(L.kemr_text_packed_workspace_bytes(eng._h, rows, batch))
        calls = F.run_both(run, [eng._h, IntIn(ids), IntIn(lens), rows, batch, Out((batch, 256), F32), int(batch == 3),
                                 Work(need, need + (1 << 20), 8 * 256), SizeOf(7)], device, what=f"mpnet encode_text_packed {precision} batch={batch}")
        assert bool(torch.isfinite(calls.win[5].view).all())
        ws, out = calls.win[7], calls.win[5]
        ws.refill_body(F.POISON)
        out.refill_body(F.GUARD)
        args = calls.args(True, lambda t: C.c_void_p(t.data_ptr()))
        args[8] = ws.nbytes - 256
        with torch.cuda.device(device):
            rc = fn(*args, _stream(device))
        torch.cuda.synchronize(device)
        assert rc == ERR_WORKSPACE, (rc, L.kemr_last_error())
        assert F.all_bytes(out.view, F.GUARD) and F.all_bytes(ws.view, F.POISON) and ws.margins_intact() and out.margins_intact()


# ------------------------------------------------------------------------------------------------ Python surface
@pytest.fixture(scope="module")
def checkpoint(tmp_path_factory):
    return M.save_directory(tmp_path_factory.mktemp("mpnet"), _weights("plain"), pooling="mean")


def test_sentence_encoder_matches_the_cpu_statement(device, checkpoint):
    """SentenceEncoder.from_pretrained(<saved MPNet dir>).encode(texts, normalize_embeddings=True): rows in input order, each within the
    bar of mpnet_ref on the tokenizer's own ids (<s> ... </s>, the last text truncated at 512 keeping </s>)."""
    enc = SentenceEncoder.from_pretrained(checkpoint, device=device)
    assert enc.arch == M.ARCH and enc.arch.relative_bias and enc.get_sentence_embedding_dimension() == 256
    texts = M.sentences(24, seed=6, lo=1, hi=120) + ["", M.sentences(1, seed=8, lo=600, hi=600)[0]]
    got = enc.encode(texts, normalize_embeddings=True)
    assert got.shape == (26, 256) and got.dtype.name == "float32"
    ids, lens = enc.tokenize(texts)
    assert int(lens.max()) == 512 and int(lens.min()) == 2
    assert all(int(ids[i, 0]) == M.BOS and int(ids[i, int(lens[i]) - 1]) == M.EOS for i in range(26))
    ref = M.encode(_weights("plain"), M.ARCH, ids, lens, normalize=True)
    gap = M.one_minus_cos(torch.from_numpy(got), ref)
    print(f"MPNET sentence_encoder_max_1_minus_cos {float(gap.max()):.3g}")
    assert float(gap.max()) <= BAR, gap.tolist()
    one = enc.encode(texts[3], convert_to_tensor=True, normalize_embeddings=True)
    assert one.is_cuda and one.shape == (256,) and float(M.one_minus_cos(one[None], ref[3:4])) <= BAR


def test_evaluate_text_model_on_the_toy_set(device, checkpoint):
    """evaluate_text_model on 64 (query, target) pairs whose oracle score margins exceed 2e-3: the metrics (ranks) are the ones
    oracle.metrics_ref gives on the oracle embeddings."""
    from knowledge_enhanced_multimodal_retrieval_amd import evaluators as E
    from oracle import metrics_ref
    enc = SentenceEncoder.from_pretrained(checkpoint, device=device)
    queries, targets, q, t = M.toy_set(_weights("plain"), enc.tokenize)
    assert M.score_margin(q, t) > 2e-3
    dataset = list(zip(queries, targets))
    want = metrics_ref.retrieval_metrics(q.numpy(), t.numpy(), prefix="T2T")
    got = E.evaluate_text_model(enc, dataset, batch_size=24, device="cuda", seed=42)
    print(f"MPNET evaluate_text_model {got}")
    assert sorted(got) == sorted(want) == ["T2T_MRR", "T2T_Mean_Rank", "T2T_R@1", "T2T_R@10", "T2T_R@20", "T2T_R@5"]
    for k in want:
        assert got[k] == pytest.approx(want[k], rel=1e-9, abs=1e-9), (k, got[k], want[k])


def test_family_2_is_untouched_by_a_family_3_model_in_the_process(device):
    """A BERT (family 2) engine gives bit-identical embeddings before and after an MPNet (family 3) model was built and ran."""
    bert = engine.BertEngine(B.ARCH, device)
    bert.load_state_dict(B.cached("sd0", lambda: B.random_state_dict(B.ARCH, 0)))
    ids, lens = B.random_ids(B.SHUFFLED, seed=2)
    before = bert.encode_ids(ids, lens, normalize=True).clone()
    mp = _engine(device)
    mids, mlens = _inputs("shuffled")
    other = mp.encode_ids(mids, mlens, normalize=True).clone()
    after = bert.encode_ids(ids, lens, normalize=True)
    assert F.same_bits(before, after)
    assert float(B.one_minus_cos(before.cpu(), B.cached(("oracle", "plain", "shuffled", "mean"),
                                                       lambda: B.encode(B.cached("sd0", lambda: B.random_state_dict(B.ARCH, 0)), B.ARCH, ids, lens, "mean", normalize=True))).max()) <= BAR
    assert F.same_bits(mp.encode_ids(mids, mlens, normalize=True), other)
