"""GPU: the knowledge-fused rerank -- FusionModel.rerank(bonus=...) (CLIP shortlist with bonus -> learned head on the listed pairs ->
head_weight * head + bonus by kemr_list_fuse -> ranks and top-k), the online route of CLIPRetriever / RetrievalEngine and the
evaluator's --sparql_results.  The fuse stage is compared bit for bit with its numpy restatement (tests/list_fuse_ref.py) applied to
the head's own listed scores; the linear head, whose listed scores are bit-identical to forward(), also against the dense route."""
import json
import warnings

import numpy as np
import pytest
import torch

import list_fuse_ref as ref
from knowledge_enhanced_multimodal_retrieval_amd import ranking
from knowledge_enhanced_multimodal_retrieval_amd.fusion_model import FusionModel
from oracle import clip_ref, metrics_ref

pytestmark = pytest.mark.gpu

N, M, D = 70, 300, 128
HEAD_WEIGHT = 0.8


def _unit(n, d, g):
    return torch.nn.functional.normalize(torch.randn(n, d, generator=g), dim=-1).numpy()


def _head(ft, d, g, matrix_scale, vector_scale):
    fm = FusionModel(torch.nn.Linear(1, 1), fusion_type=ft, embed_dim=d)
    with torch.no_grad():
        for p_ in fm.fusion_head.parameters():
            p_.copy_(torch.randn(p_.shape, generator=g) * (matrix_scale if p_.dim() > 1 else vector_scale))
    return fm


def _bonus(rng, n, m, per_row=8):
    """A CSR of ~per_row hits of 0.2 per query; row 0 is empty, row 1 lists one candidate three times with an order-dependent sum,
    row 2 has columns outside the gallery."""
    ptr, cols, vals = [0], [], []
    for r in range(n):
        entries = [] if r == 0 else [(int(c), 0.2) for c in rng.choice(m, per_row, replace=False)]
        if r == 1:
            entries += [(17, 1e8), (17, -1e8), (17, 1.0)]
        if r == 2:
            entries += [(m + 4, 0.5), (2 ** 31 - 2, 0.5)]
        entries.sort(key=lambda e: e[0])
        cols += [e[0] for e in entries]
        vals += [e[1] for e in entries]
        ptr.append(len(cols))
    return np.asarray(ptr, np.int32), np.asarray(cols, np.int32), np.asarray(vals, np.float32)


@pytest.fixture(scope="module")
def case(device):
    """Per head: the model, its prepared gallery, and the shared queries / candidates / bonus (computed once, never modified)."""
    g = torch.Generator().manual_seed(31)
    q, im, tg = _unit(N, D, g), _unit(M, D, g), _unit(M, D, g)
    out = {"q": q, "im": im, "tg": tg, "bonus": _bonus(np.random.default_rng(31), N, M), "gt": np.arange(N, dtype=np.int32)}
    for ft in ("linear", "cross_attention"):
        fm = _head(ft, D, g, 0.1 if ft == "cross_attention" else 0.5, 0.1 if ft == "cross_attention" else 0.3).to(device)
        out[ft] = (fm, fm.prepare_gallery(im, tg))
    return out


def _check_against_restatement(fm, gal, q, result, depth, k, head_weight, bonus, gt, device):
    ranks, top_s, top_i, list_s, list_i = result
    ids = list_i.cpu().numpy()
    head = fm.list_scores(ranking.to_device_f32(q, device), gal, list_i).cpu().numpy()                # the head's own listed scores
    fused, ahead, found, _ = ref.list_fuse(head, ids, depth, head_weight, bonus, gt)
    assert np.array_equal(ref.bits(list_s.cpu().numpy()), ref.bits(fused))
    want_s, want_i = ref.sorted_rows(fused, ids, k)
    assert np.array_equal(top_i.cpu().numpy(), want_i) and np.array_equal(ref.bits(top_s.cpu().numpy()), ref.bits(want_s))
    if gt is None:
        assert ranks is None
    else:
        assert ranks.dtype == torch.int64
        assert np.array_equal(ranks.cpu().numpy(), np.where(found == 1, ahead.astype(np.int64) + 1, depth + 1))
    return fused, found


@pytest.mark.parametrize("ft", ["linear", "cross_attention"])
@pytest.mark.parametrize("depth", [64, 300])
def test_fused_rerank_equals_the_restatement_on_the_heads_own_lists(device, case, ft, depth):
    fm, gal = case[ft]
    q, bonus, gt = case["q"], case["bonus"], case["gt"]
    res = fm.rerank(q, gal, depth=depth, k=10, gt_idx="diag", bonus=bonus, head_weight=HEAD_WEIGHT)
    _, found = _check_against_restatement(fm, gal, q, res, depth, 10, HEAD_WEIGHT, bonus, gt, device)
    assert found.all() if depth == M else 0 < found.sum()
    # the shortlist is the deep route's list under the fused score PLUS the bonus
    _, _, theirs = ranking.ranks_and_topk_deep([q, q], [case["im"], case["tg"]], weights=[0.5, 0.5], k=depth, gt_idx=None, bonus=bonus)
    assert torch.equal(res[4], theirs)
    # without a ground truth: the same lists and top-k, no ranks
    res2 = fm.rerank(q, gal, depth=depth, k=10, bonus=bonus, head_weight=HEAD_WEIGHT)
    assert res2[0] is None and all(torch.equal(a, b) for a, b in zip(res[1:], res2[1:]))
    # an external list replaces the shortlist stage
    cand = res[4].cpu().numpy()[:, ::-1].copy()
    res3 = fm.rerank(q, gal, depth=depth, k=10, gt_idx=gt, cand_idx=cand, bonus=bonus, head_weight=HEAD_WEIGHT)
    _check_against_restatement(fm, gal, q, res3, depth, 10, HEAD_WEIGHT, bonus, gt, device)
    assert torch.equal(res3[0], res[0]) and torch.equal(res3[2], res[2])


def test_linear_fused_rerank_at_full_depth_equals_the_dense_route(device, case):
    """depth = M: the list holds every candidate and the linear head's listed scores have the bits of forward(), so ranks and top-k
    must equal those of head_weight * forward() + dense bonus ranked over the full matrix (kemr_rank_dense) -- no tolerance."""
    fm, gal = case["linear"]
    q, bonus, gt = case["q"], case["bonus"], case["gt"]
    dense = fm(ranking.to_device_f32(q, device), ranking.to_device_f32(case["im"], device), ranking.to_device_f32(case["tg"], device))
    F = (np.float32(HEAD_WEIGHT) * dense.cpu().numpy()).astype(np.float32)
    ptr, col, val = bonus
    with np.errstate(over="ignore"):
        for r in range(N):
            for e in range(ptr[r], ptr[r + 1]):
                if col[e] < M:
                    F[r, col[e]] = np.float32(F[r, col[e]] + val[e])
    d_ranks, d_top_s, d_top_i = ranking.ranks_of_matrix(torch.from_numpy(F).to(device), k=10, gt_idx=gt)
    ranks, top_s, top_i, list_s, list_i = fm.rerank(q, gal, depth=M, k=10, gt_idx=gt, bonus=bonus, head_weight=HEAD_WEIGHT)
    assert torch.equal(list_s, torch.gather(torch.from_numpy(F).to(device), 1, list_i.long()))
    assert torch.equal(ranks, d_ranks) and torch.equal(top_i, d_top_i) and torch.equal(top_s, d_top_s)


@pytest.mark.parametrize("ft", ["linear", "cross_attention"])
def test_a_hit_that_clip_ranks_below_the_depth_reaches_the_list(device, case, ft):
    fm, gal = case[ft]
    q, depth = case["q"], 50
    _, _, order = ranking.ranks_and_topk_deep([q, q], [case["im"], case["tg"]], weights=[0.5, 0.5], k=M, gt_idx=None)
    hit = order[:, 200].cpu().numpy().astype(np.int32)                                  # CLIP rank 201 > depth
    bonus = (np.arange(N + 1, dtype=np.int32), hit, np.full(N, 100.0, np.float32))
    ranks, top_s, top_i, list_s, list_i = fm.rerank(q, gal, depth=depth, k=5, gt_idx=hit, bonus=bonus, head_weight=HEAD_WEIGHT)
    assert bool((list_i == torch.from_numpy(hit).to(device)[:, None]).any(dim=1).all())
    assert np.array_equal(top_i[:, 0].cpu().numpy(), hit) and bool((ranks == 1).all())
    ranks, top_s, top_i, list_s, list_i = fm.rerank(q, gal, depth=depth, k=5, gt_idx=hit, bonus=bonus, head_weight=HEAD_WEIGHT,
                                                    shortlist_bonus=False)
    assert not bool((list_i == torch.from_numpy(hit).to(device)[:, None]).any()) and bool((ranks == depth + 1).all())
    plain = fm.rerank(q, gal, depth=depth, k=5)
    assert torch.equal(list_i, plain[4])                                               # the plain shortlist, fused scores on it


@pytest.mark.parametrize("ft", ["linear", "cross_attention"])
def test_without_bonus_the_call_is_the_plain_rerank(device, case, ft):
    fm, gal = case[ft]
    q, gt, depth = case["q"], case["gt"], 64
    qd = ranking.to_device_f32(q, device)
    before = fm._rerank_lists(qd, gal, fm.shortlist(qd, gal.fused_panel, depth), 10, torch.from_numpy(gt).to(device))
    now = fm.rerank(q, gal, depth=depth, k=10, gt_idx=gt, bonus=None, head_weight=1.0, shortlist_bonus=True)
    assert all(torch.equal(a, b) for a, b in zip(before, now))
    # ... and a bonus without any hit at head_weight 1 gives its bits by the fused route
    empty = (np.zeros(N + 1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32))
    fused = fm.rerank(q, gal, depth=depth, k=10, gt_idx=gt, bonus=empty, head_weight=1.0)
    assert all(torch.equal(a, b) for a, b in zip(now, fused))
    nowhere = (np.arange(N + 1, dtype=np.int32), np.full(N, M + 7, np.int32), np.ones(N, np.float32))      # hits outside the gallery
    fused = fm.rerank(q, gal, depth=depth, k=10, gt_idx=gt, bonus=nowhere, head_weight=1.0)
    assert all(torch.equal(a, b) for a, b in zip(now, fused))
    with pytest.raises(ValueError, match="head_weight"):
        fm.rerank(q, gal, depth=depth, k=10, head_weight=0.5)
    with pytest.raises(ValueError, match=f"{N + 1} entries"):
        fm.rerank(q, gal, depth=depth, k=10, bonus=(empty[0][:-1], empty[1], empty[2]))


@pytest.mark.parametrize("ft", ["linear", "cross_attention"])
def test_online_fused_reranked_search(device, ft):
    from knowledge_enhanced_multimodal_retrieval_amd.clip_module import CLIP
    from knowledge_enhanced_multimodal_retrieval_amd.config import ARCHS
    from knowledge_enhanced_multimodal_retrieval_amd.retriever import CLIPRetrieval, CLIPRetriever, EmbeddingStore, RetrievalEngine
    arch, oa = ARCHS["tiny"], clip_ref.ARCHS["tiny"]
    model = CLIP(arch)
    model.load_state_dict(clip_ref.random_state_dict(oa, seed=0))
    model = model.to(device).eval()
    n = 300
    img, _, txt = metrics_ref.planted_embeddings(n, arch.embed_dim, seed=1)
    store = EmbeddingStore(img, txt, [f"u{i:04d}" for i in range(n)], device)
    words = {}

    def tok(texts):                                        # tiny vocab: a fixed toy tokenizer
        out = torch.zeros(len(texts), arch.ctx, dtype=torch.int32)
        for r, s in enumerate(texts):
            ids = [arch.sot] + [1 + words.setdefault(w, len(words)) % (arch.sot - 1) for w in s.split()][:arch.ctx - 2] + [arch.eot]
            out[r, :len(ids)] = torch.tensor(ids, dtype=torch.int32)
        return out

    ret = CLIPRetriever(model, store, tokenize_fn=tok)
    fm = _head(ft, arch.embed_dim, torch.Generator().manual_seed(4), 0.1 if ft == "cross_attention" else 0.5, 0.1).to(device)
    gal = fm.prepare_gallery(store.image, store.text)
    queries = ["bronze statue of a seated king", "blue glazed bowl", "a map of the northern coast drawn in ink"]
    hits = [["u0007", "http://example.org/artefact/u0250", "unknown-id"], [], ["u0299", "u0299", "u0001"]]
    top_s, top_i = ret.search_batch_reranked_fused(queries, hits, fm, gal, depth=120, top_k=50, head_weight=0.7, hit_bonus=0.3)
    assert tuple(top_i.shape) == (3, 50) and bool((top_i >= 0).all())
    q = model.encode_text(tok(queries), normalize=True)
    bonus = store.hits_csr(hits, 0.3)
    assert bonus[1].tolist() == [7, 250, 1, 299]
    _, want_s, want_i, _, list_i = fm.rerank(q, gal, depth=120, k=50, bonus=bonus, head_weight=0.7)
    assert torch.equal(top_i, want_i) and torch.equal(top_s, want_s)
    for r, cols in enumerate(([7, 250], [], [1, 299])):                                # every hit was shortlisted
        assert set(cols) <= set(list_i[r].cpu().tolist())
    one = ret.search_reranked_fused(queries[0], hits[0], fm, gal, depth=120, top_k=50, head_weight=0.7, hit_bonus=0.3)
    assert [h["uuid"] for h in one] == [store.uuids[i] for i in top_i[0].cpu().tolist()]
    assert [h["score"] for h in one] == [float(s) for s in top_s[0].cpu().tolist()]
    with pytest.raises(ValueError):
        ret.search_batch_reranked_fused(queries, hits[:2], fm, gal)
    with pytest.raises(ValueError):
        ret.search_batch_reranked_fused(queries, hits, fm, gal, depth=40, top_k=41)

    class T2S:
        def retrieval(self, query):
            return hits[queries.index(query)]
    eng = RetrievalEngine(CLIPRetrieval(retriever=ret), T2S())
    got = eng.retrieve_text_reranked(queries[2], fm, gal, alpha=0.7, beta=0.3, threshold=-1e9, depth=120)
    full = ret.search_reranked_fused(queries[2], hits[2], fm, gal, depth=120, top_k=120, head_weight=0.7, hit_bonus=0.3)
    assert got == [{"uuid": h["uuid"], "score": round(h["score"], 4)} for h in full] and len(got) == 120
    cut = sorted(h["score"] for h in got)[60]
    assert eng.retrieve_text_reranked(queries[2], fm, gal, alpha=0.7, beta=0.3, threshold=cut, depth=120) == [h for h in got if h["score"] >= cut]


def _fusion_main(tmp_path, name, *extra):
    from src.clip.eval import evaluator_fusion as EF
    out = tmp_path / f"{name}.json"
    torch.manual_seed(1234)                                    # the head is freshly initialised inside main: the same one in every call
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = EF.main(["--model_name", "ViT-B/32", "--fusion_type", "linear", "--device", "cuda", "--synthetic", "80",
                       "--output_file", str(out), *extra])
    assert json.loads(out.read_text())["metrics"] == res["metrics"]
    return res["metrics"]


def test_evaluator_with_sparql_results(device, tmp_path):
    """Every query's result file names its own ground truth: under the additive strategy (head_weight 1, + 0.5 on the hit) no rank
    can get worse than the plain rerank's, and the list holds every ground truth."""
    hits = tmp_path / "t2s"
    hits.mkdir()
    for i in range(80):
        (hits / f"synthetic-{i:06d}.txt").write_text(f"http://example.org/artefact/synthetic-{i:06d}\n")
    plain = _fusion_main(tmp_path, "plain", "--rerank_depth", "40")
    fused = _fusion_main(tmp_path, "fused", "--rerank_depth", "40", "--sparql_results", str(hits), "--sparql_strategy", "additive")
    assert fused["Head_Weight"] == 1.0 and fused["SPARQL_Strategy"] == "additive" and fused["Rerank_Depth"] == 40
    assert fused["Shortlist_Recall"] == 100.0 >= plain["Shortlist_Recall"]
    assert fused["MRR"] >= plain["MRR"] and fused["Mean_Rank"] <= plain["Mean_Rank"] and fused["R@1"] >= plain["R@1"]
    weighted = _fusion_main(tmp_path, "weighted", "--rerank_depth", "40", "--sparql_results", str(hits))
    assert weighted["Head_Weight"] == pytest.approx(0.7) and weighted["SPARQL_Strategy"] == "weighted"
