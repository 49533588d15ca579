"""GPU: the knowledge-fused deep route (kemr_sim_topk_deep_fused) -- SPARQL bonus applied to the block of scores, ground-truth rank
count in the selection's first sweep -- from the C ABI up to RetrievalEngine.retrieve_text_fused.  Every expectation is exact (ids,
score BITS, integer counts) except the online scores, which pass through a four-decimal rounding (see that test)."""
import ctypes as C

import numpy as np
import pytest
import torch

from knowledge_enhanced_multimodal_retrieval_amd import _lib, engine, ranking, sparql_fusion
from oracle import clip_ref, fusion_ref, metrics_ref

pytestmark = pytest.mark.gpu

NQ, NG, D = 300, 1003, 64             # three query blocks of 128 (the last ragged); rows of 1003 floats: padded to a stride of 1004


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _ibits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------ exact-grid data, computed once
class Grid:
    """Embeddings with entries m / 8, m in -4 .. 4, two parts weighted 0.5 / 0.5: every product (m / 16)(m' / 8) and every partial
    sum of the 128 of them is a multiple of 1 / 128 below 2^24 / 128, exact in bf16 operands and fp32 accumulation (terms 1 and 3
    alike: the bf16 residuals are zero).  Bonus values are multiples of 1 / 64.  So the fp64 oracle's fused scores are the kernel's,
    and 1 003 candidates on a grid with a standard deviation of some 75 steps hold hundreds of exact ties per row."""

    def __init__(self):
        rng = np.random.default_rng(2024)
        self.q = (rng.integers(-4, 5, (NQ, D)) / 8.0).astype(np.float32)
        self.img = (rng.integers(-4, 5, (NG, D)) / 8.0).astype(np.float32)
        self.txt = (rng.integers(-4, 5, (NG, D)) / 8.0).astype(np.float32)
        self.gt = rng.permutation(NG)[:NQ].astype(np.int64)
        self.quuids = [f"q{i:03d}" for i in range(NQ)]
        self.auuids = [f"a{i:04d}" for i in range(NG)]
        uri = lambda c: f"http://example.org/artefact/{self.auuids[c]}" if c % 3 == 0 else self.auuids[c]
        pick = lambda n: [uri(int(c)) for c in rng.choice(NG, n, replace=False)]
        # one result dictionary per bonus value (the additive strategy: every LISTED hit adds delta, a duplicate adds twice)
        res = {0.25: {}, 0.5: {}, -0.25: {}}
        res[0.25]["q000"] = pick(60)                                        # 60 hits
        # q001: no hit
        res[0.5]["q002"] = pick(1) + ["http://example.org/artefact/unknown"]            # one hit (+ an id nobody knows)
        res[0.5]["q003"] = pick(80)                                         # more hits than k = 40
        dup = pick(5)
        res[0.25]["q004"] = dup + [dup[2]]                                  # a duplicated column: added twice
        res[-0.25]["q005"] = pick(40)                                       # negative values
        res[0.5]["q005"] = pick(10)
        res[0.5]["q006"] = [uri(int(self.gt[6]))] + pick(3)                 # a hit on the ground truth itself
        res[0.25]["q006"] = [uri(int(self.gt[6]))]                          # ... by two lists: one column, two values
        res[0.5]["q260"] = pick(30)                                         # third block; nothing like q000's list
        res[-0.25]["q299"] = pick(7)                                        # last row of the ragged block
        for r in range(7, NQ):
            if r not in (260, 299) and rng.random() < 0.5:
                res[float(rng.choice([0.25, 0.5, -0.25]))][self.quuids[r]] = pick(int(rng.integers(1, 12)))
        self.results = res
        S = 0.5 * (self.q.astype(np.float64) @ self.img.astype(np.float64).T) + 0.5 * (self.q.astype(np.float64) @ self.txt.astype(np.float64).T)
        self.S = S
        F = S
        rows, cols, vals = [], [], []
        for delta, results in res.items():
            F = fusion_ref.fuse(F, results, self.quuids, self.auuids, "additive", {"delta": delta})
            _, (ptr, col, val) = sparql_fusion.sparql_bonus(results, self.quuids, self.auuids, "additive", {"delta": delta})
            rows.append(np.repeat(np.arange(NQ), np.diff(ptr)))
            cols.append(col)
            vals.append(val)
        rows, cols, vals = np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)
        order = np.lexsort((cols, rows))                                    # stable: ascending columns within a row
        ptr = np.zeros(NQ + 1, np.int64)
        np.add.at(ptr, rows + 1, 1)
        self.bonus = (np.cumsum(ptr).astype(np.int32), cols[order].astype(np.int32), vals[order].astype(np.float32))
        self.F = F                                                          # fp64, exact
        assert np.array_equal(F.astype(np.float32).astype(np.float64), F)
        self.order = np.argsort(-F, axis=1, kind="stable")
        self.ranks = metrics_ref.ranks_by_count(F, self.gt)
        assert np.array_equal(self.ranks, metrics_ref.ranks_by_sort(F, self.gt))
        # the data does what the issue asks of it
        col_of = self.bonus[1][self.bonus[0][4]:self.bonus[0][5]]
        assert len(col_of) == 6 and len(set(col_of.tolist())) == 5
        assert self.bonus[0][2] - self.bonus[0][1] == 0 and self.bonus[0][3] - self.bonus[0][2] == 1 and self.bonus[0][1] == 60
        assert self.bonus[0][4] - self.bonus[0][3] == 80
        ties = np.mean([NG - len(np.unique(F[r])) for r in range(NQ)])
        assert ties > 200, ties


@pytest.fixture(scope="module")
def grid():
    return Grid()


@pytest.mark.parametrize("terms", [1, 3])
@pytest.mark.parametrize("k", [40, 1000])
def test_exact_grid_oracle_parity(device, grid, k, terms):
    """ids == stable argsort of the reference's fused matrix, scores == its fp32 cast, ahead + 1 == its ranks (three query blocks)."""
    precision = {1: "bf16", 3: "fp32x3"}[terms]
    ranks, top_s, top_i = ranking.ranks_and_topk_deep([grid.q, grid.q], [grid.img, grid.txt], weights=[0.5, 0.5], k=k,
                                                      precision=precision, gt_idx=grid.gt, bonus=grid.bonus, query_block=128)
    exp_i = grid.order[:, :k]
    exp_s = np.take_along_axis(grid.F, exp_i, 1).astype(np.float32)
    assert np.array_equal(top_i.cpu().numpy(), exp_i.astype(np.int32))
    assert np.array_equal(_bits(top_s.cpu().numpy()), _bits(exp_s))
    assert np.array_equal(ranks.cpu().numpy(), grid.ranks)


def _unit(rng, n, d):
    x = rng.standard_normal((n, d)).astype(np.float32)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def _random_bonus(rng, nq, n_cols, per_row=8):
    """Random-valued CSR (inexact fp32 sums), ascending columns, duplicated columns in every fourth row."""
    ptr, cols, vals = [0], [], []
    for r in range(nq):
        c = np.sort(rng.choice(n_cols, int(rng.integers(0, per_row + 1)), replace=False))
        if r % 4 == 0 and len(c):
            c = np.sort(np.concatenate([c, c[:2]]))
        cols.append(c)
        vals.append((rng.random(len(c)) * 0.4 - 0.1).astype(np.float32))
        ptr.append(ptr[-1] + len(c))
    return np.asarray(ptr, np.int32), np.concatenate(cols).astype(np.int32), np.concatenate(vals).astype(np.float32)


def test_routes_agree_bit_for_bit(device):
    """The first 32 entries of the fused deep list at k = 100 and the ahead counts are those of sim_topk(k = 32) with the same
    bonus list and ground truth: the bonus is added in the same order in fp32, the count uses the same predicate."""
    rng = np.random.default_rng(77)
    nq, ng, d = 130, 700, 768
    qp = engine.build_panel([torch.from_numpy(_unit(rng, nq, d)).to(device)], _lib.SIDE_QUERY, 3)
    gp = engine.build_panel([torch.from_numpy(_unit(rng, ng, d)).to(device)], _lib.SIDE_GALLERY, 3)
    bonus = _random_bonus(rng, nq, ng)
    gt = torch.from_numpy(rng.integers(0, ng, nq).astype(np.int32)).to(device)
    gt[:4] = torch.from_numpy(bonus[1][:4].copy()).to(device)           # some ground truths that sit on entries of the list
    sgt = engine.pair_scores(qp, gp, torch.arange(nq, dtype=torch.int32, device=device), gt) + ranking._bonus_of_pairs(bonus, gt, device)
    a32 = torch.zeros(nq, dtype=torch.int32, device=device)
    a100 = torch.zeros(nq, dtype=torch.int32, device=device)
    s32, i32 = engine.sim_topk(qp, gp, 32, 0, gt, sgt, a32, bonus)
    s100, i100 = engine.sim_topk_deep(qp, gp, 100, gt_idx=gt, gt_score=sgt, ahead=a100, bonus=bonus)
    assert torch.equal(i100[:, :32], i32) and torch.equal(_ibits(s100[:, :32]), _ibits(s32))
    assert torch.equal(a100, a32) and int(a32.sum()) > 0
    plain_s, _ = engine.sim_topk_deep(qp, gp, 100)
    assert not torch.equal(plain_s, s100)                                # the bonus did move the lists


def _fused_raw(qp, gp, k, top_s, top_i, gt=None, sgt=None, ahead=None, ptr=None, col=None, val=None, gallery_offset=0):
    """The C entry point itself (the wrapper refuses partial triples before the library sees them)."""
    L = _lib.lib()
    ws = torch.empty(int(L.kemr_sim_topk_deep_workspace_bytes(qp.rows, gp.rows, qp.kdim, max(k, 1))), dtype=torch.uint8, device=qp.device)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    status = L.kemr_sim_topk_deep_fused(p(qp.data), qp.rows, p(gp.data), gp.rows, qp.kdim, gallery_offset, k, p(top_s), p(top_i),
                                        p(gt), p(sgt), p(ahead), p(ptr), p(col), p(val), p(ws), ws.numel(),
                                        C.c_void_p(torch.cuda.current_stream(qp.device).cuda_stream))
    return status, (L.kemr_last_error() or b"").decode()


def test_identity_without_knowledge_arguments(device):
    """All six optional pointers NULL: the bits of kemr_sim_topk_deep."""
    rng = np.random.default_rng(5)
    nq, ng, k = 200, 1003, 333
    qp = engine.build_panel([torch.from_numpy(_unit(rng, nq, 96)).to(device)], _lib.SIDE_QUERY, 1)
    gp = engine.build_panel([torch.from_numpy(_unit(rng, ng, 96)).to(device)], _lib.SIDE_GALLERY, 1)
    want_s, want_i = engine.sim_topk_deep(qp, gp, k)
    top_s = torch.zeros((nq, k), dtype=torch.float32, device=device)
    top_i = torch.zeros((nq, k), dtype=torch.int32, device=device)
    status, msg = _fused_raw(qp, gp, k, top_s, top_i)
    assert status == 0, msg
    assert torch.equal(top_i, want_i) and torch.equal(_ibits(top_s), _ibits(want_s))


def test_shards_sum_and_merge(device, grid):
    """ng = 1003 split at 517: ahead accumulates over the two calls (on top of what it held) to the single-gallery count, ground
    truths in the other shard included; the two lists merge to the single-gallery list."""
    k, cut = 100, 517
    dev = device
    q = torch.from_numpy(grid.q).to(dev)
    qp = engine.build_panel([q, q], _lib.SIDE_QUERY, 3, part_scale=[0.5, 0.5])
    gt = torch.from_numpy(grid.gt.astype(np.int32)).to(dev)
    sgt = torch.from_numpy(grid.F[np.arange(NQ), grid.gt].astype(np.float32)).to(dev)
    assert ((grid.gt < cut).sum() > 50) and ((grid.gt >= cut).sum() > 50)
    cols = grid.bonus[1]
    assert (cols < cut).any() and (cols >= cut).any()
    ahead = torch.full((NQ,), 7, dtype=torch.int32, device=dev)          # pre-filled: added to, not overwritten
    parts_s, parts_i = [], []
    for lo, hi in ((0, cut), (cut, NG)):
        gp = engine.build_panel([torch.from_numpy(grid.img[lo:hi]).to(dev), torch.from_numpy(grid.txt[lo:hi]).to(dev)], _lib.SIDE_GALLERY, 3)
        s_, i_ = engine.sim_topk_deep(qp, gp, k, gallery_offset=lo, query_block=128, gt_idx=gt, gt_score=sgt, ahead=ahead, bonus=grid.bonus)
        parts_s.append(s_)
        parts_i.append(i_)
    assert np.array_equal(ahead.cpu().numpy().astype(np.int64), grid.ranks - 1 + 7)
    ms, mi = engine.select_topk(torch.cat(parts_s, 1), k, idx=torch.cat(parts_i, 1))
    exp_i = grid.order[:, :k]
    assert np.array_equal(mi.cpu().numpy(), exp_i.astype(np.int32))
    assert np.array_equal(_bits(ms.cpu().numpy()), _bits(np.take_along_axis(grid.F, exp_i, 1)))


def test_same_call_twice_same_bits(device, grid):
    q = torch.from_numpy(grid.q).to(device)
    qp = engine.build_panel([q, q], _lib.SIDE_QUERY, 1, part_scale=[0.5, 0.5])
    gp = engine.build_panel([torch.from_numpy(grid.img).to(device), torch.from_numpy(grid.txt).to(device)], _lib.SIDE_GALLERY, 1)
    gt = torch.from_numpy(grid.gt.astype(np.int32)).to(device)
    sgt = torch.from_numpy(grid.F[np.arange(NQ), grid.gt].astype(np.float32)).to(device)
    out = []
    for _ in range(2):
        ahead = torch.zeros(NQ, dtype=torch.int32, device=device)
        s, i = engine.sim_topk_deep(qp, gp, 500, gt_idx=gt, gt_score=sgt, ahead=ahead, bonus=grid.bonus)
        out.append((s, i, ahead))
    assert torch.equal(out[0][1], out[1][1]) and torch.equal(_ibits(out[0][0]), _ibits(out[1][0])) and torch.equal(out[0][2], out[1][2])


def test_errors(device):
    rng = np.random.default_rng(4)
    nq, ng, k = 20, 300, 10
    qp = engine.build_panel([torch.from_numpy(_unit(rng, nq, 64)).to(device)], _lib.SIDE_QUERY, 1)
    gp = engine.build_panel([torch.from_numpy(_unit(rng, ng, 64)).to(device)], _lib.SIDE_GALLERY, 1)
    top_s = torch.zeros((nq, k), dtype=torch.float32, device=device)
    top_i = torch.zeros((nq, k), dtype=torch.int32, device=device)
    ptr = torch.zeros(nq + 1, dtype=torch.int32, device=device)
    col = torch.zeros(1, dtype=torch.int32, device=device)
    val = torch.zeros(1, dtype=torch.float32, device=device)
    gt = torch.zeros(nq, dtype=torch.int32, device=device)
    sgt = torch.zeros(nq, dtype=torch.float32, device=device)
    ahead = torch.zeros(nq, dtype=torch.int32, device=device)
    for kw in (dict(ptr=ptr), dict(ptr=ptr, col=col), dict(col=col, val=val)):
        status, msg = _fused_raw(qp, gp, k, top_s, top_i, **kw)
        assert status == -1 and "bonus CSR arrays must be given together" in msg, kw
    for kw in (dict(gt=gt), dict(gt=gt, sgt=sgt), dict(ahead=ahead), dict(sgt=sgt, ahead=ahead)):
        status, msg = _fused_raw(qp, gp, k, top_s, top_i, **kw)
        assert status == -1 and "gt_idx, gt_score and ahead must be given together" in msg, kw
    status, msg = _fused_raw(qp, gp, 0, top_s, top_i, gt=gt, sgt=sgt, ahead=ahead)
    assert status == -1 and "sim_topk_deep_fused: k=0 not in 1..1024" in msg
    with pytest.raises(RuntimeError, match="given together"):             # through the wrapper: the library's message
        engine.sim_topk_deep(qp, gp, k, ahead=ahead)
    with pytest.raises(RuntimeError, match="k=0"):
        engine.sim_topk_deep(qp, gp, 0, bonus=(ptr, col, val))
    with pytest.raises(RuntimeError, match="nq \\+ 1"):
        engine.sim_topk_deep(qp, gp, k, bonus=(ptr[:-1], col, val))
    with pytest.raises(RuntimeError, match="gt_idx needs"):
        engine.sim_topk_deep(qp, gp, k, gt_idx=gt)
    assert int(ahead.sum()) == 0                                          # no refused call counted anything
    s0, i0 = engine.sim_topk_deep(qp, gp, k, bonus=(ptr, col[:0], val[:0]))         # an empty hit list: no bonus
    s1, i1 = engine.sim_topk_deep(qp, gp, k)
    assert torch.equal(i0, i1) and torch.equal(_ibits(s0), _ibits(s1))


def test_evaluation_fused_ranks_deep_and_shallow(device, grid):
    """sparql_fusion.fused_ranks at k = 100 (the deep route; an error before) equals the dense reference on the exact-grid data;
    k = 10 still is ranking.ranks_and_topk, bit for bit."""
    results = grid.results[0.25]
    params = {"delta": 0.25}
    parts = ([grid.q, grid.q], [grid.img, grid.txt], [0.5, 0.5])
    F = fusion_ref.fuse(grid.S, results, grid.quuids, grid.auuids, "additive", params)
    assert not np.array_equal(F, grid.S)
    gt = np.arange(NQ)                                                    # fused_ranks: the diagonal
    ranks, top_s, top_i = sparql_fusion.fused_ranks(*parts, results, grid.quuids, grid.auuids, "additive", params, k=100)
    exp_i = np.argsort(-F, axis=1, kind="stable")[:, :100]
    assert np.array_equal(top_i.cpu().numpy(), exp_i.astype(np.int32))
    assert np.array_equal(_bits(top_s.cpu().numpy()), _bits(np.take_along_axis(F, exp_i, 1)))
    assert np.array_equal(ranks.cpu().numpy(), metrics_ref.ranks_by_count(F, gt))
    r10, s10, i10 = sparql_fusion.fused_ranks(*parts, results, grid.quuids, grid.auuids, "additive", params, k=10)
    _, bonus = sparql_fusion.sparql_bonus(results, grid.quuids, grid.auuids, "additive", params)
    rb, sb, ib = ranking.ranks_and_topk(parts[0], parts[1], weights=parts[2], k=10, bonus=bonus)
    assert torch.equal(r10, rb) and torch.equal(i10, ib) and torch.equal(_ibits(s10), _ibits(sb))
    assert np.array_equal(i10.cpu().numpy(), exp_i[:, :10].astype(np.int32)) and np.array_equal(r10.cpu().numpy(), ranks.cpu().numpy())


def test_online_fused_search_lifts_a_hit_from_the_bottom_of_the_gallery(device):
    """retrieve_text_fused scores EVERY item: the hit CLIP ranks last of 600 comes first, while retrieve_text_deep(depth=50) never
    sees it.  The store's embeddings lie in a cone, as CLIP's do (a shared direction + noise of 0.3): the CLIP scores of one query
    then span less than 0.2 / 0.8, the premise of the issue's "a hit anywhere should land near the top" -- asserted below.
    Scores: the fused search folds alpha = 0.8 into the bf16-split query panel, the list fusion multiplies fp32 scores on the host;
    the two differ by about 1e-7, which moves a four-decimal rounding by at most one unit: 1e-4 (+ 1e-9 for the decimal repr)."""
    from knowledge_enhanced_multimodal_retrieval_amd.config import ARCHS
    from knowledge_enhanced_multimodal_retrieval_amd.clip_module import CLIP
    from knowledge_enhanced_multimodal_retrieval_amd.retriever import CLIPRetriever, EmbeddingStore
    from src.clip.clip_retrieval import CLIPRetrieval
    from src.retrieval import RetrievalEngine
    arch, oa = ARCHS["tiny"], clip_ref.ARCHS["tiny"]
    model = CLIP(arch)
    model.load_state_dict(clip_ref.random_state_dict(oa, seed=0))
    model = model.to(device).eval()
    n = 600
    rng = np.random.default_rng(11)
    centre = _unit(rng, 1, arch.embed_dim)
    cone = lambda: (lambda x: x / np.linalg.norm(x, axis=1, keepdims=True))(centre + 0.3 * _unit(rng, n, arch.embed_dim))
    store = EmbeddingStore(cone().astype(np.float32), cone().astype(np.float32), [f"u{i:04d}" for i in range(n)], device)
    words = {}

    def tok(texts):                                        # tiny vocab: a fixed toy tokenizer
        out = torch.zeros(len(texts), arch.ctx, dtype=torch.int32)
        for r, s in enumerate(texts):
            ids = [arch.sot] + [1 + words.setdefault(w, len(words)) % (arch.sot - 1) for w in s.split()][:arch.ctx - 2] + [arch.eot]
            out[r, :len(ids)] = torch.tensor(ids, dtype=torch.int32)
        return out

    ret = CLIPRetriever(model, store, tokenize_fn=tok)
    query = "bronze statue of a seated king"
    clip_all = ret.search_deep(query, alpha=0.5, top_k=n)
    assert len(clip_all) == n
    last = clip_all[-1]
    assert 0.8 * (clip_all[0]["score"] - last["score"]) < 0.2 - 1e-3      # the premise: the bonus outweighs CLIP's whole spread
    calls = []

    class T2S:
        def retrieval(self, q):
            calls.append(q)
            return [last["uuid"], "unknown-uuid", "http://example.org/artefact/" + last["uuid"]]

    eng = RetrievalEngine(clip_retriever=CLIPRetrieval(retriever=ret), t2s_retriever=T2S())
    tol = 1e-4 + 1e-9
    fused = eng.retrieve_text_fused(query, alpha=0.8, beta=0.2, alpha_clip=0.5, threshold=-1, depth=50)
    assert calls == [query] and len(fused) == 50
    assert fused[0]["uuid"] == last["uuid"] and abs(fused[0]["score"] - round(0.8 * last["score"] + 0.2, 4)) <= tol
    assert [it["score"] for it in fused] == sorted((it["score"] for it in fused), reverse=True)
    assert abs(fused[1]["score"] - round(0.8 * clip_all[0]["score"], 4)) <= tol          # behind the hit: CLIP's own best
    deep = eng.retrieve_text_deep(query, alpha=0.8, beta=0.2, alpha_clip=0.5, threshold=-1, depth=50)
    assert len(deep) == 50 and last["uuid"] not in [it["uuid"] for it in deep]
    fused_all = {it["uuid"]: it["score"] for it in eng.retrieve_text_fused(query, threshold=-1, depth=n)}
    deep_all = {it["uuid"]: it["score"] for it in eng.retrieve_text_deep(query, threshold=-1, depth=n)}
    assert len(fused_all) == n and set(fused_all) == set(deep_all)
    assert max(abs(fused_all[u] - deep_all[u]) for u in fused_all) <= tol
    # the head of the list does not depend on depth, and threshold cuts the fused list
    assert [it["uuid"] for it in eng.retrieve_text_fused(query, threshold=-1, depth=200)[:50]] == [it["uuid"] for it in fused]
    cut = eng.retrieve_text_fused(query, threshold=fused[1]["score"] + 1e-4, depth=50)
    assert [it["uuid"] for it in cut] == [last["uuid"]]
    # the other entry points keep their limits
    with pytest.raises(ValueError):
        ret.search(query, top_k=100)
    with pytest.raises(ValueError):
        ret.search_fused(query, [], top_k=1025)
    assert ret.search_fused(query, [], alpha=0.5, top_k=20) == ret.search_deep(query, alpha=0.5, top_k=20)      # no hit: CLIP's own list
