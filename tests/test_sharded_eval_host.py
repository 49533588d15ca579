"""CPU, gloo: the drop-in evaluators over a process group (dist.init_from_env, encode_dataset(shard=...), the equal-rows padding,
ShardedGallery.ranks / rerank and dist.sharded_ranks_dense behind evaluate_clip_model / _baseline / evaluate_fusion_model) against a
single-process numpy statement, at world 2 with n = 37 and world 4 with n = 5 (shards 2, 2, 1, 0: a rank that encodes nothing).
The kernel calls are the numpy stand-in of tests/test_dist_rerank_gloo.py plus one for rank_dense_shard, the encoder is a stand-in
that counts the items it is given (TEST ONLY: the product path always uses the HIP ``engine`` module).  Also the host-side refusals
of kemr_rank_dense_shard (no GPU call is made) and the no-process-group switches."""
import ctypes as C
import json
import os
import sys
import zlib

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, "tests")
for _p in (ROOT, TESTS):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from test_dist_rerank_gloo import OracleHeadGallery, RerankOracleOps, oracle_score_lists  # noqa: E402

D, DEPTH = 16, 20
K_VALUES = [1, 5, 10, 20]
INT32_MAX = 2 ** 31 - 1


# ------------------------------------------------------------------------------------------------ stand-ins
class ShardOps(RerankOracleOps):
    """RerankOracleOps + the per-row gate in build_panel + rank_dense_shard (the order rule, by counting)."""

    @staticmethod
    def build_panel(parts, side, terms=3, part_scale=None, row_scale=None):
        cols = []
        for p, t in enumerate(parts):
            x = t.double().numpy().copy()
            if part_scale is not None:
                x *= part_scale[p]
            if row_scale is not None and row_scale[p] is not None:
                x *= row_scale[p].double().numpy()[:, None]
            cols.append(x)
        return RerankOracleOps.P(np.concatenate(cols, 1))

    @staticmethod
    def rank_dense_shard(scores, id_offset=0, gt_idx=None, gt_score=None, k=0):
        S = scores.numpy().astype(np.float32)
        nq, ng = S.shape
        ids = np.arange(ng, dtype=np.int64) + id_offset
        ahead = None
        if gt_idx is not None:
            ahead = np.zeros(nq, np.int32)
            for r in range(nq):
                g, sg = int(gt_idx[r]), np.float32(gt_score[r])
                if g >= 0:
                    ahead[r] = int((((S[r] > sg) | ((S[r] == sg) & (ids < g))) & (ids != g)).sum())
            ahead = torch.from_numpy(ahead)
        if k <= 0:
            return ahead, None, None
        s, i = RerankOracleOps._take(S, np.broadcast_to(ids.astype(np.int32), S.shape), k)
        return ahead, s, i


def tokenize(texts):
    """8 word hashes per text (deterministic across processes)."""
    out = torch.zeros((len(texts), 8), dtype=torch.int64)
    for r, t in enumerate(texts):
        for c, w in enumerate(t.split()[:8]):
            out[r, c] = zlib.crc32(w.encode()) % 997 + 1
    return out


class CountingEncoder(torch.nn.Module):
    """Row-wise float64 projections, L2-normalised: a row's bits do not depend on what else is in the call.  Counts its rows."""
    embed_dim = D

    def __init__(self):
        super().__init__()
        self.anchor = torch.nn.Parameter(torch.zeros(1))
        rng = np.random.default_rng(11)
        self.w_img, self.w_txt = rng.standard_normal((D, 48)), rng.standard_normal((D, 8))
        self.rows = {"image": 0, "text": 0, "image_calls": 0}

    @staticmethod
    def _unit(rows):
        out = np.stack(rows) if rows else np.zeros((0, D))
        return torch.from_numpy((out / np.linalg.norm(out, axis=1, keepdims=True)).astype(np.float32))

    def encode_image(self, x, normalize=True):
        self.rows["image"] += int(x.shape[0])
        self.rows["image_calls"] += 1
        return self._unit([self.w_img @ r for r in x.double().reshape(x.shape[0], -1).numpy()])

    def encode_text(self, ids, normalize=True, lens=None):
        self.rows["text"] += int(ids.shape[0])
        return self._unit([self.w_txt @ np.cos(r) + 0.25 * self.w_txt[:, 0] for r in ids.double().numpy()])


class CountingSentenceEncoder:
    """SentenceTransformer.encode's contract over CountingEncoder's text projection."""

    def __init__(self):
        self.inner = CountingEncoder()

    def to(self, device):
        return self

    def eval(self):
        return self

    def get_sentence_embedding_dimension(self):
        return D

    def encode(self, sentences, convert_to_tensor=True, device=None, show_progress_bar=False, normalize_embeddings=True):
        return self.inner.encode_text(tokenize(sentences))


class TextPairs(torch.utils.data.Dataset):
    def __init__(self, n):
        self.items = dataset(n)

    def __len__(self):
        return len(self.items)

    def __getitem__(self, idx):
        _, query, target, _ = self.items[idx]
        return query, target


class OracleFusion:
    """What evaluate_fusion_model needs of a FusionModel, as row-wise float64 statements."""

    def __init__(self, fusion_type):
        self.fusion_type, self.clip_model = fusion_type, CountingEncoder()
        self.w = torch.from_numpy(np.random.default_rng(5).standard_normal(D))

    def eval(self):
        return self

    def gate(self, q):
        return torch.sigmoid((q.double() * self.w).sum(1)).float()

    def _parts(self, q, img, tgt):
        g = self.gate(q)
        return [q, q], [img, tgt], None, [g, 1.0 - g]

    def forward(self, q, img, tgt):
        idx = torch.arange(img.shape[0], dtype=torch.int32).repeat(q.shape[0], 1)
        return oracle_score_lists(q, OracleHeadGallery(img.numpy(), tgt.numpy()), idx)

    def prepare_gallery(self, img, tgt):
        return OracleHeadGallery(img.numpy(), tgt.numpy())

    list_scores = staticmethod(oracle_score_lists)


def sparql_results(n):
    """Hits on both sides of every shard boundary, a query's own artefact, a duplicate, an unknown uuid, a query without a file."""
    uri = lambda i: f"http://example.org/artefact/synthetic-{i:06d}"
    out = {}
    for i in range(n):
        if i % 4 == 3:
            continue
        hits = [uri((i * 7 + 3) % n), uri((i + n // 2) % n)]
        if i % 2 == 0:
            hits.append(uri(i))
        if i % 5 == 0:
            hits += [uri((i * 7 + 3) % n), "http://example.org/artefact/unknown"]
        out[f"synthetic-{i:06d}"] = hits
    return out


def dataset(n):
    from knowledge_enhanced_multimodal_retrieval_amd.datasets import SyntheticRetrievalDataset
    return SyntheticRetrievalDataset(n, image_size=4, seed=3)


# ------------------------------------------------------------------------------------------------ the single-process statement
def _metrics(r, prefix="", recall=True, mrr=True):
    out = {}
    if recall:
        for k in K_VALUES:
            out[f"R@{k}"] = float(np.mean(r <= k) * 100.0)
    if mrr:
        out["MRR"] = float(np.mean(1.0 / r) * 100.0)
        out["Mean_Rank"] = float(np.mean(r))
    return {(f"{prefix}_{k}" if prefix else k): v for k, v in out.items()}


def _diag_ranks(S):
    n = S.shape[0]
    ids = np.arange(S.shape[1])
    return np.asarray([1 + int((((S[r] > S[r, r]) | ((S[r] == S[r, r]) & (ids < r))) & (ids != r)).sum()) for r in range(n)], np.int64)


def _scores(q_parts, g_parts, weights=None, gates=None, bonus=None):
    """fp32(float64 dot) of the weighted / gated concatenation, then one fp32 add per bonus entry: the stand-in's arithmetic."""
    qs = []
    for p, q in enumerate(q_parts):
        x = q.astype(np.float64).copy()
        if weights is not None:
            x *= weights[p]
        if gates is not None:
            x *= gates[p].astype(np.float64)[:, None]
        qs.append(x)
    S = (np.concatenate(qs, 1) @ np.concatenate([g.astype(np.float64) for g in g_parts], 1).T).astype(np.float32)
    if bonus is not None:
        ptr, col, val = bonus
        np.add.at(S, (np.repeat(np.arange(len(ptr) - 1), np.diff(ptr)), col), val.astype(np.float32))
    return S


def expected(n):
    """Every evaluator's ranks and metric dict from the whole dataset in one process."""
    import list_fuse_ref as ref
    from knowledge_enhanced_multimodal_retrieval_amd import evaluators as E, sparql_fusion as SF
    ds, enc = dataset(n), CountingEncoder()
    items = [ds[i] for i in range(n)]
    img = enc.encode_image(torch.stack([it[0] for it in items])).numpy()
    q = enc.encode_text(tokenize([it[1] for it in items])).numpy()
    t = enc.encode_text(tokenize([it[2] for it in items])).numpy()
    uuids = [it[3] for it in items]
    t2s = sparql_results(n)
    out = {"ranks": {}, "uuids": uuids}
    for task, (a, b) in {"T2I": (q, img), "I2T": (img, t), "T2T": (q, t)}.items():
        out["ranks"][task] = _diag_ranks(_scores([a], [b]))
    out["clip"] = {k: v for task in ("T2I", "I2T", "T2T") for k, v in _metrics(out["ranks"][task], task).items()}
    out["clip_train"] = {k: v for task in ("T2I", "T2T") for k, v in _metrics(out["ranks"][task], task, recall=False).items()}
    out["text"] = _metrics(out["ranks"]["T2T"], "T2T")
    out["analysis"] = {}
    for wi, wt in ((0.5, 0.5), (0.1, 0.9)):
        sweep = {"T2I": _metrics(out["ranks"]["T2I"]), "T2T": _metrics(out["ranks"]["T2T"]),
                 "Fused": _metrics(_diag_ranks(_scores([q, q], [img, t], [wi, wt])))}
        for alpha in E.ALPHAS:
            scale, bonus = SF.sparql_bonus(t2s, uuids, uuids, "weighted", {"alpha": alpha, "sparql_weight": 1 - alpha})
            sweep[f"weighted_alpha={alpha}"] = _metrics(_diag_ranks(_scores([q, q], [img, t], [scale * wi, scale * wt], bonus=bonus)))
        out["analysis"][f"{wi}_{wt}"] = sweep
    out["ranks"]["baseline"] = _diag_ranks(_scores([q, q], [img, t], [0.3, 0.7]))
    out["baseline"] = _metrics(out["ranks"]["baseline"])
    fm = OracleFusion("simple_gated")
    g = fm.gate(torch.from_numpy(q)).numpy()
    out["ranks"]["gated"] = _diag_ranks(_scores([q, q], [img, t], None, [g, (1.0 - torch.from_numpy(g)).numpy()]))
    out["gated"] = _metrics(out["ranks"]["gated"])
    out["ranks"]["dense"] = _diag_ranks(fm.forward(torch.from_numpy(q), torch.from_numpy(img), torch.from_numpy(t)).numpy())
    out["dense"] = _metrics(out["ranks"]["dense"])
    ids_all = np.broadcast_to(np.arange(n, dtype=np.int32), (n, n))
    whole = OracleHeadGallery(img, t)
    gt = np.arange(n, dtype=np.int32)
    for name, results in (("rerank", None), ("rerank_sparql", t2s)):
        head_weight, bonus = (1.0, None) if results is None else SF.sparql_bonus(results, uuids, uuids, "weighted", None)
        _, short = ref.sorted_rows(_scores([q, q], [img, t], [0.5, 0.5], bonus=bonus), ids_all, DEPTH)
        head = oracle_score_lists(torch.from_numpy(q), whole, torch.from_numpy(short)).numpy()
        _, ahead, found, _ = ref.list_fuse(head, short, DEPTH, head_weight, bonus, gt)
        r = np.where(found == 1, ahead.astype(np.int64) + 1, DEPTH + 1)
        out["ranks"][name] = r
        m = _metrics(r)
        m["Shortlist_Recall"] = float(np.mean(r <= DEPTH) * 100.0)
        m["Rerank_Depth"] = DEPTH
        if results is not None:
            m["Head_Weight"], m["SPARQL_Strategy"] = float(head_weight), "weighted"
        out[name] = m
    return out


# ------------------------------------------------------------------------------------------------ the ranks of the process group
def _worker(rank, world, port, n, tmp, q_out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank),
                      KEMR_DIST_BACKEND="gloo")
    os.environ.pop("KEMR_EVAL_SHARDED", None)
    from knowledge_enhanced_multimodal_retrieval_amd import dist as KD, evaluators as E, ranking
    assert KD.init_from_env()[:2] == (world, rank) and dist.get_backend() == "gloo"
    KD.eval_ops = ShardOps
    seen = []                                                   # every ranks array a metric is computed from
    plain = ranking.metrics_from_ranks

    def recording(ranks, *a, **kw):
        seen.append(np.asarray(ranks.numpy(), np.int64).copy())
        return plain(ranks, *a, **kw)
    ranking.metrics_from_ranks = recording
    lo, hi = KD.shard_bounds(n, world, rank)
    ds, t2s = dataset(n), sparql_results(n)
    out = {"ranks": {}, "rows": {}, "lo_hi": (lo, hi)}

    def call(name, fn, model, *a, **kw):
        enc = getattr(model, "clip_model", model)
        seen.clear()
        out[name] = fn(model, ds, 8, "cpu", 42, *a, tokenize_fn=tokenize, num_workers=0, **kw)
        out["ranks"][name] = [s.copy() for s in seen]
        out["rows"][name] = dict(enc.rows)

    call("clip", E.evaluate_clip_model, CountingEncoder(), text2sparql_results=t2s)
    out["analysis"] = E.evaluate_clip_model.last_analysis
    seen.clear()
    out["clip_train"] = E.evaluate_clip_model_for_training(CountingEncoder(), ds, 8, "cpu", 42, ("T2I", "T2T"), tokenize_fn=tokenize)
    call("baseline", E.evaluate_clip_model_baseline, CountingEncoder(), t2i_weight=0.3, t2t_weight=0.7)
    call("gated", E.evaluate_fusion_model, OracleFusion("simple_gated"))
    call("dense", E.evaluate_fusion_model, OracleFusion("linear"))
    call("rerank", E.evaluate_fusion_model, OracleFusion("linear"), rerank_depth=DEPTH)
    call("rerank_sparql", E.evaluate_fusion_model, OracleFusion("linear"), rerank_depth=DEPTH, text2sparql_results=t2s)
    seen.clear()
    sent = CountingSentenceEncoder()
    out["text"] = E.evaluate_text_model(sent, TextPairs(n), 8, "cpu", 42)
    out["ranks"]["text"] = [s.copy() for s in seen]
    out["rows"]["text"] = dict(sent.inner.rows)
    # the encode step itself: local rows, local uuids
    enc = CountingEncoder()
    i_l, q_l, t_l, uu = E.encode_dataset(enc, ds, 8, 42, 0, tokenize, shard=(rank, world))
    out["local"] = (i_l.numpy(), q_l.numpy(), t_l.numpy(), uu, dict(enc.rows))
    # top-k through sharded_ranks_dense (k > 0: the candidate exchange and merge)
    fm = OracleFusion("linear")
    even = KD.EvenRows(n)
    all_q = KD.all_gather_rows(even.pad(q_l))
    S = fm.forward(all_q, i_l, t_l) if hi > lo else torch.zeros((all_q.shape[0], 0))
    r, ts, ti = KD.sharded_ranks_dense(S, lo, even.all_gt("cpu"), k=3, ops=ShardOps)
    out["dense_topk"] = (even.real(r).numpy(), even.real(ts).numpy(), even.real(ti).numpy())
    # the CLIs' output files: the writer rank only
    log = E._open_outputs(os.path.join(tmp, "out", "results.json"), f"test.sharded.{rank}")
    log.info(f"rank {rank} done")
    E._save_results({"written_by": rank, **E._sharding_record(n)}, os.path.join(tmp, "out", "results.json"))
    out["is_writer"] = KD.is_writer()
    # the opt-out, with the process group still up
    os.environ["KEMR_EVAL_SHARDED"] = "0"
    out["opt_out"] = (KD.active_shard(), KD.init_from_env()[:2])
    os.environ.pop("KEMR_EVAL_SHARDED")
    out["shard"] = KD.active_shard()
    q_out.put((rank, out))
    KD.finish()
    assert not dist.is_initialized()


_EXPECTED = {}


def _expected(n):
    if n not in _EXPECTED:
        _EXPECTED[n] = expected(n)
    return _EXPECTED[n]


@pytest.mark.parametrize("world,n", [(2, 37), (4, 5)])
def test_sharded_evaluators_equal_the_single_process_statement(world, n, tmp_path):
    from knowledge_enhanced_multimodal_retrieval_amd.dist import shard_bounds
    port = 29500 + (os.getpid() + 977 * world) % 2000
    ctx = mp.get_context("spawn")
    q_out = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, n, str(tmp_path), q_out)) for r in range(world)]
    for p in procs:
        p.start()
    results = dict(q_out.get(timeout=240) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    want = _expected(n)
    sizes = [hi - lo for lo, hi in (shard_bounds(n, world, r) for r in range(world))]
    assert sizes == ([19, 18] if world == 2 else [2, 2, 1, 0])
    per_call = {"clip": ["T2I", "I2T", "T2T"], "baseline": ["baseline"], "gated": ["gated"], "dense": ["dense"], "rerank": ["rerank"],
                "rerank_sparql": ["rerank_sparql"]}
    for rank in range(world):
        out = results[rank]
        assert out["shard"] == (rank, world)
        for name, tasks in per_call.items():
            assert out[name] == want[name], (rank, name, out[name], want[name])          # metric dicts: exact, on every rank
            got = out["ranks"][name]
            if name == "clip":                                                             # + 2 x (T2I, T2T, Fused, 9 alphas) of the sweeps
                assert len(got) == 3 + 2 * 12
                got = got[:3]
            assert len(got) == len(tasks)
            for task, r in zip(tasks, got):
                assert np.array_equal(r, want["ranks"][task]), (rank, task)
            for r in out["ranks"][name]:                                                   # no pad row reached a metric
                assert r.shape == (n,)
            # each rank's encoder saw exactly its shard's items (queries and targets go through one text call)
            assert out["rows"][name]["image"] == sizes[rank] and out["rows"][name]["text"] == 2 * sizes[rank], (rank, name)
        assert out["analysis"] == want["analysis"], rank
        assert out["text"] == want["text"] and out["rows"]["text"]["text"] == 2 * sizes[rank], rank          # evaluate_text_model (T2T)
        assert len(out["ranks"]["text"]) == 1 and np.array_equal(out["ranks"]["text"][0], want["ranks"]["T2T"]), rank
        assert out["clip_train"] == want["clip_train"], rank
        # the local embeddings are the rows of the whole-dataset encode, the uuids partition the dataset in order
        lo, hi = out["lo_hi"]
        i_l, q_l, t_l, uu, rows = out["local"]
        assert uu == want["uuids"][lo:hi] and i_l.shape == q_l.shape == t_l.shape == (hi - lo, D)
        assert rows["image"] == hi - lo and (rows["image_calls"] == 0) == (hi == lo)      # an empty shard encodes nothing
        r, ts, ti = out["dense_topk"]
        assert np.array_equal(r, want["ranks"]["dense"]) and ti.shape == (n, 3)
        assert np.array_equal(ti[:, 0] == np.arange(n), r == 1)
        assert out["is_writer"] == (rank == 0)
        assert out["opt_out"] == (None, (1, 0))
    assert sum(len(results[r]["local"][3]) for r in range(world)) == n
    if n == 37:
        assert all((want["ranks"][t] > 1).any() for t in want["ranks"])                   # the statement is not trivially all-ones
        assert want["analysis"]["0.5_0.5"]["weighted_alpha=0.1"] != want["analysis"]["0.5_0.5"]["Fused"]      # the bonus changes ranks
    # only rank 0 wrote files: one log, one results file, and the file says who wrote it
    assert sorted(os.listdir(tmp_path / "out")) == ["evaluation.log", "results.json"]
    saved = json.loads((tmp_path / "out" / "results.json").read_text())
    assert saved == {"written_by": 0, "world_size": world, "items_per_rank": sizes}
    log = (tmp_path / "out" / "evaluation.log").read_text()
    assert "rank 0 done" in log and "rank 1 done" not in log


# ------------------------------------------------------------------------------------------------ no process group
def test_init_from_env_without_torchrun_is_a_no_op(monkeypatch):
    from knowledge_enhanced_multimodal_retrieval_amd import dist as KD
    for key in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(key, raising=False)
    assert KD.init_from_env()[:2] == (1, 0) and not dist.is_initialized()
    monkeypatch.setenv("RANK", "0")
    monkeypatch.setenv("WORLD_SIZE", "1")                       # WORLD_SIZE=1 is "no process group" too
    assert KD.init_from_env()[:2] == (1, 0) and not dist.is_initialized()
    KD.finish()                                                 # nothing to end
    assert KD.active_shard() is None and KD.is_writer()
    assert KD.all_gather_list(["a"]) == ["a"]


def test_eval_sharded_0_restores_one_rank_behaviour(monkeypatch):
    """Under torchrun with KEMR_EVAL_SHARDED=0 no group is created and the evaluators take today's path: the whole dataset through
    encode_dataset(shard=None) and metrics.compute_all_retrieval_metrics."""
    from knowledge_enhanced_multimodal_retrieval_amd import dist as KD, evaluators as E
    monkeypatch.setenv("RANK", "1")
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("LOCAL_RANK", "1")
    monkeypatch.setenv("KEMR_EVAL_SHARDED", "0")
    assert KD.init_from_env()[:2] == (1, 0) and not dist.is_initialized()
    assert KD.active_shard() is None and E._sharding_record(37) == {}
    calls = []
    monkeypatch.setattr(E.M, "compute_all_retrieval_metrics", lambda q, t, i, **kw: calls.append((q.shape[0], t.shape[0], i.shape[0])) or {"ok": 1.0})
    enc = CountingEncoder()
    assert E.evaluate_clip_model(enc, dataset(9), 4, "cpu", tokenize_fn=tokenize, analysis=False) == {"ok": 1.0}
    assert calls == [(9, 9, 9)] and enc.rows["image"] == 9 and enc.rows["text"] == 18
    assert E.usable_loader_workers(dataset(9), None, 8) == 4    # the loader workers are still divided by the local world size


def test_encode_dataset_shard_none_is_todays_function():
    import inspect
    from knowledge_enhanced_multimodal_retrieval_amd import evaluators as E
    assert inspect.signature(E.encode_dataset).parameters["shard"].default is None
    ds = dataset(11)
    whole = E.encode_dataset(CountingEncoder(), ds, 4, 42, 0, tokenize)
    again = E.encode_dataset(CountingEncoder(), ds, 4, 42, 0, tokenize, shard=None)
    for a, b in zip(whole[:3], again[:3]):
        assert a.shape == (11, D) and torch.equal(a, b)
    assert whole[3] == again[3] == [f"synthetic-{i:06d}" for i in range(11)]
    parts = [E.encode_dataset(CountingEncoder(), ds, 4, 42, 0, tokenize, shard=(r, 3)) for r in range(4 - 1)]
    for j in range(3):
        assert torch.equal(torch.cat([p[j] for p in parts]), whole[j])
    assert [u for p in parts for u in p[3]] == whole[3]
    enc = CountingEncoder()
    empty = E.encode_dataset(enc, dataset(5), 4, 42, 0, tokenize, shard=(3, 4))
    assert all(x.shape == (0, D) for x in empty[:3]) and empty[3] == [] and enc.rows["image_calls"] == 0


# ------------------------------------------------------------------------------------------------ kemr_rank_dense_shard refuses
def test_rank_dense_shard_refusals_leave_the_outputs_untouched():
    """Every refusal comes before any launch (the library loads without a GPU), says why, and writes nothing."""
    from knowledge_enhanced_multimodal_retrieval_amd import _lib
    lib = _lib.lib()
    nq, ng, k = 2, 8, 4
    scores = np.zeros((nq, ng), np.float32)
    gt, sgt = np.zeros(nq, np.int32), np.zeros(nq, np.float32)
    ahead = np.full(nq, -77, np.int32)
    top_s, top_i = np.full((nq, k), 7.5, np.float32), np.full((nq, k), -77, np.int32)
    p = lambda a: None if a is None else C.c_void_p(a.ctypes.data)

    def call(nq=nq, ng=ng, ld=ng, off=0, gt=gt, sgt=sgt, ahead=ahead, k=k, top_s=top_s, top_i=top_i):
        return lib.kemr_rank_dense_shard(p(scores), nq, ng, ld, off, p(gt), p(sgt), p(ahead), k, p(top_s), p(top_i), None)

    cases = [(dict(off=-1), "id_offset"), (dict(off=INT32_MAX - ng + 1), "id_offset"), (dict(off=2 ** 40), "id_offset"),
             (dict(ld=ng - 1), "ld="), (dict(k=0), "k=0 not in 1..32"), (dict(k=33), "k=33 not in 1..32"),
             (dict(gt=None), "gt_idx, gt_score and ahead together"), (dict(sgt=None), "gt_idx, gt_score and ahead together"),
             (dict(ahead=None), "gt_idx, gt_score and ahead together"), (dict(gt=None, sgt=None), "gt_idx, gt_score and ahead together"),
             (dict(top_s=None), "top_scores/top_idx together"), (dict(top_i=None), "top_scores/top_idx together"),
             (dict(ng=0), "bad argument"), (dict(nq=-1), "bad argument")]
    for kw, words in cases:
        assert call(**kw) == -1, kw
        text = lib.kemr_last_error().decode()
        assert text.startswith("rank_dense_shard:") and words in text, (kw, text)
    assert call(nq=0, off=-1) == 0                              # nq == 0 is a no-op, whatever else is passed
    assert (ahead == -77).all() and (top_s == 7.5).all() and (top_i == -77).all()
    assert "kemr_rank_dense_shard" in _lib.SIGNATURES and lib.kemr_abi_version() == 4
