"""Retrieve-then-rerank timings (tools only): the cross_attention head on deep shortlists against the dense route, in one process.

    python tools/bench_rerank.py [--out profiles/rerank_bench.txt] [--calls 12] [--only offline|online|fused]

offline  N = M = 4 096, dim 768, a cross_attention head with seeded random parameters:
  dense        FusionModel.rank(q, img, tgt, k=10): the head on all N x M pairs, then kemr_rank_dense
  rerank_d200  FusionModel.rerank(q, gallery, depth=200, k=10, gt_idx="diag"): shortlist + head on N x 200 pairs + sort
  rerank_d1024 the same at depth 1 024
  kernel_d*    engine.cross_attention_rerank alone on those lists (the gathered pair-scoring kernel)
  shortlist_d* the shortlist stage alone (query panel + engine.sim_topk_deep)
  prepare      FusionModel.prepare_gallery(img, tgt): once per gallery, timed apart
fused    N = M = 4 096, depth 200, gt_idx given, a bonus of ~50 hits per query (knowledge-fused rerank):
  rerank_ms        FusionModel.rerank(q, gallery, depth=200, k=10, gt_idx="diag"): the plain ranked rerank, for comparison
  fused_rerank_ms  the same call with bonus=..., head_weight=0.8: shortlist with bonus + head + kemr_list_fuse + kemr_select_topk
  list_fuse_ms     engine.list_fuse alone on those lists (scale + bonus + ranks), select_ms: engine.select_topk(k=10) on them,
  shortlist*_ms    the shortlist stage with and without the bonus, head_ms: FusionModel.list_scores on the lists
online   nq = 1, M = 43 000, depth 200, k = 10: the whole rerank call behind the text tower, its kernel and its shortlist stage.
hipEvents around every call, median of >= 10 calls after >= 100 ms (and 3 calls) of warm-up; per-pair times are the median
divided by the pairs the route scores.  One JSON line per case.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from knowledge_enhanced_multimodal_retrieval_amd import engine  # noqa: E402
from knowledge_enhanced_multimodal_retrieval_amd.fusion_model import FusionModel  # noqa: E402


def timed(fn, calls):
    """Median ms per call: hipEvents around each call, after at least 100 ms (and 3 calls) of warm-up."""
    t0, n = time.perf_counter(), 0
    while n < 3 or time.perf_counter() - t0 < 0.1:
        fn()
        torch.cuda.synchronize()
        n += 1
    ms = []
    for _ in range(max(calls, 10)):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def head(dim, dev):
    fm = FusionModel(torch.nn.Linear(1, 1), fusion_type="cross_attention", embed_dim=dim)
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for p in fm.fusion_head.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * (0.05 if p.dim() > 1 else 0.1))
    return fm.to(dev).eval()


def embeddings(n, nq, dim, dev):
    gg = torch.Generator(device=dev).manual_seed(7)
    img = torch.nn.functional.normalize(torch.randn(n, dim, generator=gg, device=dev), dim=-1)
    tgt = torch.nn.functional.normalize(img + 0.5 * torch.randn(n, dim, generator=gg, device=dev), dim=-1)
    qry = torch.nn.functional.normalize(img[:nq] + 1.2 * torch.randn(nq, dim, generator=gg, device=dev), dim=-1)
    return qry, img, tgt


def rerank_legs(fm, gal, q, depth, calls):
    c = gal.cand
    Q = fm._cross_attention_query(q)
    lists = fm.shortlist(q, gal.fused_panel, depth)
    pairs = q.shape[0] * depth
    total = timed(lambda: fm.rerank(q, gal, depth=depth, k=10, gt_idx="diag" if q.shape[0] > 1 else None), calls)
    kern = timed(lambda: engine.cross_attention_rerank(Q, c["Ki"], c["Kt"], c["Pi"], c["Pt"], c["c0"], c["w2t"], c["b2"], c["w3"], c["b3"],
                                                       lists, depth), calls)
    short = timed(lambda: fm.shortlist(q, gal.fused_panel, depth), calls)
    gathered = pairs * (2 * q.shape[1] + 2 * c["H"] * c["hid1"]) * 4
    return {"depth": depth, "pairs": pairs, "rerank_ms": total, "kernel_ms": kern, "shortlist_ms": short,
            "rerank_ns_per_pair": total * 1e6 / pairs, "kernel_ns_per_pair": kern * 1e6 / pairs,
            "kernel_gathered_TB_per_s": gathered / (kern * 1e-3) / 1e12}


def fused_legs(fm, gal, q, depth, hits, calls):
    """The knowledge-fused route beside the plain ranked rerank at the same shape, and where its time goes."""
    import numpy as np
    n, m = q.shape[0], len(gal)
    rng = np.random.default_rng(11)
    cols = np.sort(rng.integers(0, m, (n, hits)), axis=1).astype(np.int32)
    dev = q.device
    bonus = (torch.arange(0, n * hits + 1, hits, dtype=torch.int32, device=dev), torch.from_numpy(cols.reshape(-1)).to(dev),
             torch.full((n * hits,), 0.2, dtype=torch.float32, device=dev))
    gt = torch.arange(n, dtype=torch.int32, device=dev)
    lists = fm.shortlist(q, gal.fused_panel, depth, bonus=bonus)
    scores = fm.list_scores(q, gal, lists)
    out = torch.empty_like(scores)
    res = {"depth": depth, "pairs": n * depth, "bonus_hits_per_query": hits,
           "rerank_ms": timed(lambda: fm.rerank(q, gal, depth=depth, k=10, gt_idx="diag"), calls),
           "fused_rerank_ms": timed(lambda: fm.rerank(q, gal, depth=depth, k=10, gt_idx="diag", bonus=bonus, head_weight=0.8), calls),
           "list_fuse_ms": timed(lambda: engine.list_fuse(scores, lists, depth, 0.8, bonus, gt, out=out), calls),
           "select_ms": timed(lambda: engine.select_topk(out, 10, idx=lists), calls),
           "select_depth_ms": timed(lambda: engine.select_topk(out, depth, idx=lists), calls),
           "head_ms": timed(lambda: fm.list_scores(q, gal, lists), calls),
           "shortlist_ms": timed(lambda: fm.shortlist(q, gal.fused_panel, depth), calls),
           "shortlist_bonus_ms": timed(lambda: fm.shortlist(q, gal.fused_panel, depth, bonus=bonus), calls)}
    res["list_fuse_MB"] = (3 * n * depth * 4 + bonus[1].numel() * 8 + (n + 1) * 4 + 4 * n * 4) / 1e6
    res["list_fuse_GB_per_s"] = res["list_fuse_MB"] / res["list_fuse_ms"]
    res["fused_over_plain"] = res["fused_rerank_ms"] / res["rerank_ms"]
    return res


def rounded(res):
    return {key: (round(v, 4) if isinstance(v, float) else v) for key, v in res.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    ap.add_argument("--calls", type=int, default=12)
    ap.add_argument("--n", type=int, default=4096, help="offline: queries = candidates")
    ap.add_argument("--ng", type=int, default=43000, help="online: gallery size")
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--only", default=None, choices=["offline", "online", "fused"])
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    fm = head(args.d, dev)
    lines = []

    def emit(res):
        line = json.dumps(rounded(res))
        print(line, flush=True)
        lines.append(line)

    if args.only in (None, "offline"):
        q, img, tgt = embeddings(args.n, args.n, args.d, dev)
        gal = fm.prepare_gallery(img, tgt)
        dense_ms = timed(lambda: fm.rank(q, img, tgt, k=10), args.calls)
        emit({"case": "offline_dense", "nq": args.n, "ng": args.n, "dim": args.d, "pairs": args.n * args.n, "dense_ms": dense_ms,
              "dense_ns_per_pair": dense_ms * 1e6 / (args.n * args.n), "prepare_ms": timed(lambda: fm.prepare_gallery(img, tgt), args.calls)})
        d_ranks = fm.rank(q, img, tgt, k=10)[0]
        for depth in (200, 1024):
            res = {"case": f"offline_rerank_d{depth}", "nq": args.n, "ng": args.n, "dim": args.d}
            res.update(rerank_legs(fm, gal, q, depth, args.calls))
            ranks = fm.rerank(q, gal, depth=depth, k=10, gt_idx="diag")[0]
            listed = ranks <= depth
            res.update({"dense_over_rerank": dense_ms / res["rerank_ms"], "faster_than_dense": bool(res["rerank_ms"] < dense_ms),
                        "shortlist_recall": float(listed.double().mean() * 100.0),
                        # with the same candidates ahead of it or fewer: a listed ground truth never ranks behind its dense rank
                        "listed_ranks_le_dense": bool((ranks[listed] <= d_ranks[listed]).all())})
            emit(res)
        del gal
    if args.only in (None, "fused"):
        q, img, tgt = embeddings(args.n, args.n, args.d, dev)
        gal = fm.prepare_gallery(img, tgt)
        res = {"case": "offline_fused_rerank_d200", "nq": args.n, "ng": args.n, "dim": args.d}
        res.update(fused_legs(fm, gal, q, 200, 50, args.calls))
        emit(res)
        del gal
    if args.only in (None, "online"):
        q, img, tgt = embeddings(args.ng, 1, args.d, dev)
        gal = fm.prepare_gallery(img, tgt)
        res = {"case": "online_d200", "nq": 1, "ng": args.ng, "dim": args.d}
        res.update(rerank_legs(fm, gal, q, 200, args.calls))
        res["gallery_GB"] = (gal.cand["Pi"].numel() + gal.cand["Ki"].numel()) * 2 * 4 / 1e9
        emit(res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
