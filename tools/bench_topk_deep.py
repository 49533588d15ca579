"""Deep top-k timings (tools only): kemr_sim_topk_deep against its two yardsticks on the same operands, in one process.

    python tools/bench_topk_deep.py [--out profiles/topk_deep_bench.txt] [--calls 30] [--only NAME]

Shapes: Q = 1024 x N = 43 000 on bf16 panels (kdim 768) at k = 100 and k = 1000; Q = 1 x N = 43 000 on the store's fused fp32x3
panel ([image ; text], kdim 4608) at k = 200 -- the online case.  Per shape, hipEvents around every call, median of >= 20 calls
after >= 100 ms of warm-up:
  deep        engine.sim_topk_deep(qp, gp, k)
  select      engine.select_topk on the materialised matrix alone (the selection pass without the score pass)
  dense       engine.scores_dense alone (the score pass)
  shallow32   (a) engine.sim_topk at k = 32: what going deep costs over the existing path
  torch_topk  (b) engine.scores_dense + torch.topk(sorted=True): a library yardstick, here only
The shape fused_k100 (Q = 1024 x N = 43 000, k = 100, a ground truth and a SPARQL bonus list of about ten hits per query) times the
knowledge-fused call against the same result made without it, the two alternating call by call in one process:
  fused       engine.sim_topk_deep(qp, gp, 100, gt_idx, gt_score, ahead, bonus): lists of fused scores + rank counts, one scoring pass
  pair        engine.sim_topk_deep(qp, gp, 100) followed by engine.sim_topk(qp, gp, 0, gt_idx, gt_score, ahead, bonus): two scoring
              passes (and lists WITHOUT the bonus: the pair is the cheaper half of what the fused call returns)
One JSON line per shape.  For the per-kernel split run it under `rocprofv3 --kernel-trace --stats -- python tools/bench_topk_deep.py
--only NAME` in a run of its own.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from knowledge_enhanced_multimodal_retrieval_amd import _lib, engine  # noqa: E402


def timed(fn, calls):
    """Median ms per call: hipEvents around each call, after at least 100 ms (and 3 calls) of warm-up."""
    t0, n = time.perf_counter(), 0
    while n < 3 or time.perf_counter() - t0 < 0.1:
        fn()
        torch.cuda.synchronize()
        n += 1
    ms = []
    for _ in range(max(calls, 20)):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def timed_alternating(fns, calls):
    """Median ms per call of each of `fns`, timed in turn (a, b, a, b, ...) so that both see the same clocks and neighbours."""
    t0, n = time.perf_counter(), 0
    while n < 3 or time.perf_counter() - t0 < 0.2:
        for fn in fns:
            fn()
        torch.cuda.synchronize()
        n += 1
    ms = [[] for _ in fns]
    for _ in range(max(calls, 20)):
        for j, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[j].append(a.elapsed_time(b))
    return [statistics.median(m) for m in ms]


def fused_leg(qry, gal, args):
    """Q = 1024 x N, k = 100, ground truth + about ten hits per query: the fused call against sim_topk_deep + a rank-only sim_topk."""
    dev = qry.device
    nq, ng, k = qry.shape[0], gal.shape[0], 100
    qp = engine.build_panel([qry], _lib.SIDE_QUERY, 1)
    gp = engine.build_panel([gal], _lib.SIDE_GALLERY, 1)
    gg = torch.Generator().manual_seed(11)
    counts = torch.randint(6, 15, (nq,), generator=gg)
    rowptr = torch.zeros(nq + 1, dtype=torch.int32)
    rowptr[1:] = torch.cumsum(counts, 0)
    col = torch.cat([torch.sort(torch.randperm(ng, generator=gg)[:int(c)]).values for c in counts]).to(torch.int32)
    val = torch.full((col.numel(),), 0.2)
    bonus = tuple(t.to(dev) for t in (rowptr, col, val))
    gt = torch.arange(nq, dtype=torch.int32, device=dev)                   # the query's own image, as in the evaluators
    sgt = engine.pair_scores(qp, gp, gt, gt)
    ahead_f = torch.zeros(nq, dtype=torch.int32, device=dev)
    ahead_p = torch.zeros(nq, dtype=torch.int32, device=dev)

    def fused():
        return engine.sim_topk_deep(qp, gp, k, gt_idx=gt, gt_score=sgt, ahead=ahead_f, bonus=bonus)

    def pair():
        out = engine.sim_topk_deep(qp, gp, k)
        engine.sim_topk(qp, gp, 0, 0, gt, sgt, ahead_p, bonus)
        return out

    fused()
    pair()
    same_ranks = bool(torch.equal(ahead_f, ahead_p))
    fused_ms, pair_ms = timed_alternating([fused, pair], args.calls)
    res = {"shape": "fused_k100", "nq": nq, "ng": ng, "kdim": qp.kdim, "k": k, "hits": int(col.numel()),
           "fused_ms": fused_ms, "pair_ms": pair_ms, "fused_over_pair": fused_ms / pair_ms, "ranks_equal": same_ranks}
    return {key: (round(v, 4) if isinstance(v, float) else v) for key, v in res.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--ng", type=int, default=43000)
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--only", default=None, help="one of batch_k100, batch_k1000, online_k200, fused_k100")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    gg = torch.Generator(device=dev).manual_seed(7)
    gal = torch.nn.functional.normalize(torch.randn(args.ng, args.d, generator=gg, device=dev), dim=-1)
    txt = torch.nn.functional.normalize(gal + 0.5 * torch.randn(args.ng, args.d, generator=gg, device=dev), dim=-1)
    qry = torch.nn.functional.normalize(gal[:1024] + 1.2 * torch.randn(1024, args.d, generator=gg, device=dev), dim=-1)
    shapes = [("batch_k100", 1024, 100, 1, False), ("batch_k1000", 1024, 1000, 1, False), ("online_k200", 1, 200, 3, True)]
    lines = []
    for name, nq, k, terms, fused in shapes:
        if args.only and name != args.only:
            continue
        q = qry[:nq]
        if fused:
            qp = engine.build_panel([q, q], _lib.SIDE_QUERY, terms, part_scale=[0.5, 0.5])
            gp = engine.build_panel([gal, txt], _lib.SIDE_GALLERY, terms)
        else:
            qp = engine.build_panel([q], _lib.SIDE_QUERY, terms)
            gp = engine.build_panel([gal], _lib.SIDE_GALLERY, terms)
        S = engine.scores_dense(qp, gp)
        deep_s, deep_i = engine.sim_topk_deep(qp, gp, k)
        ts, ti = torch.topk(S, k, dim=1, sorted=True)
        res = {
            "shape": name, "nq": nq, "ng": args.ng, "kdim": qp.kdim, "k": k,
            "deep_ms": timed(lambda: engine.sim_topk_deep(qp, gp, k), args.calls),
            "select_ms": timed(lambda: engine.select_topk(S, k), args.calls),
            "dense_ms": timed(lambda: engine.scores_dense(qp, gp), args.calls),
            "shallow32_ms": timed(lambda: engine.sim_topk(qp, gp, 32), args.calls),
            "torch_topk_ms": timed(lambda: torch.topk(engine.scores_dense(qp, gp), k, dim=1, sorted=True), args.calls),
            "torch_topk_alone_ms": timed(lambda: torch.topk(S, k, dim=1, sorted=True), args.calls),
            # torch.topk does not promise an order among equal scores: compare the score lists, and the ids where scores are distinct
            "scores_equal_torch": bool(torch.equal(deep_s, ts)),
            "ids_equal_torch": bool(torch.equal(deep_i.long(), ti)),
        }
        res = {key: (round(v, 4) if isinstance(v, float) else v) for key, v in res.items()}
        line = json.dumps(res)
        print(line, flush=True)
        lines.append(line)
    if not args.only or args.only == "fused_k100":
        line = json.dumps(fused_leg(qry, gal, args))
        print(line, flush=True)
        lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
