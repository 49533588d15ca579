"""kemr_rank_dense_shard against kemr_rank_dense on the same matrix in one process: median of 9 device-event-timed repetitions.

    python tools/bench_rank_dense_shard.py [--n 6450] [--k 0]

Both kernels stream the same 4 * N bytes per row (one workgroup per row, one pass); the shard kernel reads 16 bytes per load.
Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from knowledge_enhanced_multimodal_retrieval_amd import _lib  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=6450, help="rows and columns (the test split: 6 450)")
    ap.add_argument("--k", type=int, default=0, help="list length (0: ranks only, what the evaluators ask for)")
    ap.add_argument("--reps", type=int, default=9)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    n, k = args.n, args.k
    L = _lib.lib()
    S = torch.randn(n, n, device=dev, generator=torch.Generator(device=dev).manual_seed(0))
    gt = torch.arange(n, dtype=torch.int32, device=dev)
    sgt = S.diagonal().contiguous()
    ahead = torch.zeros(n, dtype=torch.int32, device=dev)
    ts = torch.empty((n, max(k, 1)), dtype=torch.float32, device=dev) if k else None
    ti = torch.empty((n, max(k, 1)), dtype=torch.int32, device=dev) if k else None
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    calls = {"rank_dense": lambda: L.kemr_rank_dense(p(S), n, n, n, p(gt), p(ahead), k, p(ts), p(ti), stream),
             "rank_dense_shard": lambda: L.kemr_rank_dense_shard(p(S), n, n, n, 0, p(gt), p(sgt), p(ahead), k, p(ts), p(ti), stream)}
    out = {"n": n, "k": k, "reps": args.reps, "bytes": 4 * n * n}
    results = {}
    for name, fn in calls.items():
        for _ in range(3):
            _lib.check(fn(), name)
        torch.cuda.synchronize()
        times = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            _lib.check(fn(), name)
            b.record()
            b.synchronize()
            times.append(a.elapsed_time(b) * 1e3)
        results[name] = ahead.clone()
        out[name] = {"median_us": statistics.median(times), "min_us": min(times), "max_us": max(times),
                     "GB_per_s": 4 * n * n / statistics.median(times) / 1e3}
    out["same_ahead"] = bool(torch.equal(results["rank_dense"], results["rank_dense_shard"]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
