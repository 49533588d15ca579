#!/usr/bin/env python3
"""The fused pair-score contrastive loss (forward + backward) on one MI355X, against the torch fp32 formulation on the same device.

    python tools/bench_fusion_train.py [--sizes 64 4096 32768] [--width 768] [--reps 5] [--out profiles/fusion_train_bench.json]

Per n and per kernel mode -- `gated` (a simple_gated_with_bias head) and `linear` (the reference's MLP(2 -> 128 -> 1)) -- on unit-norm
embeddings [n, D]:

* `fused_ms`: losses.FusionContrastiveLoss forward + backward into the head's parameters -- the kernels of csrc/pairhead.hip;
* `torch_ms`: the same loss and parameter gradients as torch fp32 on the device.  `torch_mode` says which formulation ran: the dense
  one (autograd through the n x n scores; for the linear head through the n x n x 128 hidden activations) where `--dense_gib` holds
  what autograd keeps, else the same mathematics chunked over query rows with recomputation -- a pass without autograd for the row and
  column lse values, then per chunk the scores again with autograd and the softmax gradient pushed through them -- so that nothing of
  size n x n (x 128) is alive at once;
* `fused_peak_mib` / `torch_peak_mib`: the allocator's peak during one forward + backward, above what was allocated before it;
* `max_grad_diff`: the largest difference between the two formulations' parameter gradients relative to the largest gradient entry.

Each time is the median of `reps` repetitions after one warm-up, timed with device events around work that ends in a synchronise.
Nothing here says which is faster in advance: the result is the file.  Prints one JSON object (also written to --out)."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from knowledge_enhanced_multimodal_retrieval_amd import losses  # noqa: E402
from knowledge_enhanced_multimodal_retrieval_amd.fusion_model import FusionModel  # noqa: E402

TEMPERATURE = 0.07
HEAD_OF_MODE = {"gated": "simple_gated_with_bias", "linear": "linear"}


def score_rows(fm, q, img, tgt):
    """The head's scores of the query rows `q` against the whole gallery, plain torch (differentiable in the head's parameters)."""
    t2i, t2t = q @ img.T, q @ tgt.T
    if fm.fusion_type == "linear":
        return fm.fusion_head.fusion(torch.stack([t2i, t2t], dim=-1)).squeeze(-1)
    g = fm.fusion_head.gate(q).reshape(-1, 1)
    return g * t2i + (1 - g) * t2t


def torch_dense(fm, q, img, tgt):
    z = score_rows(fm, q, img, tgt) / TEMPERATURE
    diag = torch.diagonal(z)
    loss = ((torch.logsumexp(z, 1) - diag).mean() + (torch.logsumexp(z, 0) - diag).mean()) / 2
    loss.backward()
    return loss.detach()


def torch_chunked(fm, q, img, tgt, rows):
    """Two passes over chunks of `rows` queries; parameter gradients accumulate in .grad."""
    n = q.shape[0]
    dev = q.device
    lse_r = torch.empty(n, device=dev)
    diag = torch.empty(n, device=dev)
    col_m = torch.full((n,), -float("inf"), device=dev)
    col_s = torch.zeros(n, device=dev)
    with torch.no_grad():
        for s in range(0, n, rows):
            z = score_rows(fm, q[s:s + rows], img, tgt) / TEMPERATURE
            lse_r[s:s + rows] = torch.logsumexp(z, 1)
            idx = torch.arange(z.shape[0], device=dev)
            diag[s:s + rows] = z[idx, idx + s]
            m = torch.maximum(col_m, z.max(0).values)
            col_s = col_s * torch.exp(col_m - m) + torch.exp(z - m).sum(0)
            col_m = m
        lse_c = col_m + torch.log(col_s)
    for s in range(0, n, rows):
        scores = score_rows(fm, q[s:s + rows], img, tgt)
        with torch.no_grad():
            z = scores / TEMPERATURE
            gz = (torch.exp(z - lse_r[s:s + rows, None]) + torch.exp(z - lse_c[None, :])) / (2 * n)
            idx = torch.arange(z.shape[0], device=dev)
            gz[idx, idx + s] -= 1.0 / n
            gz /= TEMPERATURE
        (scores * gz).sum().backward()
    return ((lse_r - diag).mean() + (lse_c - diag).mean()) / 2


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms)


def peak_mib(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def bench(mode, n, d, reps, dense_gib, chunk_gib, dev):
    g = torch.Generator(device="cpu").manual_seed(n)
    unit = lambda x: (x / x.norm(dim=-1, keepdim=True)).to(dev)           # noqa: E731
    base = torch.randn(n, d, generator=g)
    q, img, tgt = [unit(base + torch.randn(n, d, generator=g)) for _ in range(3)]
    torch.manual_seed(n)
    fm = FusionModel(torch.nn.Linear(1, 1), fusion_type=HEAD_OF_MODE[mode], embed_dim=d).to(dev).eval()
    if mode == "gated":
        with torch.no_grad():
            fm.fusion_head.query_weight.normal_(0.0, 1.0)                # the default (all zeros) makes every gate equal
    params = list(fm.fusion_head.parameters())
    fused = losses.FusionContrastiveLoss(TEMPERATURE)
    per_pair = 4 * (2 + 3 * 128) if mode == "linear" else 4 * 8          # bytes autograd keeps per pair, roughly: logits, hidden + mask + product
    dense = n * n * per_pair <= dense_gib * 2 ** 30
    rows = n if dense else max(1, min(n, int(chunk_gib * 2 ** 30) // (n * per_pair)))

    def zero():
        for p in params:
            p.grad = None

    def run_fused():
        zero()
        fused(fm, q, img, tgt)[0].backward()

    def run_torch():
        zero()
        return torch_dense(fm, q, img, tgt) if dense else torch_chunked(fm, q, img, tgt, rows)

    out = {"mode": mode, "head": HEAD_OF_MODE[mode], "n": n, "d": d,
           "torch_mode": "dense, autograd through n x n" + (" x 128" if mode == "linear" else "") if dense
           else f"chunked over {rows} query rows with recomputation, nothing of size n x n alive"}
    run_fused()
    g_fused = [p.grad.clone() for p in params]
    loss_fused = float(fused(fm, q, img, tgt)[0].detach())
    loss_torch = float(run_torch())
    scale = max(float(p.grad.abs().max()) for p in params)
    out["loss_fused"], out["loss_torch"] = loss_fused, loss_torch
    out["max_grad_diff"] = max(float((a - p.grad).abs().max()) for a, p in zip(g_fused, params)) / max(scale, 1e-30)
    out["fused_peak_mib"], out["torch_peak_mib"] = peak_mib(run_fused), peak_mib(run_torch)
    out["fused_ms"] = timed(run_fused, reps)
    out["torch_ms"] = timed(run_torch, max(1, reps if dense else min(reps, 2)))
    # useful matrix work of the fused loss: 2 logit matrices x (row pass + column pass + backward) products of 2 n^2 d, three bf16 products each not counted
    out["fused_useful_tflops"] = 6 * 2.0 * n * n * d / (out["fused_ms"] * 1e-3) / 1e12
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[64, 4096, 32768])
    ap.add_argument("--modes", type=str, nargs="+", default=["gated", "linear"], choices=["gated", "linear"])
    ap.add_argument("--width", type=int, default=768)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dense_gib", type=float, default=48.0, help="run the dense torch formulation while what autograd keeps fits in this")
    ap.add_argument("--chunk_gib", type=float, default=4.0, help="what one chunk of the recomputing formulation may keep")
    ap.add_argument("--out", type=str, default=os.path.join("profiles", "fusion_train_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_fusion_train needs the GPU: a timing taken anywhere else says nothing about it")
    dev = torch.device("cuda:0")
    result = {"device": torch.cuda.get_device_name(0), "temperature": TEMPERATURE, "reps": args.reps,
              "results": [bench(m, n, args.width, args.reps, args.dense_gib, args.chunk_gib, dev) for n in args.sizes for m in args.modes]}
    print(json.dumps(result))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
