#!/usr/bin/env python3
"""The fused InfoNCE loss (forward + backward) and one full head step on one MI355X, against the torch fp32 formulation on the same device.

    python tools/bench_finetune.py [--sizes 64 4096 32768] [--width 768] [--reps 5] [--out profiles/finetune_bench.json]

ViT-L/14 widths: tower rows 1024 (vision) / 768 (text), embeddings D = 768.  Per n:

* `loss_fused_ms`: JointContrastiveLoss (two InfoNCE pairs, as the trainer calls it) forward + backward on unit-norm features
  [n, D] that require grad -- the kernels of csrc/infonce.hip through losses.py;
* `loss_torch_ms`: the same loss and gradients as torch fp32 on the device: cross entropy of (a @ b.T) / tau both ways where the
  n x n logits fit (n <= 8192), else the same mathematics chunked over 4096 rows with its own hand-written backward (a pass for the
  row and column lse values, a pass for the gradients), so that no n x n buffer exists -- `torch_mode` says which ran;
* `step_fused_ms` / `step_torch_ms`: one whole head step on cached pooled rows -- ProjectionHeads forward, the loss, backward, AdamW
  step -- with either loss;
* `max_grad_diff`: the largest difference between the two formulations' feature gradients relative to the largest gradient entry (what
  the comparison is a comparison of).

Each figure is the median of `reps` repetitions after one warm-up, timed with device events around work that ends in a synchronise.
Nothing here says which is faster in advance: the result is the file.  Prints one JSON object (also written to --out)."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from knowledge_enhanced_multimodal_retrieval_amd import finetune, losses  # noqa: E402

TEMPERATURE, T2I_W, T2T_W = 0.07, 0.7, 0.3
DENSE_MAX, CHUNK = 8192, 4096


def torch_infonce_dense(a, b):
    z = (a @ b.T) / TEMPERATURE
    lab = torch.arange(a.shape[0], device=a.device)
    return (F.cross_entropy(z, lab) + F.cross_entropy(z.T, lab)) / 2


class _ChunkedInfoNCE(torch.autograd.Function):
    """torch fp32, no n x n buffer: row chunks of CHUNK items; the column lse needs its own pass before the gradients."""

    @staticmethod
    def forward(ctx, a, b):
        n = a.shape[0]
        lse_r = torch.empty(n, device=a.device)
        col_m = torch.full((n,), -float("inf"), device=a.device)
        col_s = torch.zeros(n, device=a.device)
        diag = (a * b).sum(-1) / TEMPERATURE
        for s in range(0, n, CHUNK):
            z = (a[s:s + CHUNK] @ b.T) / TEMPERATURE
            lse_r[s:s + CHUNK] = torch.logsumexp(z, 1)
            m = torch.maximum(col_m, z.max(0).values)
            col_s = col_s * torch.exp(col_m - m) + torch.exp(z - m).sum(0)
            col_m = m
        lse_c = col_m + torch.log(col_s)
        ctx.save_for_backward(a, b, lse_r, lse_c)
        return ((lse_r - diag).mean() + (lse_c - diag).mean()) / 2

    @staticmethod
    def backward(ctx, g):
        a, b, lse_r, lse_c = ctx.saved_tensors
        n = a.shape[0]
        ga, gb = torch.empty_like(a), torch.zeros_like(b)
        for s in range(0, n, CHUNK):
            z = (a[s:s + CHUNK] @ b.T) / TEMPERATURE
            gz = (torch.exp(z - lse_r[s:s + CHUNK, None]) + torch.exp(z - lse_c[None, :])) / (2 * n)
            rows = torch.arange(z.shape[0], device=a.device)
            gz[rows, rows + s] -= 1.0 / n
            ga[s:s + CHUNK] = (gz @ b) / TEMPERATURE
            gb += (gz.T @ a[s:s + CHUNK]) / TEMPERATURE
        return ga * g, gb * g


def torch_joint(image, query, target):
    nce = torch_infonce_dense if image.shape[0] <= DENSE_MAX else _ChunkedInfoNCE.apply
    return T2I_W * nce(target, image) + T2T_W * nce(query, target), None


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


class _Heads(torch.nn.Module):
    """ProjectionHeads' arithmetic on parameters of its own (ViT-L/14 shapes), for the step timing."""

    def __init__(self, vw, tw, d, dev):
        super().__init__()
        self.ln_post, self.ln_final = torch.nn.LayerNorm(vw).to(dev), torch.nn.LayerNorm(tw).to(dev)
        self.visual_proj = torch.nn.Parameter(torch.randn(vw, d, device=dev) * vw ** -0.5)
        self.text_projection = torch.nn.Parameter(torch.randn(tw, d, device=dev) * tw ** -0.5)

    def forward(self, pi, pq, pt):
        return (finetune.project(pi, self.ln_post.weight, self.ln_post.bias, self.visual_proj, 1e-5),
                finetune.project(pq, self.ln_final.weight, self.ln_final.bias, self.text_projection, 1e-5),
                finetune.project(pt, self.ln_final.weight, self.ln_final.bias, self.text_projection, 1e-5))


def bench_size(n, d, reps, dev):
    g = torch.Generator(device="cpu").manual_seed(n)
    unit = lambda x: (x / x.norm(dim=-1, keepdim=True)).to(dev)           # noqa: E731
    base = torch.randn(n, d, generator=g)
    feats = [unit(base + torch.randn(n, d, generator=g)).requires_grad_(True) for _ in range(3)]
    fused = losses.JointContrastiveLoss(TEMPERATURE, T2I_W, T2T_W)

    def run(loss_fn):
        for f in feats:
            f.grad = None
        loss_fn(*feats)[0].backward()

    out = {"n": n, "d": d, "torch_mode": "dense n x n" if n <= DENSE_MAX else f"chunked over {CHUNK} rows, no n x n buffer"}
    run(fused)
    g_fused = [f.grad.clone() for f in feats]
    run(torch_joint)
    scale = max(float(f.grad.abs().max()) for f in feats)
    out["max_grad_diff"] = max(float((a - f.grad).abs().max()) for a, f in zip(g_fused, feats)) / scale
    out["loss_fused_ms"] = timed(lambda: run(fused), reps)
    out["loss_torch_ms"] = timed(lambda: run(torch_joint), reps)
    vw, tw = 1024, 768
    heads = _Heads(vw, tw, d, dev)
    opt = torch.optim.AdamW(heads.parameters(), lr=1e-5, weight_decay=0.01, betas=(0.9, 0.98), eps=1e-6)
    pooled = (torch.randn(n, vw, generator=g).to(dev), torch.randn(n, tw, generator=g).to(dev), torch.randn(n, tw, generator=g).to(dev))

    def step(loss_fn):
        opt.zero_grad()
        loss_fn(*heads(*pooled))[0].backward()
        opt.step()

    out["step_fused_ms"] = timed(lambda: step(fused), reps)
    out["step_torch_ms"] = timed(lambda: step(torch_joint), reps)
    # useful work of the loss, forward + backward, both pairs: 2 (row and column logits) + 1 (recomputed logits) + 2 (two gradients) products of 2 n^2 d
    out["loss_fused_useful_tflops"] = 2 * 5 * 2.0 * n * n * d / (out["loss_fused_ms"] * 1e-3) / 1e12
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[64, 4096, 32768])
    ap.add_argument("--width", type=int, default=768)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", type=str, default=os.path.join("profiles", "finetune_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_finetune needs the GPU: a timing taken anywhere else says nothing about it")
    dev = torch.device("cuda:0")
    result = {"device": torch.cuda.get_device_name(0), "temperature": TEMPERATURE, "weights": [T2I_W, T2T_W], "reps": args.reps,
              "sizes": [bench_size(n, args.width, args.reps, dev) for n in args.sizes]}
    line = json.dumps(result)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
