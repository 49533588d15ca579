#!/usr/bin/env python3
"""End-to-end fine-tuning on one MI355X: the fused training ops of csrc/train_ops.hip alone, one vision-tower step and one whole
end-to-end step at ViT-L/14 with 64 images, with elementwise="op" and with elementwise="torch" (the torch autograd formulation: the
baseline), and the peak device memory of both.

    python tools/bench_end_to_end_train.py [--images 64] [--reps 20] [--out profiles/end_to_end_train_bench.json]

* `ops`: `kemr_op_layernorm_backward` at [16 448, 1024] (dy bf16) against autograd's backward of an fp32 `F.layer_norm` fed the same
  gradient (the bf16 -> fp32 cast of dy included: it is what the cast's backward does in the tower); `kemr_op_act_forward` /
  `kemr_op_act_backward` at [16 448, 4096], QuickGELU and exact GELU, against the chain the tower runs under autocast (bf16 -> fp32, the
  activation in fp32, -> bf16) and autograd's backward of it.  `gbytes_per_s` is the ALGORITHMIC bytes of the fused op over
  the measured time, for both columns: the torch chain moves more than that, which is the point.
* `vision_step`: VisionTower forward on `images` images, a linear probe loss, backward, AdamW over the vision parameters.
* `end_to_end_step`: EndToEndTuning forward on `images` images and 2 x `images` texts of 77 positions (every text fills the context),
  JointContrastiveLoss, backward, AdamW over every trained parameter.
* `max_memory_allocated_gb`: torch.cuda.max_memory_allocated over the timed steps of each setting (weights, gradients and optimizer
  state included; they are the same in both settings).

Each figure is the median of `reps` repetitions, each timed between two device events, after three warm-up repetitions (ops: windows
of 10 back-to-back launches, so that a window is about a millisecond; the figure is per launch).  Nothing here says which is faster in
advance: the result is the file.  Prints one JSON object (also written to --out)."""
import argparse
import gc
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from knowledge_enhanced_multimodal_retrieval_amd import clip_module, engine, finetune, losses, tower_train  # noqa: E402

TEMPERATURE, T2I_W, T2T_W = 0.07, 0.7, 0.3
MODEL = "ViT-L/14"
ROWS, WIDTH = 16448, 1024                # 64 images x 257 tokens, ViT-L/14's vision width


def timed(fn, reps, inner=1):
    for _ in range(3):
        for _ in range(inner):
            fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / inner)
    return {"ms": statistics.median(ms), "ms_min_max": [min(ms), max(ms)]}


def _rate(entry, nbytes):
    entry["gbytes_per_s"] = nbytes / (entry["ms"] * 1e-3) / 1e9
    return entry


def bench_ops(reps, dev):
    g = torch.Generator().manual_seed(0)
    out = {"rows": ROWS}
    # ---- LayerNorm backward
    x = (torch.randn(ROWS, WIDTH, generator=g) + 0.5).to(dev)
    gamma, beta = (torch.rand(WIDTH, generator=g) + 0.5).to(dev), torch.randn(WIDTH, generator=g).to(dev)
    dy = torch.randn(ROWS, WIDTH, generator=g).to(dev).to(torch.bfloat16)
    xr, gr, br = x.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    y = F.layer_norm(xr, (WIDTH,), gr, br, 1e-5)
    nbytes = ROWS * WIDTH * (4 + 2 + 4)
    ref = torch.autograd.grad(y, (xr, gr, br), dy.float(), retain_graph=True)
    got = engine.layernorm_backward(x, gamma, dy)
    out["layernorm_backward"] = {
        "shape": [ROWS, WIDTH], "algorithmic_bytes": nbytes,
        "max_diff_vs_torch": [float((a - b).abs().max() / b.abs().max()) for a, b in zip(got, ref)],
        "op": _rate(timed(lambda: engine.layernorm_backward(x, gamma, dy), reps, 10), nbytes),
        "torch": _rate(timed(lambda: torch.autograd.grad(y, (xr, gr, br), dy.float(), retain_graph=True), reps, 10), nbytes)}
    del xr, gr, br, y, ref, got
    # ---- the activation
    n = ROWS * 4 * WIDTH
    pre = (torch.randn(ROWS, 4 * WIDTH, generator=g) * 2).to(dev).to(torch.bfloat16)
    dout = torch.randn(ROWS, 4 * WIDTH, generator=g).to(dev).to(torch.bfloat16)
    for kind in ("quick_gelu", "gelu"):
        def chain(p):
            h = p.float()
            return (F.gelu(h) if kind == "gelu" else h * torch.sigmoid(1.702 * h)).to(torch.bfloat16)
        pr = pre.clone().requires_grad_(True)
        yr = chain(pr)
        out[f"act_forward_{kind}"] = {"shape": [ROWS, 4 * WIDTH], "algorithmic_bytes": 4 * n,
                                      "op": _rate(timed(lambda: engine.act_forward(pre, kind), reps, 10), 4 * n),
                                      "torch": _rate(timed(lambda: chain(pre), reps, 10), 4 * n)}
        out[f"act_backward_{kind}"] = {"shape": [ROWS, 4 * WIDTH], "algorithmic_bytes": 6 * n,
                                       "op": _rate(timed(lambda: engine.act_backward(pre, dout, kind), reps, 10), 6 * n),
                                       "torch": _rate(timed(lambda: torch.autograd.grad(yr, pr, dout, retain_graph=True), reps, 10), 6 * n)}
        del pr, yr
    return out


def bench_steps(images, reps, dev):
    g = torch.Generator().manual_seed(1)
    arch = clip_module.get_arch(MODEL)
    pixels = torch.randn(images, 3, arch.image_size, arch.image_size, generator=g).to(dev)
    ids = torch.randint(1, arch.vocab - 2, (2 * images, arch.ctx), generator=g, dtype=torch.int32)
    ids[:, 0], ids[:, -1] = arch.vocab - 2, arch.vocab - 1
    ids = ids.to(dev)
    probe = torch.randn(images, arch.embed_dim, generator=g).to(dev)
    loss_fn = losses.JointContrastiveLoss(TEMPERATURE, T2I_W, T2T_W)
    out = {"vision_step": {}, "end_to_end_step": {}}
    for what in ("vision_step", "end_to_end_step"):
        for elementwise in ("op", "torch"):
            gc.collect()
            torch.cuda.empty_cache()
            torch.manual_seed(0)
            model = clip_module.build_model(MODEL, device=dev).float()
            if what == "vision_step":
                for p in model.parameters():
                    p.requires_grad = False
                tune = tower_train.VisionTower(model, elementwise=elementwise)

                def forward():
                    return (tune(pixels) * probe).sum()
            else:
                tune = tower_train.EndToEndTuning(model, elementwise=elementwise)

                def forward():
                    return loss_fn(*tune(pixels, ids[:images], ids[images:]))[0]
            opt, _ = finetune.build_optimizer(tune, lr=1e-5, weight_decay=0.01, num_epochs=1)

            def step():
                opt.zero_grad()
                forward().backward()
                opt.step()

            step()                                       # the optimizer state exists before the peak is reset
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats(dev)
            entry = timed(step, reps)
            entry["max_memory_allocated_gb"] = torch.cuda.max_memory_allocated(dev) / 1e9
            out[what][elementwise] = entry
            del model, tune, opt, forward, step
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", type=str, default=os.path.join("profiles", "end_to_end_train_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_end_to_end_train: needs a GPU (a CPU run says nothing about the MI355X)")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "model": MODEL, "images": args.images, "texts": 2 * args.images, "reps": args.reps,
           "ops": bench_ops(args.reps, dev)}
    res.update(bench_steps(args.images, args.reps, dev))
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
