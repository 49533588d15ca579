#!/usr/bin/env python3
"""Training ViT-H-14's vision tower (width 1280 = 16 heads of 80, 32 blocks, 257 tokens) on one MI355X: its attention forward + backward
alone, with the library's kernels (kemr_op_attention_hd forward, kemr_op_attention_backward_hd backward) and with
torch.nn.functional.scaled_dot_product_attention in their place, and one whole training step of the tower with attention="op" and
with attention="torch" (the plain formulation, the only alternative a user of tower_train has).

    python tools/bench_attention_backward_hd80.py [--batch 8 32] [--reps 20] [--out profiles/attention_backward_hd80_bench.json]

Per batch size (random weights and pixels):

* `attn_op_ms` / `attn_sdpa_ms`: attention forward + backward on bf16 q | k | v of one block's shape [batch x 257, 3 x 1280], non-causal:
  the two kernels through the autograd function the tower uses (the 80 ** -0.5 scaling of q and dq included), and SDPA on the same
  values viewed as [batch, 16, 257, 80] (the backend torch picks);
* `attn_max_grad_diff`: the largest difference between the two formulations' dqkv relative to the largest entry (what is compared);
* `attn_op_peak_bytes` / `attn_sdpa_peak_bytes`: the peak of device memory allocated during one forward + backward above what was
  allocated before it (inputs and the gradient buffer excluded);
* `step_op_ms` / `step_torch_ms`: one whole step -- VisionTower(head_dims=HEAD_DIMS, elementwise="op") forward under bf16 autocast, a
  linear probe loss, backward, AdamW step -- with either attention;
* `step_op_peak_bytes` / `step_torch_peak_bytes`: the peak of device memory allocated during one such step above what was allocated
  before it (weights, gradients and optimizer states of BOTH towers are resident and excluded: what is left is the step's activations).

Each time is the median of `reps` timed windows after three warm-up windows, a window being `inner` back-to-back repetitions between
two device events; the figure is per repetition.  The two formulations' windows alternate, so that whatever else the machine does falls
on both.  Nothing here says which is faster in advance: the result is the file.  Prints one JSON object (also written to --out)."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from knowledge_enhanced_multimodal_retrieval_amd import clip_module, tower_train  # noqa: E402
from knowledge_enhanced_multimodal_retrieval_amd.config import ARCHS  # noqa: E402

NAME = "ViT-H-14"
ARCH = ARCHS[NAME]
WIDTH, T, HD = ARCH.v_width, ARCH.v_tokens, ARCH.v_head_dim


def sdpa_attention(qkv, batch, t, width):
    q, k, v = (x.reshape(batch, t, width // HD, HD).transpose(1, 2) for x in qkv.split(width, dim=-1))
    return F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(batch * t, width)


def timed_alternating(fns, reps, inner):
    """{name: (median, min, max)} ms per repetition; the windows of the formulations alternate."""
    for _ in range(3):
        for fn in fns.values():
            for _ in range(inner):
                fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1) / inner)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in ms.items()}


def peak_above(fn):
    """The peak of allocated device memory during fn() above what was allocated before it, in bytes (fn has run before: warm)."""
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated() - base)


def bench_size(n, reps, dev):
    g = torch.Generator().manual_seed(n)
    out = {"batch": n, "t": T, "width": WIDTH, "head_dim": HD}
    # ---- attention alone
    rows = n * T
    qkv = torch.randn(rows, 3 * WIDTH, generator=g).to(dev).to(torch.bfloat16).requires_grad_(True)
    dout = torch.randn(rows, WIDTH, generator=g).to(dev).to(torch.bfloat16)

    def attn(which):
        qkv.grad = None
        o = tower_train._OpAttention.apply(qkv, n, T, WIDTH, False, HD) if which == "op" else sdpa_attention(qkv, n, T, WIDTH)
        o.backward(dout)
        return qkv.grad

    g_op, g_sdpa = attn("op").float().clone(), attn("sdpa").float().clone()
    out["attn_max_grad_diff"] = float((g_op - g_sdpa).abs().max() / g_sdpa.abs().max())
    del g_op, g_sdpa
    res = timed_alternating({"op": lambda: attn("op"), "sdpa": lambda: attn("sdpa")}, reps, max(1, 64 // n))
    for which, (med, lo, hi) in res.items():
        out[f"attn_{which}_ms"], out[f"attn_{which}_ms_min_max"] = med, [lo, hi]
    for which in ("op", "sdpa"):
        qkv.grad = None
        out[f"attn_{which}_peak_bytes"] = peak_above(lambda: attn(which)) - qkv.numel() * 2       # less the gradient buffer itself
    qkv.grad = None
    del qkv, dout
    # ---- one whole step of the tower
    pixels = torch.randn(n, 3, ARCH.image_size, ARCH.image_size, generator=g).to(dev)
    probe = torch.randn(n, ARCH.embed_dim, generator=g).to(dev)
    steps = {}
    keep = []
    for which in ("op", "torch"):
        torch.manual_seed(0)
        model = clip_module.build_model(ARCH, device=dev).float()
        tower = tower_train.VisionTower(model, attention=which, elementwise="op", autocast=True, head_dims=tower_train.HEAD_DIMS)
        opt = torch.optim.AdamW(list(tower.named_vision_parameters().values()), lr=1e-5, weight_decay=0.01)

        def step(tower=tower, opt=opt):
            opt.zero_grad(set_to_none=False)
            (tower(pixels) * probe).sum().backward()
            opt.step()

        for p in tower.named_vision_parameters().values():      # resident gradients: the peak below is the activations'
            p.grad = torch.zeros_like(p)
        steps[which] = step
        keep.append((model, tower, opt))
    res = timed_alternating(steps, max(3, reps // 2), 1)
    for which, (med, lo, hi) in res.items():
        out[f"step_{which}_ms"], out[f"step_{which}_ms_min_max"] = med, [lo, hi]
    for which in ("op", "torch"):
        out[f"step_{which}_peak_bytes"] = peak_above(steps[which])
    del keep, steps
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, nargs="+", default=[8, 32])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", type=str, default=os.path.join("profiles", "attention_backward_hd80_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_attention_backward_hd80: needs a GPU (a CPU run says nothing about the MI355X)")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "model": NAME,
           "tower": {"width": WIDTH, "layers": ARCH.v_layers, "tokens": T, "heads": WIDTH // HD, "head_dim": HD},
           "reps": args.reps, "sizes": [bench_size(n, args.reps, dev) for n in args.batch]}
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
