#!/usr/bin/env python3
"""One locked-image training step of the ViT-L/14 text tower (width 768, 12 blocks, 77 positions) on one MI355X, and its attention alone,
with the library's attention (kemr_op_attention forward, kemr_op_attention_backward backward) and with
torch.nn.functional.scaled_dot_product_attention in its place.

    python tools/bench_text_tower_train.py [--pairs 64 512] [--reps 20] [--out profiles/text_tower_train_bench.json]

Per size (n pairs = 2 n texts of 77 positions, random weights and token ids; every text fills the context, the longest case):

* `step_op_ms` / `step_sdpa_ms`: one whole step -- LockedImageTuning forward (the text tower under bf16 autocast on 2 n texts, the image
  head on n cached rows), JointContrastiveLoss, backward, AdamW step -- with either attention;
* `attn_op_ms` / `attn_sdpa_ms`: attention forward + backward alone on bf16 q | k | v of one block's shape [2 n x 77, 3 x 768], causal:
  the two kernels through the autograd function the tower uses (the 1/8 scaling of q and dq included), and SDPA on the same values
  viewed as [2 n, 12, 77, 64] (`is_causal=True`; the backend torch picks);
* `attn_max_grad_diff`: the largest difference between the two formulations' dqkv relative to the largest entry (what is compared).

Each figure is the median of `reps` timed windows after three warm-up windows, a window being `inner` back-to-back repetitions between
two device events (so that a window is milliseconds, not one launch); the figure is per repetition.  Nothing here says which is faster
in advance: the result is the file.  Prints one JSON object (also written to --out)."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from knowledge_enhanced_multimodal_retrieval_amd import clip_module, finetune, losses, tower_train  # noqa: E402
from knowledge_enhanced_multimodal_retrieval_amd.config import ClipArch  # noqa: E402

TEMPERATURE, T2I_W, T2T_W = 0.07, 0.7, 0.3
WIDTH, LAYERS, CTX, VOCAB, EMBED = 768, 12, 77, 49408, 768
# the text tower of ViT-L/14 next to a one-block vision tower: the image tower is locked and only its cached rows take part
ARCH = ClipArch(EMBED, 32, 8, 256, 1, WIDTH, LAYERS, vocab=VOCAB, ctx=CTX)


def sdpa_attention(qkv, batch, t, width):
    q, k, v = (x.reshape(batch, t, width // 64, 64).transpose(1, 2) for x in qkv.split(width, dim=-1))
    return F.scaled_dot_product_attention(q, k, v, is_causal=True).transpose(1, 2).reshape(batch * t, width)


class SdpaTower(tower_train.TextTower):
    def _attend(self, qkv, batch, t):
        return sdpa_attention(qkv, batch, t, self.width)


def timed(fn, reps, inner):
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
    return statistics.median(ms), min(ms), max(ms)


def bench_size(n, reps, dev):
    g = torch.Generator().manual_seed(n)
    out = {"pairs": n, "texts": 2 * n, "t": CTX}
    # ---- attention alone
    rows = 2 * n * CTX
    qkv = torch.randn(rows, 3 * WIDTH, generator=g).to(dev).to(torch.bfloat16).requires_grad_(True)
    dout = torch.randn(rows, WIDTH, generator=g).to(dev).to(torch.bfloat16)

    def attn(which):
        qkv.grad = None
        o = tower_train._OpAttention.apply(qkv, 2 * n, CTX, WIDTH, True) if which == "op" else sdpa_attention(qkv, 2 * n, CTX, WIDTH)
        o.backward(dout)
        return qkv.grad

    g_op, g_sdpa = attn("op").float().clone(), attn("sdpa").float().clone()
    out["attn_max_grad_diff"] = float((g_op - g_sdpa).abs().max() / g_sdpa.abs().max())
    inner = max(1, 2048 // (2 * n))
    for which in ("op", "sdpa"):
        med, lo, hi = timed(lambda: attn(which), reps, inner)
        out[f"attn_{which}_ms"], out[f"attn_{which}_ms_min_max"] = med, [lo, hi]
    # ---- one whole step
    img = torch.randn(n, ARCH.v_width, generator=g).to(dev)
    ids = torch.randint(1, VOCAB - 2, (2 * n, CTX), generator=g, dtype=torch.int32)
    ids[:, 0], ids[:, -1] = VOCAB - 2, VOCAB - 1
    ids = ids.to(dev)
    loss_fn = losses.JointContrastiveLoss(TEMPERATURE, T2I_W, T2T_W)
    for which in ("op", "sdpa"):
        torch.manual_seed(0)
        model = clip_module.build_model(ARCH, device=dev).float()
        tune = tower_train.LockedImageTuning(model)
        if which == "sdpa":
            tune.tower = SdpaTower(model)
        opt, _ = finetune.build_optimizer(tune, lr=1e-5, weight_decay=0.01, num_epochs=1)

        def step():
            opt.zero_grad()
            loss, _ = loss_fn(*tune(img, ids[:n], ids[n:]))
            loss.backward()
            opt.step()

        med, lo, hi = timed(step, reps, 1 if n >= 256 else 4)
        out[f"step_{which}_ms"], out[f"step_{which}_ms_min_max"] = med, [lo, hi]
        del model, tune, opt
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--pairs", type=int, nargs="+", default=[64, 512])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", type=str, default=os.path.join("profiles", "text_tower_train_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_text_tower_train: needs a GPU (a CPU run says nothing about the MI355X)")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "tower": {"width": WIDTH, "layers": LAYERS, "ctx": CTX, "heads": WIDTH // 64},
           "reps": args.reps, "sizes": [bench_size(n, args.reps, dev) for n in args.pairs]}
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
