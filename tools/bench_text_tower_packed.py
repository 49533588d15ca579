#!/usr/bin/env python3
"""Training the ViT-L/14 text tower (width 768, 12 blocks) on packed texts on one MI355X: the dense route -- one batch at its longest
text, ``TextTower(packed=False)`` -- against ``packed=True``, every text up to its own end-of-text token.

    python tools/bench_text_tower_packed.py [--pairs 256] [--reps 20] [--out profiles/text_tower_packed_bench.json]

Cases (n pairs = n queries followed by n targets, random weights and token ids; a text's length is its end-of-text position + 1):

* `ctx77_mixed`:   77 positions (CLIP), queries of 8 .. 40 tokens (uniform), every target at 77;
* `ctx248_mixed`:  248 positions (Long-CLIP), queries of 8 .. 40, targets of 150 .. 248 (uniform);
* `ctx77_full`, `ctx248_full`: every text at the full context -- nothing to gain, the packed route is expected not to be slower.

Per case:

* `rows_dense` / `rows_packed`: the rows every linear, LayerNorm, activation and attention of the tower runs on, either route;
* `attn_*_ms`: attention forward + backward alone on bf16 q | k | v of one block's shape, through the autograd functions the tower uses
  (the 1/8 scaling of q and dq included): `dense` = ``_OpAttention`` on [2 n x longest, 3 x 768]; `packed` = ``_OpAttentionPacked`` on
  [rows_packed, 3 x 768] with the calls ``packed_segments`` chooses; `packed_one_call` = the same with one call at the longest item
  (what the split is measured against; equal to `packed` where nothing is split);
* `step_*_ms`: one whole step -- ``LockedImageTuning`` forward (the text tower under bf16 autocast on 2 n texts, the image head on n
  cached rows), JointContrastiveLoss, backward, AdamW step -- `dense` and `packed`, on models with the same weights.  The packed route
  gathers its embeddings with ``F.embedding`` where the dense one indexes (``token_embedding.weight[ids]``), and the two differ in their
  backward; `dense_embedding` is the dense layout with the packed route's gather (``DenseEmbeddingTower``, this tool's own), so that
  `step_speedup_layout` = dense_embedding / packed is the gain of the layout alone and `step_speedup` = dense / packed is what a user
  of the trainer sees;
* `loss_dense` / `loss_packed`: the first step's loss on either route (what is compared: the same texts, another layout).

Each figure is the median of `reps` timed windows after three warm-up windows, a window being `inner` back-to-back repetitions between
two device events; the figure is per repetition, with the windows' minimum and maximum next to it (the spread).  The routes' windows
alternate, so that whatever else the machine does falls on all of them.  `*_speedup` = dense median / packed median; `rows_ratio` =
rows_dense / rows_packed.  Nothing here says which is faster in advance: the result is the file.  Prints one JSON object (also written
to --out)."""
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
WIDTH, LAYERS, VOCAB, EMBED = 768, 12, 49408, 768
# (context, query lengths, target lengths), lengths inclusive
CASES = {"ctx77_mixed": (77, (8, 40), (77, 77)), "ctx248_mixed": (248, (8, 40), (150, 248)),
         "ctx77_full": (77, (77, 77), (77, 77)), "ctx248_full": (248, (248, 248), (248, 248))}


def arch(ctx):
    """The text tower of ViT-L/14 at `ctx` positions next to a one-block vision tower: the image tower is locked and only its cached rows
    take part."""
    return ClipArch(EMBED, 32, 8, 256, 1, WIDTH, LAYERS, vocab=VOCAB, ctx=ctx)


def make_ids(n, ctx, lo_hi, g):
    lens = torch.randint(lo_hi[0], lo_hi[1] + 1, (n,), generator=g)
    ids = torch.randint(1, VOCAB - 2, (n, ctx), generator=g, dtype=torch.int32)
    ids[torch.arange(ctx)[None, :] >= lens[:, None]] = 0
    ids[:, 0] = VOCAB - 2
    ids[torch.arange(n), lens - 1] = VOCAB - 1               # the end-of-text token: the row maximum
    return ids, lens.tolist()


class DenseEmbeddingTower(tower_train.TextTower):
    """The dense tower at the batch's longest text, gathering token and positional embeddings with F.embedding as the packed route
    does: what separates the layout's share of a step from the gather's."""

    def pooled(self, ids, t=None):
        dev = self.positional_embedding.device
        ids = ids.to(dev).long()
        batch, eot = ids.shape[0], ids.argmax(dim=-1)
        pos = torch.arange(t, device=dev)
        x = (F.embedding(ids[:, :t], self.token_embedding.weight) + F.embedding(pos, self.positional_embedding)).reshape(batch * t, self.width)
        for blk in self.transformer.resblocks:
            x = self._block(x, blk, lambda qkv: self._attend(qkv, batch, t))
        return x.reshape(batch, t, self.width)[torch.arange(batch, device=dev), eot]


def timed_alternating(fns, reps, inner):
    """{name: (median, min, max)} ms per repetition; the windows of the routes alternate."""
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


def bench_case(name, n, reps, dev):
    ctx, q_lens, t_lens = CASES[name]
    g = torch.Generator().manual_seed(n + ctx)
    q_ids, ql = make_ids(n, ctx, q_lens, g)
    t_ids, tl = make_ids(n, ctx, t_lens, g)
    lens = ql + tl
    longest, rows_packed = max(lens), sum(lens)
    rows_dense = 2 * n * longest
    segments = tower_train.packed_segments(lens)
    out = {"case": name, "ctx": ctx, "pairs": n, "texts": 2 * n, "longest": longest, "rows_dense": rows_dense, "rows_packed": rows_packed,
           "rows_ratio": rows_dense / rows_packed, "segments": [list(s) for s in segments]}
    # ---- attention alone
    dense_qkv = torch.randn(rows_dense, 3 * WIDTH, generator=g).to(dev).to(torch.bfloat16).requires_grad_(True)
    dense_dout = torch.randn(rows_dense, WIDTH, generator=g).to(dev).to(torch.bfloat16)
    packed_qkv = torch.randn(rows_packed, 3 * WIDTH, generator=g).to(dev).to(torch.bfloat16).requires_grad_(True)
    packed_dout = torch.randn(rows_packed, WIDTH, generator=g).to(dev).to(torch.bfloat16)
    ends = torch.tensor(lens).cumsum(0)
    row_start = torch.cat([ends.new_zeros(1), ends]).to(torch.int32).to(dev)
    one_call = ((0, 2 * n, longest),)

    def attn_dense():
        dense_qkv.grad = None
        tower_train._OpAttention.apply(dense_qkv, 2 * n, longest, WIDTH, True).backward(dense_dout)

    def attn_packed(seg):
        packed_qkv.grad = None
        tower_train._OpAttentionPacked.apply(packed_qkv, row_start, seg, WIDTH).backward(packed_dout)

    res = timed_alternating({"dense": attn_dense, "packed": lambda: attn_packed(segments), "packed_one_call": lambda: attn_packed(one_call)},
                            reps, 4)
    for which, (med, lo, hi) in res.items():
        out[f"attn_{which}_ms"], out[f"attn_{which}_ms_min_max"] = med, [lo, hi]
    out["attn_speedup"] = res["dense"][0] / res["packed"][0]
    del dense_qkv, dense_dout, packed_qkv, packed_dout
    # ---- one whole step
    img = torch.randn(n, arch(ctx).v_width, generator=g).to(dev)
    q_dev, t_dev = q_ids.to(dev), t_ids.to(dev)
    loss_fn = losses.JointContrastiveLoss(TEMPERATURE, T2I_W, T2T_W)
    steps, keep = {}, []
    for which in ("dense", "dense_embedding", "packed"):
        torch.manual_seed(0)
        model = clip_module.build_model(arch(ctx), device=dev).float()
        tune = tower_train.LockedImageTuning(model, packed=(which == "packed"))
        if which == "dense_embedding":
            tune.tower = DenseEmbeddingTower(model)
        opt, _ = finetune.build_optimizer(tune, lr=1e-5, weight_decay=0.01, num_epochs=1)
        with torch.no_grad():
            out[f"loss_{which}"] = float(loss_fn(*tune(img, q_dev, t_dev))[0])

        def step(tune=tune, opt=opt):
            opt.zero_grad()
            loss, _ = loss_fn(*tune(img, q_dev, t_dev))
            loss.backward()
            opt.step()

        steps[which] = step
        keep.append((model, tune, opt))
    res = timed_alternating(steps, reps, 1)
    for which, (med, lo, hi) in res.items():
        out[f"step_{which}_ms"], out[f"step_{which}_ms_min_max"] = med, [lo, hi]
    out["step_speedup"] = res["dense"][0] / res["packed"][0]
    out["step_speedup_layout"] = res["dense_embedding"][0] / res["packed"][0]
    del keep, steps
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--pairs", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cases", type=str, nargs="+", default=list(CASES), choices=list(CASES))
    ap.add_argument("--out", type=str, default=os.path.join("profiles", "text_tower_packed_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_text_tower_packed: needs a GPU (a CPU run says nothing about the MI355X)")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "tower": {"width": WIDTH, "layers": LAYERS, "heads": WIDTH // 64}, "reps": args.reps,
           "cases": [bench_case(name, args.pairs, args.reps, dev) for name in args.cases]}
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
