#!/usr/bin/env python3
"""Long-CLIP text throughput (texts/s): the packed causal route against the dense route on a 248-position ViT-L/14 text tower.

The model is the text tower of LongCLIP-L (768 wide, 12 layers, 248 positions) with seeded random weights at the default precision
-- a timing does not depend on the values -- next to a one-layer vision tower that is never run (it only keeps the weight upload
short).  Three length sets, drawn with a seed; a text's length is the position of its end-of-text token + 1:

    queries   uniform in 8 .. 40       (the reference's short queries)
    targets   uniform in 150 .. 248    (its ~150-word target descriptions, cut at 248 tokens)
    full      every text at 248

Each set is encoded on the packed route (ClipEngine.encode_text's default: sum(lengths) token rows per call) and on the dense route
(`pack_text = False`: texts x 248 rows per call, what a model of this context ran on before the packed path served it) in the same
process, the two alternating.  The token ids are on the device and the lengths are passed from the host, so neither route
synchronises.  After `--warmup` untimed repetitions of both routes, every repetition is timed with a pair of device events around the
whole encode call; reported are the median texts/s per route, the spread (max - min) / median of the repetitions, and the ratio of
the medians.  One JSON line per set to stdout and to `--out`.

    python tools/bench_longclip.py --texts 4096 --reps 9 --out profiles/longclip_bench.json
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from knowledge_enhanced_multimodal_retrieval_amd import engine  # noqa: E402
from knowledge_enhanced_multimodal_retrieval_amd.config import ARCHS, ClipArch  # noqa: E402
from oracle import clip_ref  # noqa: E402

SETS = {"queries": (8, 40), "targets": (150, 248), "full": (248, 248)}


def bench_arch() -> ClipArch:
    a = ARCHS["LongCLIP-L"]
    return ClipArch(a.embed_dim, 32, 8, 256, 1, a.t_width, a.t_layers, vocab=a.vocab, ctx=a.ctx)      # the "tiny" vision tower, one layer


def draw(arch, n, lo, hi, seed):
    """(ids int32 [n, ctx], lengths int32 [n]): start-of-text, random ids, end-of-text at position length - 1, zero padding."""
    g = torch.Generator().manual_seed(seed)
    lens = torch.randint(lo, hi + 1, (n,), generator=g, dtype=torch.int32)
    ids = torch.randint(1, arch.sot, (n, arch.ctx), generator=g, dtype=torch.int32)
    pos = torch.arange(arch.ctx)[None, :]
    ids[pos >= lens[:, None]] = 0
    ids[:, 0] = arch.sot
    ids[torch.arange(n), (lens - 1).long()] = arch.eot
    return ids, lens


def timed_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--texts", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=1235)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    arch = bench_arch()
    cases = {name: draw(arch, args.texts, lo, hi, args.seed + i) for i, (name, (lo, hi)) in enumerate(SETS.items())}
    if not torch.cuda.is_available():
        raise SystemExit("no GPU visible: nothing is measured without one")
    dev = torch.device("cuda:0")
    eng = engine.ClipEngine(arch, dev)
    eng.load_state_dict(clip_ref.random_state_dict(arch.cfg_dict(), seed=0))
    lines = []
    for name, (ids, lens) in cases.items():
        ids_d = ids.to(dev)

        def run(packed):
            eng.pack_text = packed
            return eng.encode_text(ids_d, normalize=True, lens=lens)

        for _ in range(args.warmup):
            run(True), run(False)
        torch.cuda.synchronize()
        ms = {True: [], False: []}
        for _ in range(args.reps):
            for packed in (True, False):
                ms[packed].append(timed_ms(lambda: run(packed)))
        cos = torch.nn.functional.cosine_similarity(run(True).double(), run(False).double()).min().item()
        med = {k: statistics.median(v) for k, v in ms.items()}
        spread = {k: (max(v) - min(v)) / med[k] for k, v in ms.items()}
        res = {"set": name, "length_lo": SETS[name][0], "length_hi": SETS[name][1], "texts": args.texts, "ctx": arch.ctx,
               "text_tower": f"{arch.t_width} wide, {arch.t_layers} layers", "precision": eng.precision, "reps": args.reps, "warmup": args.warmup,
               "packed_token_rows": int(lens.sum()), "dense_token_rows": args.texts * arch.ctx,
               "packed_texts_per_s": args.texts / med[True] * 1e3, "dense_texts_per_s": args.texts / med[False] * 1e3,
               "packed_ms_median": med[True], "dense_ms_median": med[False], "packed_spread": spread[True], "dense_spread": spread[False],
               "packed_over_dense": med[False] / med[True], "row_ratio": args.texts * arch.ctx / int(lens.sum()),
               "min_cos_packed_vs_dense": cos, "device": torch.cuda.get_device_name(0)}
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
