#!/usr/bin/env python3
"""Sentence-encoder throughput (texts/s) at the GTE-large and E5-base shapes, next to transformers.BertModel on the same device.

Lengths are drawn as in SURVEY.md section 8(d) scaled from 77 to 512 positions: L ~ U{53 .. 505}, seed 1235; ids uniform, [CLS] first,
[SEP] last; seeded random weights (no real checkpoint is needed for a timing: the work does not depend on the values).  The engine
gets the texts sorted by length (as SentenceTransformer.encode sorts them) and packs every call; BertModel gets THE SAME sorted
batches of `--batch` texts, each padded to its longest text with the attention mask -- what sentence-transformers feeds it -- with fp32
and with bf16 weights and activations (eager and, where the installed transformers offers it, SDPA attention).

Every figure is a host clock around whole passes over all texts that end in a device synchronise, after a warm-up pass of the same
shapes; `--profile` adds the engine's per-kernel-class split from device events, taken in passes of its own.  One JSON line per
model goes to stdout and, with `--out`, to that file.

    python tools/bench_sentence.py --texts 2048 --batch 32 --out profiles/sentence_bench.json

`--mpnet` measures the all-mpnet-base-v2 shape instead (model family 3: the relative position bias in the packed attention kernel):
the same texts -- E5's length distribution, sorted batches -- at max_seq_length 512 and 384 (sentence-transformers' setting for this
model: longer texts are cut to 384 tokens), and per setting three figures: the engine's texts/s, its ratio to the E5-base-v2 shape
measured in the same run on the same lengths (same width and depth: the cost of the bias), and its ratio to transformers.MPNetModel in
bf16 on the same device and batches.  One JSON line per setting.

    python tools/bench_sentence.py --mpnet --texts 2048 --batch 32 --out profiles/mpnet_bench.json
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))

import torch  # noqa: E402

from knowledge_enhanced_multimodal_retrieval_amd import _lib, engine  # noqa: E402
from knowledge_enhanced_multimodal_retrieval_amd.config import BERT_ARCHS  # noqa: E402

CLASSES = ("gemm", "layernorm", "attention", "embed_tail", "sim")


def draw_lengths(n, ctx=512, seed=1235):
    lo, hi = round(8 * ctx / 77), round(76 * ctx / 77)
    return torch.randint(lo, hi + 1, (n,), generator=torch.Generator().manual_seed(seed)).sort(descending=True).values


def timed(fn, passes):
    fn()                                            # warm-up: every shape of the timed window
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(passes):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / passes


def hf_pass(model, ids, lens, host_lens, batch):
    for s in range(0, ids.shape[0], batch):
        l = lens[s:s + batch]
        p = int(host_lens[s])                       # sorted longest first; the tokenizer's side knows the lengths: no device sync
        mask = (torch.arange(p, device=ids.device)[None, :] < l[:, None]).long()
        h = model(input_ids=ids[s:s + batch, :p], attention_mask=mask).last_hidden_state
        m = mask[..., None].to(h.dtype)
        torch.nn.functional.normalize((h * m).sum(1) / m.sum(1), dim=-1)


def engine_texts_per_s(arch, sd, ids, lens, passes, dev):
    eng = engine.BertEngine(arch, dev)
    eng.load_state_dict(sd)
    ids_d = ids.to(dev)
    t = timed(lambda: eng.encode_ids(ids_d, lens, normalize=True), passes)
    L = _lib.lib()                                          # the per-kernel-class split from device events, in a pass of its own
    _lib.check(L.kemr_profile_begin(1 << 16), "profile_begin")
    eng.encode_ids(ids_d, lens, normalize=True)
    ms, n = (C.c_double * 5)(), (C.c_int64 * 5)()
    _lib.check(L.kemr_profile_end(ms, n, 5), "profile_end")
    prof = {c: round(ms[i], 3) for i, c in enumerate(CLASSES) if n[i]}
    del eng
    return ids.shape[0] / t, prof


def mpnet_bench(args, dev):
    """all-mpnet-base-v2 next to E5-base-v2 on the same lengths, and next to transformers.MPNetModel (bf16, fp32 for reference)."""
    import dataclasses

    import bert_ref as B
    import mpnet_ref as M
    from transformers import MPNetModel
    lines = []
    drawn = draw_lengths(args.texts, 512)
    for max_len in (512, 384):
        lens = drawn.clamp(max=max_len)                     # the same texts, cut at max_seq_length (still sorted longest first)
        rows = int(lens.sum())
        mp = dataclasses.replace(BERT_ARCHS["all-mpnet-base-v2"], ctx=max_len, positions=0 if max_len == 512 else 512)
        e5 = dataclasses.replace(BERT_ARCHS["e5-base-v2"], ctx=max_len, positions=0 if max_len == 512 else 512)
        ids_mp, _ = M.random_ids(lens.tolist(), mp, seed=3)
        ids_e5, _ = B.random_ids(lens.tolist(), e5, seed=3)
        mp_tps, mp_prof = engine_texts_per_s(mp, M.random_state_dict(mp, seed=0), ids_mp, lens, args.passes, dev)
        e5_tps, e5_prof = engine_texts_per_s(e5, B.random_state_dict(e5, seed=0), ids_e5, lens, args.passes, dev)
        res = {"model": "all-mpnet-base-v2", "max_seq_length": max_len, "texts": args.texts, "token_rows": rows, "mean_length": rows / args.texts,
               "batch": args.batch, "precision": _lib.DEFAULT_PRECISION, "engine_texts_per_s": mp_tps, "e5_base_engine_texts_per_s": e5_tps,
               "engine_over_e5_base": mp_tps / e5_tps, "engine_ms_per_class": mp_prof, "e5_base_engine_ms_per_class": e5_prof,
               "device": torch.cuda.get_device_name(0)}
        ids_d, lens_d = ids_mp.to(dev), lens.to(dev)
        for dt, tag in ((torch.bfloat16, "bf16"), (torch.float32, "fp32")):
            cfg = M.mpnet_config(mp, positions=512)
            cfg._attn_implementation = "eager"              # the only attention MPNetModel has
            model = MPNetModel(cfg, add_pooling_layer=False).eval().to(device=dev, dtype=dt)
            with torch.no_grad():
                t = timed(lambda: hf_pass(model, ids_d, lens_d, lens.tolist(), args.batch), args.passes)
            res[f"torch_eager_{tag}_texts_per_s"] = args.texts / t
            del model
        res["engine_over_torch_bf16"] = res["engine_texts_per_s"] / res["torch_eager_bf16_texts_per_s"]
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", nargs="+", default=["gte-large", "e5-base-v2"], choices=sorted(k for k, a in BERT_ARCHS.items() if not a.relative_bias))
    ap.add_argument("--texts", type=int, default=2048)
    ap.add_argument("--batch", type=int, default=32, help="texts per BertModel call (SentenceTransformer.encode's batch_size)")
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--out", default="")
    ap.add_argument("--mpnet", action="store_true", help="the all-mpnet-base-v2 shape at max_seq_length 512 and 384, next to E5-base and MPNetModel")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU visible: nothing is measured without one")
    if args.mpnet:
        lines = mpnet_bench(args, torch.device("cuda:0"))
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        return
    import bert_ref as B
    from transformers import BertModel
    dev = torch.device("cuda:0")
    lines = []
    for name in args.models:
        arch = BERT_ARCHS[name]
        sd = B.random_state_dict(arch, seed=0)
        lens = draw_lengths(args.texts, arch.ctx)
        ids, _ = B.random_ids(lens.tolist(), arch, seed=3)
        rows = int(lens.sum())
        flops = sum(arch.text_flops(int(n)) for n in lens.tolist())
        eng = engine.BertEngine(arch, dev)
        eng.load_state_dict(sd)
        ids_d = ids.to(dev)
        t_eng = timed(lambda: eng.encode_ids(ids_d, lens, normalize=True), args.passes)
        res = {"model": name, "texts": args.texts, "token_rows": rows, "mean_length": rows / args.texts, "batch": args.batch,
               "precision": eng.precision, "engine_texts_per_s": args.texts / t_eng, "engine_tflops": flops / t_eng / 1e12,
               "device": torch.cuda.get_device_name(0)}
        if args.profile:
            L = _lib.lib()
            _lib.check(L.kemr_profile_begin(1 << 16), "profile_begin")
            eng.encode_ids(ids_d, lens, normalize=True)
            ms, n = (C.c_double * 5)(), (C.c_int64 * 5)()
            _lib.check(L.kemr_profile_end(ms, n, 5), "profile_end")
            res["engine_ms_per_class"] = {c: round(ms[i], 3) for i, c in enumerate(CLASSES) if n[i]}
        del eng
        lens_d = lens.to(dev)
        for impl in ("eager", "sdpa"):
            for dt, tag in ((torch.float32, "fp32"), (torch.bfloat16, "bf16")):
                try:
                    cfg = B.bert_config(arch)
                    cfg._attn_implementation = impl
                    model = BertModel(cfg, add_pooling_layer=False).eval().to(device=dev, dtype=dt)      # weights in the compute type
                except Exception as e:          # noqa: BLE001 - an attention implementation this transformers does not offer for BERT
                    res[f"torch_{impl}_{tag}"] = f"not available ({type(e).__name__})"
                    continue
                with torch.no_grad():
                    t = timed(lambda: hf_pass(model, ids_d, lens_d, lens.tolist(), args.batch), args.passes)
                res[f"torch_{impl}_{tag}_texts_per_s"] = args.texts / t
                del model
        best_bf16 = max(v for k, v in res.items() if k.endswith("bf16_texts_per_s"))
        res["engine_over_best_torch_bf16"] = res["engine_texts_per_s"] / best_bf16
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
