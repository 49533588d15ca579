"""ViT-B-16-SigLIP (224 px: 196 vision tokens, 768 wide, 12 layers, attention-pooling head; text 768 wide, 12 layers, 64 unmasked
positions) next to ViT-B/16 (197 tokens; text 512 wide, 77 causal positions) on seeded random weights at the default precision:
time of one image call (255 images) and of one text call (851 texts) each.

    python tools/bench_siglip.py [--steps ViT-B/16,ViT-B-16-SigLIP] [--repeats 7] [--limit 600] [--out FILE]

Every GPU step runs in a child process of its own under its own time limit; the first step that fails, is killed by a signal or runs
into its limit ends the run (nothing more is started on the GPU).  One JSON line per step on stdout (and appended to --out); every
figure comes with the min and max over the repeats.  The two models differ in more than the family (text width, context, vocabulary):
the figures say what a call costs, not what the family costs.  bench.py (the flagship ViT-L/14 workload) is not involved."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = ("ViT-B/16", "ViT-B-16-SigLIP")


def _spread(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1], "n": len(xs)}


def run_step(name, repeats):
    import torch
    from knowledge_enhanced_multimodal_retrieval_amd import _lib, engine
    from knowledge_enhanced_multimodal_retrieval_amd.config import ARCHS
    assert torch.cuda.is_available(), "bench_siglip.py needs a GPU: nothing here is measured on a CPU"
    dev = torch.device("cuda:0")
    arch = ARCHS[name]
    if arch.family == "siglip":
        # the module's own seeded initialisation; texts as the tokenizer leaves them: ids >= 2, the end-of-sequence id 1, pads of id 1
        from knowledge_enhanced_multimodal_retrieval_amd.clip_module import SigLIP
        torch.manual_seed(0)
        sd = {k: v.detach() for k, v in SigLIP(arch, name).state_dict().items() if k not in ("logit_scale", "logit_bias")}
        g = torch.Generator().manual_seed(2)
        ids = torch.randint(2, arch.vocab, (engine.MAX_TEXT_BATCH, arch.ctx), generator=g, dtype=torch.int32)
        keep = torch.arange(arch.ctx)[None, :] < torch.randint(4, arch.ctx, (engine.MAX_TEXT_BATCH, 1), generator=g)
        ids = torch.where(keep, ids, torch.ones_like(ids))
        lens = None
    else:
        from oracle import clip_ref
        sd = clip_ref.random_state_dict(arch.cfg_dict(), seed=0)
        ids = clip_ref.synthetic_ids(arch.cfg_dict(), engine.MAX_TEXT_BATCH)
        lens = engine.text_lengths(ids)
    eng = engine.ClipEngine(arch, dev, precision=_lib.DEFAULT_PRECISION)
    eng.load_state_dict(sd)
    del sd
    n_img, n_txt = eng.image_batch, engine.MAX_TEXT_BATCH
    px = torch.randn(n_img, 3, arch.image_size, arch.image_size, generator=torch.Generator().manual_seed(1)).to(dev)
    ids_dev = ids.to(dev)
    ms = {"image_call_ms": [], "text_call_ms": []}
    for rnd in range(repeats + 2):
        for key, fn in (("image_call_ms", lambda: eng.encode_image(px, normalize=True)),
                        ("text_call_ms", lambda: eng.encode_text(ids_dev, normalize=True, lens=lens))):
            torch.cuda.synchronize()
            t1 = time.time()
            out = fn()
            torch.cuda.synchronize()
            dt = time.time() - t1
            assert bool(torch.isfinite(out).all())
            if rnd >= 2:
                ms[key].append(dt * 1e3)
    img, txt = _spread(ms["image_call_ms"]), _spread(ms["text_call_ms"])
    return {"step": name, "model": name, "family": arch.family, "precision": _lib.DEFAULT_PRECISION, "images_per_call": n_img,
            "texts_per_call": n_txt, "vision_tokens": arch.v_tokens, "text_positions": arch.ctx, "image_call_ms": img, "text_call_ms": txt,
            "images_per_s": n_img / img["median"] * 1e3, "texts_per_s": n_txt / txt["median"] * 1e3,
            "image_tflops": arch.image_flops() * n_img / img["median"] / 1e9}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", default=",".join(STEPS))
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--limit", type=int, default=600, help="time limit of each GPU step, seconds")
    ap.add_argument("--out", default="")
    ap.add_argument("--child", default="", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        print("RESULT " + json.dumps(run_step(args.child, args.repeats)), flush=True)
        return 0
    steps = [s for s in args.steps.split(",") if s]
    bad = [s for s in steps if s not in STEPS]
    if bad:
        ap.error(f"unknown steps {bad}; known: {list(STEPS)}")
    for step in steps:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", step, "--repeats", str(args.repeats)]
        try:
            res = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
        except subprocess.TimeoutExpired:
            print(json.dumps({"step": step, "error": f"time limit of {args.limit} s"}), flush=True)
            return 1                                   # nothing more is started on the GPU
        line = next((ln[7:] for ln in res.stdout.splitlines() if ln.startswith("RESULT ")), None)
        if res.returncode != 0 or line is None:
            print(json.dumps({"step": step, "error": f"exit status {res.returncode}", "stderr": res.stderr[-2000:]}), flush=True)
            return 1
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
