"""ViT-H-14 (OpenCLIP / LAION: vision 1280 wide = 16 heads of 80, 32 layers, 257 tokens; text 1024 wide, 24 layers; joint dim 1024;
exact GELU) on seeded random weights: encoder throughput at the default precision and at "fp32x3", and the head-dim-80 attention
kernel alone at B = 255 next to the head-dim-64 kernel at the same batch, head count and T.

    python tools/bench_vit_h14.py [--steps attention,default,fp32x3] [--repeats 5] [--limit 900] [--out FILE]

Every GPU step runs in a child process of its own under its own time limit; the first step that fails, is killed by a signal or runs
into its limit ends the run (nothing more is started on the GPU).  One JSON line per step on stdout (and appended to --out); every
figure comes with the min and max over the repeats.  bench.py (the flagship ViT-L/14 workload) is not involved."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NAME = "ViT-H-14"
STEPS = ("attention", "default", "fp32x3")


def _spread(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1], "n": len(xs)}


def step_attention(repeats):
    """Per-launch time (device events around 100 launches) of the tile kernels at B = 255, 16 heads, T = 257: head dim 80 with eight
    and with four waves per workgroup (debug switch attn80_waves), head dim 64 (width 1024); the variants alternate inside every
    repeat.  The head-dim-80 outputs are first checked against torch's fp32 softmax(QK^T)V of the same bf16 inputs."""
    import torch
    from knowledge_enhanced_multimodal_retrieval_amd import debug, engine
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    b, t, heads = 255, 257, 16
    qkv = {hd: (torch.randn(b * t, 3 * heads * hd, generator=g, device=dev) * 0.5).to(torch.bfloat16) for hd in (80, 64)}
    x = qkv[80][: 4 * t].float().view(4, t, 3, heads, 80)
    q, k, v = (x[:, :, j].transpose(1, 2) for j in range(3))
    want = (torch.softmax(q @ k.transpose(-1, -2), -1) @ v).transpose(1, 2).reshape(4 * t, heads * 80)
    variants = (("hd80_8waves", 80, 8), ("hd80_4waves", 80, 4), ("hd64", 64, 0))
    for name, hd, waves in variants:
        with debug.override(attn80_waves=waves):
            got = engine.op_attention(qkv[hd], b, t, heads * hd, False, head_dim=hd)
            if hd == 80:
                err = (got[: 4 * t].float() - want).abs().max().item()
                assert err < 2e-2, (name, err)
            for _ in range(50):
                engine.op_attention(qkv[hd], b, t, heads * hd, False, head_dim=hd)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    us = {name: [] for name, _, _ in variants}
    for _ in range(repeats):
        for name, hd, waves in variants:
            with debug.override(attn80_waves=waves):
                e0.record()
                for _ in range(100):
                    engine.op_attention(qkv[hd], b, t, heads * hd, False, head_dim=hd)
                e1.record()
                torch.cuda.synchronize()
            us[name].append(e0.elapsed_time(e1) * 10.0)
    out = {"step": "attention", "batch": b, "tokens": t, "heads": heads, "launches_per_repeat": 100}
    for name, hd, _ in variants:
        out[name + "_us_per_launch"] = _spread(us[name])
        out[name + "_useful_tflops"] = 4.0 * t * t * hd * b * heads / out[name + "_us_per_launch"]["median"] / 1e6
    return out


def step_encode(precision, repeats):
    """Images/s and texts/s of the packed model: `repeats` timed rounds of one full call each (255 images; 851 texts of the synthetic
    length distribution through the packed text route), after two warm-up rounds; host clock around work that ends in a synchronise."""
    import torch
    from knowledge_enhanced_multimodal_retrieval_amd import engine
    from knowledge_enhanced_multimodal_retrieval_amd.config import ARCHS
    from oracle import clip_ref
    dev = torch.device("cuda:0")
    arch = ARCHS[NAME]
    t0 = time.time()
    sd = clip_ref.random_state_dict(arch.cfg_dict(), seed=0)
    eng = engine.ClipEngine(arch, dev, precision=precision, activation="gelu")
    eng.load_state_dict(sd)
    del sd
    torch.cuda.synchronize()
    load_s = time.time() - t0
    n_img, n_txt = eng.image_batch, engine.MAX_TEXT_BATCH
    px = torch.randn(n_img, 3, arch.image_size, arch.image_size, generator=torch.Generator().manual_seed(1)).to(dev)
    ids = clip_ref.synthetic_ids(arch.cfg_dict(), n_txt)
    lens = engine.text_lengths(ids)
    ids_dev = ids.to(dev)
    rates = {"images_per_s": [], "texts_per_s": []}
    for rnd in range(repeats + 2):
        for key, n, fn in (("images_per_s", n_img, lambda: eng.encode_image(px, normalize=True)),
                           ("texts_per_s", n_txt, lambda: eng.encode_text(ids_dev, normalize=True, lens=lens))):
            torch.cuda.synchronize()
            t1 = time.time()
            out = fn()
            torch.cuda.synchronize()
            dt = time.time() - t1
            assert bool(torch.isfinite(out).all())
            if rnd >= 2:
                rates[key].append(n / dt)
    return {"step": precision, "model": NAME, "precision": precision, "activation": "gelu", "images_per_call": n_img, "texts_per_call": n_txt,
            "load_and_pack_s": load_s, "images_per_s": _spread(rates["images_per_s"]), "texts_per_s": _spread(rates["texts_per_s"]),
            "image_tflops": arch.image_flops() * _spread(rates["images_per_s"])["median"] / 1e12}


def run_step(step, repeats):
    import torch
    from knowledge_enhanced_multimodal_retrieval_amd import _lib
    assert torch.cuda.is_available(), "bench_vit_h14.py needs a GPU: nothing here is measured on a CPU"
    if step == "attention":
        return step_attention(repeats)
    return step_encode(_lib.DEFAULT_PRECISION if step == "default" else "fp32x3", repeats)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", default=",".join(STEPS))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--limit", type=int, default=900, help="time limit of each GPU step, seconds")
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
