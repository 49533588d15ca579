#!/usr/bin/env python3
"""The streaming attention kernel (csrc/attention_stream.hip, the fixed-length instantiation) alone at the ViT-L/14@336px shape: T = 577, width 1024 (16 heads), B =
the engine's images per call (engine.image_call_items), checked against a torch fp32 softmax(QK^T)V of the same bf16 inputs.  Every
rep is timed on its own hipEvent pair after a warm-up; prints the median us, TFLOP/s (4 T^2 64 heads B) with its share of the
2.5 PF bf16 MFMA peak, and GB/s (q | k | v read once, the output written once).  For comparison the same for the 257-token
kernel of ViT-L/14 at B = 255.

    python tools/bench_attention_long.py [--reps 50] [--batch B] [--t 577]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from knowledge_enhanced_multimodal_retrieval_amd import engine  # noqa: E402
from knowledge_enhanced_multimodal_retrieval_amd.config import ARCHS  # noqa: E402

PEAK_BF16 = 2.5e15


def ref(qkv, b, t, w):
    h = w // 64
    x = qkv.float().view(b, t, 3, h, 64)
    q, k, v = x[:, :, 0].transpose(1, 2), x[:, :, 1].transpose(1, 2), x[:, :, 2].transpose(1, 2)
    return (torch.softmax(q @ k.transpose(-1, -2), -1) @ v).transpose(1, 2).reshape(b * t, w)


def run(dev, b, t, w, reps, warmup):
    g = torch.Generator(device=dev).manual_seed(0)
    qkv = (torch.randn(b * t, 3 * w, generator=g, device=dev) * 0.5).to(torch.bfloat16)
    nchk = min(b, 4)
    err = (engine.op_attention(qkv, b, t, w, False)[: nchk * t].float() - ref(qkv[: nchk * t], nchk, t, w)).abs().max().item()
    assert err < 3e-2, err
    for _ in range(warmup):
        engine.op_attention(qkv, b, t, w, False)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for e0, e1 in ev:
        e0.record()
        engine.op_attention(qkv, b, t, w, False)
        e1.record()
    torch.cuda.synchronize()
    us = statistics.median(e0.elapsed_time(e1) * 1e3 for e0, e1 in ev)
    flops = 4.0 * t * t * 64 * (w // 64) * b
    nbytes = b * t * 3 * w * 2 + b * t * w * 2
    return dict(t=t, width=w, batch=b, median_us=round(us, 2), tflops=round(flops / us / 1e6, 1),
                peak_share=round(flops / us / 1e-6 / PEAK_BF16, 3), gbps=round(nbytes / us / 1e3, 1), max_err=err)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=0, help="0 = engine.image_call_items(ViT-L/14@336px)")
    ap.add_argument("--t", type=int, default=577)
    ap.add_argument("--no-ref257", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    b = a.batch or engine.image_call_items(ARCHS["ViT-L/14@336px"])
    print(json.dumps(dict(kernel="attention_long", **run(dev, b, a.t, 1024, a.reps, a.warmup))), flush=True)
    if not a.no_ref257:
        print(json.dumps(dict(kernel="attention 257", **run(dev, 255, 257, 1024, a.reps, a.warmup))), flush=True)


if __name__ == "__main__":
    main()
