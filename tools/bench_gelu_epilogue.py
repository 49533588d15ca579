#!/usr/bin/env python3
"""The fc1 GEMM of ViT-L/14 (65 535 x 4096 x 1024) with the GELU epilogue against the QuickGELU epilogue, bf16 and fp8 operands.

    python tools/bench_gelu_epilogue.py [--reps 15] [--out profiles/gelu_epilogue.json]

One process, one device.  Per (operands, epilogue): at least 100 ms of warm-up launches, then `reps` repetitions, each ONE launch
between two hipEvents; the figure is the median.  The two epilogues of an operand type are interleaved repetition by
repetition, so that clock drift hits both.  Then the ViT-L/14 image tower end to end (images/s) with either activation, on one
engine whose option is flipped call by call.  The yardstick is the QuickGELU epilogue of the same run: the ratio, never an
absolute time.  Prints one JSON object (also written to --out)."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from knowledge_enhanced_multimodal_retrieval_amd import _lib, engine  # noqa: E402

M, N, K = 65535, 4096, 1024


def encode_items_per_s(dev, reps):
    """ViT-L/14 images/s of one engine (default precision, its own images-per-call) with the option flipped call by call."""
    from knowledge_enhanced_multimodal_retrieval_amd.clip_module import CLIP
    from knowledge_enhanced_multimodal_retrieval_amd.config import ARCHS
    arch = ARCHS["ViT-L/14"]
    torch.manual_seed(0)
    eng = engine.ClipEngine(arch, dev)
    eng.load_state_dict({k: v for k, v in CLIP(arch).state_dict().items() if k != "logit_scale"})
    px = torch.randn(eng.image_batch, 3, arch.image_size, arch.image_size, device=dev)
    times = {"quick_gelu": [], "gelu": []}
    for it in range(3 + reps):
        for act in times:
            eng.set_activation(act)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            eng.encode_image(px)
            e1.record()
            torch.cuda.synchronize()
            if it >= 3:
                times[act].append(e0.elapsed_time(e1))
    med = {a: statistics.median(t) for a, t in times.items()}
    return {"precision": eng.precision, "images_per_call": eng.image_batch, "median_ms": med,
            "images_per_s": {a: eng.image_batch / v * 1e3 for a, v in med.items()},
            "gelu_over_quick_gelu": med["gelu"] / med["quick_gelu"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    reps = max(10, args.reps)
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    ma = (M + 255) // 256 * 256
    a = torch.randn(ma, K, generator=g, device=dev)
    w = torch.randn(N, K, generator=g, device=dev) * K ** -0.5
    bias = torch.randn(N, generator=g, device=dev)
    a16, w16 = a.to(torch.bfloat16), w.to(torch.bfloat16)
    a8, w8 = a.to(torch.float8_e4m3fn), (w * 16).to(torch.float8_e4m3fn)
    ws = torch.full((N,), 1 / 16, device=dev)
    c = torch.zeros(ma, N, dtype=torch.bfloat16, device=dev)
    epis = {"quick_gelu": _lib.EPI_BIAS_QGELU_BF16, "gelu": _lib.EPI_BIAS_GELU_BF16}
    runs = {
        "bf16": lambda epi: engine.op_gemm(a16, w16, bias, M, epi, c=c),
        "fp8": lambda epi: engine.op_gemm_fp8(a8, w8, ws, bias, M, epi),
    }
    result = {"shape": [M, N, K], "reps": reps, "device": torch.cuda.get_device_name(dev)}
    for operands, fn in runs.items():
        for epi in epis.values():                          # >= 100 ms of launches per epilogue before anything is timed
            t0 = time.perf_counter()
            while time.perf_counter() - t0 < 0.1:
                for _ in range(20):
                    fn(epi)
                torch.cuda.synchronize()
        times = {name: [] for name in epis}
        for _ in range(reps):
            for name, epi in epis.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn(epi)
                e1.record()
                torch.cuda.synchronize()
                times[name].append(e0.elapsed_time(e1) * 1e3)
        med = {name: statistics.median(t) for name, t in times.items()}
        result[operands] = {"median_us": med, "min_us": {n: min(t) for n, t in times.items()},
                            "tflops": {n: 2.0 * M * N * K / v / 1e6 for n, v in med.items()},
                            "gelu_over_quick_gelu": med["gelu"] / med["quick_gelu"]}
    result["encode_ViT-L-14"] = encode_items_per_s(dev, reps)
    line = json.dumps(result, sort_keys=True)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
