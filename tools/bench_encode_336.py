#!/usr/bin/env python3
"""ViT-L/14@336px vision-tower throughput (random weights, inputs resident in HBM) by images per encoder call; the engine's own
call size (engine.image_call_items) is marked.  Same pattern as tools/bench_encode_batch.py, one JSON line per size."""
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from knowledge_enhanced_multimodal_retrieval_amd import engine  # noqa: E402
from knowledge_enhanced_multimodal_retrieval_amd.config import ARCHS  # noqa: E402
from oracle import clip_ref  # noqa: E402

NAME = "ViT-L/14@336px"
dev = torch.device("cuda:0")
arch = ARCHS[NAME]
eng = engine.ClipEngine(arch, dev)
eng.load_state_dict(clip_ref.random_state_dict(dict(clip_ref.ARCHS["ViT-L/14"], image_size=336), seed=0))
px = torch.randn(2 * eng.image_batch, 3, 336, 336, device=dev)
for b in sorted({32, 64, eng.image_batch, 2 * eng.image_batch}):
    reps = max(3, 680 // b)
    for _ in range(2):
        eng.encode_image(px[:b], normalize=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        eng.encode_image(px[:b], normalize=True)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(json.dumps(dict(model=NAME, images_per_call=b, engine_call_size=eng.image_batch, reps=reps,
                          images_per_s=round(b * reps / dt, 1), tflops=round(b * reps * arch.image_flops() / dt / 1e12, 1))), flush=True)
