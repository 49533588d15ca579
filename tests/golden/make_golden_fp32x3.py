#!/usr/bin/env python3
"""Generate tests/golden/fp32x3_heavy_ViT-B-32.npz: what this project's CPU oracle (oracle/clip_ref.py) gives on ViT-B/32 with
LayerNorm gains in the regime bf16 operands cannot hold, so that the GPU test of the "fp32x3" precision does not have to run
ViT-B/32 on the CPU (tests/test_fp32x3_gpu.py).  The sibling of make_golden_gelu.py; runs on the CPU only.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_fp32x3.py

Weights: ``add_outliers(random_state_dict(arch, 0), arch, 0, gain_lo=30, gain_hi=100)`` -- uncompensated gains of 30 .. 100.
Inputs: 4 images ``randn`` with seed 1234, 8 texts ``synthetic_ids(arch, 8)``.  Stored: the fp32 oracle's embeddings, and per
embedding the 1 - cos against them of two CPU emulations of the operand rounding (``clip_ref._block(bf16_operands=True)``):

* ``bf16``: ``clip_ref._bf16`` as it stands, one bf16 rounding of every GEMM / attention operand and stored intermediate;
* ``split2``: ``clip_ref._bf16`` replaced by :func:`split2`, the two-term rounding ``hi + rne_bf16(t - hi)`` -- what the operand pairs
  of KEMR_PREC_FP32X3 keep of a value (the emulation leaves out the dropped lo.lo product and rounds values the mode keeps in fp32).

The GPU test rebuilds the weights and inputs from the seeds and checks them by their abs-sums.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.dont_write_bytecode = True
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

WEIGHT_SEED = 0
PIXEL_SEED = 1234
N_IMAGES, N_TEXTS = 4, 8
HEAVY_GAINS = (30.0, 100.0)
NAME = "ViT-B/32"


def split2(t: torch.Tensor) -> torch.Tensor:
    """The value an operand pair (hi, lo) of KEMR_PREC_FP32X3 carries: hi = rne_bf16(t), lo = rne_bf16(t - hi), hi + lo in fp32."""
    hi = t.to(torch.bfloat16).to(torch.float32)
    return hi + (t - hi).to(torch.bfloat16).to(torch.float32)


def heavy_state_dict(arch, gains=HEAVY_GAINS, seed=WEIGHT_SEED):
    from oracle import clip_ref
    return clip_ref.add_outliers(clip_ref.random_state_dict(arch, seed), arch, seed, gain_lo=gains[0], gain_hi=gains[1])


def fixture_inputs(arch, n_images=N_IMAGES, n_texts=N_TEXTS):
    from oracle import clip_ref
    g = torch.Generator().manual_seed(PIXEL_SEED)
    return torch.randn(n_images, 3, arch["image_size"], arch["image_size"], generator=g), clip_ref.synthetic_ids(arch, n_texts)


def one_minus_cos(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return 1.0 - torch.nn.functional.cosine_similarity(a, b, dim=-1)


def oracle_and_emulations(sd, arch, px, ids, setattr_fn):
    """(fp32 oracle image / text embeddings, per-embedding 1 - cos of the bf16-operand emulation, of the split2 emulation).
    setattr_fn(module, name, value) swaps ``clip_ref._bf16`` (pytest's monkeypatch.setattr in the tests, setattr here)."""
    from oracle import clip_ref
    oi, ot = clip_ref.encode_image(sd, arch, px), clip_ref.encode_text(sd, arch, ids)
    bi, bt = clip_ref.encode_image(sd, arch, px, bf16_operands=True), clip_ref.encode_text(sd, arch, ids, bf16_operands=True)
    keep = clip_ref._bf16
    setattr_fn(clip_ref, "_bf16", split2)
    try:
        si, st = clip_ref.encode_image(sd, arch, px, bf16_operands=True), clip_ref.encode_text(sd, arch, ids, bf16_operands=True)
    finally:
        setattr_fn(clip_ref, "_bf16", keep)
    return (oi, ot), (one_minus_cos(bi, oi), one_minus_cos(bt, ot)), (one_minus_cos(si, oi), one_minus_cos(st, ot))


def fixture_path():
    return os.path.join(HERE, "fp32x3_heavy_%s.npz" % NAME.replace("/", "-"))


def main():
    from oracle import clip_ref
    arch = clip_ref.ARCHS[NAME]
    sd = heavy_state_dict(arch)
    px, ids = fixture_inputs(arch)
    (oi, ot), (bi, bt), (si, st) = oracle_and_emulations(sd, arch, px, ids, setattr)
    meta = {"weight_seed": WEIGHT_SEED, "pixel_seed": PIXEL_SEED, "gains": list(HEAVY_GAINS), "n_images": N_IMAGES, "n_texts": N_TEXTS,
            "pixel_abs_sum": float(px.double().abs().sum()),
            "weight_abs_sums": {k: float(v.double().abs().sum()) for k, v in sd.items()}}
    np.savez_compressed(fixture_path(), image_features=oi.numpy(), text_features=ot.numpy(), ids=ids.numpy(),
                        bf16_image=bi.numpy(), bf16_text=bt.numpy(), split2_image=si.numpy(), split2_text=st.numpy(),
                        meta_json=np.frombuffer(json.dumps(meta, sort_keys=True).encode(), dtype=np.uint8))
    print(NAME, "worst 1 - cos image / text: bf16 operands %.2e / %.2e, two-term operands %.2e / %.2e | bytes %d" % (
        float(bi.max()), float(bt.max()), float(si.max()), float(st.max()), os.path.getsize(fixture_path())), flush=True)


if __name__ == "__main__":
    main()
