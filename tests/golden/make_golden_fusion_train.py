#!/usr/bin/env python3
"""Generate tests/golden/fusion_train_golden.npz (the sibling of make_golden_infonce.py for the fusion-head objective).

Runs ONLY in the build container, on the CPU: it imports the reference's own head classes from /root/reference
(``src.clip.model.fusion_model``: LinearFusionHead, GatedFusionHead, SimpleGatedFusion, SimpleGatedFusionWithBias), loads seeded
parameters into them (the state dicts of tests/fusion_train_cases.make_model: the keys must match), puts them in eval mode and
differentiates the symmetric cross entropy of their scores at temperature 0.07 with autograd in fp64 -- n = 48 items, D = 64.  Stored:
the three inputs, and per head its parameters, the three losses and the gradient of `loss` with respect to every parameter, all fp64.
tests/test_fusion_train_host.py holds tests/pairhead_ref.py to them at 1e-10; tests/test_fusion_train_gpu.py holds the kernels'
autograd path to them within the budget.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_fusion_train.py
"""
import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import fusion_train_cases as cases  # noqa: E402

N, D, TEMPERATURE, SEED = 48, 64, 0.07, 11
CLASSES = {"linear": "LinearFusionHead", "gated": "GatedFusionHead", "simple_gated": "SimpleGatedFusion",
           "simple_gated_with_bias": "SimpleGatedFusionWithBias"}


def ref_heads():
    """The reference's fusion_model module, without shadowing this repository's own ``src`` package."""
    saved = {k: v for k, v in sys.modules.items() if k == "src" or k.startswith("src.")}
    for k in saved:
        del sys.modules[k]
    sys.path.insert(0, REF)
    try:
        mod = importlib.import_module("src.clip.model.fusion_model")
        assert mod.__file__.startswith(REF), mod.__file__
    finally:
        sys.path.remove(REF)
        for k in [k for k in sys.modules if k == "src" or k.startswith("src.")]:
            del sys.modules[k]
        sys.modules.update(saved)
    return mod


def main():
    mod = ref_heads()
    q, img, tgt = cases.triplet(N, D, SEED, dtype=torch.float64)
    out = {"temperature": np.float64(TEMPERATURE), "query": q.numpy(), "image": img.numpy(), "target": tgt.numpy()}
    for ft, cls in CLASSES.items():
        state = {k: v.double() for k, v in cases.make_model(ft, D, SEED).fusion_head.state_dict().items()}
        head = getattr(mod, cls)(128) if ft == "linear" else getattr(mod, cls)(D)
        head = head.double()
        head.load_state_dict(state)                   # strict: the key names are the reference's
        head.eval()
        scores = head(q @ img.T, q @ tgt.T) if ft == "linear" else head(q, img, tgt)
        loss, l_q2g, l_g2q = cases.symmetric_cross_entropy(scores, TEMPERATURE)
        loss.backward()
        out[f"{ft}_loss"], out[f"{ft}_loss_q2g"], out[f"{ft}_loss_g2q"] = (np.float64(float(x.detach())) for x in (loss, l_q2g, l_g2q))
        for k, p in head.named_parameters():
            out[f"{ft}_param_{k}"] = p.detach().numpy()
            out[f"{ft}_grad_{k}"] = p.grad.numpy()
    path = os.path.join(HERE, "fusion_train_golden.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", {ft: float(out[f"{ft}_loss"]) for ft in CLASSES})


if __name__ == "__main__":
    main()
