#!/usr/bin/env python3
"""Generate tests/golden/infonce.npz (the sibling of make_golden.py for the contrastive loss).

Runs ONLY in the build container, on the CPU: it imports the reference's own ``src.clip.train.losses`` from /root/reference and runs
its ``JointContrastiveLoss`` with autograd on fp64 inputs -- n = 48 items, D = 64, weights 0.7 / 0.3 (the recipe of the reference's
``scripts/fine-tuning/train.sh``), L2-normalised seeded features, at temperature 0.07 and at 0.01.  Stored per case: the three inputs,
the three losses and the three gradients, all fp64.  tests/test_infonce_host.py holds tests/infonce_ref.py to them at fp64 rounding;
tests/test_infonce_gpu.py holds the kernels' autograd path to them within the budget.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_infonce.py
"""
import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.dont_write_bytecode = True

N, D = 48, 64
T2I_WEIGHT, T2T_WEIGHT = 0.7, 0.3
CASES = (("t07", 0.07, 0), ("t01", 0.01, 1))          # (name, temperature, seed)


def ref_losses():
    """The reference's loss module, without shadowing this repository's own ``src`` package."""
    saved = {k: v for k, v in sys.modules.items() if k == "src" or k.startswith("src.")}
    for k in saved:
        del sys.modules[k]
    sys.path.insert(0, REF)
    try:
        mod = importlib.import_module("src.clip.train.losses")
        assert mod.__file__.startswith(REF), mod.__file__
    finally:
        sys.path.remove(REF)
        for k in [k for k in sys.modules if k == "src" or k.startswith("src.")]:
            del sys.modules[k]
        sys.modules.update(saved)
    return mod


def features(seed):
    """Three related sets of unit rows: image and query are noisy copies of the target, so the diagonal carries signal
    without the loss vanishing at either temperature."""
    g = torch.Generator().manual_seed(seed)
    target = torch.randn(N, D, generator=g, dtype=torch.float64)
    image = target + 3.0 * torch.randn(N, D, generator=g, dtype=torch.float64)
    query = target + 2.5 * torch.randn(N, D, generator=g, dtype=torch.float64)
    return [x / x.norm(dim=1, keepdim=True) for x in (image, query, target)]


def main():
    losses = ref_losses()
    out = {"t2i_weight": np.float64(T2I_WEIGHT), "t2t_weight": np.float64(T2T_WEIGHT)}
    for name, temperature, seed in CASES:
        image, query, target = [x.requires_grad_(True) for x in features(seed)]
        crit = losses.JointContrastiveLoss(temperature=temperature, t2i_weight=T2I_WEIGHT, t2t_weight=T2T_WEIGHT)
        total, _ = crit(image, query, target)
        l_t2i, _ = crit.infonce(target, image)
        l_t2t, _ = crit.infonce(query, target)
        total.backward()
        out.update({f"{name}_temperature": np.float64(temperature),
                    f"{name}_image": image.detach().numpy(), f"{name}_query": query.detach().numpy(), f"{name}_target": target.detach().numpy(),
                    f"{name}_loss": total.detach().numpy(), f"{name}_loss_t2i": l_t2i.detach().numpy(), f"{name}_loss_t2t": l_t2t.detach().numpy(),
                    f"{name}_grad_image": image.grad.numpy(), f"{name}_grad_query": query.grad.numpy(), f"{name}_grad_target": target.grad.numpy()})
        print(name, float(total.detach()), float(l_t2i.detach()), float(l_t2t.detach()))
    path = os.path.join(HERE, "infonce.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
