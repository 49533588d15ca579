#!/usr/bin/env python3
"""Generate the exact-GELU encoder fixtures under tests/golden/ (the siblings of make_golden.py section 4 / 4b).

Runs ONLY in the build container, on the CPU: a from-config ``transformers.CLIPModel`` (the class the reference calls in
``src/clip/eval/evaluator_hf.py``) with both ``hidden_act`` set to ``"gelu"``, seeded weights through
``oracle.clip_ref.to_hf_state_dict``, seeded inputs.  The GPU tests rebuild the weights from the seeds with
:func:`gelu_fixture_state_dict` (they load this file as a module; ``transformers`` is imported only by :func:`main`) and
read only the files written here.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_gelu.py

Which weights.  The fixtures must tell the two activations apart: 1 - cos between the HF gelu and the HF quick_gelu outputs of
the same weights and inputs has to exceed ten times the engine's bar of 1e-3, for every embedding.  Measured here (tiny /
tiny-long, worst embedding of either tower):

* plain ``random_state_dict(arch, 0)``: 1.2e-5 / 2.0e-5 -- the pre-activations of fc1 are N(0, 0.7), where the two functions
  differ by at most 0.02 of outputs of 0.5, and c_proj passes a small share of that into the residual stream;
* ``scale`` = 2, 3, 8, 16: 2.5e-5, 1.3e-5, 2.3e-7, 4e-9 -- larger pre-activations sit where both functions are the identity or 0;
* ``outliers=True`` (also at scale 4) and ``add_outliers`` with 64 ungated gains of 3 .. 6 per LayerNorm: 2e-6 .. 8e-5.

Neither knob of ``random_state_dict`` gets near 1e-2, so the fixtures post-process the plain weights instead (NEEDED: both steps):

* ``mlp.c_fc.bias -= 2.5`` in every block: the pre-activations sit around -2.5, the negative flank, where GELU and QuickGELU
  differ by their own size (x = -3: -0.0040 against -0.0181) -- and where most pre-activations of a trained MLP sit;
* ``mlp.c_proj.weight *= 16`` in every block: the MLP update carries the residual stream instead of being 1 % of it.

That gives 2.4e-2 / 2.5e-2 at the worst embedding (tiny / tiny-long) and is asserted below and, on the stored pairs, in
tests/test_gelu_host.py.
"""
import copy
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

FC1_BIAS_SHIFT = 2.5
C_PROJ_GAIN = 16.0
WEIGHT_SEED = 0
PIXEL_SEED = 1234
SEPARATION = 10 * 1e-3           # ten times the engine's bar (COS_TOL)
# (architecture, images, texts, store the inputs)
CASES = (("tiny", 4, 6, True), ("tiny-long", 4, 6, True), ("ViT-B/32", 4, 8, False))


def gelu_fixture_state_dict(arch, seed=WEIGHT_SEED):
    """The fixtures' weights (OpenAI names): ``clip_ref.random_state_dict(arch, seed)`` with the two steps of the module docstring."""
    from oracle import clip_ref
    sd = clip_ref.random_state_dict(arch, seed=seed)
    for k in sd:
        if k.endswith(".mlp.c_fc.bias"):
            sd[k] = sd[k] - FC1_BIAS_SHIFT
        elif k.endswith(".mlp.c_proj.weight"):
            sd[k] = sd[k] * C_PROJ_GAIN
    return sd


def fixture_inputs(arch, n_images, n_texts):
    from oracle import clip_ref
    gg = torch.Generator().manual_seed(PIXEL_SEED)
    px = torch.randn(n_images, 3, arch["image_size"], arch["image_size"], generator=gg)
    return px, clip_ref.synthetic_ids(arch, n_texts)


def fixture_path(name):
    full = "" if name.startswith("tiny") else "full_"
    return os.path.join(HERE, "clip_hf_gelu_%s%s.npz" % (full, name.replace("/", "-")))


def one_minus_cos(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return 1.0 - torch.nn.functional.cosine_similarity(a, b, dim=-1)


def hf_features(arch, act, sd, px, ids):
    from transformers import CLIPConfig, CLIPModel
    from oracle import clip_ref
    kw = copy.deepcopy(clip_ref.hf_config_kwargs(arch))
    kw["text_config"]["hidden_act"] = kw["vision_config"]["hidden_act"] = act
    cfg = CLIPConfig(**kw)
    cfg._attn_implementation = "eager"
    m = CLIPModel(cfg).eval().float()
    m.load_state_dict(clip_ref.to_hf_state_dict(sd, arch), strict=True)
    with torch.no_grad():
        hi = m.get_image_features(pixel_values=px)
        hi = hi if torch.is_tensor(hi) else hi.pooler_output
        ht = m.get_text_features(input_ids=ids.long())
        ht = ht if torch.is_tensor(ht) else ht.pooler_output
    return hi, ht


def main():
    from oracle import clip_ref
    for name, n_img, n_txt, store_inputs in CASES:
        arch = clip_ref.ARCHS[name]
        sd = gelu_fixture_state_dict(arch)
        px, ids = fixture_inputs(arch, n_img, n_txt)
        gi, gt = hf_features(arch, "gelu", sd, px, ids)
        # the quick_gelu outputs of the SAME weights: the existing clip_hf_*.npz hold other weights (no shift, no gain)
        qi, qt = hf_features(arch, "quick_gelu", sd, px, ids)
        sep = min(float(one_minus_cos(gi, qi).min()), float(one_minus_cos(gt, qt).min()))
        assert sep > SEPARATION, (name, sep)
        meta = {"weight_seed": WEIGHT_SEED, "fc1_bias_shift": FC1_BIAS_SHIFT, "c_proj_gain": C_PROJ_GAIN, "pixel_seed": PIXEL_SEED,
                "pixel_abs_sum": float(px.double().abs().sum()), "n_images": n_img, "n_texts": n_txt,
                "weight_abs_sums": {k: float(v.double().abs().sum()) for k, v in sd.items()}}
        out = dict(image_features=gi.numpy(), text_features=gt.numpy(), image_features_quick_gelu=qi.numpy(),
                   text_features_quick_gelu=qt.numpy(), ids=ids.numpy(),
                   meta_json=np.frombuffer(json.dumps(meta, sort_keys=True).encode(), dtype=np.uint8))
        if store_inputs:
            out["pixels"] = px.numpy()
        np.savez_compressed(fixture_path(name), **out)
        print(name, "gelu vs quick_gelu, worst 1 - cos:", sep, "| bytes:", os.path.getsize(fixture_path(name)), flush=True)


if __name__ == "__main__":
    main()
