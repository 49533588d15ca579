"""GPU: end-to-end fine-tuning of towers whose vision heads are 80 wide (tower_train.VisionTower(head_dims=HEAD_DIMS), EndToEndTuning;
the attention is ``kemr_op_attention_hd`` forward and ``kemr_op_attention_backward_hd`` backward, csrc/attention_bwd80.hip) on "tiny-h"
(5 vision tokens) and "tiny-h-257" (257, ViT-H-14's count), width 1280 in 16 heads of 80, two blocks.  The bars are those of
tests/test_end_to_end_train_gpu.py: the forward against the fp64 statement of tests/headdim_ref.py with 16 heads and against the served
engine at 1 - cos <= 1e-3; every gradient against the fp32 plain formulation within twice the error of the plain formulation under
bf16 autocast; what three optimizer steps change and the served engine after them; the CLI.  Measured figures are printed (pytest -s)."""
import json
import warnings

import pytest
import torch

import headdim_ref as H
from knowledge_enhanced_multimodal_retrieval_amd import clip_model, config, evaluators, finetune, losses, tower_train
from oracle import clip_ref
from test_finetune_gpu import tiny_tokenize
from test_text_tower_train_gpu import _random_ids, _rel_l2

pytestmark = pytest.mark.gpu

NAMES = ["tiny-h", "tiny-h-257"]
COS_TOL = 1e-3                          # the project's standing bar for embeddings
TEMPERATURE, T2I_W, T2T_W = 0.07, 0.7, 0.3


def _model(name, outliers=False):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m, _ = clip_model.load_clip_model(name, None, "cuda")
    oa = config.get_arch(name).cfg_dict()
    sd = clip_ref.random_state_dict(oa, seed=0, outliers=outliers)
    m.load_state_dict(sd)
    return m.float(), oa, sd


def _pixels(arch, n, seed):
    return torch.randn(n, 3, arch.image_size, arch.image_size, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("outliers", [False, True], ids=["plain", "heavy_tailed"])
@pytest.mark.parametrize("name", NAMES)
def test_vision_forward_against_the_16_head_statement(device, name, outliers):
    model, oa, sd = _model(name, outliers)
    assert model.arch.v_head_dim == 80
    pixels = _pixels(model.arch, 3, 3)
    with pytest.raises(ValueError, match="heads of 64"):
        tower_train.VisionTower(model)
    tower = tower_train.VisionTower(model, head_dims=tower_train.HEAD_DIMS)
    assert tower.attention == "op" and tower.elementwise == "op" and tower.autocast is True and tower.head_dim == 80
    with torch.no_grad():
        emb, pooled = tower(pixels), tower.pooled(pixels)
    want = H.encode_image(sd, oa, pixels, heads=16, activation=model.activation)
    miss = float(H.one_minus_cos(emb, want).max())
    print(f"hd80_vision_forward_{name}_outliers={outliers}_one_minus_cos {miss:.3e}")
    assert emb.dtype == torch.float32 and miss <= COS_TOL
    served = model.encode_image_pooled(pixels.to(device))                 # what kemr_encode_image_pooled returns
    assert pooled.shape == served.shape
    assert float(H.one_minus_cos(pooled, served).max()) <= COS_TOL


@pytest.mark.parametrize("name", NAMES)
def test_gradients_against_fp32_with_the_bf16_formulation_as_the_yardstick(device, name):
    model, _, _ = _model(name)
    arch = model.arch
    g = torch.Generator().manual_seed(21)
    pixels, ids = _pixels(arch, 3, 22), _random_ids(arch, 6, g)
    probe_v, probe_t = torch.randn(3, arch.embed_dim, generator=g).to(device), torch.randn(6, arch.embed_dim, generator=g).to(device)

    def run(attention, elementwise, autocast):
        vision = tower_train.VisionTower(model, attention=attention, elementwise=elementwise, autocast=autocast,
                                         head_dims=tower_train.HEAD_DIMS)
        text = tower_train.TextTower(model, attention=attention, autocast=autocast, elementwise=elementwise)
        params = {**vision.named_vision_parameters(), **text.named_text_parameters()}
        for p in params.values():
            p.grad = None
        ((vision(pixels) * probe_v).sum() + (text(ids.to(device), tower_train.longest(ids)) * probe_t).sum()).backward()
        return {k: p.grad.detach().clone() for k, p in params.items()}

    g_op = run("op", "op", None)
    g_ref = run("torch", "torch", False)         # fp32, no autocast: the reference
    g_yard = run("torch", "torch", True)         # the plain formulation under the same bf16 autocast: the yardstick
    assert set(g_op) == {k for k in model.state_dict() if k != "logit_scale"}
    worst = 0.0
    for k in g_ref:
        assert bool(torch.isfinite(g_op[k]).all()), k
        e_op, e_yard = _rel_l2(g_op[k], g_ref[k]), _rel_l2(g_yard[k], g_ref[k])
        print(f"hd80_end_to_end_grad_{name} {k}: op {e_op:.3e} yardstick {e_yard:.3e}")
        worst = max(worst, e_op / e_yard)
    print(f"hd80_end_to_end_grad_{name}_worst_ratio {worst:.3f}")
    for k in g_ref:
        e_op, e_yard = _rel_l2(g_op[k], g_ref[k]), _rel_l2(g_yard[k], g_ref[k])
        assert e_op <= 2.0 * e_yard, (k, e_op, e_yard)


def test_three_steps_change_every_tower_parameter_and_the_served_engine_follows(device):
    model, _, _ = _model("tiny-h")
    arch = model.arch
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    tune = tower_train.EndToEndTuning(model)
    assert tune.vision.head_dim == 80 and tune.vision.attention == "op" and tune.tower.attention == "op"
    opt, _ = finetune.build_optimizer(tune, lr=1e-3, weight_decay=0.01, num_epochs=3)
    loss_fn = losses.JointContrastiveLoss(TEMPERATURE, T2I_W, T2T_W)
    g = torch.Generator().manual_seed(9)
    px, q, t = torch.randn(32, 3, arch.image_size, arch.image_size, generator=g), _random_ids(arch, 32, g), _random_ids(arch, 32, g)
    for _ in range(3):
        opt.zero_grad()
        loss, _ = loss_fn(*tune(px, q, t))
        loss.backward()
        opt.step()
    after = model.state_dict()
    for k in before:
        same = torch.equal(after[k], before[k])
        if k == "logit_scale":
            assert same and dict(model.named_parameters())[k].grad is None
        else:
            assert not same, f"{k} did not train"
    # the served engine has re-packed by itself and agrees with the training module
    with torch.no_grad():
        own = tune.vision(px)
        served = model.encode_image(px.to(device), normalize=True)
    miss = float(H.one_minus_cos(own, served).max())
    print(f"hd80_served_engine_after_three_steps_image_one_minus_cos {miss:.3e}")
    assert miss <= COS_TOL


def test_cli_trains_one_epoch_end_to_end(device, tmp_path, monkeypatch):
    """--end_to_end --synthetic 16 on "tiny-h", with the tiny tokenizer in place of CLIP's BPE (the tiny text tower has 16 positions)."""
    monkeypatch.setattr(evaluators, "model_tokenize", lambda m: tiny_tokenize)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert finetune.main(["--model_name", "tiny-h", "--output_dir", str(tmp_path), "--experiment_name", "e2e", "--num_epochs", "1",
                          "--batch_size", "8", "--synthetic", "16", "--t2i_weight", "0.7", "--t2t_weight", "0.3", "--end_to_end"]) == 0
    lines = [json.loads(x) for x in (tmp_path / "e2e" / "metrics_epoch.jsonl").read_text().splitlines()]
    assert len(lines) == 1 and all(k in lines[0] for k in ("train_loss", "T2I_MRR", "T2T_MRR", "val_mrr_avg", "epoch", "lr"))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        loaded, _ = clip_model.load_clip_model("tiny-h", str(tmp_path / "e2e" / "checkpoint_best.pt"), "cuda")
    assert bool(torch.isfinite(loaded.encode_image(_pixels(loaded.arch, 2, 1).to(device))).all())
