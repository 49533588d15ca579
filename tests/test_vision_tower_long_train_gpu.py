"""GPU: training a vision tower past the 288 rows of the LDS attention backward (tower_train.VisionTower(max_tokens=MAX_T_LONG) over
``kemr_op_attention_backward_long``, csrc/attention_bwd_stream.hip) on "tiny-290" (a 17 x 17 grid + class token = 290 tokens, width 256,
two blocks), with the bars of tests/test_end_to_end_train_gpu.py: the forward against the fp32 oracle on plain and heavy-tailed weights,
every vision gradient against the fp32 plain formulation with the plain bf16 formulation as the yardstick, what one optimizer step
changes, the CLI, and one gradient check at 577 tokens (ViT-L/14@336px's count).  Measured figures are printed (pytest -s)."""
import json
import warnings

import pytest
import torch

from knowledge_enhanced_multimodal_retrieval_amd import clip_model, clip_module, config, evaluators, finetune, losses, tower_train
from oracle import clip_ref
from test_finetune_gpu import tiny_tokenize
from test_text_tower_train_gpu import _random_ids, _rel_l2

pytestmark = pytest.mark.gpu

NAME = "tiny-290"
COS_TOL = 1e-3                          # the project's standing bar for embeddings
LONG = tower_train.MAX_T_LONG


def _model(outliers=False):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m, _ = clip_model.load_clip_model(NAME, None, "cuda")
    oa = config.get_arch(NAME).cfg_dict()
    sd = clip_ref.random_state_dict(oa, seed=0, outliers=outliers)
    m.load_state_dict(sd)
    return m.float(), oa, sd


def _pixels(arch, n, seed):
    return torch.randn(n, 3, arch.image_size, arch.image_size, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("outliers", [False, True], ids=["plain", "heavy_tailed"])
def test_vision_forward_against_the_oracle(device, outliers):
    model, oa, sd = _model(outliers)
    pixels = _pixels(model.arch, 3, 3)
    with pytest.raises(ValueError, match="290 tokens"):                   # the default range is the LDS kernel's
        tower_train.VisionTower(model)
    tower = tower_train.VisionTower(model, max_tokens=LONG)
    assert tower.attention == "op" and tower.elementwise == "op" and tower.autocast is True and tower.tokens == 290
    with torch.no_grad():
        emb, pooled = tower(pixels), tower.pooled(pixels)
    want = clip_ref.l2_normalize(clip_ref.encode_image(sd, oa, pixels))
    miss = float((1 - torch.nn.functional.cosine_similarity(emb.double().cpu(), want.double(), dim=-1)).max())
    print(f"vision_forward_{NAME}_outliers={outliers}_one_minus_cos {miss:.3e}")
    assert emb.dtype == torch.float32 and miss <= COS_TOL
    served = model.encode_image_pooled(pixels.to(device))                 # what kemr_encode_image_pooled returns
    assert pooled.shape == served.shape
    assert float((1 - torch.nn.functional.cosine_similarity(pooled.double(), served.double(), dim=-1)).max()) <= COS_TOL


def _vision_gradients(model, pixels, probe, what):
    """Every vision gradient of the op tower against the fp32 plain formulation; the yardstick is the plain formulation under bf16 autocast."""
    def run(attention, elementwise, autocast):
        vision = tower_train.VisionTower(model, attention=attention, elementwise=elementwise, autocast=autocast, max_tokens=LONG)
        params = vision.named_vision_parameters()
        for p in params.values():
            p.grad = None
        (vision(pixels) * probe).sum().backward()
        return {k: p.grad.detach().clone() for k, p in params.items()}

    g_op = run("op", "op", None)
    g_ref = run("torch", "torch", False)
    g_yard = run("torch", "torch", True)
    assert set(g_op) == {k for k in model.state_dict() if k.startswith("visual.")}
    ratios = {}
    for k in g_ref:
        assert bool(torch.isfinite(g_op[k]).all()), k
        e_op, e_yard = _rel_l2(g_op[k], g_ref[k]), _rel_l2(g_yard[k], g_ref[k])
        print(f"vision_long_grad_{what} {k}: op {e_op:.3e} yardstick {e_yard:.3e}")
        ratios[k] = (e_op, e_yard)
    print(f"vision_long_grad_{what}_worst_ratio {max(a / b for a, b in ratios.values()):.3f}")
    for k, (e_op, e_yard) in ratios.items():
        assert e_op <= 2.0 * e_yard, (k, e_op, e_yard)


def test_gradients_against_fp32_with_the_bf16_formulation_as_the_yardstick(device):
    model, _, _ = _model()
    g = torch.Generator().manual_seed(21)
    pixels = _pixels(model.arch, 3, 22)
    _vision_gradients(model, pixels, torch.randn(3, model.arch.embed_dim, generator=g).to(device), NAME)


def test_gradients_at_577_tokens(device):
    """A one-block tower with a 24 x 24 grid, the shape tests/test_vision_tower_train_host.py refuses by default."""
    arch = config.ClipArch(128, 192, 8, 256, 1, 256, 1, vocab=512, ctx=16)
    assert arch.v_tokens == 577
    model = clip_module.build_model(arch, device="cuda")
    model.load_state_dict(clip_ref.random_state_dict(arch.cfg_dict(), seed=0))
    model = model.float()
    g = torch.Generator().manual_seed(23)
    pixels = _pixels(arch, 2, 24)
    _vision_gradients(model, pixels, torch.randn(2, arch.embed_dim, generator=g).to(device), "577")


def test_one_step_changes_every_tower_parameter(device):
    model, _, _ = _model()
    arch = model.arch
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    tune = tower_train.EndToEndTuning(model)
    assert tune.vision.attention == "op" and tune.vision.tokens == 290
    opt, _ = finetune.build_optimizer(tune, lr=1e-3, weight_decay=0.01, num_epochs=1)
    g = torch.Generator().manual_seed(9)
    px, q, t = _pixels(arch, 8, 10), _random_ids(arch, 8, g), _random_ids(arch, 8, g)
    opt.zero_grad()
    loss, _ = losses.JointContrastiveLoss(0.07, 0.7, 0.3)(*tune(px, q, t))
    loss.backward()
    opt.step()
    assert bool(torch.isfinite(loss))
    after = model.state_dict()
    for k in before:
        same = torch.equal(after[k], before[k])
        if k == "logit_scale":
            assert same and before[k].view(torch.int32).equal(after[k].view(torch.int32)), "logit_scale changed"
            assert dict(model.named_parameters())[k].grad is None
        else:
            assert not same, f"{k} did not train"


def test_cli_trains_one_epoch_end_to_end(device, tmp_path, monkeypatch):
    """--end_to_end --synthetic 16 on "tiny-290", with the tiny tokenizer in place of CLIP's BPE as in tests/test_end_to_end_train_gpu.py."""
    from src.clip.train import trainer as shim
    monkeypatch.setattr(evaluators, "model_tokenize", lambda m: tiny_tokenize)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert shim.main(["--model_name", NAME, "--output_dir", str(tmp_path), "--experiment_name", "e2e", "--num_epochs", "1",
                          "--batch_size", "8", "--synthetic", "16", "--t2i_weight", "0.7", "--t2t_weight", "0.3", "--mixed_precision",
                          "--end_to_end"]) == 0
    lines = [json.loads(x) for x in (tmp_path / "e2e" / "metrics_epoch.jsonl").read_text().splitlines()]
    assert len(lines) == 1 and all(k in lines[0] for k in ("train_loss", "T2I_MRR", "T2T_MRR", "val_mrr_avg", "epoch", "lr"))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        loaded, _ = clip_model.load_clip_model(NAME, str(tmp_path / "e2e" / "checkpoint_best.pt"), "cuda")
    assert bool(torch.isfinite(loaded.encode_image(_pixels(loaded.arch, 2, 1).to(device))).all())
