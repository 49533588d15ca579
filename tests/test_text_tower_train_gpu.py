"""GPU: the differentiable text tower with the library's attention in both directions (tower_train.py; kemr_op_attention forward,
kemr_op_attention_backward backward) on the tiny architectures -- "tiny" (16 positions), "tiny-ctx248" (Long-CLIP's 248) and
"tiny-long" (77 positions, width 512, three blocks): the forward against the fp32 oracle, every text parameter's gradient against the
fp32 plain formulation with the plain bf16 formulation as the yardstick, which tensors an optimizer step changes, a planted task, the
served engine after the re-pack, and the checkpoint.  Measured figures are printed (pytest -s)."""
import copy
import warnings

import pytest
import torch

from knowledge_enhanced_multimodal_retrieval_amd import clip_model, config, datasets, finetune, losses, tower_train
from oracle import clip_ref

pytestmark = pytest.mark.gpu

NAMES = ["tiny", "tiny-ctx248", "tiny-long"]
COS_TOL = 1e-3                          # the project's standing bar for embeddings
TEMPERATURE, T2I_W, T2T_W = 0.07, 0.7, 0.3
# the planted run: AdamW (the trainer's) at this rate, whole-batch steps.  With them the CPU attention="torch" path in fp32 (the same
# module, a plain torch statement of the loss) reaches a quarter of the initial loss on every architecture, measured when this test was
# written: tiny 5.5543 -> 0.4050, tiny-ctx248 5.5279 -> 0.1180, tiny-long 5.1878 -> 0.0615.  The GPU run must reach a half.
PLANTED_N, PLANTED_LR, PLANTED_STEPS = 128, 1e-3, 10


def _model(name, device):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m, _ = clip_model.load_clip_model(name, None, "cuda")
    oa = config.get_arch(name).cfg_dict()
    sd = clip_ref.random_state_dict(oa, seed=0)
    m.load_state_dict(sd)
    return m.float(), oa, sd


def _random_ids(arch, n, g):
    """Random token ids with random end-of-text positions (lengths 2 .. ctx): start-of-text, ids, the end-of-text token = the row maximum."""
    out = torch.zeros(n, arch.ctx, dtype=torch.int32)
    lens = torch.randint(2, arch.ctx + 1, (n,), generator=g)
    body = torch.randint(1, arch.vocab - 2, (n, arch.ctx), generator=g, dtype=torch.int32)
    for i in range(n):
        length = int(lens[i])
        out[i, :length] = body[i, :length]
        out[i, 0] = arch.vocab - 2
        out[i, length - 1] = arch.vocab - 1
    return out


def planted(name, n=PLANTED_N, seed=9):
    """(fixed random image rows fp32 [n, v_width], query ids, target ids int32 [n, ctx]); item i's three belong together."""
    arch = config.get_arch(name)
    g = torch.Generator().manual_seed(seed)
    img = torch.randn(n, arch.v_width, generator=g)
    return img, _random_ids(arch, n, g), _random_ids(arch, n, g)


def _mrr(text, image):
    """Mean reciprocal rank of item i's image among all images for text i (ties count against)."""
    s = text.double() @ image.double().T
    rank = (s >= s.diag()[:, None]).sum(dim=1)
    return float((1.0 / rank.double()).mean())


def _rel_l2(x, ref):
    return float((x.double() - ref.double()).norm() / ref.double().norm())


# ------------------------------------------------------------------------------------------------ forward and gradients
@pytest.mark.parametrize("name", NAMES)
def test_forward_against_the_oracle_and_gradients_against_fp32(device, name):
    model, oa, sd = _model(name, device)
    arch = config.get_arch(name)
    g = torch.Generator().manual_seed(21)
    ids = _random_ids(arch, 6, g)
    ids[0] = 0
    ids[0, 0], ids[0, arch.ctx - 1] = arch.vocab - 2, arch.vocab - 1                 # one text that fills the context
    ids[0, 1:arch.ctx - 1] = torch.randint(1, arch.vocab - 2, (arch.ctx - 2,), generator=g, dtype=torch.int32)
    probe = torch.randn(6, arch.embed_dim, generator=g).to(device)
    want = clip_ref.l2_normalize(clip_ref.encode_text(sd, oa, ids))

    def run(attention, autocast):
        tower = tower_train.TextTower(model, attention=attention, autocast=autocast)
        for p in tower.parameters():
            p.grad = None
        emb = tower(ids.to(device), tower_train.longest(ids))
        (emb * probe).sum().backward()
        return emb.detach(), {k: p.grad.detach().clone() for k, p in tower.named_text_parameters().items()}

    emb_op, g_op = run("op", True)
    miss = float((1 - torch.nn.functional.cosine_similarity(emb_op.double().cpu(), want.double(), dim=-1)).max())
    print(f"tower_forward_{name}_one_minus_cos {miss:.3e}")
    assert emb_op.dtype == torch.float32 and miss <= COS_TOL
    _, g_ref = run("torch", False)            # fp32, no autocast: the reference
    _, g_yard = run("torch", True)            # the plain formulation under the same bf16 autocast: the yardstick
    worst = 0.0
    for k in g_ref:
        assert bool(torch.isfinite(g_op[k]).all()), k
        e_op, e_yard = _rel_l2(g_op[k], g_ref[k]), _rel_l2(g_yard[k], g_ref[k])
        print(f"tower_grad_{name} {k}: op {e_op:.3e} yardstick {e_yard:.3e}")
        worst = max(worst, e_op / e_yard)
        assert e_op <= 2.0 * e_yard, (k, e_op, e_yard)
    print(f"tower_grad_{name}_worst_ratio {worst:.3f}")


# ------------------------------------------------------------------------------------------------ what a step changes
def test_three_steps_change_every_text_parameter_and_no_locked_vision_parameter(device):
    model, _, _ = _model("tiny", device)
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    tune = tower_train.LockedImageTuning(model)
    opt, _ = finetune.build_optimizer(tune, lr=1e-3, weight_decay=0.01, num_epochs=3)
    loss_fn = losses.JointContrastiveLoss(TEMPERATURE, T2I_W, T2T_W)
    img, q, t = (x.to(device) for x in planted("tiny", 32))
    for _ in range(3):
        opt.zero_grad()
        loss, _ = loss_fn(*tune(img, q, t))
        loss.backward()
        opt.step()
    after = model.state_dict()
    free = ("visual.ln_post.weight", "visual.ln_post.bias", "visual.proj")
    for k in before:
        same = torch.equal(after[k], before[k])
        if k.startswith("visual.") and k not in free or k == "logit_scale":
            assert same, f"{k} is locked and changed"
            assert dict(model.named_parameters())[k].grad is None, k
        else:
            assert not same, f"{k} did not train"


# ------------------------------------------------------------------------------------------------ a planted task, the engine, the checkpoint
@pytest.mark.parametrize("name", NAMES)
def test_planted_run_learns_and_the_served_engine_follows(device, name, tmp_path):
    model, _, _ = _model(name, device)
    rows = tuple(x.to(device) for x in planted(name))
    img, _, t_ids = rows
    tune = tower_train.LockedImageTuning(model)

    def mrrs():
        with torch.no_grad():
            image = tune.heads.image(img)
            own = tune.tower(t_ids, tower_train.longest(t_ids))
            served = model.encode_text(t_ids, normalize=True)        # the engine: re-packed by itself after the optimizer's steps
        return _mrr(own, image), _mrr(served, image)

    _, untrained = mrrs()
    opt, _ = finetune.build_optimizer(tune, lr=PLANTED_LR, weight_decay=0.01, num_epochs=PLANTED_STEPS)
    served_per_epoch = []

    def validate(m):
        served_per_epoch.append(mrrs()[1])
        return {"T2I_MRR": 100.0 * served_per_epoch[-1], "T2T_MRR": 100.0 * served_per_epoch[-1]}

    tr = tower_train.TextTowerTrainer(model, tune, rows, losses.JointContrastiveLoss(TEMPERATURE, T2I_W, T2T_W), opt, None,
                                      output_dir=str(tmp_path), total_epochs=PLANTED_STEPS, batch_size=PLANTED_N, grad_clip=0.0,
                                      early_stopping_patience=PLANTED_STEPS + 1, validate_fn=validate)
    tr.train()
    assert tr.optimizer_steps == PLANTED_STEPS                       # whole-batch steps: one per epoch
    own, served = mrrs()
    print(f"planted_{name} loss {tr.step_losses[0]:.4f} -> {tr.step_losses[-1]:.4f}; MRR untrained {untrained:.4f}, served {served:.4f}, "
          f"training module {own:.4f}")
    assert tr.step_losses[-1] < 0.5 * tr.step_losses[0]
    assert served > untrained
    assert abs(served - own) <= 0.05
    # checkpoint_best.pt through load_clip_model: the bits of the trainer's own model at that epoch
    best = torch.load(tmp_path / "checkpoint_best.pt", weights_only=True)
    probe = model
    if best["epoch"] != PLANTED_STEPS - 1:                           # an earlier epoch was the best: its state through this model's class
        probe = copy.deepcopy(model)
        probe.load_state_dict(best["model_state_dict"], strict=True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        loaded, _ = clip_model.load_clip_model(name, str(tmp_path / "checkpoint_best.pt"), "cuda")
    assert torch.equal(loaded.encode_text(t_ids), probe.encode_text(t_ids))


def test_dataset_run_validates_through_the_evaluator_and_checkpoints(device, tmp_path):
    """What the CLI does, on the tiny model with its own tokenizer: cache_image_pooled over a dataset, two epochs with the per-epoch
    validation through evaluate_clip_model_for_training (the served engine), the checkpoints."""
    from test_finetune_gpu import tiny_tokenize
    model, _, _ = _model("tiny", device)
    ds = datasets.SyntheticRetrievalDataset(96, model.arch.image_size, 42)
    val = datasets.SyntheticRetrievalDataset(64, model.arch.image_size, 43)
    rows = finetune.cache_image_pooled(model, ds, batch_size=64, tokenize_fn=tiny_tokenize)
    assert tuple(rows[0].shape) == (96, 256) and rows[0].dtype == torch.float32 and all(r.is_cuda for r in rows)
    assert torch.equal(rows[0], finetune.cache_pooled(model, ds, batch_size=64, tokenize_fn=tiny_tokenize)[0])      # cache_pooled's image half
    for r, col in ((rows[1], 1), (rows[2], 2)):
        assert r.dtype == torch.int32 and torch.equal(r.cpu(), tiny_tokenize([ds[i][col] for i in range(96)]))
    tune = tower_train.LockedImageTuning(model)
    opt, sched = finetune.build_optimizer(tune, lr=1e-3, weight_decay=0.01, num_epochs=2)
    tr = tower_train.TextTowerTrainer(model, tune, rows, losses.JointContrastiveLoss(TEMPERATURE, T2I_W, T2T_W), opt, sched,
                                      val_eval_dataset=val, output_dir=str(tmp_path), total_epochs=2, batch_size=32,
                                      tokenize_fn=tiny_tokenize)
    last = tr.train()
    assert {"T2I_MRR", "T2T_MRR", "val_mrr_avg", "train_loss", "epoch", "lr"} <= set(last) and tr.optimizer_steps == 6
    assert (tmp_path / "checkpoint_latest.pt").exists() and (tmp_path / "metrics_epoch.jsonl").exists()
    best = torch.load(tmp_path / "checkpoint_best.pt", weights_only=True)
    probe = model
    if best["epoch"] != last["epoch"]:
        probe = copy.deepcopy(model)
        probe.load_state_dict(best["model_state_dict"], strict=True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        loaded, _ = clip_model.load_clip_model("tiny", str(tmp_path / "checkpoint_best.pt"), "cuda")
    assert torch.equal(loaded.encode_text(rows[2]), probe.encode_text(rows[2]))


def test_cli_trains_one_epoch_with_a_locked_image_tower(device, tmp_path):
    import json
    from src.clip.train import trainer as shim
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert shim.main(["--model_name", "ViT-B/32", "--output_dir", str(tmp_path), "--experiment_name", "lit", "--num_epochs", "1",
                          "--batch_size", "32", "--synthetic", "64", "--t2i_weight", "0.7", "--t2t_weight", "0.3", "--mixed_precision",
                          "--lock_image_tower"]) == 0
    lines = [json.loads(x) for x in (tmp_path / "lit" / "metrics_epoch.jsonl").read_text().splitlines()]
    assert len(lines) == 1 and all(k in lines[0] for k in ("train_loss", "T2I_MRR", "T2T_MRR", "val_mrr_avg", "epoch", "lr"))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        loaded, _ = clip_model.load_clip_model("ViT-B/32", str(tmp_path / "lit" / "checkpoint_best.pt"), "cuda")
    ids = torch.zeros(1, 77, dtype=torch.int32)
    ids[0, 0], ids[0, 3] = 49406, 49407
    assert bool(torch.isfinite(loaded.encode_text(ids)).all())            # the evaluators' loader takes the checkpoint
