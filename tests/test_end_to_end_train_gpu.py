"""GPU: end-to-end fine-tuning (tower_train.py: VisionTower, TextTower(elementwise="op"), EndToEndTuning, EndToEndTrainer) on the tiny
architectures -- "tiny" (17 vision tokens, width 256, two blocks) and "tiny-long" (197 vision tokens, ViT-B/16's count, three blocks,
text width 512): the vision forward against the fp32 oracle on plain and heavy-tailed weights, every gradient against the fp32 plain
formulation with the plain bf16 formulation as the yardstick, what three optimizer steps change, the served engine after them, a
planted task, the checkpoints, the CLI and a step on a side stream.  Measured figures are printed (pytest -s)."""
import copy
import json
import warnings

import pytest
import torch

from knowledge_enhanced_multimodal_retrieval_amd import clip_model, config, datasets, evaluators, finetune, losses, tower_train
from oracle import clip_ref
from test_finetune_gpu import tiny_tokenize
from test_text_tower_train_gpu import _mrr, _random_ids, _rel_l2

pytestmark = pytest.mark.gpu

NAMES = ["tiny", "tiny-long"]
COS_TOL = 1e-3                          # the project's standing bar for embeddings
TEMPERATURE, T2I_W, T2T_W = 0.07, 0.7, 0.3
# the planted run: AdamW (the trainer's) at this rate, whole-batch steps.  With them the CPU formulation (attention="torch",
# elementwise="torch", fp32, a plain torch statement of the loss) takes the loss from 4.816 to 0.133 and text -> image MRR from 0.086
# (chance) to 0.970, measured when this test was written.  The GPU run must reach half the initial loss, the bar of the planted test of
# tests/test_text_tower_train_gpu.py.
PLANTED_N, PLANTED_LR, PLANTED_STEPS = 64, 1e-3, 30


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


def planted(name, n=PLANTED_N, seed=9):
    """(fixed random images fp32 [n, 3, S, S], query ids, target ids int32 [n, ctx]) on the host; item i's three belong together."""
    arch = config.get_arch(name)
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, 3, arch.image_size, arch.image_size, generator=g), _random_ids(arch, n, g), _random_ids(arch, n, g)


# ------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("outliers", [False, True], ids=["plain", "heavy_tailed"])
@pytest.mark.parametrize("name", NAMES)
def test_vision_forward_against_the_oracle(device, name, outliers):
    model, oa, sd = _model(name, outliers)
    pixels = _pixels(model.arch, 5, 3)
    tower = tower_train.VisionTower(model)
    assert tower.attention == "op" and tower.elementwise == "op" and tower.autocast is True
    with torch.no_grad():
        emb, pooled = tower(pixels), tower.pooled(pixels)
    want = clip_ref.l2_normalize(clip_ref.encode_image(sd, oa, pixels))
    miss = float((1 - torch.nn.functional.cosine_similarity(emb.double().cpu(), want.double(), dim=-1)).max())
    print(f"vision_forward_{name}_outliers={outliers}_one_minus_cos {miss:.3e}")
    assert emb.dtype == torch.float32 and miss <= COS_TOL
    served = model.encode_image_pooled(pixels.to(device))                 # what kemr_encode_image_pooled returns
    assert pooled.shape == served.shape
    assert float((1 - torch.nn.functional.cosine_similarity(pooled.double(), served.double(), dim=-1)).max()) <= COS_TOL


# ------------------------------------------------------------------------------------------------ gradients
@pytest.mark.parametrize("name", NAMES)
def test_gradients_against_fp32_with_the_bf16_formulation_as_the_yardstick(device, name):
    model, _, _ = _model(name)
    arch = model.arch
    g = torch.Generator().manual_seed(21)
    pixels, ids = _pixels(arch, 4, 22), _random_ids(arch, 6, g)
    probe_v, probe_t = torch.randn(4, arch.embed_dim, generator=g).to(device), torch.randn(6, arch.embed_dim, generator=g).to(device)

    def run(attention, elementwise, autocast):
        vision = tower_train.VisionTower(model, attention=attention, elementwise=elementwise, autocast=autocast)
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
        print(f"end_to_end_grad_{name} {k}: op {e_op:.3e} yardstick {e_yard:.3e}")
        worst = max(worst, e_op / e_yard)
    print(f"end_to_end_grad_{name}_worst_ratio {worst:.3f}")
    for k in g_ref:
        e_op, e_yard = _rel_l2(g_op[k], g_ref[k]), _rel_l2(g_yard[k], g_ref[k])
        assert e_op <= 2.0 * e_yard, (k, e_op, e_yard)


# ------------------------------------------------------------------------------------------------ what a step changes; the engine after it
def test_three_steps_change_every_tower_parameter_and_the_served_engine_follows(device):
    model, _, _ = _model("tiny")
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    tune = tower_train.EndToEndTuning(model)
    assert tune.vision.elementwise == tune.tower.elementwise and tune.vision.attention == "op" and tune.tower.attention == "op"
    opt, _ = finetune.build_optimizer(tune, lr=1e-3, weight_decay=0.01, num_epochs=3)
    loss_fn = losses.JointContrastiveLoss(TEMPERATURE, T2I_W, T2T_W)
    px, q, t = planted("tiny", 32)
    for _ in range(3):
        opt.zero_grad()
        loss, _ = loss_fn(*tune(px, q, t))
        loss.backward()
        opt.step()
    after = model.state_dict()
    for k in before:
        same = torch.equal(after[k], before[k])
        if k == "logit_scale":
            assert same and before[k].view(torch.int32).equal(after[k].view(torch.int32)), "logit_scale changed"
            assert dict(model.named_parameters())[k].grad is None
        else:
            assert not same, f"{k} did not train"
    # the served engine has re-packed by itself and agrees with the training module
    with torch.no_grad():
        own = tune.vision(px)
        served = model.encode_image(px.to(device), normalize=True)
        own_t = tune.tower(q.to(device), tower_train.longest(q))
        served_t = model.encode_text(q.to(device), normalize=True)
    for a, b, what in ((own, served, "image"), (own_t, served_t, "text")):
        miss = float((1 - torch.nn.functional.cosine_similarity(a.double(), b.double(), dim=-1)).max())
        print(f"served_engine_after_three_steps_{what}_one_minus_cos {miss:.3e}")
        assert miss <= COS_TOL, what


# ------------------------------------------------------------------------------------------------ a planted task and the checkpoints
def test_planted_run_learns_and_the_checkpoint_loads(device, tmp_path):
    model, _, _ = _model("tiny")
    rows = planted("tiny")
    rows = (rows[0].pin_memory(), rows[1], rows[2])
    px, q_ids, _ = rows
    tune = tower_train.EndToEndTuning(model)

    def mrrs():
        with torch.no_grad():
            own = _mrr(tune.tower(q_ids.to(device), tower_train.longest(q_ids)), tune.vision(px))
            served = _mrr(model.encode_text(q_ids.to(device), normalize=True), model.encode_image(px.to(device), normalize=True))
        return own, served

    _, untrained = mrrs()
    opt, _ = finetune.build_optimizer(tune, lr=PLANTED_LR, weight_decay=0.01, num_epochs=PLANTED_STEPS)

    def validate(m):
        s = mrrs()[1]
        return {"T2I_MRR": 100.0 * s, "T2T_MRR": 100.0 * s}

    tr = tower_train.EndToEndTrainer(model, tune, rows, losses.JointContrastiveLoss(TEMPERATURE, T2I_W, T2T_W), opt, None,
                                     output_dir=str(tmp_path), total_epochs=PLANTED_STEPS, batch_size=PLANTED_N, grad_clip=0.0,
                                     early_stopping_patience=PLANTED_STEPS + 1, validate_fn=validate)
    tr.train()
    assert tr.optimizer_steps == PLANTED_STEPS                       # whole-batch steps: one per epoch
    own, served = mrrs()
    print(f"planted_end_to_end loss {tr.step_losses[0]:.4f} -> {tr.step_losses[-1]:.4f}; text -> image MRR untrained {untrained:.4f}, "
          f"served {served:.4f}, training module {own:.4f}")
    assert untrained < 0.2                                           # chance: about ln(64) / 64
    assert tr.step_losses[-1] < 0.5 * tr.step_losses[0]
    assert served > untrained
    assert abs(served - own) <= 0.05
    # checkpoint_best.pt through load_clip_model: the bits of the trainer's own model at that epoch, both towers
    best = torch.load(tmp_path / "checkpoint_best.pt", weights_only=True)
    probe = model
    if best["epoch"] != PLANTED_STEPS - 1:                           # an earlier epoch was the best: its state through this model's class
        probe = copy.deepcopy(model)
        probe.load_state_dict(best["model_state_dict"], strict=True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        loaded, _ = clip_model.load_clip_model("tiny", str(tmp_path / "checkpoint_best.pt"), "cuda")
    assert torch.equal(loaded.encode_image(px.to(device)), probe.encode_image(px.to(device)))
    assert torch.equal(loaded.encode_text(q_ids.to(device)), probe.encode_text(q_ids.to(device)))


def test_dataset_run_collects_pixels_and_validates_through_the_evaluator(device, tmp_path):
    model, _, _ = _model("tiny")
    ds = datasets.SyntheticRetrievalDataset(48, model.arch.image_size, 42)
    val = datasets.SyntheticRetrievalDataset(32, model.arch.image_size, 43)
    rows = finetune.cache_pixels(model, ds, batch_size=32, tokenize_fn=tiny_tokenize)
    assert tuple(rows[0].shape) == (48, 3, 32, 32) and rows[0].dtype == torch.float32 and rows[0].is_pinned() and not any(r.is_cuda for r in rows)
    for r, col in ((rows[1], 1), (rows[2], 2)):
        assert r.dtype == torch.int32 and torch.equal(r, tiny_tokenize([ds[i][col] for i in range(48)]))
    tune = tower_train.EndToEndTuning(model)
    opt, sched = finetune.build_optimizer(tune, lr=1e-4, weight_decay=0.01, num_epochs=2)
    tr = tower_train.EndToEndTrainer(model, tune, rows, losses.JointContrastiveLoss(TEMPERATURE, T2I_W, T2T_W), opt, sched,
                                     val_eval_dataset=val, output_dir=str(tmp_path), total_epochs=2, batch_size=16, tokenize_fn=tiny_tokenize)
    last = tr.train()
    assert {"T2I_MRR", "T2T_MRR", "val_mrr_avg", "train_loss", "epoch", "lr"} <= set(last) and tr.optimizer_steps == 6
    assert (tmp_path / "checkpoint_latest.pt").exists() and (tmp_path / "checkpoint_best.pt").exists()


def test_cli_trains_one_epoch_end_to_end(device, tmp_path, monkeypatch):
    """--end_to_end --synthetic 16 on "tiny".  The CLI tokenises with CLIP's BPE (77 positions, 49 408 ids), which the tiny architecture
    (16 positions, 512 ids) cannot take: the tokenizer the CLI resolves for a model is replaced by the tiny one for this run."""
    from src.clip.train import trainer as shim
    monkeypatch.setattr(evaluators, "model_tokenize", lambda m: tiny_tokenize)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert shim.main(["--model_name", "tiny", "--output_dir", str(tmp_path), "--experiment_name", "e2e", "--num_epochs", "1",
                          "--batch_size", "8", "--synthetic", "16", "--t2i_weight", "0.7", "--t2t_weight", "0.3", "--mixed_precision",
                          "--end_to_end"]) == 0
    lines = [json.loads(x) for x in (tmp_path / "e2e" / "metrics_epoch.jsonl").read_text().splitlines()]
    assert len(lines) == 1 and all(k in lines[0] for k in ("train_loss", "T2I_MRR", "T2T_MRR", "val_mrr_avg", "epoch", "lr"))
    assert (tmp_path / "e2e" / "checkpoint_latest.pt").exists()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        loaded, _ = clip_model.load_clip_model("tiny", str(tmp_path / "e2e" / "checkpoint_best.pt"), "cuda")
    assert bool(torch.isfinite(loaded.encode_image(_pixels(loaded.arch, 2, 1).to(device))).all())


# ------------------------------------------------------------------------------------------------ a side stream
def test_one_step_on_a_side_stream_leaves_the_same_parameter_bits(device):
    px, q, t = planted("tiny", 16)
    states = []
    for side in (None, torch.cuda.Stream(device)):
        model, _, _ = _model("tiny")
        tune = tower_train.EndToEndTuning(model)
        opt, _ = finetune.build_optimizer(tune, lr=1e-3, weight_decay=0.01, num_epochs=1)
        loss_fn = losses.JointContrastiveLoss(TEMPERATURE, T2I_W, T2T_W)
        torch.cuda.synchronize(device)
        with torch.cuda.stream(side) if side is not None else torch.cuda.stream(torch.cuda.current_stream(device)):
            opt.zero_grad()
            loss, _ = loss_fn(*tune(px, q, t))
            loss.backward()
            opt.step()
        torch.cuda.synchronize(device)
        states.append({k: v.detach().clone() for k, v in model.state_dict().items()})
    for k in states[0]:
        a, b = (st[k].reshape(-1).view(torch.uint8) for st in states)
        assert a.equal(b), f"{k}: a step on a side stream left other bits"
