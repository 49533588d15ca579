"""CPU: the head trainer's host side (finetune.py) -- which tensors ProjectionHeads trains, the batch schedule, the accumulation
arithmetic and the early-stopping bookkeeping against a stub loss, the CLI's argument surface -- and the declarations of the pooled-row
entry points."""
import json
import os
import re
import warnings

import pytest
import torch

from knowledge_enhanced_multimodal_retrieval_amd import _lib, clip_model, finetune

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the options of the reference's trainer (its argparse block), by name
REFERENCE_OPTIONS = ["model_name", "checkpoint", "images_dir", "texts_dir", "max_text_length", "temperature", "t2i_weight", "t2t_weight",
                     "batch_size", "num_epochs", "lr", "weight_decay", "grad_clip", "gradient_accumulation_steps",
                     "early_stopping_patience", "early_stopping_metric", "num_workers", "mixed_precision", "output_dir",
                     "experiment_name", "use_wandb", "wandb_project", "seed"]


@pytest.fixture()
def model():
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m, _ = clip_model.load_clip_model("tiny", None, "cpu")
    return m


def test_pooled_entry_points_are_declared():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "kemr.h")).read(), flags=re.S)
    for name, counterpart in (("kemr_encode_image_pooled", "kemr_encode_image"), ("kemr_encode_text_pooled", "kemr_encode_text"),
                              ("kemr_encode_text_packed_pooled", "kemr_encode_text_packed")):
        assert re.search(r"\b%s\s*\(" % name, header) and hasattr(_lib.lib(), name)
        assert len(_lib.SIGNATURES[name][1]) == len(_lib.SIGNATURES[counterpart][1]) - 1          # the counterpart minus `normalize`
    assert _lib.ABI_VERSION == 4


def test_projection_heads_train_exactly_the_six_head_tensors_of_the_model_itself(model):
    clip_model.freeze_clip_encoders(model)                       # the reference's helper leaves the blocks' *proj* tensors trainable ...
    assert any("in_proj" in n or "c_proj" in n for n, p in model.named_parameters() if p.requires_grad)
    heads = finetune.ProjectionHeads(model)                      # ... ProjectionHeads sets the flags itself
    trainable = sorted(n for n, p in model.named_parameters() if p.requires_grad)
    assert trainable == sorted(finetune.HEAD_PARAMETERS)
    named = dict(model.named_parameters())
    for name, p in heads.named_head_parameters().items():
        assert p is named[name], name                            # references, not copies
    assert sorted(id(p) for p in heads.parameters()) == sorted(id(named[n]) for n in finetune.HEAD_PARAMETERS)
    a = model.arch
    out = heads(torch.randn(5, a.v_width), torch.randn(5, a.t_width), torch.randn(5, a.t_width))
    assert [tuple(o.shape) for o in out] == [(5, a.embed_dim)] * 3
    for o in out:
        assert float((o.detach().norm(dim=-1) - 1).abs().max()) < 1e-5 and o.dtype == torch.float32
    before = model._fingerprint()
    torch.optim.SGD(heads.parameters(), lr=0.1).zero_grad()
    out[0].sum().backward()
    torch.optim.SGD([p for p in heads.parameters() if p.grad is not None], lr=0.1).step()
    assert model._fingerprint() != before                        # a step on the heads is a change of the model: the engine re-packs


def test_batch_schedule():
    g = torch.Generator().manual_seed(3)
    b = finetune.batch_schedule(256, 64, g)
    assert [len(x) for x in b] == [64] * 4 and sorted(torch.cat(b).tolist()) == list(range(256))
    b2 = finetune.batch_schedule(256, 64, g)
    assert not torch.equal(torch.cat(b), torch.cat(b2))                                   # another epoch, another order
    assert torch.equal(torch.cat(finetune.batch_schedule(256, 64, torch.Generator().manual_seed(3))), torch.cat(b))      # seeded
    assert [len(x) for x in finetune.batch_schedule(250, 64, g)] == [64] * 3              # incomplete last batch dropped
    for bs in (0, 256, 1000):
        whole = finetune.batch_schedule(256, bs, g)
        assert len(whole) == 1 and sorted(whole[0].tolist()) == list(range(256))          # the whole split as one batch


class _StubLoss:
    """loss = mean of the three feature sums' squares: a function whose gradient is easy to state; metrics with the trainer's keys."""

    def __call__(self, image, query, target):
        loss = (image.sum(-1) ** 2).mean() + 0.5 * ((query - target) ** 2).sum(-1).mean()
        v = float(loss.detach())
        return loss, {"loss": v, "loss_t2i": 2 * v, "loss_t2t": 3 * v}


def _rows(model, n, seed=0):
    g = torch.Generator().manual_seed(seed)
    a = model.arch
    return torch.randn(n, a.v_width, generator=g), torch.randn(n, a.t_width, generator=g), torch.randn(n, a.t_width, generator=g)


def test_accumulation_arithmetic_and_metrics_against_a_stub_loss(model, tmp_path):
    heads = finetune.ProjectionHeads(model)
    rows = _rows(model, 40)
    start = {k: p.detach().clone() for k, p in heads.named_head_parameters().items()}
    opt = torch.optim.SGD(heads.parameters(), lr=0.05)
    tr = finetune.HeadTrainer(model, heads, rows, _StubLoss(), opt, None, output_dir=str(tmp_path), total_epochs=1, batch_size=8,
                              grad_clip=0.0, gradient_accumulation_steps=2, seed=11)
    m = tr.train_epoch(0)
    assert tr.optimizer_steps == 2 and len(tr.step_losses) == 5                          # 5 batches of 8: two steps, the fifth batch's gradient is left over
    assert m["train_loss"] == pytest.approx(sum(tr.step_losses) / 5) and m["train_loss_t2i"] == pytest.approx(2 * m["train_loss"])
    # the same two steps by hand: each the gradient of the MEAN of its two batches' losses
    batches = finetune.batch_schedule(40, 8, torch.Generator().manual_seed(11))
    P = {k: v.clone().requires_grad_(True) for k, v in start.items()}

    def feats(idx):
        f = lambda r, w, b, p: finetune.project(r[idx], P[w], P[b], P[p], 1e-5)          # noqa: E731
        return (f(rows[0], "visual.ln_post.weight", "visual.ln_post.bias", "visual.proj"),
                f(rows[1], "ln_final.weight", "ln_final.bias", "text_projection"), f(rows[2], "ln_final.weight", "ln_final.bias", "text_projection"))

    for step in range(2):
        loss = sum(_StubLoss()(*feats(batches[2 * step + j]))[0] for j in range(2)) / 2
        grads = torch.autograd.grad(loss, list(P.values()))
        with torch.no_grad():
            for p, g in zip(P.values(), grads):
                p -= 0.05 * g
    for k, p in heads.named_head_parameters().items():
        assert float((p.detach() - P[k].detach()).abs().max()) <= 1e-5 * max(1.0, float(P[k].abs().max())), k
    with pytest.raises(ValueError):
        finetune.HeadTrainer(model, heads, rows, _StubLoss(), opt, gradient_accumulation_steps=0, output_dir=str(tmp_path))


def test_early_stopping_bookkeeping_metrics_file_and_checkpoints(model, tmp_path):
    heads = finetune.ProjectionHeads(model)
    opt, sched = finetune.build_optimizer(heads, lr=1e-3, weight_decay=0.01, num_epochs=10)
    assert isinstance(opt, torch.optim.AdamW) and opt.defaults["betas"] == (0.9, 0.98) and opt.defaults["eps"] == 1e-6
    assert sched.T_max == 10 and sched.eta_min == pytest.approx(1e-4)
    mrr = iter([(10.0, 30.0), (12.0, 30.0), (11.0, 30.0), (11.5, 30.0), (50.0, 50.0)])

    def validate(m):
        assert m is model
        a, b = next(mrr)
        return {"T2I_MRR": a, "T2T_MRR": b}

    tr = finetune.HeadTrainer(model, heads, _rows(model, 16), _StubLoss(), opt, sched, output_dir=str(tmp_path / "run"), total_epochs=10,
                              batch_size=0, early_stopping_patience=2, early_stopping_metric="avg", validate_fn=validate)
    tr.train()
    lines = [json.loads(x) for x in (tmp_path / "run" / "metrics_epoch.jsonl").read_text().splitlines()]
    assert [x["epoch"] for x in lines] == [0, 1, 2, 3]                                   # best at epoch 1, two epochs without improvement: stop
    assert [x["val_mrr_avg"] for x in lines] == [20.0, 21.0, 20.5, 20.75]
    for key in ("train_loss", "train_loss_t2i", "train_loss_t2t", "T2I_MRR", "T2T_MRR", "val_mrr_avg", "epoch", "lr"):
        assert key in lines[0], key
    assert lines[0]["lr"] > lines[1]["lr"] > lines[2]["lr"]                              # the cosine schedule steps once per epoch
    assert (tr.best_metric, tr.best_epoch, tr.patience_counter) == (21.0, 1, 2)
    best = torch.load(tmp_path / "run" / "checkpoint_best.pt", weights_only=True)
    latest = torch.load(tmp_path / "run" / "checkpoint_latest.pt", weights_only=True)
    assert best["epoch"] == 1 and latest["epoch"] == 3 and best["best_metric"] == 21.0
    assert sorted(best["model_state_dict"]) == sorted(model.state_dict())                # the full state dict: every evaluator takes it
    t2i = finetune.HeadTrainer(model, heads, _rows(model, 16), _StubLoss(), opt, None, output_dir=str(tmp_path / "r2"),
                               early_stopping_metric="t2i", validate_fn=lambda m: {"T2I_MRR": 7.0, "T2T_MRR": 9.0})
    assert t2i.validate(0)["val_mrr_avg"] == 7.0
    with pytest.raises(ValueError):
        finetune.HeadTrainer(model, heads, _rows(model, 16), _StubLoss(), opt, early_stopping_metric="mean", output_dir=str(tmp_path))


def test_cli_argument_surface_and_the_refusal_without_freeze_encoders(capsys):
    from src.clip.train import trainer as shim
    parser = shim.build_parser()
    dests = {a.dest for a in parser._actions}
    assert set(REFERENCE_OPTIONS) <= dests and "freeze_encoders" in dests
    args = parser.parse_args(["--output_dir", "o", "--experiment_name", "e", "--mixed_precision", "--images_dir", "i", "--texts_dir", "t"])
    ref_defaults = dict(model_name="ViT-L/14", checkpoint=None, max_text_length=150, temperature=0.07, t2i_weight=0.5, t2t_weight=0.5,
                        batch_size=64, num_epochs=20, lr=1e-5, weight_decay=0.01, grad_clip=1.0, gradient_accumulation_steps=1,
                        early_stopping_patience=5, early_stopping_metric="avg", num_workers=4, use_wandb=False,
                        wandb_project="clip-art-retrieval", seed=42)
    for k, v in ref_defaults.items():
        assert getattr(args, k) == v, k
    assert args.mixed_precision is True and args.freeze_encoders is False
    assert shim.main(["--output_dir", "o", "--experiment_name", "e"]) != 0
    err = capsys.readouterr().err
    assert "end-to-end fine-tuning is not served" in err and "--freeze_encoders" in err
    from src.clip.train import losses as shim_losses
    from knowledge_enhanced_multimodal_retrieval_amd import losses
    assert shim_losses.JointContrastiveLoss is losses.JointContrastiveLoss and shim_losses.InfoNCELoss is losses.InfoNCELoss


def test_loss_modules_keep_the_reference_signatures_and_refuse_cpu_tensors():
    from knowledge_enhanced_multimodal_retrieval_amd import losses
    j = losses.JointContrastiveLoss(temperature=0.05, t2i_weight=0.7, t2t_weight=0.7)
    assert j.t2i_weight == 0.5 and j.t2t_weight == 0.5 and j.temperature == 0.05 and losses.InfoNCELoss().temperature == 0.07
    x = torch.randn(4, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        j(x, x, x)
