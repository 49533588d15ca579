"""GPU: the fusion heads' training path end to end -- parameter gradients of all four heads through losses.FusionContrastiveLoss against
the goldens of the reference's own head classes and against tests/pairhead_ref.py; learning on planted data; bit-identical reruns; the
CLI writing a checkpoint that the fusion evaluator loads.  Every measured ratio is printed (pytest -s)."""
import json
import os
import warnings

import numpy as np
import pytest
import torch

import footprint as F
import pairhead_ref as PR
from fusion_train_cases import HEADS, head_kernel_inputs, mrr_of_scores, planted
from knowledge_enhanced_multimodal_retrieval_amd import fusion_train, losses, ranking
from knowledge_enhanced_multimodal_retrieval_amd.finetune import build_optimizer
from knowledge_enhanced_multimodal_retrieval_amd.fusion_model import FusionModel
from oracle import rounding as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24


def _golden_model(g, fusion_type, dtype):
    fm = FusionModel(torch.nn.Linear(1, 1), fusion_type=fusion_type, embed_dim=64)
    prefix = f"{fusion_type}_param_"
    fm.fusion_head.load_state_dict({k[len(prefix):]: torch.from_numpy(g[k]) for k in g.files if k.startswith(prefix)})
    return fm.to(dtype).eval()


def _chain(fm64, q64, dgate, e_dgate):
    """The gated heads' parameter gradients from dL/dgate, in fp64 on the CPU, and their bound: |J|^T e_dgate for what the kernel's
    gradient carries, plus torch's fp32 chain through gate() and its backward -- a dot product of D terms, one of 128, the bias, the
    ReLU mask and the sigmoid, every product and sum rounded once in each direction: (D + 144) u |J|^T (|dL/dgate| + e_dgate)."""
    h = fm64.fusion_head
    names = [k for k, _ in h.named_parameters()]
    params = [p for _, p in h.named_parameters()]
    gate = h.gate(q64).reshape(-1)
    grads = {k: torch.zeros_like(p) for k, p in zip(names, params)}
    reach = {k: torch.zeros_like(p) for k, p in zip(names, params)}
    carried = {k: torch.zeros_like(p) for k, p in zip(names, params)}
    for i in range(gate.numel()):
        row = torch.autograd.grad(gate[i], params, retain_graph=True)
        for k, r in zip(names, row):
            grads[k] += r * dgate[i]
            carried[k] += r.abs() * e_dgate[i]
            reach[k] += r.abs() * (dgate[i].abs() + e_dgate[i])
    d = q64.shape[1]
    return grads, {k: carried[k] + (d + 144) * U * reach[k] for k in names}


@pytest.mark.parametrize("fusion_type", HEADS)
def test_parameter_gradients_through_autograd_match_the_goldens_and_the_statement(device, fusion_type):
    g = np.load(os.path.join(ROOT, "tests", "golden", "fusion_train_golden.npz"))
    t = float(g["temperature"])
    # the goldens are fp64 of fp64 inputs and parameters; the device gets their fp32 roundings, so the budget is taken at those and the
    # golden's own distance from the fp64 statement at the rounded values is added (what rounding them costs: not the kernel's)
    q, img, tgt = [torch.from_numpy(g[k]).float() for k in ("query", "image", "target")]
    fm = _golden_model(g, fusion_type, torch.float32).to(device)
    for p in fm.fusion_head.parameters():
        p.requires_grad_(True)
    crit = losses.FusionContrastiveLoss(temperature=t)
    loss, metrics = crit(fm, q.to(device), img.to(device), tgt.to(device))
    loss.backward()
    assert sorted(metrics) == ["loss", "loss_g2q", "loss_q2g"] and all(isinstance(v, float) for v in metrics.values())
    assert metrics["loss"] == float(loss.detach()) and loss.requires_grad
    got = {k: p.grad.detach().cpu() for k, p in fm.fusion_head.named_parameters()}

    mode, gate, linear = head_kernel_inputs(fm, q)            # what the kernels were given: the fp32 parameters / the device's fp32 gate
    ref = PR.pairhead(mode, q, img, tgt, t, gate, linear)
    bud = PR.budget(mode, q, img, tgt, t, gate, linear, ref)
    for k in ("loss", "loss_q2g", "loss_g2q"):
        gold = torch.tensor(float(g[f"{fusion_type}_{k}"]), dtype=torch.float64)
        top, _ = R.check_budget(torch.tensor(metrics[k], dtype=torch.float32), gold, bud[k] + (gold - ref[k]).abs(), fmt="fp32",
                                what=f"{fusion_type} {k}")
        print(f"fusion_train_{fusion_type}_{k}_ratio", round(top, 4))
    if fusion_type == "linear":
        h = linear[1].numel()
        names = ("fusion.0.weight", "fusion.0.bias", "fusion.3.weight", "fusion.3.bias")
        ref_p = dict(zip(names, PR.split_linear_grad(ref["grad"], h)))
        bud_p = dict(zip(names, PR.split_linear_grad(bud["grad"], h)))
    else:
        fm64 = _golden_model(g, fusion_type, torch.float32).double()          # the fp32 parameters, in fp64 arithmetic
        ref_p, bud_p = _chain(fm64, q.double(), ref["grad"], bud["grad"])
    assert sorted(ref_p) == sorted(got)
    for k, v in got.items():
        gold = torch.from_numpy(g[f"{fusion_type}_grad_{k}"])
        want = ref_p[k].reshape(gold.shape)
        extra = bud_p[k].reshape(gold.shape) + (gold - want).abs()
        top_s, _ = R.check_budget(v, want, bud_p[k].reshape(gold.shape), fmt="fp32", what=f"{fusion_type} grad {k} against the statement")
        top_g, _ = R.check_budget(v, gold, extra, fmt="fp32", what=f"{fusion_type} grad {k} against the golden")
        print(f"fusion_train_{fusion_type}_grad_{k}_ratios statement {round(top_s, 4)} golden {round(top_g, 4)}")
        assert float(gold.abs().max()) > 0


# ------------------------------------------------------------------------------------------------ learning
def _fresh(fusion_type, device, seed=0):
    torch.manual_seed(seed)
    return FusionModel(torch.nn.Linear(1, 1), fusion_type=fusion_type, embed_dim=64).to(device).eval()


@pytest.fixture(scope="module")
def planted_splits(device):
    train, val = planted(300, 64, seed=1), planted(300, 64, seed=2)
    q, img, tgt = [x.double() for x in val]
    mix = mrr_of_scores(0.5 * (q @ img.T) + 0.5 * (q @ tgt.T))
    return [x.to(device) for x in train], [x.to(device) for x in val], mix


@pytest.mark.parametrize("fusion_type", ["linear", "simple_gated_with_bias", "gated"])
def test_a_head_learns_to_ignore_a_signal_free_t2t(device, planted_splits, fusion_type):
    """Planted data whose targets are noise: 100 whole-split AdamW steps (lr 0.05, no decay, temperature 0.07) must lower the training
    loss and lift the SERVED validation ranking to at least 1.5 x the fixed 0.5 / 0.5 mix's MRR.  The same recipe in fp64 torch on the
    CPU (dense formulation) gives 1.99 x (linear), 1.81 x (simple_gated_with_bias) and 2.01 x (gated): the bar is the recipe's, not
    the kernels'."""
    train, val, mix = planted_splits
    fm = _fresh(fusion_type, device)
    crit = losses.FusionContrastiveLoss(temperature=0.07)
    opt = torch.optim.AdamW(fm.fusion_head.parameters(), lr=0.05, weight_decay=0.0)
    history = []
    for _ in range(100):
        opt.zero_grad()
        loss, metrics = crit(fm, *train)
        loss.backward()
        opt.step()
        history.append(metrics["loss"])
    final = crit(fm, *train)[1]["loss"]
    ranks, _, _ = fm.rank(*val, k=0)
    mrr = ranking.metrics_from_ranks(ranks, [1])["MRR"] / 100.0
    print(f"fusion_train_learning_{fusion_type}: loss {history[0]:.4f} -> {final:.4f}, val MRR {mrr:.4f} = {mrr / mix:.2f} x the mix's {mix:.4f}")
    assert all(np.isfinite(history)) and final < history[0]
    assert mrr >= 1.5 * mix


def _run_trainer(fusion_type, device, out_dir):
    train, val = planted(96, 64, seed=1), planted(96, 64, seed=2)
    fm = _fresh(fusion_type, device, seed=3)
    opt, sched = build_optimizer(fm.fusion_head, 0.02, 0.01, 3)
    trainer = fusion_train.FusionHeadTrainer(fm, [x.to(device) for x in train], [x.to(device) for x in val],
                                             losses.FusionContrastiveLoss(0.07), opt, sched, output_dir=str(out_dir), total_epochs=3,
                                             batch_size=32, early_stopping_patience=5, grad_clip=1.0, seed=7)
    trainer.train()
    return trainer


@pytest.mark.parametrize("fusion_type", ["linear", "gated"])
def test_two_identical_runs_write_bit_identical_checkpoints(device, tmp_path, fusion_type):
    a, b = _run_trainer(fusion_type, device, tmp_path / "a"), _run_trainer(fusion_type, device, tmp_path / "b")
    assert len(a.step_losses) == 9 and a.step_losses == b.step_losses            # 3 epochs x 3 batches of 32 (the last 0 items dropped)
    ca, cb = [torch.load(str(tmp_path / d / "fusion_best.pt"), map_location="cpu", weights_only=True) for d in ("a", "b")]
    assert tuple(ca) == fusion_train.CHECKPOINT_KEYS and ca["fusion_type"] == fusion_type and ca["embed_dim"] == 64
    assert sorted(ca["fusion_head_state_dict"]) == sorted(cb["fusion_head_state_dict"])
    for k, v in ca["fusion_head_state_dict"].items():
        assert F.same_bits(v, cb["fusion_head_state_dict"][k]), k
    assert ca["epoch"] == cb["epoch"] and ca["best_metric"] == cb["best_metric"]
    lines = [json.loads(x) for x in open(tmp_path / "a" / "metrics_epoch.jsonl")]
    assert len(lines) == 3 and all("train_loss" in x and "val_MRR" in x and "lr" in x for x in lines)
    assert (tmp_path / "a" / "fusion_latest.pt").exists()
    fresh = FusionModel(torch.nn.Linear(1, 1), fusion_type=fusion_type, embed_dim=64)
    fresh.fusion_head.load_state_dict(ca["fusion_head_state_dict"])             # round trip into a fresh model


def test_cli_trains_and_the_fusion_evaluator_loads_the_checkpoint(device, tmp_path):
    from knowledge_enhanced_multimodal_retrieval_amd import evaluators
    from src.clip.train import train_fusion as shim
    out = tmp_path / "run"
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert shim.main(["--synthetic", "96", "--model_name", "ViT-B/32", "--fusion_type", "simple_gated_with_bias", "--num_epochs", "2",
                          "--batch_size", "0", "--output_dir", str(out)]) == 0
        best, latest = out / "fusion_best.pt", out / "fusion_latest.pt"
        assert best.exists() and latest.exists()
        lines = [json.loads(x) for x in open(out / "metrics_epoch.jsonl")]
        assert [x["epoch"] for x in lines] == [0, 1] and all(np.isfinite(x["train_loss"]) and 0 < x["val_MRR"] <= 100 for x in lines)
        ckpt = torch.load(str(best), map_location="cpu", weights_only=True)
        assert tuple(ckpt) == fusion_train.CHECKPOINT_KEYS and ckpt["fusion_type"] == "simple_gated_with_bias" and ckpt["embed_dim"] == 512
        assert sorted(ckpt["fusion_head_state_dict"]) == ["bias", "query_weight"]
        assert bool(ckpt["fusion_head_state_dict"]["query_weight"].any())       # the default is all zeros: it moved
        res = evaluators.main_fusion(["--model_name", "ViT-B/32", "--fusion_type", "simple_gated_with_bias", "--fusion_checkpoint", str(best),
                                      "--synthetic", "96", "--output_file", str(tmp_path / "eval.json")])
    assert res["fusion_checkpoint"] == str(best) and res["num_samples"] == 96
    assert 0 < res["metrics"]["MRR"] <= 100 and "R@10" in res["metrics"]
