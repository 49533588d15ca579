"""GPU: the pooled tower rows (kemr_encode_*_pooled) and the head trainer on frozen towers (finetune.py) on the tiny architecture:
pooled rows against the tail's budget, parity of a training run with fp64 on the CPU, a task a projection can learn, the round trip
through the engine and a checkpoint, the CLI.  Measured figures are printed (pytest -s)."""
import copy
import ctypes as C
import json
import warnings
import zlib

import pytest
import torch

import infonce_ref
from knowledge_enhanced_multimodal_retrieval_amd import _lib, clip_model, datasets, engine, finetune, losses
from knowledge_enhanced_multimodal_retrieval_amd.config import ARCHS
from oracle import clip_ref
from oracle import rounding as R

pytestmark = pytest.mark.gpu
COS_TOL = 1e-3                  # the project's standing bar for embeddings
TAIL_KAPPA, LN_F32_FACTOR = 1, 2.0 ** -21          # the tail's budget, as tests/test_rounding_budget.py applies it
N_ITEMS = 256
TEMPERATURE, T2I_W, T2T_W = 0.07, 0.7, 0.3


def tiny_tokenize(texts, ctx=16, vocab=512):
    """Token ids for the tiny architecture (16 positions, 512 ids): a hash of each word, the end-of-text token = the highest id."""
    out = torch.zeros(len(texts), ctx, dtype=torch.int32)
    for i, t in enumerate(texts):
        ids = [1 + (zlib.crc32(w.encode()) % (vocab - 2)) for w in t.split()][:ctx - 1]
        out[i, :len(ids)] = torch.tensor(ids, dtype=torch.int32)
        out[i, len(ids)] = vocab - 1
    return out


# ------------------------------------------------------------------------------------------------ pooled rows
@pytest.mark.parametrize("precision", [_lib.DEFAULT_PRECISION, "bf16", "bf16-res16"])
def test_pooled_rows_feed_the_tail_and_leave_no_state(device, precision):
    arch, oa = ARCHS["tiny"], clip_ref.ARCHS["tiny"]
    sd = clip_ref.random_state_dict(oa, seed=0)
    eng = engine.ClipEngine(arch, device, precision=precision)
    eng.load_state_dict(sd)
    px = torch.randn(9, 3, arch.image_size, arch.image_size, generator=torch.Generator().manual_seed(1234)).to(device)
    ids = clip_ref.synthetic_ids(oa, 11).to(device)

    def check(pooled, got, gamma, beta, proj, what):
        assert pooled.dtype == torch.float32 and bool(torch.isfinite(pooled).all())
        ref, extra = R.tail_emulation(pooled.cpu(), sd[gamma], sd[beta], sd[proj], TAIL_KAPPA, LN_F32_FACTOR)
        top, _ = R.check_budget(got.cpu(), ref, extra, fmt="fp32", what=what)
        print(f"pooled_{what}_{precision}_ratio", round(top, 4))

    before = eng.encode_image(px)
    pooled = eng.encode_image_pooled(px)
    assert tuple(pooled.shape) == (9, arch.v_width)
    assert torch.equal(eng.encode_image(px), before)                         # the new mode leaves no state behind
    check(pooled, before, "visual.ln_post.weight", "visual.ln_post.bias", "visual.proj", "image")
    for pack in (True, False):                                               # packed (the default route) and dense text calls
        eng.pack_text = pack
        before = eng.encode_text(ids)
        pooled = eng.encode_text_pooled(ids)
        assert tuple(pooled.shape) == (11, arch.t_width)
        assert torch.equal(eng.encode_text(ids), before)
        check(pooled, before, "ln_final.weight", "ln_final.bias", "text_projection", "text_packed" if pack else "text_dense")


def test_pooled_rows_are_refused_for_siglip_and_bert(device):
    import bert_ref as B
    L = _lib.lib()
    p = C.c_void_p(4096)
    sig = engine.ClipEngine(ARCHS["tiny-siglip"], device)
    assert L.kemr_encode_image_pooled(sig._h, p, 1, p, p, 1 << 20, None) == -1
    msg = L.kemr_last_error().decode()
    assert "family 1 (SigLIP)" in msg and "attention pool" in msg
    assert L.kemr_encode_text_pooled(sig._h, p, 1, p, p, 1 << 20, None) == -1 and "family 1 (SigLIP)" in L.kemr_last_error().decode()
    with pytest.raises(RuntimeError, match="CLIP family only"):
        sig.encode_image_pooled(torch.zeros(1, 3, 32, 32, device=device))
    bert = engine.BertEngine(B.BertArch(256, 2, vocab=1024, ctx=512), device)
    assert L.kemr_encode_text_packed_pooled(bert._h, p, p, 1, 1, p, p, 1 << 20, None) == -1
    msg = L.kemr_last_error().decode()
    assert "family 2 (BERT)" in msg and "no projection head" in msg


# ------------------------------------------------------------------------------------------------ trainer
@pytest.fixture(scope="module")
def base(device):
    """(model, dataset, its pixels, the cached pooled rows): computed once; the tests train deep copies of the model."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        model, _ = clip_model.load_clip_model("tiny", None, "cuda")
    ds = datasets.SyntheticRetrievalDataset(N_ITEMS, model.arch.image_size, 42)
    pooled = finetune.cache_pooled(model, ds, batch_size=64, tokenize_fn=tiny_tokenize)
    pixels = torch.stack([ds[i][0] for i in range(N_ITEMS)])
    assert [tuple(p.shape) for p in pooled] == [(N_ITEMS, 256)] * 3 and all(p.is_cuda for p in pooled)
    return model, ds, pixels, pooled


def _fp64_heads(model):
    return {k: p.detach().double().cpu().clone().requires_grad_(True) for k, p in finetune.ProjectionHeads(copy.deepcopy(model).cpu()).named_head_parameters().items()}


def _fp64_features(P, rows, idx=slice(None)):
    f = lambda r, w, b, p: finetune.project(r[idx], P[w], P[b], P[p], 1e-5)              # noqa: E731
    return (f(rows[0], "visual.ln_post.weight", "visual.ln_post.bias", "visual.proj"),
            f(rows[1], "ln_final.weight", "ln_final.bias", "text_projection"), f(rows[2], "ln_final.weight", "ln_final.bias", "text_projection"))


def _fp64_loss(feats):
    def nce(a, b):
        z = a @ b.T / TEMPERATURE
        lab = torch.arange(a.shape[0])
        return (torch.nn.functional.cross_entropy(z, lab) + torch.nn.functional.cross_entropy(z.T, lab)) / 2
    image, query, target = feats
    return T2I_W * nce(target, image) + T2T_W * nce(query, target)


def _r_at_1(image, target):
    return float(((target.double() @ image.double().T).argmax(1).cpu() == torch.arange(image.shape[0])).double().mean())


def test_twenty_sgd_steps_match_fp64_on_the_cpu(base, tmp_path):
    model, _, _, pooled = base
    model = copy.deepcopy(model)
    heads = finetune.ProjectionHeads(model)
    lr, seed = 0.5, 5
    tr = finetune.HeadTrainer(model, heads, pooled, losses.JointContrastiveLoss(TEMPERATURE, T2I_W, T2T_W),
                              torch.optim.SGD(heads.parameters(), lr=lr), None, output_dir=str(tmp_path), total_epochs=5, batch_size=64,
                              grad_clip=0.0, seed=seed)
    P = _fp64_heads(model)
    start = {k: v.detach().clone() for k, v in P.items()}
    tr.train()
    assert tr.optimizer_steps == 20 and len(tr.step_losses) == 20
    rows = [p.double().cpu() for p in pooled]
    gen = torch.Generator().manual_seed(seed)
    worst, step = 0.0, 0
    for _ in range(5):
        for idx in finetune.batch_schedule(N_ITEMS, 64, gen):
            feats = _fp64_features(P, rows, idx)
            loss = _fp64_loss(feats)
            det = [f.detach() for f in feats]
            ref = infonce_ref.joint(*det, TEMPERATURE, T2I_W, T2T_W)
            assert abs(float(ref["loss"]) - float(loss.detach())) < 1e-12
            bud = float(infonce_ref.joint_budget(*det, TEMPERATURE, T2I_W, T2T_W, ref)["loss"])
            ratio = abs(tr.step_losses[step] - float(loss.detach())) / (bud + 0.5 * float(R.ulp(torch.tensor(tr.step_losses[step]), "fp32")))
            worst = max(worst, ratio)
            assert ratio <= 1.0, (step, tr.step_losses[step], float(loss.detach()), bud)
            grads = torch.autograd.grad(loss, list(P.values()))
            with torch.no_grad():
                for p, g in zip(P.values(), grads):
                    p -= lr * g
            step += 1
    print("sgd_parity_worst_loss_budget_ratio", round(worst, 4), "losses", round(tr.step_losses[0], 4), "->", round(tr.step_losses[-1], 4))
    moved = max(float((P[k].detach() - start[k]).abs().max()) for k in P)
    assert moved > 1e-3                                                                  # the run did train something
    got = heads(*pooled)
    want = _fp64_features(P, rows)
    for g, w, name in zip(got, want, ("image", "query", "target")):
        miss = float((1 - torch.nn.functional.cosine_similarity(g.detach().double().cpu(), w.detach(), dim=-1)).max())
        print(f"sgd_parity_{name}_one_minus_cos", f"{miss:.3e}")
        assert miss <= COS_TOL, (name, miss)


def test_a_task_a_projection_can_learn_is_learned(base, tmp_path):
    """Image rows = a fixed random orthogonal map of the target rows + 1 % noise; AdamW (the trainer's), 30 steps at lr 3e-3, the whole
    split as one batch.  The same loop in fp64 on the CPU, on the fp32 CPU oracle's pooled rows of the same texts, measured when this test
    was written: loss 5.5011 -> 0.3255, T2I R@1 0.0000 -> 1.0000 (the fp64 loop below, on the device's cached rows, printed 5.7047 ->
    0.3709 and 0.0 -> 1.0 on the MI355X run; the trainer 5.7047 -> 0.3950 before its last step, 0.0 -> 1.0).  Both runs must start below
    0.1 and end above 0.9."""
    model, _, _, pooled = base
    model = copy.deepcopy(model)
    g = torch.Generator().manual_seed(77)
    target64 = pooled[2].double().cpu()
    q, _ = torch.linalg.qr(torch.randn(256, 256, generator=g, dtype=torch.float64))
    image64 = target64 @ q + 0.01 * target64.std() * torch.randn(target64.shape, generator=g, dtype=torch.float64)
    rows64 = [image64, pooled[1].double().cpu(), target64]
    rows = (image64.float().to(pooled[2].device), pooled[1], pooled[2])
    steps, lr = 30, 3e-3
    # fp64 on the CPU
    P = _fp64_heads(model)
    opt = torch.optim.AdamW(list(P.values()), lr=lr, weight_decay=0.01, betas=(0.9, 0.98), eps=1e-6)
    f0 = _fp64_features(P, rows64)
    cpu = {"loss0": float(_fp64_loss(f0).detach()), "r0": _r_at_1(f0[0].detach(), f0[2].detach())}
    for _ in range(steps):
        opt.zero_grad()
        _fp64_loss(_fp64_features(P, rows64)).backward()
        opt.step()
    f1 = _fp64_features(P, rows64)
    cpu.update(loss1=float(_fp64_loss(f1).detach()), r1=_r_at_1(f1[0].detach(), f1[2].detach()))
    # the trainer on the GPU
    heads = finetune.ProjectionHeads(model)
    with torch.no_grad():
        h0 = heads(*rows)
    gpu = {"r0": _r_at_1(h0[0], h0[2])}
    opt, _ = finetune.build_optimizer(heads, lr=lr, weight_decay=0.01, num_epochs=steps)
    tr = finetune.HeadTrainer(model, heads, rows, losses.JointContrastiveLoss(TEMPERATURE, T2I_W, T2T_W), opt, None,
                              output_dir=str(tmp_path), total_epochs=steps, batch_size=0, grad_clip=0.0,
                              early_stopping_patience=steps + 1)          # no validation set: no epoch is ever "best"
    tr.train()
    with torch.no_grad():
        h1 = heads(*rows)
    gpu.update(loss0=tr.step_losses[0], loss1=tr.step_losses[-1], r1=_r_at_1(h1[0], h1[2]))
    print("learning_cpu_fp64", {k: round(v, 4) for k, v in cpu.items()}, "learning_gpu", {k: round(v, 4) for k, v in gpu.items()})
    assert tr.optimizer_steps == steps
    for run in (cpu, gpu):
        assert run["r0"] < 0.1 and run["r1"] > 0.9, run
    assert gpu["loss1"] < 0.5 * gpu["loss0"]


def test_round_trip_through_the_engine_and_a_checkpoint(base, tmp_path):
    model0, ds, pixels, pooled = base
    model = copy.deepcopy(model0)
    initial = {k: v.detach().clone() for k, v in model.state_dict().items()}
    heads = finetune.ProjectionHeads(model)
    opt, sched = finetune.build_optimizer(heads, lr=1e-3, weight_decay=0.01, num_epochs=2)
    val = datasets.SyntheticRetrievalDataset(64, model.arch.image_size, 43)
    tr = finetune.HeadTrainer(model, heads, pooled, losses.JointContrastiveLoss(TEMPERATURE, T2I_W, T2T_W), opt, sched, val_eval_dataset=val,
                              output_dir=str(tmp_path), total_epochs=2, batch_size=64, tokenize_fn=tiny_tokenize)
    last = tr.train()                                            # validates on the engine path after every epoch's steps: the re-pack
    assert {"T2I_MRR", "T2T_MRR", "val_mrr_avg", "train_loss", "epoch", "lr"} <= set(last)
    assert (tmp_path / "checkpoint_best.pt").exists() and (tmp_path / "checkpoint_latest.pt").exists()
    changed = sorted(k for k, v in model.state_dict().items() if not torch.equal(v, initial[k]))
    assert changed == sorted(finetune.HEAD_PARAMETERS), changed                          # the head tensors, all of them, and nothing else
    # engine path (re-packed by the fingerprint, no refresh()) against the heads on the cached rows
    ids_t = tiny_tokenize([ds[i][2] for i in range(N_ITEMS)])
    got_i, got_t = model.encode_image(pixels.to("cuda")), model.encode_text(ids_t)
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    with torch.no_grad():
        h_i, _, h_t = heads(*pooled)
    for got, rows, gamma, beta, proj, h, what in ((got_i, pooled[0], "visual.ln_post.weight", "visual.ln_post.bias", "visual.proj", h_i, "image"),
                                                  (got_t, pooled[2], "ln_final.weight", "ln_final.bias", "text_projection", h_t, "text")):
        ref, extra = R.tail_emulation(rows.cpu(), sd[gamma], sd[beta], sd[proj], TAIL_KAPPA, LN_F32_FACTOR)
        top, _ = R.check_budget(got.cpu(), ref, extra, fmt="fp32", what=f"round trip {what}")
        # the heads' own output: fp32 torch on the same rows, normalised -- the same fp64 value, torch's rounding instead of the kernel's
        norm = ref.norm(dim=-1, keepdim=True)
        ref_n = ref / norm
        tol = 2 * (extra / norm + ref_n.abs() * (extra.norm(dim=-1, keepdim=True) / norm)) + 64 * 2.0 ** -24
        off = float(((h.double().cpu() - ref_n).abs() / tol).max())
        print(f"round_trip_{what}_engine_ratio", round(top, 4), "heads_ratio", round(off, 4))
        assert off <= 1.0, (what, off)
    # the best checkpoint through load_clip_model (strict): the engine path reproduces the embeddings bit for bit
    best = torch.load(tmp_path / "checkpoint_best.pt", weights_only=True)
    if best["epoch"] == last["epoch"]:
        want_i, want_t = got_i, got_t
    else:                                                        # an earlier epoch was the best: its own state, through this model's engine
        probe = copy.deepcopy(model0)
        probe.load_state_dict(best["model_state_dict"], strict=True)
        want_i, want_t = probe.encode_image(pixels.to("cuda")), probe.encode_text(ids_t)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        loaded, _ = clip_model.load_clip_model("tiny", str(tmp_path / "checkpoint_best.pt"), "cuda")
    assert torch.equal(loaded.encode_image(pixels.to("cuda")), want_i) and torch.equal(loaded.encode_text(ids_t), want_t)


def test_cli_trains_one_epoch_on_synthetic_data(device, tmp_path, capsys):
    from src.clip.train import trainer as shim
    common = ["--model_name", "ViT-B/32", "--output_dir", str(tmp_path), "--experiment_name", "heads", "--num_epochs", "1", "--batch_size", "32",
              "--synthetic", "64", "--t2i_weight", "0.7", "--t2t_weight", "0.3", "--mixed_precision"]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert shim.main(common) != 0
        assert "--freeze_encoders" in capsys.readouterr().err and not (tmp_path / "heads" / "metrics_epoch.jsonl").exists()
        assert shim.main(common + ["--freeze_encoders"]) == 0
    lines = [json.loads(x) for x in (tmp_path / "heads" / "metrics_epoch.jsonl").read_text().splitlines()]
    assert len(lines) == 1
    for key in ("train_loss", "train_loss_t2i", "train_loss_t2t", "T2I_MRR", "T2T_MRR", "val_mrr_avg", "epoch", "lr"):
        assert key in lines[0], key
    assert (tmp_path / "heads" / "checkpoint_latest.pt").exists()
