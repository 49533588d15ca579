"""CPU (attention="torch", elementwise="torch"): the differentiable vision tower of tower_train.py against the oracle, its gradient
against fp64 finite differences, the refusals, what EndToEndTuning trains, and the CLI surface of --end_to_end."""
import copy
import warnings

import pytest
import torch
import torch.nn.functional as F

from knowledge_enhanced_multimodal_retrieval_amd import clip_model, clip_module, config, finetune, tower_train
from oracle import clip_ref


def _model(name, seed=0):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m, _ = clip_model.load_clip_model(name, None, "cpu")
    oa = config.get_arch(name).cfg_dict()
    sd = clip_ref.random_state_dict(oa, seed=seed)          # LayerNorm gains and biases that are not 1 and 0
    m.load_state_dict(sd)
    return m.float(), oa, sd


def _pixels(oa, n, seed=5):
    return torch.randn(n, 3, oa["image_size"], oa["image_size"], generator=torch.Generator().manual_seed(seed))


def _oracle_hidden_fp64(sd, oa, pixels):
    """clip_ref.encode_image(return_hidden=True) line by line with the oracle's own block (clip_ref._block) on fp64 tensors: the oracle's
    entry point casts its state dict to fp32, which cannot carry a bar of 1e-9."""
    sd = {k: v.double() for k, v in sd.items() if k.startswith("visual.")}
    vw = oa["v_width"]
    x = F.conv2d(pixels.double(), sd["visual.conv1.weight"], stride=oa["patch"]).flatten(2).transpose(1, 2)
    x = torch.cat([sd["visual.class_embedding"].expand(x.shape[0], 1, vw), x], dim=1) + sd["visual.positional_embedding"]
    x = F.layer_norm(x, (vw,), sd["visual.ln_pre.weight"], sd["visual.ln_pre.bias"], 1e-5)
    for i in range(oa["v_layers"]):
        x = clip_ref._block(x, sd, f"visual.transformer.resblocks.{i}", vw // 64, causal=False)
    return x


def test_fp64_pooled_rows_match_the_oracle():
    model, oa, sd = _model("tiny")
    pixels = _pixels(oa, 5)
    tower = tower_train.VisionTower(copy.deepcopy(model).double(), attention="torch", elementwise="torch")
    assert tower.autocast is False and tower.causal is False and tower.tokens == 17
    with torch.no_grad():
        pooled, emb = tower.pooled(pixels.double()), tower(pixels.double())
    want = _oracle_hidden_fp64(sd, oa, pixels)[:, 0]
    miss = float((pooled - want).abs().max() / want.abs().max())
    print(f"vision_tower_tiny_fp64_pooled_rel {miss:.3e}")
    assert pooled.dtype == torch.float64 and miss <= 1e-9
    # the oracle's own entry point (fp32): its pooled rows and its embeddings at fp32's grade
    hidden32 = clip_ref.encode_image(sd, oa, pixels, return_hidden=True)[:, 0]
    assert float((pooled - hidden32).abs().max() / want.abs().max()) <= 1e-5
    want_emb = clip_ref.l2_normalize(clip_ref.encode_image(sd, oa, pixels))
    assert float((1 - F.cosine_similarity(emb, want_emb.double(), dim=-1)).max()) <= 1e-9
    assert float((emb.norm(dim=-1) - 1).abs().max()) < 1e-12
    # fp32 parameters: the same module in the parameters' dtype
    with torch.no_grad():
        emb32 = tower_train.VisionTower(model, attention="torch", elementwise="torch")(pixels)
    assert emb32.dtype == torch.float32 and float((1 - F.cosine_similarity(emb32, want_emb, dim=-1)).max()) <= 1e-6


def test_gradient_against_fp64_finite_differences():
    """Central differences at h = 1e-6 on an fp64 copy, as tests/test_text_tower_train_host.py: the bar is 1e-6 of the tensor's largest
    gradient entry."""
    model, oa, _ = _model("tiny")
    model = copy.deepcopy(model).double()
    pixels = _pixels(oa, 3).double()
    tower = tower_train.VisionTower(model, attention="torch", elementwise="torch")
    g = torch.Generator().manual_seed(11)
    probe = torch.randn(3, oa["embed_dim"], generator=g, dtype=torch.float64)
    f = lambda: (tower(pixels) * probe).sum()                            # noqa: E731
    params = tower.named_vision_parameters()
    assert all(p.requires_grad and p.dtype == torch.float64 for p in params.values())
    assert set(params) == {k for k in model.state_dict() if k.startswith("visual.")}
    f().backward()
    h, worst = 1e-6, 0.0
    for pname, p in params.items():
        grad = p.grad.reshape(-1)
        assert bool(torch.isfinite(grad).all()) and float(grad.abs().max()) > 0, pname
        picks = set(grad.abs().topk(min(2, grad.numel())).indices.tolist()) | set(torch.randint(0, grad.numel(), (2,), generator=g).tolist())
        flat = p.data.view(-1)
        for i in picks:
            keep = float(flat[i])
            with torch.no_grad():
                flat[i] = keep + h
                up = float(f())
                flat[i] = keep - h
                down = float(f())
                flat[i] = keep
            err = abs((up - down) / (2 * h) - float(grad[i])) / float(grad.abs().max())
            worst = max(worst, err)
            assert err <= 1e-6, (pname, i, err)
    print(f"vision_tower_tiny_finite_difference_worst {worst:.3e}")
    # no text parameter takes part in the graph
    assert all(p.grad is None for k, p in model.named_parameters() if not k.startswith("visual."))


def test_refusals():
    with pytest.raises(ValueError, match="heads of 64"):
        tower_train.VisionTower(clip_module.build_model("tiny-h", device="cpu"), attention="torch", elementwise="torch")
    with pytest.raises(ValueError, match="siglip"):
        tower_train.VisionTower(clip_module.build_model("tiny-siglip", device="cpu"), attention="torch", elementwise="torch")

    class Bert(torch.nn.Module):
        arch = config.BertArch(256, 2, vocab=1024, ctx=512)
    with pytest.raises(ValueError, match="bert"):
        tower_train.VisionTower(Bert(), attention="torch", elementwise="torch")
    big = clip_module.build_model(config.ClipArch(128, 192, 8, 256, 1, 256, 1, vocab=512, ctx=16), device="cpu")      # 24 x 24 + 1 tokens
    with pytest.raises(ValueError, match="577 tokens"):
        tower_train.VisionTower(big, attention="torch", elementwise="torch")
    model, oa, _ = _model("tiny")
    with pytest.raises(ValueError, match="attention"):
        tower_train.VisionTower(model, attention="sdpa")
    with pytest.raises(ValueError, match="elementwise"):
        tower_train.VisionTower(model, elementwise="fused")
    with pytest.raises(ValueError, match="autocast"):
        tower_train.VisionTower(model, attention="torch", elementwise="op", autocast=False)
    with pytest.raises(ValueError, match="autocast"):
        tower_train.TextTower(model, attention="torch", elementwise="op", autocast=False)
    for kw in ({"attention": "op", "elementwise": "torch"}, {"attention": "torch", "elementwise": "op"}, {}):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            tower_train.VisionTower(model, **kw)(_pixels(oa, 1))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tower_train.TextTower(model, attention="torch", elementwise="op")(torch.ones(1, oa["ctx"], dtype=torch.int32))
    with pytest.raises(ValueError, match="pixels must be"):
        tower_train.VisionTower(model, attention="torch", elementwise="torch")(torch.zeros(1, 3, 16, 16))
    assert tower_train.TextTower(model, attention="torch").elementwise == "torch"          # the text tower's default stays


def test_end_to_end_tuning_trains_everything_but_logit_scale():
    model, oa, _ = _model("tiny")
    tune = tower_train.EndToEndTuning(model, attention="torch", elementwise="torch")
    trainable = {k for k, p in model.named_parameters() if p.requires_grad}
    assert trainable == {k for k, _ in model.named_parameters()} - {"logit_scale"}
    ids = torch.zeros(4, oa["ctx"], dtype=torch.int32)
    ids[:, 0], ids[:, 5] = oa["vocab"] - 2, oa["vocab"] - 1
    out = tune(_pixels(oa, 2), ids[:2], ids[2:])
    assert [tuple(o.shape) for o in out] == [(2, oa["embed_dim"])] * 3
    sum(o.sum() for o in out).backward()
    assert all((p.grad is not None) == (k != "logit_scale") for k, p in model.named_parameters())
    with pytest.raises(ValueError, match="activations of a whole split"):
        tower_train.EndToEndTrainer(model, tune, (_pixels(oa, 2), ids[:2], ids[2:]), None, None, batch_size=0)


def test_cache_pixels_collects_host_rows():
    from test_finetune_gpu import tiny_tokenize
    from knowledge_enhanced_multimodal_retrieval_amd import datasets
    model, oa, _ = _model("tiny")
    ds = datasets.SyntheticRetrievalDataset(10, model.arch.image_size, 42)
    px, q, t = finetune.cache_pixels(model, ds, batch_size=4, tokenize_fn=tiny_tokenize)
    assert tuple(px.shape) == (10, 3, 32, 32) and px.dtype == torch.float32 and px.device.type == "cpu"
    for r, col in ((q, 1), (t, 2)):
        assert r.dtype == torch.int32 and r.device.type == "cpu" and torch.equal(r, tiny_tokenize([ds[i][col] for i in range(10)]))
    assert torch.equal(px[3], ds[3][0].float())


def test_cli_surface(capsys):
    from src.clip.train import trainer as shim
    parser = shim.build_parser()
    assert "end_to_end" in {a.dest for a in parser._actions}
    base = ["--output_dir", "o", "--experiment_name", "e"]
    # the reference's train.sh line with the flag added: parsed with the reference's defaults
    args = parser.parse_args(base + ["--model_name", "ViT-L/14", "--batch_size", "64", "--mixed_precision", "--end_to_end"])
    assert args.end_to_end is True and args.freeze_encoders is False and args.lock_image_tower is False and args.mixed_precision is True
    assert (args.lr, args.weight_decay, args.temperature, args.num_epochs, args.grad_clip, args.gradient_accumulation_steps,
            args.early_stopping_patience, args.seed) == (1e-5, 0.01, 0.07, 20, 1.0, 1, 5, 42)
    for other in ("--freeze_encoders", "--lock_image_tower"):
        with pytest.raises(SystemExit) as e:                              # two modes: a parser error
            shim.main(base + ["--end_to_end", other])
        assert e.value.code == 2 and "not allowed with" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:                                  # the whole split as one batch: refused before anything is loaded
        shim.main(base + ["--end_to_end", "--batch_size", "0"])
    err = capsys.readouterr().err
    assert e.value.code == 2 and "--end_to_end" in err and "activations of a whole split" in err
    assert shim.main(base) == 2                                           # no mode: the refusal as it was
    assert capsys.readouterr().err == f"error: {finetune.NOT_SERVED}\n"
    assert shim.EndToEndTrainer is tower_train.EndToEndTrainer and shim.VisionTower is tower_train.VisionTower
