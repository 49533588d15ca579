"""CPU (attention="torch"): the differentiable text tower of tower_train.py against the fp32 oracle, its gradient against fp64 finite
differences, the running length, the refusals, and the CLI surface of --lock_image_tower."""
import copy
import warnings

import pytest
import torch

import longclip_ref as LC
from knowledge_enhanced_multimodal_retrieval_amd import clip_model, clip_module, config, finetune, tower_train
from oracle import clip_ref

COS_BAR = 1e-6


def _model(name, seed=0):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m, _ = clip_model.load_clip_model(name, None, "cpu")
    oa = config.get_arch(name).cfg_dict()
    sd = clip_ref.random_state_dict(oa, seed=seed)          # LayerNorm gains and biases that are not 1 and 0
    m.load_state_dict(sd)
    return m.float(), oa, sd


def _ids(oa, lens, seed=3):
    g = torch.Generator().manual_seed(seed)
    ids = torch.zeros(len(lens), oa["ctx"], dtype=torch.int32)
    for i, n in enumerate(lens):
        row = torch.randint(1, oa["vocab"] - 2, (n,), generator=g, dtype=torch.int32)
        row[0], row[-1] = oa["vocab"] - 2, oa["vocab"] - 1
        ids[i, :n] = row
    return ids


CASES = {"tiny": [1, 2, 7, 16, 11], "tiny-ctx248": [1, 17, 77, 129, 248, 200]}
SHORT = {"tiny": [1, 2, 7, 5], "tiny-ctx248": [1, 17, 33, 5]}          # texts that end well before the context does


@pytest.mark.parametrize("name", list(CASES))
def test_fp32_embeddings_match_the_oracle(name):
    model, oa, sd = _model(name)
    ids = _ids(oa, CASES[name])
    tower = tower_train.TextTower(model, attention="torch")
    assert tower.autocast is False
    with torch.no_grad():
        got = tower(ids)
    want = clip_ref.l2_normalize(clip_ref.encode_text(sd, oa, ids))
    miss = float(LC.one_minus_cos(got, want).max())
    print(f"text_tower_{name}_fp32_one_minus_cos {miss:.3e}")
    assert miss <= COS_BAR and float((got.norm(dim=-1) - 1).abs().max()) < 1e-5
    # the pooled row is the one the served tower hands to ln_final
    with torch.no_grad():
        pooled = tower.pooled(ids)
    hidden = clip_ref.encode_text(sd, oa, ids, return_hidden=True)[torch.arange(len(ids)), ids.long().argmax(-1)]
    assert float((pooled - hidden).abs().max()) <= 1e-4 * float(hidden.abs().max())


@pytest.mark.parametrize("name", list(CASES))
def test_running_at_the_longest_text_gives_the_same_embeddings(name):
    model, oa, _ = _model(name)
    ids = _ids(oa, SHORT[name])
    t = tower_train.longest(ids)
    assert t == max(SHORT[name]) < oa["ctx"]
    for m, bar in ((model, 1e-6), (copy.deepcopy(model).double(), 1e-12)):
        tower = tower_train.TextTower(m, attention="torch")
        with torch.no_grad():
            full, short = tower(ids), tower(ids, t)
        assert float((full - short).abs().max()) <= bar
    with pytest.raises(ValueError, match="cuts a text"):
        tower(ids, t - 1)
    with pytest.raises(ValueError, match="outside"):
        tower(ids, 0)


@pytest.mark.parametrize("name", list(CASES))
def test_gradient_against_fp64_finite_differences(name):
    """Central differences at h = 1e-6 on an fp64 copy: truncation ~ h^2 f''' and rounding ~ 2^-53 |f| / h are both below 1e-8 of the
    gradient scale here; the bar is 1e-6 of the tensor's largest gradient entry."""
    model, oa, _ = _model(name)
    model = copy.deepcopy(model).double()
    ids = _ids(oa, SHORT[name])
    t = tower_train.longest(ids)
    tower = tower_train.TextTower(model, attention="torch")
    g = torch.Generator().manual_seed(11)
    probe = torch.randn(len(ids), oa["embed_dim"], generator=g, dtype=torch.float64)
    f = lambda: (tower(ids, t) * probe).sum()                            # noqa: E731
    params = tower.named_text_parameters()
    assert all(p.requires_grad and p.dtype == torch.float64 for p in params.values())
    assert set(params) == {k for k in model.state_dict() if not k.startswith("visual.") and k != "logit_scale"}
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
    print(f"text_tower_{name}_finite_difference_worst {worst:.3e}")
    # no vision parameter takes part in the graph
    assert all(p.grad is None for k, p in model.named_parameters() if k.startswith("visual."))


def test_exact_gelu_models_use_exact_gelu():
    model, oa, _ = _model("tiny")
    ids = _ids(oa, [5, 9])
    quick = tower_train.TextTower(model, attention="torch")
    model.activation = "gelu"
    exact = tower_train.TextTower(model, attention="torch")
    with torch.no_grad():
        assert exact.activation == "gelu" and float((quick(ids) - exact(ids)).abs().max()) > 1e-4


def test_siglip_and_bert_models_and_the_op_on_the_cpu_are_refused():
    sig = clip_module.build_model("tiny-siglip", device="cpu")
    with pytest.raises(ValueError, match="siglip"):
        tower_train.TextTower(sig, attention="torch")

    class Bert(torch.nn.Module):
        arch = config.BertArch(256, 2, vocab=1024, ctx=512)
    with pytest.raises(ValueError, match="bert"):
        tower_train.TextTower(Bert(), attention="torch")
    model, oa, _ = _model("tiny")
    with pytest.raises(ValueError, match="attention"):
        tower_train.TextTower(model, attention="sdpa")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tower_train.TextTower(model, attention="op")(_ids(oa, [4]))


def test_locked_image_tuning_trains_the_heads_and_the_text_tower_only():
    model, oa, _ = _model("tiny")
    tune = tower_train.LockedImageTuning(model, attention="torch")
    trainable = {k for k, p in model.named_parameters() if p.requires_grad}
    text = {k for k in model.state_dict() if not k.startswith("visual.") and k != "logit_scale"}
    assert trainable == text | {"visual.ln_post.weight", "visual.ln_post.bias", "visual.proj"}
    ids = _ids(oa, [4, 9, 16, 3])
    img = torch.randn(2, oa["v_width"], generator=torch.Generator().manual_seed(1))
    out = tune(img, ids[:2], ids[2:])
    assert [tuple(o.shape) for o in out] == [(2, oa["embed_dim"])] * 3
    sum(o.sum() for o in out).backward()
    assert all((p.grad is not None) == (k in trainable) for k, p in model.named_parameters())
    with pytest.raises(ValueError, match="activations of a whole split"):
        tower_train.TextTowerTrainer(model, tune, (img, ids[:2], ids[2:]), None, None, batch_size=0)


def test_cli_surface(capsys):
    from src.clip.train import trainer as shim
    parser = shim.build_parser()
    assert "lock_image_tower" in {a.dest for a in parser._actions}
    base = ["--output_dir", "o", "--experiment_name", "e"]
    args = parser.parse_args(base + ["--lock_image_tower", "--mixed_precision"])
    assert args.lock_image_tower is True and args.freeze_encoders is False and args.mixed_precision is True
    with pytest.raises(SystemExit) as e:                                  # both flags: a parser error
        shim.main(base + ["--lock_image_tower", "--freeze_encoders"])
    assert e.value.code == 2 and "not allowed with" in capsys.readouterr().err
    assert shim.main(base) == 2                                           # neither: the refusal as it was, word for word
    assert capsys.readouterr().err == f"error: {finetune.NOT_SERVED}\n"
    assert finetune.NOT_SERVED == ("end-to-end fine-tuning is not served: there is no backward pass through the towers. Pass "
                                   "--freeze_encoders to train the projection heads (visual.ln_post, visual.proj, ln_final, "
                                   "text_projection) on frozen towers.")
    with pytest.raises(SystemExit) as e:                                  # the whole split as one batch: refused before anything is loaded
        shim.main(base + ["--lock_image_tower", "--batch_size", "0"])
    assert e.value.code == 2 and "activations of a whole split" in capsys.readouterr().err
