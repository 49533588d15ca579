"""CPU (attention="torch"): ``TextTower(packed=True)`` of tower_train.py -- every text computed up to its own end-of-text token on
packed rows -- against the fp32 oracle, against the dense tower in fp64 (embeddings and every text parameter's gradient), its refusals,
and the CLI surface of --packed_texts.  Models, length sets and bars are those of tests/test_text_tower_train_host.py."""
import copy

import pytest
import torch

import longclip_ref as LC
from knowledge_enhanced_multimodal_retrieval_amd import finetune, tower_train
from oracle import clip_ref
from test_text_tower_train_host import CASES, COS_BAR, SHORT, _ids, _model

GRAD_BAR = 9.3e-15          # 10 x the worst measured (below); the issue's ceiling for it is 1e-9


@pytest.mark.parametrize("name", list(CASES))
def test_packed_fp32_embeddings_match_the_oracle(name):
    model, oa, sd = _model(name)
    ids = _ids(oa, CASES[name])
    tower = tower_train.TextTower(model, attention="torch", packed=True)
    assert tower.packed is True and tower.autocast is False
    with torch.no_grad():
        got = tower(ids)
    want = clip_ref.l2_normalize(clip_ref.encode_text(sd, oa, ids))
    miss = float(LC.one_minus_cos(got, want).max())
    print(f"text_tower_packed_{name}_fp32_one_minus_cos {miss:.3e}")
    assert miss <= COS_BAR and float((got.norm(dim=-1) - 1).abs().max()) < 1e-5


@pytest.mark.parametrize("lens", [CASES, SHORT], ids=["full", "short"])
@pytest.mark.parametrize("name", list(CASES))
def test_packed_fp64_embeddings_are_the_dense_ones(name, lens):
    model, oa, _ = _model(name)
    model = copy.deepcopy(model).double()
    ids = _ids(oa, lens[name])
    with torch.no_grad():
        dense = tower_train.TextTower(model, attention="torch")(ids)
        packed = tower_train.TextTower(model, attention="torch", packed=True)(ids)
    worst = float((dense - packed).abs().max())
    print(f"text_tower_packed_{name}_fp64_max_abs {worst:.3e}")
    assert packed.dtype == torch.float64 and worst <= 1e-12


@pytest.mark.parametrize("name", list(CASES))
def test_packed_fp64_gradients_are_the_dense_ones(name):
    """Every text parameter's gradient of (emb * probe).sum(), packed against dense, in fp64: the same mathematics on the same rows,
    so what is left is the summation order of fp64 sums.  Measured worst relative L2 when this test was written: tiny 6.5e-16,
    tiny-ctx248 9.2e-16.  The bar is 10 x the worst of the two, 9.3e-15 (the rule allows nothing looser than 1e-9; this is far
    inside it): one mis-gathered row of a batch would show at 1e-10 and above."""
    model, oa, _ = _model(name)
    model = copy.deepcopy(model).double()
    ids = _ids(oa, CASES[name])
    probe = torch.randn(len(ids), oa["embed_dim"], generator=torch.Generator().manual_seed(11), dtype=torch.float64)

    def grads(packed):
        tower = tower_train.TextTower(model, attention="torch", packed=packed)
        for p in tower.parameters():
            p.grad = None
        (tower(ids) * probe).sum().backward()
        return {k: p.grad.detach().clone() for k, p in tower.named_text_parameters().items()}

    dense, packed = grads(False), grads(True)
    assert set(dense) == set(packed) == {k for k in model.state_dict() if not k.startswith("visual.") and k != "logit_scale"}
    worst = 0.0
    for k in dense:
        assert bool(torch.isfinite(packed[k]).all()) and float(packed[k].abs().max()) > 0, k
        err = float((packed[k] - dense[k]).norm() / dense[k].norm())
        worst = max(worst, err)
        assert err <= GRAD_BAR, (k, err)
    print(f"text_tower_packed_{name}_fp64_grad_worst_rel_l2 {worst:.3e}")
    assert all(p.grad is None for k, p in model.named_parameters() if k.startswith("visual."))


def test_packed_refusals():
    model, oa, _ = _model("tiny")
    ids = _ids(oa, SHORT["tiny"])
    tower = tower_train.TextTower(model, attention="torch", packed=True)
    with pytest.raises(ValueError, match="no running\\s+length"):
        tower(ids, tower_train.longest(ids))
    with pytest.raises(ValueError, match="ids must be"):
        tower(ids[0])
    with pytest.raises(RuntimeError, match="no CPU fallback"):              # the dense tower's refusals hold here too
        tower_train.TextTower(model, attention="op", packed=True)(ids)
    with pytest.raises(ValueError, match="attention"):
        tower_train.TextTower(model, attention="sdpa", packed=True)
    from knowledge_enhanced_multimodal_retrieval_amd import clip_module
    with pytest.raises(ValueError, match="siglip"):
        tower_train.TextTower(clip_module.build_model("tiny-siglip", device="cpu"), attention="torch", packed=True)


def test_locked_image_tuning_passes_the_setting_on():
    model, oa, _ = _model("tiny")
    ids = _ids(oa, [4, 9, 16, 3])
    img = torch.randn(2, oa["v_width"], generator=torch.Generator().manual_seed(1))
    dense = tower_train.LockedImageTuning(model, attention="torch")
    assert dense.tower.packed is False
    with torch.no_grad():
        want = dense(img, ids[:2], ids[2:])
    tune = tower_train.LockedImageTuning(model, attention="torch", packed=True)
    assert tune.tower.packed is True
    got = tune(img, ids[:2], ids[2:])
    assert all(float((a - b).abs().max()) <= 1e-5 for a, b in zip(got, want))
    sum(o.sum() for o in got).backward()
    trainable = {k for k, p in model.named_parameters() if p.requires_grad}
    assert all((p.grad is not None) == (k in trainable) for k, p in model.named_parameters())
    e2e = tower_train.EndToEndTuning(model, attention="torch", elementwise="torch", packed=True)
    assert e2e.tower.packed is True and tower_train.EndToEndTuning(model, attention="torch", elementwise="torch").tower.packed is False


def test_cli_surface(capsys):
    from src.clip.train import trainer as shim
    parser = shim.build_parser()
    assert "packed_texts" in {a.dest for a in parser._actions}
    base = ["--output_dir", "o", "--experiment_name", "e"]
    assert parser.parse_args(base + ["--lock_image_tower"]).packed_texts is False            # the default is off
    assert parser.parse_args(base + ["--lock_image_tower", "--packed_texts"]).packed_texts is True
    assert parser.parse_args(base + ["--end_to_end", "--packed_texts"]).packed_texts is True
    with pytest.raises(SystemExit) as e:
        shim.main(base + ["--freeze_encoders", "--packed_texts"])
    err = capsys.readouterr().err
    assert e.value.code == 2 and "--packed_texts is not served with --freeze_encoders" in err
    assert finetune.PACKED_TEXTS_REFUSED in err
    assert shim.main(base + ["--packed_texts"]) == 2                       # no mode: the refusal as it was
    assert capsys.readouterr().err == f"error: {finetune.NOT_SERVED}\n"
    with pytest.raises(SystemExit) as e:
        shim.main(["--help"])
    assert e.value.code == 0 and "--packed_texts" in capsys.readouterr().out
