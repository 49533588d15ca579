"""CPU: the fusion-head training path without a GPU -- tests/pairhead_ref.py (the fp64 statement the GPU tests compare against) held to
fp64 torch autograd through the dense formulation and to the goldens of the reference's own head classes
(tests/golden/fusion_train_golden.npz, make_golden_fusion_train.py); the pairhead entry points' host-side refusals and workspace
formula; the CLI's argument surface and refusals; the batch schedule; the checkpoint's keys and round trip."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import pairhead_ref as PR
from fusion_train_cases import HEADS, dense_scores, make_model, symmetric_cross_entropy, triplet
from knowledge_enhanced_multimodal_retrieval_amd import _lib, fusion_train, losses
from knowledge_enhanced_multimodal_retrieval_amd.finetune import batch_schedule, build_optimizer
from knowledge_enhanced_multimodal_retrieval_amd.fusion_model import FusionModel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GATED, LINEAR = _lib.PAIRHEAD_GATED, _lib.PAIRHEAD_LINEAR
REFUSED = {"bilinear": ("dL/dS contracted with the gallery", "1280"), "cross_attention": ("backward pass through the pair kernel",)}


def _close(a, b, rel=1e-10):
    a, b = torch.as_tensor(a, dtype=torch.float64).reshape(-1), torch.as_tensor(b, dtype=torch.float64).reshape(-1)
    scale = max(float(b.abs().max()), 1e-300)
    return float((a - b).abs().max()) <= rel * scale


def _ref_inputs(fm64, q):
    """(mode, gate, linear) in fp64 from a double head."""
    h = fm64.fusion_head
    if fm64.fusion_type == "linear":
        f = h.fusion
        return LINEAR, None, (f[0].weight.detach(), f[0].bias.detach(), f[3].weight.detach().reshape(-1), f[3].bias.detach())
    return GATED, h.gate(q).detach().reshape(-1), None


def _param_grads_from_ref(fm64, q, ref):
    """The statement's gradient as {parameter name: tensor}: linear directly; the gated heads through autograd of their gate()."""
    h = fm64.fusion_head
    if fm64.fusion_type == "linear":
        dw0, db0, dw1, db1 = PR.split_linear_grad(ref["grad"], h.fusion[0].bias.numel())
        return {"fusion.0.weight": dw0, "fusion.0.bias": db0, "fusion.3.weight": dw1.reshape(1, -1), "fusion.3.bias": db1}
    for p in h.parameters():
        p.grad = None
    h.gate(q).reshape(-1).backward(ref["grad"])
    return {k: p.grad.clone() for k, p in h.named_parameters()}


@pytest.mark.parametrize("fusion_type", HEADS)
@pytest.mark.parametrize("n", [1, 2, 33])
def test_the_fp64_statement_equals_torch_autograd_through_the_dense_formulation(fusion_type, n):
    d, t = 16, 0.07
    fm = make_model(fusion_type, d, seed=3).double()
    q, img, tgt = triplet(n, d, seed=n, dtype=torch.float64)
    loss, l_q2g, l_g2q = symmetric_cross_entropy(dense_scores(fm.fusion_head, fusion_type, q, img, tgt), t)
    loss.backward()
    auto = {k: p.grad.clone() for k, p in fm.fusion_head.named_parameters()}
    mode, gate, linear = _ref_inputs(fm, q)
    ref = PR.pairhead(mode, q, img, tgt, t, gate, linear)
    assert _close(ref["loss"], loss.detach()) and _close(ref["loss_q2g"], l_q2g.detach()) and _close(ref["loss_g2q"], l_g2q.detach())
    got = _param_grads_from_ref(fm, q, ref)
    assert sorted(got) == sorted(auto)
    scale = max(float(g.abs().max()) for g in auto.values())
    for k in auto:
        assert float((got[k] - auto[k]).abs().max()) <= 1e-10 * max(scale, 1e-300), k
    if n == 1:
        assert float(ref["loss"]) == 0.0 and not bool(ref["grad"].any())


def _golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "fusion_train_golden.npz"))


def golden_model(g, fusion_type):
    """A double FusionModel holding the golden's parameters (strict load: the reference's key names)."""
    fm = FusionModel(torch.nn.Linear(1, 1), fusion_type=fusion_type, embed_dim=64).double()
    prefix = f"{fusion_type}_param_"
    fm.fusion_head.load_state_dict({k[len(prefix):]: torch.from_numpy(g[k]) for k in g.files if k.startswith(prefix)})
    return fm.eval()


@pytest.mark.parametrize("fusion_type", HEADS)
def test_the_fp64_statement_matches_the_reference_heads_goldens(fusion_type):
    g = _golden()
    q, img, tgt = [torch.from_numpy(g[k]) for k in ("query", "image", "target")]
    assert q.shape == (48, 64) and q.dtype == torch.float64 and float(g["temperature"]) == 0.07
    fm = golden_model(g, fusion_type)
    mode, gate, linear = _ref_inputs(fm, q)
    ref = PR.pairhead(mode, q, img, tgt, 0.07, gate, linear)
    for k in ("loss", "loss_q2g", "loss_g2q"):
        assert _close(ref[k], float(g[f"{fusion_type}_{k}"])), k
    got = _param_grads_from_ref(fm, q, ref)
    names = [k[len(fusion_type) + 6:] for k in g.files if k.startswith(f"{fusion_type}_grad_")]
    assert sorted(names) == sorted(got)
    scale = max(float(np.abs(g[f"{fusion_type}_grad_{k}"]).max()) for k in names)
    assert scale > 0
    for k in names:
        assert float((got[k] - torch.from_numpy(g[f"{fusion_type}_grad_{k}"])).abs().max()) <= 1e-10 * scale, k


def test_the_budget_is_positive_and_small_against_the_loss():
    q, img, tgt = triplet(48, 64, seed=1)
    for mode, gate, linear in ((GATED, torch.sigmoid(torch.randn(48, generator=torch.Generator().manual_seed(1))), None),
                               (LINEAR, None, tuple(x.float() for x in _ref_inputs(make_model("linear", 64, 1).double(), q.double())[2]))):
        ref = PR.pairhead(mode, q, img, tgt, 0.07, gate, linear)
        bud = PR.budget(mode, q, img, tgt, 0.07, gate, linear, ref)
        assert 0 < float(bud["loss"]) < 0.05 * float(ref["loss"]) and bool((bud["lse_rows"] > 0).all())
        assert bool((bud["grad"] >= 0).all()) and float(bud["grad"].max()) > 0          # a unit that is never active has gradient 0, exactly


# ------------------------------------------------------------------------------------------------ ABI
def _formula(mode, n, d, hidden):
    """include/kemr.h, restated."""
    up = lambda x, m: (x + m - 1) // m * m                      # noqa: E731
    n256, dpad = up(n, 256), up(d, 64)
    tiles = (n + 127) // 128
    per = -(-tiles // min(tiles, 16))
    chunks = -(-tiles // per)
    back = n * 16 * 4 if mode == GATED else tiles * chunks * (4 * hidden + 1) * 4
    terms = [n256 * 2 * dpad * 2] * 3 + [2 * n * 16 * 2 * 4, 2 * n * 4, 2 * n * 4, back]
    return sum(up(t, 256) for t in terms)


def test_workspace_query_is_the_headers_formula_and_zero_for_invalid_shapes():
    ws = _lib.lib().kemr_pairhead_workspace_bytes
    for n, d in ((1, 4), (64, 64), (129, 100), (257, 768), (2100, 64), (32768, 768), (65536, 1280)):
        assert ws(GATED, n, d, 0) == _formula(GATED, n, d, 0), (n, d)
        for hidden in (1, 128, 256):
            assert ws(LINEAR, n, d, hidden) == _formula(LINEAR, n, d, hidden), (n, d, hidden)
    assert ws(LINEAR, 65536, 1280, 256) < 2 ** 31                # O(n d + workgroups hidden), nowhere near n^2
    for mode, n, d, hidden in ((GATED, 0, 64, 0), (GATED, 65537, 64, 0), (GATED, 64, 6, 0), (GATED, 64, 1284, 0), (LINEAR, 64, 64, 0),
                               (LINEAR, 64, 64, 257), (2, 64, 64, 8), (-1, 64, 64, 8), (LINEAR, 0, 64, 8), (LINEAR, 64, 6, 8)):
        assert ws(mode, n, d, hidden) == 0, (mode, n, d, hidden)


@pytest.mark.parametrize("mode", [GATED, LINEAR])
@pytest.mark.parametrize("entry", ["forward", "backward"])
def test_arguments_are_refused_on_the_host_before_any_launch(entry, mode):
    """No GPU here: every call below must return before it touches the device.  The pointers are never dereferenced."""
    lib = _lib.lib()
    p = lambda v=4096: C.c_void_p(v)                             # noqa: E731
    hid = 8 if mode == LINEAR else 0
    need = lib.kemr_pairhead_workspace_bytes(mode, 64, 64, hid)
    assert need > 0

    def call(mode=mode, q=p(), img=p(), tgt=p(), n=64, d=64, inv_t=1.0 / 0.07, gate=p(), w0=p(), b0=p(), w1=p(), b1=p(), hidden=hid,
             o1=p(), o2=p(), lse=p(), ws=p(), ws_bytes=need):
        if entry == "forward":
            return lib.kemr_pairhead_forward(mode, q, img, tgt, n, d, inv_t, gate, w0, b0, w1, b1, hidden, o1, o2, ws, ws_bytes, None)
        return lib.kemr_pairhead_backward(mode, q, img, tgt, lse, n, d, inv_t, gate, w0, b0, w1, b1, hidden, o1, ws, ws_bytes, None)

    cases = [(dict(n=0), -1, "n=0"), (dict(n=65537), -1, "n=65537"), (dict(d=6), -1, "d=6"), (dict(d=1284), -1, "d=1284"),
             (dict(mode=2), -1, "mode=2"), (dict(mode=-1), -1, "mode=-1"),
             (dict(inv_t=0.0), -1, "inv_temperature"), (dict(inv_t=float("nan")), -1, "inv_temperature"),
             (dict(q=None), -1, "q_dev"), (dict(img=None), -1, "img_dev"), (dict(tgt=None), -1, "tgt_dev"),
             (dict(o1=None), -1, "loss_dev" if entry == "forward" else "grad_dev"),
             (dict(ws=None), -4, "workspace"), (dict(ws_bytes=need - 1), -4, "workspace"), (dict(ws=p(4096 + 128)), -4, "256-byte aligned")]
    if entry == "forward":
        cases.append((dict(o2=None), -1, "lse_dev"))
    else:
        cases.append((dict(lse=None), -1, "lse_dev"))
    if mode == GATED:
        cases.append((dict(gate=None), -1, "gate_dev"))
    else:
        cases += [(dict(hidden=0), -1, "hidden=0"), (dict(hidden=257), -1, "hidden=257"), (dict(w0=None), -1, "w0_dev"),
                  (dict(b0=None), -1, "b0_dev"), (dict(w1=None), -1, "w1_dev"), (dict(b1=None), -1, "b1_dev")]
    for kw, status, word in cases:
        assert call(**kw) == status, kw
        msg = lib.kemr_last_error().decode()
        assert msg.startswith(f"pairhead_{entry}:") and word in msg, (kw, msg)
    # the pointers the mode does not read may be NULL: the call gets past the checks only with a workspace, so take that away
    unused = dict(w0=None, b0=None, w1=None, b1=None) if mode == GATED else dict(gate=None)
    assert call(ws=None, **unused) == -4


# ------------------------------------------------------------------------------------------------ loss module, CLI, trainer plumbing
@pytest.mark.parametrize("fusion_type", sorted(REFUSED))
def test_untrained_heads_are_refused_with_the_reason(fusion_type, capsys, tmp_path):
    with pytest.raises(ValueError) as e:
        losses.fusion_train_mode(fusion_type)
    assert all(w in str(e.value) for w in REFUSED[fusion_type])
    fm = FusionModel(torch.nn.Linear(1, 1), fusion_type=fusion_type, embed_dim=64)
    x = torch.zeros(4, 64)
    with pytest.raises(ValueError) as e:
        losses.FusionContrastiveLoss()(fm, x, x, x)
    assert all(w in str(e.value) for w in REFUSED[fusion_type])
    assert fusion_train.main(["--fusion_type", fusion_type, "--output_dir", str(tmp_path / "out"), "--synthetic", "8"]) == 2
    err = capsys.readouterr().err
    assert all(w in err for w in REFUSED[fusion_type])
    assert not (tmp_path / "out").exists()


def test_cpu_inputs_are_refused():
    fm = make_model("simple_gated", 64, seed=1)
    q, img, tgt = triplet(8, 64, seed=1)
    with pytest.raises(ValueError, match="no CPU path"):
        losses.FusionContrastiveLoss()(fm, q, img, tgt)
    assert losses.FusionContrastiveLoss().temperature == 0.07
    assert sorted(losses.FUSION_TRAIN_MODES) == sorted(HEADS)


def test_cli_argument_surface():
    from src.clip.train import train_fusion as shim
    assert shim.main is fusion_train.main and shim.build_parser is fusion_train.build_parser
    parser = fusion_train.build_parser()
    args = parser.parse_args(["--fusion_type", "gated", "--output_dir", "o"])
    assert (args.batch_size, args.num_epochs, args.temperature, args.grad_clip, args.early_stopping_patience, args.seed, args.synthetic) == \
        (0, 20, 0.07, 1.0, 5, 42, 0)
    assert args.model_name == "ViT-L/14" and args.clip_checkpoint is None and args.dataset == "xuemduan/reevaluate-image-text-pairs"
    args = parser.parse_args(["--model_name", "ViT-B/32", "--clip_checkpoint", "c.pt", "--fusion_type", "linear", "--output_dir", "o",
                              "--synthetic", "96", "--batch_size", "32", "--num_epochs", "3", "--lr", "0.01", "--weight_decay", "0.0",
                              "--temperature", "0.05", "--grad_clip", "0", "--early_stopping_patience", "2", "--seed", "7"])
    assert (args.batch_size, args.num_epochs, args.lr, args.weight_decay, args.temperature, args.grad_clip, args.early_stopping_patience,
            args.seed, args.synthetic, args.clip_checkpoint) == (32, 3, 0.01, 0.0, 0.05, 0.0, 2, 7, 96, "c.pt")
    for bad in (["--output_dir", "o"], ["--fusion_type", "gated"], ["--fusion_type", "nope", "--output_dir", "o"]):
        with pytest.raises(SystemExit):
            parser.parse_args(bad)
    # the evaluator's model and data arguments are all accepted
    from knowledge_enhanced_multimodal_retrieval_amd.evaluators import fusion_parser
    mine = {a.dest for a in parser._actions}
    for dest in ("model_name", "tokenizer_dir", "clip_checkpoint", "fusion_checkpoint", "fusion_type", "images_dir", "texts_dir", "splits_file",
                 "max_text_length", "device", "synthetic", "dataset"):
        assert dest in mine and dest in {a.dest for a in fusion_parser()._actions}, dest


def test_the_batch_schedule_is_deterministic_in_the_seed():
    a = batch_schedule(100, 32, torch.Generator().manual_seed(5))
    b = batch_schedule(100, 32, torch.Generator().manual_seed(5))
    c = batch_schedule(100, 32, torch.Generator().manual_seed(6))
    assert len(a) == 3 and all(len(x) == 32 for x in a)                       # the incomplete last batch is dropped
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and not all(torch.equal(x, y) for x, y in zip(a, c))
    assert len(torch.cat(a).unique()) == 96
    whole = batch_schedule(100, 0, torch.Generator().manual_seed(5))
    assert len(whole) == 1 and sorted(whole[0].tolist()) == list(range(100))


@pytest.mark.parametrize("fusion_type", HEADS)
def test_the_checkpoint_has_the_stated_keys_and_round_trips(fusion_type, tmp_path):
    fm = make_model(fusion_type, 64, seed=9)
    opt, _ = build_optimizer(fm.fusion_head, 1e-3, 0.01, 4)
    ckpt = fusion_train.checkpoint_dict(fm, 64, 3, 12.5, opt)
    assert tuple(ckpt) == fusion_train.CHECKPOINT_KEYS == ("fusion_head_state_dict", "fusion_type", "embed_dim", "epoch", "best_metric",
                                                           "optimizer_state_dict")
    assert (ckpt["fusion_type"], ckpt["embed_dim"], ckpt["epoch"], ckpt["best_metric"]) == (fusion_type, 64, 3, 12.5)
    path = tmp_path / "fusion_best.pt"
    torch.save(ckpt, str(path))
    back = torch.load(str(path), map_location="cpu", weights_only=True)           # as evaluators.main_fusion loads it
    fresh = FusionModel(torch.nn.Linear(1, 1), fusion_type=fusion_type, embed_dim=64)
    fresh.fusion_head.load_state_dict(back["fusion_head_state_dict"])
    for (k, a), (_, b) in zip(fm.fusion_head.state_dict().items(), fresh.fusion_head.state_dict().items()):
        assert torch.equal(a, b), k
    assert all(v.device.type == "cpu" for v in back["fusion_head_state_dict"].values())
