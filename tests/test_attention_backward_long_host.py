"""Host (no GPU): the ABI surface of ``kemr_op_attention_backward_long`` (csrc/attention_bwd_stream.hip) and of its workspace function,
the refusals, and the Python plumbing of the long vision towers' training path: ``VisionTower(max_tokens=...)``, ``EndToEndTuning`` on
the 290-token test architecture, and the plain formulation's gradient at that grid against fp64 finite differences."""
import copy
import ctypes as C
import os
import re
import warnings

import pytest
import torch

from knowledge_enhanced_multimodal_retrieval_amd import _lib, clip_model, clip_module, config, tower_train
from oracle import clip_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEMR_ERR_INVALID = -1
T_MAX = 1025                       # include/kemr.h KEMR_MAX_VISION_TOKENS


def _need(batch, t, width):
    return batch * (width // 64) * t * 3 * 4       # what the header states: fp32 [batch * heads * t, 3]


def test_symbols_are_declared_and_abi_stays_4():
    assert _lib.SIGNATURES["kemr_attention_backward_long_workspace_bytes"] == (C.c_size_t, [C.c_int] * 3)
    assert _lib.SIGNATURES["kemr_op_attention_backward_long"] == (C.c_int, [C.c_void_p] * 3 + [C.c_int] * 3 + [C.c_void_p, C.c_size_t, C.c_void_p])
    header = open(os.path.join(ROOT, "include", "kemr.h")).read()
    assert re.search(r"\bsize_t\s+kemr_attention_backward_long_workspace_bytes\s*\(\s*int batch, int t, int width\);", header)
    assert re.search(r"\bint\s+kemr_op_attention_backward_long\s*\(\s*const void\* qkv_dev, const void\* dout_dev, void\* dqkv_dev, int batch, "
                     r"int t, int width,\s*void\* workspace_dev, size_t workspace_bytes, void\* stream\);", header)
    assert "#define KEMR_ABI_VERSION 4" in header and "Still 4: kemr_attention_backward_long_workspace_bytes" in header
    assert _lib.ABI_VERSION == 4 and _lib.lib().kemr_abi_version() == 4
    assert f"#define KEMR_MAX_VISION_TOKENS {T_MAX}" in header and tower_train.MAX_T_LONG == T_MAX and tower_train.MAX_T == 288


# never dereferenced: every case is refused on the host, before any HIP call
P = C.c_void_p(0x1000)
NULL = C.c_void_p(None)
BIG = 1 << 40


@pytest.mark.parametrize("args,names", [
    ((P, P, P, 2, 0, 128, P, BIG), "t"),
    ((P, P, P, 2, T_MAX + 1, 128, P, BIG), "t"),
    ((P, P, P, 2, 577, 96, P, BIG), "width"),
    ((P, P, P, -1, 577, 128, P, BIG), "batch"),
    ((NULL, P, P, 2, 577, 128, P, BIG), "qkv"),
    ((P, NULL, P, 2, 577, 128, P, BIG), "dout"),
    ((P, P, NULL, 2, 577, 128, P, BIG), "dqkv"),
    ((P, P, P, 2, 577, 128, P, _need(2, 577, 128) - 1), "workspace_bytes"),
    ((P, P, P, 2, 577, 128, NULL, BIG), "workspace"),
    ((P, P, P, 1 << 27, T_MAX, 64, P, BIG), "batch"),          # 2^27 items x 1 head x 17 row blocks > 2^31 - 1 workgroups
], ids=["t=0", "t=1026", "width=96", "batch=-1", "qkv=NULL", "dout=NULL", "dqkv=NULL", "workspace_one_byte_short", "workspace=NULL", "grid"])
def test_refused_on_the_host(args, names):
    L = _lib.lib()
    assert L.kemr_op_attention_backward_long(*args, None) == KEMR_ERR_INVALID
    msg = L.kemr_last_error().decode()
    assert msg.startswith("op_attention_backward_long:") and re.search(rf"\b{names}\b", msg), msg
    with pytest.raises(RuntimeError, match=names):
        _lib.check(L.kemr_op_attention_backward_long(*args, None), "op_attention_backward_long")


def test_workspace_bytes():
    fn = _lib.lib().kemr_attention_backward_long_workspace_bytes
    for batch, t, width in ((1, 1, 64), (3, 17, 128), (3, 289, 128), (2, 577, 1024), (85, 577, 1024), (3, T_MAX, 128)):
        assert fn(batch, t, width) == _need(batch, t, width), (batch, t, width)
    assert fn(0, 577, 1024) == 0
    for bad in ((-1, 577, 1024), (2, 0, 1024), (2, T_MAX + 1, 1024), (2, 577, 96), (2, 577, 0)):
        assert fn(*bad) == 0, bad
    # an exactly sized workspace passes the size check: the next refusal (none is left on the host) would be a launch, so only the
    # empty batch is called here -- it launches nothing and needs no workspace
    assert _lib.lib().kemr_op_attention_backward_long(P, P, P, 0, 577, 128, NULL, 0, None) == 0


# ------------------------------------------------------------------------------------------------ the towers
def _model(name, seed=0):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m, _ = clip_model.load_clip_model(name, None, "cpu")
    oa = config.get_arch(name).cfg_dict()
    m.load_state_dict(clip_ref.random_state_dict(oa, seed=seed))
    return m.float(), oa


def test_vision_tower_max_tokens():
    big = clip_module.build_model(config.ClipArch(128, 192, 8, 256, 1, 256, 1, vocab=512, ctx=16), device="cpu")      # 24 x 24 + 1 tokens
    tower = tower_train.VisionTower(big, attention="torch", elementwise="torch", max_tokens=tower_train.MAX_T_LONG)
    assert tower.tokens == 577 and tower.causal is False
    with pytest.raises(ValueError, match="577 tokens"):                   # the default keeps refusing, with its message
        tower_train.VisionTower(big, attention="torch", elementwise="torch")
    with pytest.raises(ValueError, match="577 tokens"):
        tower_train.VisionTower(big, attention="torch", elementwise="torch", max_tokens=576)
    for bad in (0, 1026):
        with pytest.raises(ValueError, match="max_tokens"):
            tower_train.VisionTower(big, attention="torch", elementwise="torch", max_tokens=bad)


def test_end_to_end_tuning_constructs_on_tiny_290():
    arch = config.get_arch("tiny-290")
    assert arch == config.ClipArch(128, 136, 8, 256, 2, 256, 2, vocab=512, ctx=16) and arch.v_tokens == 290
    model, oa = _model("tiny-290")
    with pytest.raises(ValueError, match="290 tokens"):
        tower_train.VisionTower(model, attention="torch", elementwise="torch")
    tune = tower_train.EndToEndTuning(model, attention="torch", elementwise="torch")
    assert tune.vision.tokens == 290
    assert {k for k, p in model.named_parameters() if p.requires_grad} == {k for k, _ in model.named_parameters()} - {"logit_scale"}
    ids = torch.zeros(2, oa["ctx"], dtype=torch.int32)
    ids[:, 0], ids[:, 5] = oa["vocab"] - 2, oa["vocab"] - 1
    px = torch.randn(1, 3, 136, 136, generator=torch.Generator().manual_seed(1))
    out = tune(px, ids[:1], ids[1:])
    assert [tuple(o.shape) for o in out] == [(1, oa["embed_dim"])] * 3


def test_gradient_against_fp64_finite_differences_at_290_tokens():
    """The check of tests/test_vision_tower_train_host.py (central differences at h = 1e-6 on an fp64 copy, the bar 1e-6 of the tensor's
    largest gradient entry) on a one-block tower with a 17 x 17 grid: the restatement's token and position handling at another grid."""
    arch = config.ClipArch(128, 136, 8, 256, 1, 256, 1, vocab=512, ctx=16)
    model = clip_module.build_model(arch, device="cpu")
    model.load_state_dict(clip_ref.random_state_dict(arch.cfg_dict(), seed=0))
    model = copy.deepcopy(model).double()
    pixels = torch.randn(2, 3, 136, 136, generator=torch.Generator().manual_seed(5)).double()
    tower = tower_train.VisionTower(model, attention="torch", elementwise="torch", max_tokens=tower_train.MAX_T_LONG)
    assert tower.tokens == 290
    g = torch.Generator().manual_seed(11)
    probe = torch.randn(2, arch.embed_dim, generator=g, dtype=torch.float64)
    f = lambda: (tower(pixels) * probe).sum()                            # noqa: E731
    params = tower.named_vision_parameters()
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
    print(f"vision_tower_290_finite_difference_worst {worst:.3e}")
