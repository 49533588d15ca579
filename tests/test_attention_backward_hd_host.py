"""Host (no GPU): the ABI surface of ``kemr_op_attention_backward_hd`` (csrc/attention_bwd80.hip) and of its workspace function, the
refusals, the reference statements of tests/attention_bwd_hd_ref.py, and the Python plumbing of head-dim-80 training:
``VisionTower(head_dims=...)`` and ``EndToEndTuning`` on "tiny-h" (ViT-H-14's structure: width 1280 in 16 heads of 80, 5 tokens), the
tower's fp64 forward against tests/headdim_ref.py and its gradient against fp64 finite differences."""
import copy
import ctypes as C
import os
import re
import warnings

import pytest
import torch

import attention_bwd_hd_ref as RH
import attention_bwd_ref as R
import headdim_ref
from knowledge_enhanced_multimodal_retrieval_amd import _lib, clip_model, clip_module, config, tower_train
from oracle import clip_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEMR_ERR_INVALID = -1
T_MAX = 1025                       # include/kemr.h KEMR_MAX_VISION_TOKENS


def _need(batch, t, width, head_dim=80):
    return batch * (width // head_dim) * t * 12    # what the header states: fp32 [batch * heads * t, 3]


def test_symbols_are_declared_and_abi_stays_4():
    assert _lib.SIGNATURES["kemr_attention_backward_hd_workspace_bytes"] == (C.c_size_t, [C.c_int] * 4)
    assert _lib.SIGNATURES["kemr_op_attention_backward_hd"] == (C.c_int, [C.c_void_p] * 3 + [C.c_int] * 5 + [C.c_void_p, C.c_size_t, C.c_void_p])
    header = open(os.path.join(ROOT, "include", "kemr.h")).read()
    assert re.search(r"\bsize_t\s+kemr_attention_backward_hd_workspace_bytes\s*\(\s*int batch, int t, int width, int head_dim\);", header)
    assert re.search(r"\bint\s+kemr_op_attention_backward_hd\s*\(\s*const void\* qkv_dev, const void\* dout_dev, void\* dqkv_dev, int batch, "
                     r"int t, int width,\s*int head_dim, int causal, void\* workspace_dev, size_t workspace_bytes, void\* stream\);", header)
    assert "#define KEMR_ABI_VERSION 4" in header and "Still 4: kemr_attention_backward_hd_workspace_bytes" in header
    assert _lib.ABI_VERSION == 4 and _lib.lib().kemr_abi_version() == 4
    L = _lib.lib()
    assert L.kemr_attention_backward_hd_workspace_bytes and L.kemr_op_attention_backward_hd
    assert tower_train.HEAD_DIMS == (64, 80)


# never dereferenced: every case is refused on the host, before any HIP call
P = C.c_void_p(0x1000)
NULL = C.c_void_p(None)
BIG = 1 << 40


# (qkv, dout, dqkv, batch, t, width, head_dim, causal, workspace, workspace_bytes)
@pytest.mark.parametrize("args,names", [
    ((P, P, P, 2, 0, 160, 80, 0, P, BIG), "t"),
    ((P, P, P, 2, T_MAX + 1, 160, 80, 0, P, BIG), "t"),
    ((P, P, P, 2, 257, 144, 72, 0, P, BIG), "head_dim"),
    ((P, P, P, 2, 257, 128, 80, 0, P, BIG), "width"),
    ((P, P, P, 2, 257, 160, 80, 2, P, BIG), "causal"),
    ((P, P, P, 2, 257, 160, 80, 1, P, BIG), "causal"),
    ((P, P, P, -1, 257, 160, 80, 0, P, BIG), "batch"),
    ((NULL, P, P, 2, 257, 160, 80, 0, P, BIG), "qkv"),
    ((P, NULL, P, 2, 257, 160, 80, 0, P, BIG), "dout"),
    ((P, P, NULL, 2, 257, 160, 80, 0, P, BIG), "dqkv"),
    ((P, P, P, 2, 257, 160, 80, 0, P, _need(2, 257, 160) - 1), "workspace_bytes"),
    ((P, P, P, 2, 257, 160, 80, 0, NULL, BIG), "workspace"),
    ((P, P, P, 1 << 27, T_MAX, 80, 80, 0, P, BIG), "batch"),       # 2^27 items x 1 head x 17 row blocks > 2^31 - 1 workgroups
], ids=["t=0", "t=1026", "head_dim=72", "width=128", "causal=2", "causal=1_at_80", "batch=-1", "qkv=NULL", "dout=NULL", "dqkv=NULL",
        "workspace_one_byte_short", "workspace=NULL", "grid"])
def test_refused_on_the_host(args, names):
    L = _lib.lib()
    assert L.kemr_op_attention_backward_hd(*args, None) == KEMR_ERR_INVALID
    msg = L.kemr_last_error().decode()
    assert msg.startswith("op_attention_backward_hd:") and re.search(rf"\b{names}\b", msg), msg
    with pytest.raises(RuntimeError, match=names):
        _lib.check(L.kemr_op_attention_backward_hd(*args, None), "op_attention_backward_hd")


def test_misaligned_workspace_is_refused():
    L = _lib.lib()
    assert L.kemr_op_attention_backward_hd(P, P, P, 2, 257, 160, 80, 0, C.c_void_p(0x1002), BIG, None) == KEMR_ERR_INVALID
    msg = L.kemr_last_error().decode()
    assert msg.startswith("op_attention_backward_hd:") and "workspace" in msg and "aligned" in msg, msg


def test_head_dim_64_keeps_the_existing_ops_refusals_and_messages():
    L = _lib.lib()
    assert L.kemr_op_attention_backward_hd(P, P, P, 2, 289, 128, 64, 1, P, BIG, None) == KEMR_ERR_INVALID
    assert L.kemr_last_error().decode() == "op_attention_backward: t = 289 is outside 1..288"
    assert L.kemr_op_attention_backward_hd(P, P, P, 2, 577, 128, 64, 0, NULL, BIG, None) == KEMR_ERR_INVALID
    assert L.kemr_last_error().decode() == "op_attention_backward_long: workspace is NULL"


def test_workspace_bytes():
    fn = _lib.lib().kemr_attention_backward_hd_workspace_bytes
    for batch, t, width in ((1, 1, 80), (3, 17, 160), (2, 257, 1280), (3, T_MAX, 160)):
        assert fn(batch, t, width, 80) == _need(batch, t, width), (batch, t, width)
    assert fn(0, 257, 1280, 80) == 0
    for bad in ((-1, 257, 1280, 80), (2, 0, 1280, 80), (2, T_MAX + 1, 1280, 80), (2, 257, 128, 80), (2, 257, 0, 80), (2, 257, 1280, 72),
                (2, 257, 1280, 0)):
        assert fn(*bad) == 0, bad
    # head dim 64: nothing up to the LDS kernel's 288 rows, the long op's size above
    long_fn = _lib.lib().kemr_attention_backward_long_workspace_bytes
    for t in (1, 257, 288):
        assert fn(3, t, 128, 64) == 0
    for t in (289, 577, T_MAX):
        assert fn(3, t, 128, 64) == long_fn(3, t, 128) == _need(3, t, 128, 64)
    assert fn(3, T_MAX + 1, 128, 64) == 0 and fn(3, 577, 96, 64) == 0 and fn(0, 577, 128, 64) == 0
    # the empty batch launches nothing and needs no workspace
    assert _lib.lib().kemr_op_attention_backward_hd(P, P, P, 0, 257, 160, 80, 0, NULL, 0, None) == 0


# ------------------------------------------------------------------------------------------------ the reference statements
def test_helper_at_64_is_the_existing_reference_bit_for_bit():
    batch, t, width = 3, 65, 128
    qkv, dout = R.make_inputs(batch, t, width, 31, zero_item=1)
    qkv2, dout2 = RH.make_inputs(batch, t, width, 31, 64, zero_item=1)
    assert torch.equal(qkv.view(torch.int16), qkv2.view(torch.int16)) and torch.equal(dout.view(torch.int16), dout2.view(torch.int16))
    a, b = R.backward_fp64(qkv, dout, batch, t, width, 0), RH.backward_fp64(qkv, dout, batch, t, width, 64)
    assert a.dtype == b.dtype == torch.float64 and torch.equal(a.view(torch.int64), b.view(torch.int64))
    a, b = R.backward_emulated(qkv, dout, batch, t, width, 0), RH.backward_emulated(qkv, dout, batch, t, width, 64)
    assert a.dtype == b.dtype == torch.bfloat16 and torch.equal(a.view(torch.int16), b.view(torch.int16))


def test_helper_at_80_is_autograd_through_the_plain_formulation():
    batch, t, width = 2, 37, 160
    qkv, dout = RH.make_inputs(batch, t, width, 5, 80)
    # q is pre-scaled by 80 ** -0.5: its column norm says so (randn columns have unit variance)
    assert abs(float(qkv[:, :width].float().std()) * 80 ** 0.5 - 1) < 0.05 and abs(float(qkv[:, width:].float().std()) - 1) < 0.05
    x = qkv.double().requires_grad_(True)
    q, k, v = (RH.heads_of(x[:, i * width:(i + 1) * width], batch, t, width, 80) for i in range(3))
    out = RH.rows_of(RH.plain_attention(q, k, v), batch, t, width)
    (out * dout.double()).sum().backward()
    want = RH.backward_fp64(qkv, dout, batch, t, width, 80)
    for name in ("dq", "dk", "dv"):
        err = R.rel_l2(R.planes(want, width)[name], R.planes(x.grad, width)[name])
        print(f"attention_bwd_hd_ref 80 {name}: statement against autograd {err:.3e}")
        assert err <= 1e-12, (name, err)
    # the emulation rounds: it is near the statement and not the statement
    emu = RH.backward_emulated(qkv, dout, batch, t, width, 80)
    assert all(0 < R.rel_l2(R.planes(emu, width)[n], R.planes(want, width)[n]) < 1e-2 for n in ("dq", "dk", "dv"))


# ------------------------------------------------------------------------------------------------ the towers
def _model(name, seed=0):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m, _ = clip_model.load_clip_model(name, None, "cpu")
    oa = config.get_arch(name).cfg_dict()
    sd = clip_ref.random_state_dict(oa, seed=seed)
    m.load_state_dict(sd)
    return m.float(), oa, sd


def test_vision_tower_head_dims():
    model, _, _ = _model("tiny-h")
    with pytest.raises(ValueError, match="heads of 64"):                  # the default keeps refusing, with its message
        tower_train.VisionTower(model, attention="torch", elementwise="torch")
    tower = tower_train.VisionTower(model, attention="torch", elementwise="torch", head_dims=tower_train.HEAD_DIMS)
    assert tower.head_dim == 80 and tower.tokens == 5 and tower.width == 1280 and tower.causal is False
    with pytest.raises(ValueError, match="head_dims"):
        tower_train.VisionTower(model, attention="torch", elementwise="torch", head_dims=(64, 72))
    with pytest.raises(ValueError, match="heads of"):                     # opting in to 80 alone does not admit 64
        tower_train.VisionTower(_model("tiny")[0], attention="torch", elementwise="torch", head_dims=(80,))
    # a head-dim-80 tower of more than 288 tokens: 17 x 17 + 1 = 290
    big = clip_module.build_model(config.ClipArch(128, 238, 14, 1280, 1, 256, 1, vocab=512, ctx=16, v_head_dim=80), device="cpu")
    assert big.arch.v_tokens == 290
    with pytest.raises(ValueError, match="288"):
        tower_train.VisionTower(big, attention="torch", elementwise="torch", head_dims=tower_train.HEAD_DIMS, max_tokens=tower_train.MAX_T_LONG)
    with pytest.raises(ValueError, match="288"):
        tower_train.VisionTower(big, attention="torch", elementwise="torch", head_dims=tower_train.HEAD_DIMS)
    # heads of 64 keep their towers and their attention
    assert tower_train.VisionTower(_model("tiny")[0], attention="torch", elementwise="torch", head_dims=tower_train.HEAD_DIMS).head_dim == 64


def test_end_to_end_tuning_constructs_on_tiny_h():
    model, oa, _ = _model("tiny-h")
    tune = tower_train.EndToEndTuning(model, attention="torch", elementwise="torch")
    assert tune.vision.head_dim == 80 and tune.tower.head_dim == 64
    assert {k for k, p in model.named_parameters() if p.requires_grad} == {k for k, _ in model.named_parameters()} - {"logit_scale"}
    ids = torch.zeros(4, oa["ctx"], dtype=torch.int32)
    ids[:, 0], ids[:, 5] = oa["vocab"] - 2, oa["vocab"] - 1
    px = torch.randn(2, 3, 28, 28, generator=torch.Generator().manual_seed(1))
    out = tune(px, ids[:2], ids[2:])
    assert [tuple(o.shape) for o in out] == [(2, oa["embed_dim"])] * 3


def test_fp64_forward_matches_the_head_dim_reference():
    model, oa, sd = _model("tiny-h")
    pixels = torch.randn(3, 3, 28, 28, generator=torch.Generator().manual_seed(5)).double()
    tower = tower_train.VisionTower(copy.deepcopy(model).double(), attention="torch", elementwise="torch", head_dims=tower_train.HEAD_DIMS)
    with torch.no_grad():
        emb = tower(pixels)
    want = torch.nn.functional.normalize(headdim_ref.encode_image(sd, oa, pixels, heads=16, activation=model.activation), dim=-1)
    miss = float((emb - want).abs().max())
    print(f"vision_tower_tiny_h_fp64_embedding_abs {miss:.3e}")
    assert emb.dtype == torch.float64 and miss <= 1e-10
    # sixteen heads of 80 are not twenty of 64
    other = torch.nn.functional.normalize(headdim_ref.encode_image(sd, oa, pixels, heads=20, activation=model.activation), dim=-1)
    assert float((emb - other).abs().max()) > 1e-6


def test_gradient_against_fp64_finite_differences_at_head_dim_80():
    """The check of tests/test_vision_tower_train_host.py (central differences at h = 1e-6 on an fp64 copy, the bar 1e-6 of the tensor's
    largest gradient entry) on "tiny-h"."""
    model, oa, _ = _model("tiny-h")
    model = copy.deepcopy(model).double()
    pixels = torch.randn(2, 3, 28, 28, generator=torch.Generator().manual_seed(5)).double()
    tower = tower_train.VisionTower(model, attention="torch", elementwise="torch", head_dims=tower_train.HEAD_DIMS)
    g = torch.Generator().manual_seed(11)
    probe = torch.randn(2, oa["embed_dim"], generator=g, dtype=torch.float64)
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
    print(f"vision_tower_tiny_h_finite_difference_worst {worst:.3e}")
