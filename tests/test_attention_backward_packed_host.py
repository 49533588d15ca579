"""Host (no GPU): the ABI surface of ``kemr_op_attention_packed`` and ``kemr_op_attention_backward_packed`` (csrc/api.hip,
csrc/attention_bwd.hip), their host-side refusals, the engine wrappers' refusal of CPU tensors, and ``tower_train.torch_attention_packed``
against ``torch_attention`` per item."""
import ctypes as C
import os
import re

import pytest
import torch

import attention_bwd_ref as R
from knowledge_enhanced_multimodal_retrieval_amd import _lib, tower_train

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEMR_ERR_INVALID = -1


def test_symbols_are_declared_and_abi_stays_4():
    assert _lib.SIGNATURES["kemr_op_attention_packed"] == (C.c_int, [C.c_void_p] * 3 + [C.c_int] * 3 + [C.c_void_p])
    assert _lib.SIGNATURES["kemr_op_attention_backward_packed"] == (C.c_int, [C.c_void_p] * 4 + [C.c_int] * 4 + [C.c_void_p])
    header = open(os.path.join(ROOT, "include", "kemr.h")).read()
    assert re.search(r"\bint\s+kemr_op_attention_packed\s*\(\s*const void\* qkv_dev, void\* out_dev, const int\* row_start_dev,\s*int batch, "
                     r"int max_t, int width,\s*void\* stream\);", header)
    assert re.search(r"\bint\s+kemr_op_attention_backward_packed\s*\(\s*const void\* qkv_dev, const void\* dout_dev, void\* dqkv_dev, "
                     r"const int\* row_start_dev,\s*int batch,\s*int max_t, int width, int causal,\s*void\* stream\);", header)
    assert "#define KEMR_ABI_VERSION 4" in header and "Still 4: kemr_op_attention_packed" in header
    assert _lib.ABI_VERSION == 4 and _lib.lib().kemr_abi_version() == 4
    lib = _lib.lib()
    assert lib.kemr_op_attention_packed and lib.kemr_op_attention_backward_packed          # exported and bound


# never dereferenced: every case is refused on the host, before any HIP call
P = C.c_void_p(0x1000)
NULL = C.c_void_p(None)


@pytest.mark.parametrize("args,names", [
    ((NULL, P, P, P, 2, 77, 128, 1), "qkv"),
    ((P, NULL, P, P, 2, 77, 128, 1), "dout"),
    ((P, P, NULL, P, 2, 77, 128, 1), "dqkv"),
    ((P, P, P, NULL, 2, 77, 128, 1), "row_start"),
    ((P, P, P, P, 2, 0, 128, 1), "max_t"),
    ((P, P, P, P, 2, 289, 128, 0), "max_t"),
    ((P, P, P, P, 2, 77, 96, 1), "width"),
    ((P, P, P, P, 2, 77, 0, 1), "width"),
    ((P, P, P, P, 2, 77, 128, 2), "causal"),
    ((P, P, P, P, 2, 77, 128, -1), "causal"),
    ((P, P, P, P, -1, 77, 128, 0), "batch"),
    ((P, P, P, P, 2 ** 31 - 1, 77, 128, 1), "batch"),          # 2^31 - 1 items x 2 heads: beyond the grid
], ids=["qkv=NULL", "dout=NULL", "dqkv=NULL", "row_start=NULL", "max_t=0", "max_t=289", "width=96", "width=0", "causal=2", "causal=-1",
        "batch=-1", "batch*heads>2^31-1"])
def test_backward_refused_on_the_host(args, names):
    L = _lib.lib()
    assert L.kemr_op_attention_backward_packed(*args, None) == KEMR_ERR_INVALID
    msg = L.kemr_last_error().decode()
    assert msg.startswith("op_attention_backward_packed:") and re.search(rf"\b{names}\b", msg), msg
    with pytest.raises(RuntimeError, match=names):
        _lib.check(L.kemr_op_attention_backward_packed(*args, None), "op_attention_backward_packed")


@pytest.mark.parametrize("args,names", [
    ((NULL, P, P, 2, 77, 128), "qkv"),
    ((P, NULL, P, 2, 77, 128), "out"),
    ((P, P, NULL, 2, 77, 128), "row_start"),
    ((P, P, P, 2, 0, 128), "max_t"),
    ((P, P, P, 2, 289, 128), "max_t"),
    ((P, P, P, 2, 77, 96), "width"),
    ((P, P, P, 2, 77, -64), "width"),
    ((P, P, P, -1, 77, 128), "batch"),
    ((P, P, P, 65529, 77, 128), "batch"),
], ids=["qkv=NULL", "out=NULL", "row_start=NULL", "max_t=0", "max_t=289", "width=96", "width=-64", "batch=-1", "batch=65529"])
def test_forward_refused_on_the_host(args, names):
    L = _lib.lib()
    assert L.kemr_op_attention_packed(*args, None) == KEMR_ERR_INVALID
    msg = L.kemr_last_error().decode()
    assert msg.startswith("op_attention_packed:") and re.search(rf"\b{names}\b", msg), msg


def test_an_empty_batch_is_accepted_on_the_host():
    L = _lib.lib()
    assert L.kemr_op_attention_backward_packed(P, P, P, P, 0, 77, 128, 1, None) == 0
    assert L.kemr_op_attention_packed(P, P, P, 0, 77, 128, None) == 0


def test_engine_wrappers_have_no_cpu_fallback():
    from knowledge_enhanced_multimodal_retrieval_amd import engine
    qkv, dout = R.make_inputs(1, 4, 64, 0)
    rs = torch.tensor([0, 4], dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        engine.attention_backward_packed(qkv, dout, rs, 4, 64, True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        engine.op_attention_packed(qkv, rs, 4, 64)


LENS = [17, 1, 33, 16, 2, 77]


@pytest.mark.parametrize("causal", [False, True])
def test_the_packed_plain_formulation_is_the_plain_formulation_per_item(causal):
    width, rows = 128, sum(LENS)
    g = torch.Generator().manual_seed(5)
    qkv = torch.randn(rows, 3 * width, generator=g, dtype=torch.float64)
    dout = torch.randn(rows, width, generator=g, dtype=torch.float64)
    x = qkv.clone().requires_grad_(True)
    got = tower_train.torch_attention_packed(x, LENS, width, causal)
    got.backward(dout)
    y = qkv.clone().requires_grad_(True)
    parts, r = [], 0
    for n in LENS:
        parts.append(tower_train.torch_attention(y[r:r + n], 1, n, width, causal))
        r += n
    want = torch.cat(parts)
    want.backward(dout)
    assert got.dtype == torch.float64 and got.shape == (rows, width)
    assert R.rel_l2(got.detach(), want.detach()) <= 1e-14 and R.rel_l2(x.grad, y.grad) <= 1e-14
    # and it is the statement the op's tests are held to (q pre-scaled there, scaled by 1/8 here)
    scaled = qkv.clone()
    scaled[:, :width] *= 0.125
    r = 0
    for n in LENS:
        item = R.backward_fp64(scaled[r:r + n], dout[r:r + n], 1, n, width, causal)
        item[:, :width] *= 0.125
        assert R.rel_l2(x.grad[r:r + n], item) <= 1e-12
        r += n
    with pytest.raises(ValueError, match="lengths sum"):
        tower_train.torch_attention_packed(qkv, LENS[:-1], width, causal)


def test_segments_split_queries_from_targets_and_nothing_else():
    seg = tower_train.packed_segments
    assert seg([16]) == ((0, 1, 16),)
    assert seg([77] * 8) == ((0, 8, 77),)
    assert seg([9, 40, 12, 30, 248, 150, 200, 180]) == ((0, 4, 40), (4, 8, 248))
    assert seg([248, 150, 9, 40]) == ((0, 2, 248), (2, 4, 40))
    assert seg([150, 248, 200, 180]) == ((0, 4, 248),)          # nothing to gain: one call
    for lens in ([3, 5, 288, 1, 1], [1] * 5 + [77] * 5):
        s = seg(lens)
        assert s[0][0] == 0 and s[-1][1] == len(lens) and all(a[1] == b[0] for a, b in zip(s, s[1:]))
        assert all(m == max(lens[lo:hi]) for lo, hi, m in s)
