"""No GPU: the ABI entry, the argument checks of kemr_cross_attention_rerank (they run before any HIP call), the errors of
FusionModel.rerank that need no device, and the --rerank_depth flag of the fusion evaluator's parser."""
import ctypes as C

import pytest
import torch

from knowledge_enhanced_multimodal_retrieval_amd import _lib, evaluators
from knowledge_enhanced_multimodal_retrieval_amd.fusion_model import FusionModel


def _err(L):
    return (L.kemr_last_error() or b"").decode()


def test_entry_point_is_declared_and_the_abi_version_stays():
    assert "kemr_cross_attention_rerank" in _lib.SIGNATURES and _lib.ABI_VERSION == 4
    L = _lib.lib()
    assert L.kemr_abi_version() == 4 and hasattr(L, "kemr_cross_attention_rerank")


def _call(L, p, **kw):
    """kemr_cross_attention_rerank on dummy host pointers (every call here returns before a pointer is used)."""
    a = dict(q=p, k_i=p, k_t=p, p_i=p, p_t=p, c0=p, w2t=p, b2=p, w3=p, b3=0.0, heads=8, nq=2, ng=5, dim=64, hid1=256, hid2=64,
             cand=p, depth=4, ld=4, out=p)
    a.update(kw)
    return L.kemr_cross_attention_rerank(a["q"], a["k_i"], a["k_t"], a["p_i"], a["p_t"], a["c0"], a["w2t"], a["b2"], a["w3"], a["b3"],
                                         a["heads"], a["nq"], a["ng"], a["dim"], a["hid1"], a["hid2"], a["cand"], a["depth"], a["ld"],
                                         a["out"], None)


def test_argument_checks_name_the_offending_value():
    L = _lib.lib()
    buf = (C.c_float * 64)()
    p = C.c_void_p(C.addressof(buf))
    for name, arg in (("q", "q_dev"), ("k_i", "k_i_dev"), ("k_t", "k_t_dev"), ("p_i", "p_i_dev"), ("p_t", "p_t_dev"), ("c0", "c0_dev"),
                      ("w2t", "w2t_dev"), ("b2", "b2_dev"), ("w3", "w3_dev"), ("cand", "cand_idx_dev"), ("out", "out_scores_dev")):
        assert _call(L, p, **{name: None}) == -1 and arg in _err(L), name
    assert _call(L, p, heads=4) == -1 and "heads=4" in _err(L)
    assert _call(L, p, heads=12) == -1 and "heads=12" in _err(L)
    assert _call(L, p, dim=70) == -1 and "dim=70" in _err(L)
    assert _call(L, p, hid2=0) == -1 and "hid2=0" in _err(L)
    assert _call(L, p, hid2=65) == -1 and "hid2=65" in _err(L)
    assert _call(L, p, depth=1025, ld=1025) == -1 and "depth=1025" in _err(L)
    assert _call(L, p, depth=-1) == -1 and "depth=-1" in _err(L)
    assert _call(L, p, depth=8, ld=7) == -1 and "ld=7" in _err(L)
    assert _call(L, p, hid1=1024) == -1 and "hid1=1024" in _err(L) and "LDS" in _err(L)      # 320 KiB of W2^T alone
    assert _call(L, p, dim=32768, hid1=64) == -1 and "dim=32768" in _err(L) and "LDS" in _err(L)


def test_empty_calls_are_no_ops():
    L = _lib.lib()
    buf = (C.c_float * 64)()
    p = C.c_void_p(C.addressof(buf))
    assert _call(L, p, nq=0) == 0
    assert _call(L, p, depth=0) == 0
    assert _call(L, None, nq=0, q=None, out=None) == 0         # nothing is looked at, not even the pointers


@pytest.mark.parametrize("ft", ["gated", "simple_gated", "simple_gated_with_bias", "bilinear"])
def test_rerank_refuses_the_heads_that_rank_the_whole_gallery(ft):
    fm = FusionModel(torch.nn.Linear(1, 1), fusion_type=ft, embed_dim=64)
    q = torch.zeros(2, 64)
    with pytest.raises(ValueError, match=r"rank\(\)"):
        fm.rerank(q, None)
    with pytest.raises(ValueError, match=r"rank\(\)"):
        fm.prepare_gallery(q, q)


@pytest.mark.parametrize("ft", ["linear", "cross_attention"])
def test_rerank_depth_and_k_limits(ft):
    fm = FusionModel(torch.nn.Linear(1, 1), fusion_type=ft, embed_dim=64)
    q = torch.zeros(2, 64)
    with pytest.raises(ValueError, match="depth=0"):
        fm.rerank(q, None, depth=0)
    with pytest.raises(ValueError, match="depth=1025"):
        fm.rerank(q, None, depth=1025)
    with pytest.raises(ValueError, match="k=21"):
        fm.rerank(q, None, depth=20, k=21)
    with pytest.raises(ValueError, match="k=0"):
        fm.rerank(q, None, depth=20, k=0)
    with pytest.raises(ValueError, match="prepare_gallery"):
        fm.rerank(q, None, depth=20, k=10)                     # the limits hold; what is missing now is a prepared gallery


def test_fusion_parser_rerank_depth(capsys):
    parser = evaluators.fusion_parser()
    assert parser.parse_args(["--fusion_type", "linear"]).rerank_depth is None
    assert parser.parse_args(["--fusion_type", "linear", "--rerank_depth", "20"]).rerank_depth == 20
    assert parser.parse_args(["--fusion_type", "cross_attention", "--rerank_depth", "1024"]).rerank_depth == 1024
    for bad in ("19", "1025", "deep"):
        with pytest.raises(SystemExit) as e:
            parser.parse_args(["--fusion_type", "linear", "--rerank_depth", bad])
        assert e.value.code == 2
        assert "--rerank_depth" in capsys.readouterr().err
    with pytest.raises(ValueError, match="rerank_depth=19"):
        evaluators._check_rerank_depth("linear", 19)
    with pytest.raises(ValueError, match="gated"):
        evaluators._check_rerank_depth("gated", 40)
