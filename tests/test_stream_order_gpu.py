"""GPU: every entry-point family held to its stream contract (DESIGN.md "Stream contract"; helper and the three assertions:
tests/stream_order.py).  Each case makes the call twice -- plainly on the default stream, and on a side stream where it is enqueued
behind a device-side delay while its inputs are still NaN bytes (index inputs: another valid instance) and are poisoned again right
behind it -- and asserts
  S1  the call returned while the delay was still running (no host synchronisation, no blocking copy),
  S2  the same output bits (nothing ran on another stream: it would have read the poison),
  S3  the default stream stayed idle.
Shapes and operands are those of the memory-contract tests next door (test_footprint_*_gpu.py and the contract cases of the
InfoNCE / pair-head / BERT / transform tests): the smallest that reach every launch of a call."""
import ctypes as C

import pytest
import torch

import bert_ref as B
import footprint as F
import stream_order as SO
import test_footprint_ops_gpu as OPS
import test_footprint_sim_gpu as SIM
import test_footprint_towers_gpu as TOWERS
from footprint import In, IntIn, Out, SizeOf, Work
from fusion_train_cases import linear_params, triplet
from knowledge_enhanced_multimodal_retrieval_amd import _lib, debug, engine
from knowledge_enhanced_multimodal_retrieval_amd.config import ARCHS
from knowledge_enhanced_multimodal_retrieval_amd.preprocess import pack_raw

pytestmark = pytest.mark.gpu

BF16, F32, I32, U8, FP8 = torch.bfloat16, torch.float32, torch.int32, torch.uint8, torch.float8_e4m3fn
OFF = SIM.OFF


def _stream(device):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _late(device, name, specs, what, stale=None, fn=None):
    """The entry point `name` (or `fn`), the stream appended to its arguments, plainly and late."""
    fn = fn or getattr(_lib.lib(), name)

    def run(*args):
        with torch.cuda.device(device):
            _lib.check(fn(*args, _stream(device)), name)
    return SO.run_late(run, specs, device, what=what, stale=stale)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------------------------------------ GEMM routes
def _gemm(device, m, n, k, epi, variant, what):
    a, w, bias = OPS._gemm_operands(m, n, k, m + n + k)
    rows = F.ceil256(m)
    if epi == _lib.EPI_BIAS_RESID_F32:
        c = Out((rows, n), F32, init=torch.randn(rows, n, generator=_gen(2)), written=lambda v: v[:m])
    elif epi == _lib.EPI_BIAS_RESADD_BF16:
        c = Out((rows, n), BF16, init=torch.randn(rows, n, generator=_gen(4)).to(BF16), written=lambda v: v[:m])
    else:
        c = Out((rows, n), BF16, written=lambda v: v[:m])
    with debug.override(gemm_variant=variant):
        _late(device, "kemr_op_gemm", [In(a.to(BF16)), In(w.to(BF16)), In(bias), c, m, n, k, epi], what)


@pytest.mark.parametrize("epi", [_lib.EPI_BIAS_BF16, _lib.EPI_BIAS_RESID_F32], ids=["BIAS_BF16", "RESID_F32"])
def test_gemm_128x128_kernel(device, epi):
    _gemm(device, 257, 128, 64, epi, 1, f"gemm 128x128 epi={epi}")


def test_gemm_skinny(device):
    _gemm(device, 77, 768, 256, _lib.EPI_BIAS_QGELU_BF16, 0, "gemm skinny")


# 1 = the 128 x 128 kernel, 2 = the 256 x 256 kernel, 7 = the persistent kernel, 8 = the skinny kernel forced above its 512 rows.  (3, the
# staggered 256 x 256 kernel, exists in A/B builds only: the product library refuses the switch value.)
@pytest.mark.parametrize("variant", [1, 2, 7, 8])
def test_gemm_variants(device, variant):
    _gemm(device, 514, 256, 128, _lib.EPI_BIAS_BF16, variant, f"gemm variant={variant}")


def test_gemm_residual_add_bf16(device):
    _gemm(device, 1000, 256, 128, _lib.EPI_BIAS_RESADD_BF16, 0, "gemm RESADD_BF16")


def test_gemm_default_routing_splits_into_two_launches(device):
    """64 x 257 rows: the persistent kernel takes the 64 whole row tiles, the skinny kernel the 64 rows left (csrc/gemm.hip)."""
    _gemm(device, 64 * 257, 1024, 128, _lib.EPI_BIAS_BF16, 0, "gemm persistent + skinny")


def test_gemm_fp8(device):
    m, n, k = 300, 768, 256
    g = _gen(5)
    a = torch.zeros(F.ceil256(m), k)
    a[:m] = torch.randint(-8, 9, (m, k), generator=g).float()
    w = torch.randint(-8, 9, (n, k), generator=g).float()
    wscale = 2.0 ** torch.randint(-6, -2, (n,), generator=g).float()
    bias = torch.randn(n, generator=g)
    _late(device, "kemr_op_gemm_fp8", [In(a.to(FP8)), In(w.to(FP8)), In(wscale), In(bias), Out((F.ceil256(m), n), BF16, written=lambda v: v[:m]),
                                       m, n, k, _lib.EPI_BIAS_BF16], "gemm_fp8")


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_gemm_x3(device, mode):
    m, n, k = 300, 256, 192
    g = _gen(6)
    a = engine.build_panel([torch.randn(m, k, generator=g).to(device)], _lib.SIDE_QUERY, 3).data.cpu()
    w = engine.build_panel([(torch.randn(n, k, generator=g) * k ** -0.5).to(device)], _lib.SIDE_GALLERY, 3).data.cpu()
    k3 = a.shape[1]
    assert tuple(w.shape) == (n, k3)
    bias = torch.randn(n, generator=g)
    if mode == 0:
        c = Out((m, n), F32)
    elif mode == 1:
        c = Out((m, n), F32, init=torch.randn(m, n, generator=g))
    else:
        c = Out((F.ceil256(m), 3 * n), BF16, written=lambda v: v[:m])
    _late(device, "kemr_op_gemm_x3", [In(a), In(w), In(bias), c, m, n, k3, mode], f"gemm_x3 mode={mode}")


# ------------------------------------------------------------------------------------------------ LayerNorm, 300 rows x 256
LN_ROWS, LN_WIDTH = 300, 256


def _ln_params(seed):
    g = _gen(seed)
    return g, 1 + 0.1 * torch.randn(LN_WIDTH, generator=g), 0.1 * torch.randn(LN_WIDTH, generator=g)


def test_layernorm_plain(device):
    g, gamma, beta = _ln_params(1)
    x = torch.randn(LN_ROWS, LN_WIDTH, generator=g) + 0.25
    _late(device, "kemr_op_layernorm", [In(x), In(gamma), In(beta), Out((LN_ROWS, LN_WIDTH), BF16), LN_ROWS, LN_WIDTH, _lib.KEMR_BF16], "layernorm")


def test_layernorm_resid(device):
    g, gamma, beta = _ln_params(2)
    x = torch.randn(LN_ROWS, LN_WIDTH, generator=g) + 0.25
    delta = (torch.randn(LN_ROWS, LN_WIDTH, generator=g) * 0.5).to(BF16)
    _late(device, "kemr_op_layernorm_resid", [Out(tuple(x.shape), F32, init=x), In(delta), In(gamma), In(beta), Out((LN_ROWS, LN_WIDTH), BF16),
                                              LN_ROWS, LN_WIDTH], "layernorm_resid")


@pytest.mark.parametrize("kind", ["f32", "f24"])
def test_layernorm_rows(device, kind):
    """fp32 rows with two deltas and write-back; the 24-bit rows without a delta."""
    g, gamma, beta = _ln_params(3)
    x, code = OPS._ln_rows(kind, LN_ROWS, LN_WIDTH, 7)
    d1 = (torch.randn(LN_ROWS, LN_WIDTH, generator=g) * 0.5).to(BF16)
    d2 = (torch.randn(LN_ROWS, LN_WIDTH, generator=g) * 0.5).to(BF16)
    two = kind == "f32"
    xs = Out(tuple(x.shape), x.dtype, init=x) if two else In(x)
    _late(device, "kemr_op_layernorm_rows", [xs, code, In(d1) if two else None, In(d2) if two else None, int(two), In(gamma), In(beta),
                                             Out((LN_ROWS, LN_WIDTH), BF16), LN_ROWS, LN_WIDTH, _lib.KEMR_BF16], f"layernorm_rows {kind}")


def test_layernorm_x3_and_the_fill_of_its_pad_rows(device):
    """300 rows: the pad rows 300 .. 511 of the triple are zero-filled by the call (a memset on the call's stream, csrc/layernorm.hip)."""
    g, gamma, beta = _ln_params(4)
    x = torch.randn(LN_ROWS, LN_WIDTH, generator=g) + 0.25
    res = _late(device, "kemr_op_layernorm_x3", [In(x), In(gamma), In(beta), Out((F.ceil256(LN_ROWS), 3 * LN_WIDTH), BF16), LN_ROWS, LN_WIDTH],
                "layernorm_x3")
    assert F.all_bytes(res.plain[3][LN_ROWS:], 0)


def test_layernorm_post(device):
    g, gamma, beta = _ln_params(5)
    x = torch.randn(LN_ROWS, LN_WIDTH, generator=g) + 0.25
    delta = (torch.randn(LN_ROWS, LN_WIDTH, generator=g) * 0.5).to(BF16)
    _late(device, "kemr_debug_op_layernorm_post", [Out(tuple(x.shape), F32, init=x), _lib.KEMR_F32, In(delta), In(gamma), In(beta),
                                                   Out((LN_ROWS, LN_WIDTH), BF16), LN_ROWS, LN_WIDTH, 1e-12], "layernorm_post")


# ------------------------------------------------------------------------------------------------ attention, batch 3
@pytest.mark.parametrize("t,causal", [(50, 0), (77, 1), (257, 0), (577, 0)])
def test_attention_heads_of_64(device, t, causal):
    batch, width = 3, 256
    _late(device, "kemr_op_attention", [In(OPS._qkv(batch * t, width, t + causal)), Out((batch * t, width), BF16), batch, t, width, causal],
          f"attention t={t} causal={causal}")


def test_attention_heads_of_80(device):
    batch, t, width = 3, 257, 240
    _late(device, "kemr_op_attention_hd", [In(OPS._qkv(batch * t, width, 80 + t)), Out((batch * t, width), BF16), batch, t, width, 80, 0], "attention80")


def _row_starts(lens):
    """row_start of `lens`, and of the same lengths in reverse order: a valid stale instance over the same rows."""
    return torch.tensor([0] + lens).cumsum(0).int(), torch.tensor([0] + lens[::-1]).cumsum(0).int()


def test_attention_packed(device):
    width, lens = 256, [1, 16, 17, 77, 128]
    row_start, other = _row_starts(lens)
    rows = int(row_start[-1])
    _late(device, "kemr_debug_op_attention_packed", [In(OPS._qkv(rows, width, 5)), Out((rows, width), BF16), IntIn(row_start), len(lens), max(lens), width],
          "packed attention", stale={2: other})


def test_attention_pooled(device):
    items, tokens, width = 3, 257, 768
    q = (torch.randn(items, width, generator=_gen(tokens)) * 0.25).to(BF16)
    _late(device, "kemr_debug_op_attention_pooled", [In(q), In(OPS._qkv(items * tokens, width, tokens + width)), Out((items, width), BF16), None, None,
                                                     items, tokens, width, 0, 0], "pooled attention")


def test_attention_varlen(device):
    width, lens = 256, [1, 17, 512]
    row_start, other = _row_starts(lens)
    rows = int(row_start[-1])
    _late(device, "kemr_debug_op_attention_varlen", [In(OPS._qkv(rows, width, 6, qscale=0.125)), Out((rows, width), BF16), IntIn(row_start), len(lens), 512,
                                                     width], "varlen attention", stale={2: other})


def test_attention_x3(device):
    batch, t, width = 3, 50, 256
    rows = batch * t
    _late(device, "kemr_op_attention_x3", [In(OPS._qkv(rows, width, 30 + t, F32)), Out((F.ceil256(rows), 3 * width), BF16, written=lambda v: v[:rows]),
                                           None, batch, t, width, 0], "attention_x3")


# ------------------------------------------------------------------------------------------------ encoders, batch 3
@pytest.mark.parametrize("name,precision", [("tiny-long", _lib.DEFAULT_PRECISION), ("tiny-h", _lib.DEFAULT_PRECISION),
                                            ("tiny-siglip", _lib.DEFAULT_PRECISION), ("tiny", "fp8"), ("tiny", "fp32x3")])
def test_encoders(device, name, precision):
    """Token ids and lengths are stale as the batch in reverse order (the same rows in all); one model handle serves every call."""
    arch, L, batch = ARCHS[name], _lib.lib(), 3
    eng = TOWERS._engine(name, device, precision)
    px, ids = TOWERS._inputs(name, batch)
    row_bytes = 48 * max(arch.v_width, arch.t_width)
    what = f"{name} {precision}"
    need = int(L.kemr_workspace_bytes(eng._h, _lib.TOWER_VISION, batch))
    work = Work(need, need + (1 << 20), row_bytes)
    _late(device, "kemr_encode_image", [eng._h, In(px), batch, Out((batch, arch.embed_dim), F32), 1, work, SizeOf(5)], f"encode_image {what}")
    if arch.family == "clip":
        _late(device, "kemr_encode_image_pooled", [eng._h, In(px), batch, Out((batch, arch.v_width), F32), work, SizeOf(4)], f"encode_image_pooled {what}")
    need = int(L.kemr_workspace_bytes(eng._h, _lib.TOWER_TEXT, batch))
    work = Work(need, need + (1 << 20), row_bytes)
    _late(device, "kemr_encode_text", [eng._h, IntIn(ids), batch, Out((batch, arch.embed_dim), F32), 1, work, SizeOf(5)], f"encode_text {what}")
    if arch.family == "clip":
        _late(device, "kemr_encode_text_pooled", [eng._h, IntIn(ids), batch, Out((batch, arch.t_width), F32), work, SizeOf(4)], f"encode_text_pooled {what}")
    if arch.family == "siglip":                  # kemr_encode_text_packed refuses family 1
        return
    lens = torch.tensor([1, arch.ctx, 5], dtype=I32)
    rows = int(lens.sum())
    need = int(L.kemr_text_packed_workspace_bytes(eng._h, rows, batch))
    work = Work(need, need + (1 << 20), row_bytes)
    _late(device, "kemr_encode_text_packed", [eng._h, IntIn(ids), IntIn(lens), rows, batch, Out((batch, arch.embed_dim), F32), 1, work, SizeOf(7)],
          f"encode_text_packed {what}")
    _late(device, "kemr_encode_text_packed_pooled", [eng._h, IntIn(ids), IntIn(lens), rows, batch, Out((batch, arch.t_width), F32), work, SizeOf(6)],
          f"encode_text_packed_pooled {what}")


def test_bert_encoder(device):
    L = _lib.lib()
    eng = engine.BertEngine(B.BertArch(256, 2, vocab=1024, ctx=512, pooling="mean"), device)
    eng.load_state_dict(B.cached(("sd", "plain"), lambda: B.random_state_dict(B.ARCH, 0)))
    ids, lens = B.random_ids([1, 512, 5], seed=3)
    batch, rows = 3, 518
    need = int(L.kemr_text_packed_workspace_bytes(eng._h, rows, batch))
    _late(device, "kemr_encode_text_packed", [eng._h, IntIn(ids), IntIn(lens), rows, batch, Out((batch, 256), F32), 1, Work(need, need + (1 << 20), 8 * 256),
                                              SizeOf(7)], "bert encode_text_packed")


# ------------------------------------------------------------------------------------------------ retrieval
@pytest.mark.parametrize("terms", [1, 3])
def test_panel_build(device, terms):
    """Two parts; the pointer arrays of the ABI are host arrays, built per call from the two device arguments."""
    rows, d, L = 300, 64, _lib.lib()
    g = _gen(terms)
    parts = [torch.randn(rows, d, generator=g), torch.randn(rows, d, generator=g)]
    kdim = int(L.kemr_panel_kdim(d, 2, terms))

    def build(p0, p1, out, stream):
        pp = (C.c_void_p * 2)(p0.value, p1.value)
        ps = (C.c_float * 2)(1.0, 0.5)
        return L.kemr_panel_build(pp, ps, None, 2, rows, d, terms, _lib.SIDE_QUERY, out, stream)

    res = _late(device, "kemr_panel_build", [In(parts[0]), In(parts[1]), Out((engine.rows_alloc(rows), kdim), BF16)], f"panel_build terms={terms}", fn=build)
    assert F.all_bytes(res.plain[2][rows:], 0)                   # the pad rows are zero-filled by the call


def _sim_specs(qp, gp, gtg, sgt, k, need, bonus=None):
    nq, ng = qp.rows, gp.rows
    brow, bcol, bval = bonus if bonus is not None else (None, None, None)
    specs = [*SIM._panels(qp, gp), qp.kdim, OFF, k, Out((nq, k), F32), Out((nq, k), I32), IntIn(gtg), In(sgt),
             Out((nq,), I32, init=torch.zeros(nq, dtype=I32)), IntIn(brow) if bonus else None, IntIn(bcol) if bonus else None,
             In(bval) if bonus else None, Work(need, need + (1 << 20), 4 * ng), SizeOf(15)]
    # the CSR row offsets go with the length of the column array: stale = real; the columns: every query's hits rolled by one query
    stale = {12: brow, 13: bcol.roll(4)} if bonus else None
    return specs, stale


@pytest.mark.parametrize("mode", [3, 2], ids=["lists", "lists_then_forced_fallback"])
def test_sim_topk(device, mode):
    nq, ng, d, terms, k = 300, 2500, 128, 1, 10
    qp, gp, gtg, sgt = SIM._case(device, nq, ng, d, terms)
    with debug.override(sim_lists=mode):
        need = int(_lib.lib().kemr_sim_workspace_bytes(nq, ng, qp.kdim, k))
        specs, stale = _sim_specs(qp, gp, gtg, sgt, k, need)
        _late(device, "kemr_sim_topk", specs, f"sim_topk mode={mode}", stale)


def test_sim_topk_with_a_bonus_list(device):
    nq, ng, d, terms, k = 5, 1003, 64, 3, 10
    qp, gp, gtg, sgt = SIM._case(device, nq, ng, d, terms, seed=1)
    need = int(_lib.lib().kemr_sim_workspace_bytes(nq, ng, qp.kdim, k))
    specs, stale = _sim_specs(qp, gp, gtg, sgt, k, need, SIM._bonus(nq, ng, 2))
    _late(device, "kemr_sim_topk", specs, "sim_topk bonus", stale)


def test_sim_topk_deep(device):
    nq, ng, d, terms, k = 133, 1003, 64, 1, 64
    qp, gp, _, _ = SIM._case(device, nq, ng, d, terms)
    need = int(_lib.lib().kemr_sim_topk_deep_workspace_bytes(nq, ng, qp.kdim, k))
    _late(device, "kemr_sim_topk_deep", [*SIM._panels(qp, gp), qp.kdim, OFF, k, Out((nq, k), F32), Out((nq, k), I32), Work(need, need + (1 << 20), 4 * ng),
                                         SizeOf(9)], "sim_topk_deep")


def test_sim_topk_deep_fused(device):
    nq, ng, d, terms, k = 5, 1003, 64, 3, 1003
    qp, gp, gtg, sgt = SIM._case(device, nq, ng, d, terms, seed=3)
    need = int(_lib.lib().kemr_sim_topk_deep_workspace_bytes(nq, ng, qp.kdim, k))
    specs, stale = _sim_specs(qp, gp, gtg, sgt, k, need, SIM._bonus(nq, ng, 4))
    _late(device, "kemr_sim_topk_deep_fused", specs, "sim_topk_deep_fused", stale)


def _listed(nq, n, ng, seed):
    """Scores [nq, n] with a tie per row and distinct candidate ids per row (one padding entry)."""
    g = _gen(seed)
    scores = torch.randn(nq, n, generator=g)
    scores[:, 3] = scores[:, 7]
    idx = torch.stack([torch.randperm(ng, generator=g)[:n] for _ in range(nq)]).int() + OFF
    idx[:, 5] = -1
    return scores, idx


def test_select_topk(device):
    nq, n, k = 5, 1003, 10
    scores, idx = _listed(nq, n, 5000, 1)
    _late(device, "kemr_select_topk", [In(scores), IntIn(idx), nq, n, n, OFF, k, Out((nq, k), F32), Out((nq, k), I32)], "select_topk")


def test_topk_merge(device):
    nq, nlists, k = 5, 3, 10
    scores, idx = _listed(nq, nlists * k, 5000, 2)
    scores = scores.view(nq, nlists, k).sort(dim=-1, descending=True).values.contiguous()
    _late(device, "kemr_topk_merge", [In(scores), IntIn(idx.view(nq, nlists, k)), nq, nlists, k, Out((nq, k), F32), Out((nq, k), I32)], "topk_merge")


def test_pair_scores(device):
    nq, ng = 5, 1003
    qp, gp, _, _ = SIM._case(device, nq, ng, 64, 3)
    n = 40
    g = _gen(3)
    q_rows, g_rows = torch.randint(0, nq, (n,), generator=g).int(), torch.randint(0, ng, (n,), generator=g).int()
    _late(device, "kemr_pair_scores", [In(qp.data), In(gp.data), qp.kdim, IntIn(q_rows), IntIn(g_rows), n, Out((n,), F32)], "pair_scores")


def test_scores_dense(device):
    nq, ng = 133, 1003
    qp, gp, _, _ = SIM._case(device, nq, ng, 64, 1)
    ld = ng + 5
    _late(device, "kemr_scores_dense", [*SIM._panels(qp, gp), qp.kdim, Out((nq, ld), F32, written=lambda v: v[:, :ng]), ld], "scores_dense")


def test_rank_dense(device):
    nq, ng, k = 5, 1003, 10
    g = _gen(4)
    scores = torch.randn(nq, ng, generator=g)
    gt = torch.randint(0, ng, (nq,), generator=g).int()
    _late(device, "kemr_rank_dense", [In(scores), nq, ng, ng, IntIn(gt), Out((nq,), I32, init=torch.zeros(nq, dtype=I32)), k, Out((nq, k), F32),
                                      Out((nq, k), I32)], "rank_dense")


def test_list_fuse(device):
    nq, ld, ng = 5, 64, 1003
    scores, idx = _listed(nq, ld, ng, 5)
    brow, bcol, bval = SIM._bonus(nq, ng, 6)
    gt = idx[:, 9].clone()
    _late(device, "kemr_list_fuse", [In(scores), IntIn(idx), nq, ld, ld, 0.5, IntIn(brow), IntIn(bcol), In(bval), IntIn(gt), Out((nq,), I32),
                                     Out((nq,), I32), Out((nq,), F32), Out((nq, ld), F32)], "list_fuse", stale={6: brow, 7: bcol.roll(4)})


# ------------------------------------------------------------------------------------------------ fusion heads
HEADS, HID1, HID2 = 8, 16, 8


def _head_params(g, n_c):
    r = lambda *s: torch.randn(*s, generator=g) * 0.3          # noqa: E731
    return [In(r(n_c, HEADS, HID1)), In(r(n_c, HEADS, HID1)), In(r(HID1)), In(r(HID1, HID2)), In(r(HID2)), In(r(HID2))]


def test_cross_attention_pairs(device):
    n_q, n_c = 5, 33
    g = _gen(7)
    st = [In(torch.randn(HEADS, n_c, n_q, generator=g)) for _ in range(2)]
    _late(device, "kemr_cross_attention_pairs", st + _head_params(g, n_c) + [0.25, HEADS, n_q, n_c, HID1, HID2, Out((n_c, n_q), F32)], "cross_attention_pairs")


def test_cross_attention_rerank(device):
    nq, ng, dim, ld = 5, 33, 96, 16
    g = _gen(8)
    q, k_i, k_t = torch.randn(nq, dim, generator=g), torch.randn(ng, dim, generator=g), torch.randn(ng, dim, generator=g)
    cand = torch.stack([torch.randperm(ng, generator=g)[:ld] for _ in range(nq)]).int()
    cand[:, 5] = -1
    _late(device, "kemr_cross_attention_rerank", [In(q), In(k_i), In(k_t)] + _head_params(g, ng) +
          [0.25, HEADS, nq, ng, dim, HID1, HID2, IntIn(cand), ld, ld, Out((nq, ld), F32)], "cross_attention_rerank")


def test_linear_head(device):
    n, hidden = 1003, 24
    g = _gen(9)
    w0, b0, w1, b1 = linear_params(hidden, seed=9)
    _late(device, "kemr_linear_head", [In(torch.randn(n, generator=g)), In(torch.randn(n, generator=g)), n, In(w0), In(b0), In(w1), float(b1), hidden,
                                       Out((n,), F32)], "linear_head")


def test_gate_rows(device):
    rows, cols = 133, 100
    g = _gen(10)
    _late(device, "kemr_gate_rows", [In(torch.randn(rows, cols, generator=g)), rows, cols, In(torch.randn(cols, generator=g)),
                                     In(torch.randn(cols, generator=g) * 0.1), 0.125, 1, Out((rows,), F32)], "gate_rows")


# ------------------------------------------------------------------------------------------------ training losses, n = 129, d = 100
def test_infonce(device):
    n, d, L = 129, 100, _lib.lib()
    g = _gen(21)
    a = torch.nn.functional.normalize(torch.randn(n, d, generator=g), dim=-1)
    b = torch.nn.functional.normalize(a + 0.5 * torch.randn(n, d, generator=g), dim=-1)
    need = int(L.kemr_infonce_workspace_bytes(n, d))
    inv_t = 1.0 / 0.07
    work = Work(need, 2 * need, 4 * 1280)

    def fwd(pa, pb, loss, lse, ws, ws_bytes, stream):
        return L.kemr_infonce_forward(pa, pb, n, d, inv_t, loss, lse, ws, ws_bytes, stream)

    res = _late(device, "kemr_infonce_forward", [In(a), In(b), Out((3,), F32), Out((2 * n,), F32), work, SizeOf(4)], "infonce_forward", fn=fwd)
    lse = res.plain[3].cpu().clone()

    def bwd(pa, pb, plse, ga, gb, ws, ws_bytes, stream):
        return L.kemr_infonce_backward(pa, pb, plse, n, d, inv_t, ga, gb, ws, ws_bytes, stream)

    _late(device, "kemr_infonce_backward", [In(a), In(b), In(lse), Out((n, d), F32), Out((n, d), F32), work, SizeOf(5)], "infonce_backward", fn=bwd)


@pytest.mark.parametrize("mode", [_lib.PAIRHEAD_GATED, _lib.PAIRHEAD_LINEAR], ids=["gated", "linear"])
def test_pairhead(device, mode):
    n, d, L = 129, 100, _lib.lib()
    q, img, tgt = triplet(n, d, seed=21)
    if mode == _lib.PAIRHEAD_GATED:
        head, hidden = [In(torch.sigmoid(torch.randn(n, generator=_gen(4)))), None, None, None, None], 0
    else:
        head, hidden = [None] + [In(t) for t in linear_params(24, seed=4)], 24
    need = int(L.kemr_pairhead_workspace_bytes(mode, n, d, hidden))
    inv_t = 1.0 / 0.07
    work = Work(need, 2 * need, 4 * 1280)

    def fwd(pq, pi, pt, gt, w0, b0, w1, b1, loss, lse, ws, ws_bytes, stream):
        return L.kemr_pairhead_forward(mode, pq, pi, pt, n, d, inv_t, gt, w0, b0, w1, b1, hidden, loss, lse, ws, ws_bytes, stream)

    res = _late(device, "kemr_pairhead_forward", [In(q), In(img), In(tgt)] + head + [Out((3,), F32), Out((2 * n,), F32), work, SizeOf(10)],
                f"pairhead_forward mode={mode}", fn=fwd)
    lse = res.plain[9].cpu().clone()
    n_grad = n if mode == _lib.PAIRHEAD_GATED else 4 * hidden + 1

    def bwd(pq, pi, pt, plse, gt, w0, b0, w1, b1, grad, ws, ws_bytes, stream):
        return L.kemr_pairhead_backward(mode, pq, pi, pt, plse, n, d, inv_t, gt, w0, b0, w1, b1, hidden, grad, ws, ws_bytes, stream)

    _late(device, "kemr_pairhead_backward", [In(q), In(img), In(tgt), In(lse)] + head + [Out((n_grad,), F32), work, SizeOf(10)],
          f"pairhead_backward mode={mode}", fn=bwd)


# ------------------------------------------------------------------------------------------------ image transforms
def _pixels(h, w, seed):
    return torch.randint(0, 255, (h, w, 3), generator=_gen(seed), dtype=U8)          # never 0xff: the poison is no pixel of the image


def _ptr(a):
    return C.c_void_p(a.ctypes.data)


@pytest.mark.parametrize("n,h,w", [(64, 63, 65), (224, 1080, 1920), (64, 16384, 200)])
def test_single_image_transforms(device, n, h, w):
    """kemr_preprocess_u8 and kemr_transform_u8 (both kinds): the tap table of the size crosses host to device inside the call -- a
    few KiB at 63 x 65 -> 64, about 100 KiB at 1080 x 1920 -> 224, about 260 KiB for kind 1 at 16384 x 200 -> 64 (a
    vertical scale of 256: a copy no runtime sends inline)."""
    L = _lib.lib()
    img = _pixels(h, w, 21)
    need = int(L.kemr_preprocess_workspace_bytes(h, w, n))
    _late(device, "kemr_preprocess_u8", [In(img.reshape(-1)), h, w, n, Out((3, n, n), F32), Work(need, need + (1 << 20)), SizeOf(5)], "preprocess_u8")
    for kind in (_lib.TRANSFORM_CLIP, _lib.TRANSFORM_SIGLIP):
        need = int(L.kemr_transform_workspace_bytes(kind, h, w, n))
        _late(device, "kemr_transform_u8", [kind, In(img.reshape(-1)), h, w, n, Out((3, n, n), F32), Work(need, need + (1 << 20)), SizeOf(6)],
              f"transform_u8 kind={kind}")


def test_a_staging_slot_that_grows_inside_the_call(device):
    """A descriptor blob larger than any pinned staging slot can be (six tall images of different sizes: 1.6 MB of tap tables; one
    table is 0.5 MB at the most, a slot twice that) has to outgrow its slot while the stream is held back -- and freeing pinned
    memory waits for the device.  One small call per slot first, so that the slot has a buffer to outgrow.  That it did outgrow
    one inside the late call is read from the library's counter ("staging_grown"), not supposed from its slot policy."""
    L, n, kind = _lib.lib(), 64, _lib.TRANSFORM_SIGLIP
    h, w = 63, 65
    small = _pixels(h, w, 1).reshape(-1).to(device)
    need = int(L.kemr_transform_workspace_bytes(kind, h, w, n))
    ws, out = torch.empty(need, dtype=U8, device=device), torch.empty(3, n, n, device=device)
    with torch.cuda.device(device):
        for _ in range(debug.get("staging_slots")):
            _lib.check(L.kemr_transform_u8(kind, C.c_void_p(small.data_ptr()), h, w, n, C.c_void_p(out.data_ptr()), C.c_void_p(ws.data_ptr()), need,
                                           _stream(device)), "transform_u8")
            torch.cuda.synchronize(device)               # the next call takes the next slot: this one's copy has finished
    packed = pack_raw([_pixels(16384, 200 + i, 2) for i in range(6)])
    hs, wd, offs = packed.heights, packed.widths, packed.offsets
    b = len(hs)
    need = int(L.kemr_transform_batch_workspace_bytes(kind, _ptr(hs), _ptr(wd), b, n))
    grown = []

    def call(*args):
        before = debug.get("staging_grown")
        status = L.kemr_transform_u8_batch(*args)
        grown.append(debug.get("staging_grown") - before)
        return status

    _late(device, "kemr_transform_u8_batch", [kind, In(packed.data), _ptr(offs), _ptr(hs), _ptr(wd), b, n, Out((b, 3, n, n), F32),
                                              Work(need, need + (1 << 20)), SizeOf(8)], "transform_u8_batch with a slot that grows", fn=call)
    assert grown == [1, 1, 1], grown             # the two plain calls and the late one: each on another slot, each outgrew it


def test_batch_transforms(device):
    """Three images of different sizes, one of them an undecodable 0 x 0 item (zeros out) between the two others."""
    L, n = _lib.lib(), 64
    sizes = [(150, 291), (0, 0), (37, 100)]
    packed = pack_raw([_pixels(h, w, 31 + i) for i, (h, w) in enumerate(sizes)])
    hs, ws, offs = packed.heights, packed.widths, packed.offsets
    b = len(sizes)
    need = int(L.kemr_preprocess_batch_workspace_bytes(_ptr(hs), _ptr(ws), b, n))
    res = _late(device, "kemr_preprocess_u8_batch", [In(packed.data), _ptr(offs), _ptr(hs), _ptr(ws), b, n, Out((b, 3, n, n), F32),
                                                     Work(need, need + (1 << 20)), SizeOf(7)], "preprocess_u8_batch")
    assert F.all_bytes(res.plain[6][1], 0)
    for kind in (_lib.TRANSFORM_CLIP, _lib.TRANSFORM_SIGLIP):
        need = int(L.kemr_transform_batch_workspace_bytes(kind, _ptr(hs), _ptr(ws), b, n))
        _late(device, "kemr_transform_u8_batch", [kind, In(packed.data), _ptr(offs), _ptr(hs), _ptr(ws), b, n, Out((b, 3, n, n), F32),
                                                  Work(need, need + (1 << 20)), SizeOf(8)], f"transform_u8_batch kind={kind}")


# ------------------------------------------------------------------------------------------------ the calls that need a host value
def test_encode_text_with_device_ids_alone_is_exempt_from_s1_only(device):
    """ClipEngine.encode_text with ids on the GPU and no lens: one device-to-host copy of the lengths sizes the packed launches
    (engine.py; SO.HOST_SYNC_CALLS).  It waits for the stream -- and must still be ordered on it (S2) and leave the default stream
    alone (S3)."""
    name = "tiny"
    arch = ARCHS[name]
    _, ids = TOWERS._inputs(name, 3)
    eng = TOWERS._engine(name, device)
    assert eng.pack_text

    def run(ids_dev, out):
        out.copy_(eng.encode_text(ids_dev, normalize=True))

    res = SO.run_late(run, [IntIn(ids), Out((3, arch.embed_dim), F32)], device, as_arg=lambda t: t, what="ClipEngine.encode_text device ids",
                      name="ClipEngine.encode_text(device ids, no lens)")
    assert not res.pending                       # it did wait: the exemption is not idle
