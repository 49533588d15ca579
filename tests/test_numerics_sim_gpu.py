"""GPU: the similarity panels and scores held to the statements of oracle/rounding.py.

* panel_build_kernel, into a buffer pre-filled with NaN: bit for bit panel_statement -- terms 1 and 3, both sides, 1-4 parts, part
  scales != 1 and row scales on some parts, d in {1, 63, 65, 96, 768}, rows in {1, 255, 256, 257} (the pad columns and the zero pad
  rows up to ceil256 included), on RNE ties of both parities (of hi and of lo), bf16-exact values (lo = 0), negative values and an
  outlier channel; and a lo that is an fp32 subnormal (kept, not flushed).
* sim_kernel's dense form (kemr_scores_dense) against panel_scores_emulation: budget ratio <= 1 (fp32 ulps) with KAPPA (the kappa
  measured per case is printed: 0.05 .. 4.84), |relative bias| <= MAX_REL_BIAS; ragged nq / ng, kdim 64 .. 4608 (4 parts x 3 terms),
  cancelling pairs, rows scaled like the fusion heads' fp32 linear layers.  pair_scores_kernel bit-identical to the dense scores on
  the same pairs, and the scores within panel_representation_bound (+ the accumulation) of fp64 of the fp32 inputs.
Every measured worst ratio / bias / kappa is printed (pytest -s)."""
import ctypes as C

import pytest
import torch

from knowledge_enhanced_multimodal_retrieval_amd import _lib, engine
from oracle import rounding as R

pytestmark = pytest.mark.gpu

KAPPA = 10                 # accumulator bar: 2 x the worst measured on the MI355X (4.84, fusion-head rows, kdim 4608), cap 16
MAX_REL_BIAS = 4           # units of 2^-24 (rounding.relative_bias)
PART_SCALE = [1.0, 0.7, 1.3, 0.55]


def _note(name, value):
    print(f"NUMERICS {name} {value}")


def _panel_nan(parts, side, terms, part_scale=None, row_scale=None):
    """kemr_panel_build (as engine.build_panel) into a buffer of NaN: whatever the kernel does not write stays NaN."""
    L = _lib.lib()
    rows, d = parts[0].shape
    n = len(parts)
    kdim = int(L.kemr_panel_kdim(d, n, terms))
    dev = parts[0].device
    out = torch.full((engine.rows_alloc(rows), kdim), float("nan"), dtype=torch.bfloat16, device=dev)
    pp = (C.c_void_p * n)(*[p.data_ptr() for p in parts])
    ps = (C.c_float * n)(*(part_scale if part_scale is not None else [1.0] * n))
    prs = None if row_scale is None else (C.c_void_p * n)(*[None if r is None else r.data_ptr() for r in row_scale])
    with torch.cuda.device(dev):
        _lib.check(L.kemr_panel_build(pp, ps, prs, n, rows, d, terms, side, C.c_void_p(out.data_ptr()),
                                      C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "panel_build")
    return engine.Panel(out, rows, kdim, terms, side)


def _first_mismatch(got, want):
    g, w = got.view(torch.int16), want.view(torch.int16)
    bad = (g != w).nonzero()
    if not len(bad):
        return "equal"
    r, c = (int(v) for v in bad[0])
    return f"{len(bad)} mismatches, first at row {r} col {c}: got {got[r, c].item()!r} want {want[r, c].item()!r}"


def _special_part(rows, d, g):
    """Random normals with, by column: RNE ties of hi (both parities), ties of lo (v = 1 + (2 j + 1) 2^-17: hi = 1, lo a bf16 tie),
    bf16-exact values (lo = 0), and an outlier channel 1e4 x the rest."""
    x = torch.randn(rows, d, generator=g)
    sign = torch.randint(0, 2, (rows, d), generator=g).float() * 2 - 1
    k = torch.randint(128, 256, (rows, d), generator=g).float()
    j = torch.randint(64, 128, (rows, d), generator=g).float()
    col = torch.arange(d) % 8
    x = torch.where(col == 1, sign * (k + 0.5) * 2.0 ** -7, x)
    x = torch.where(col == 3, sign * (1 + (2 * j + 1) * 2.0 ** -17), x)
    x = torch.where(col == 5, x.to(torch.bfloat16).float(), x)
    x[:, d // 2] *= 1e4
    return x


def _panel_cases():
    """Every (d, rows) pair; (terms, side) all four ways for each, the part count cycling through 1 .. 4."""
    i = 0
    for d in (1, 63, 65, 96, 768):
        for rows in (1, 255, 256, 257):
            for terms, side in ((1, 0), (1, 1), (3, 0), (3, 1)):
                yield d, rows, terms, side, 1 + i % 4
                i += 1


def test_panel_build_is_the_statement_bit_for_bit(device):
    g = torch.Generator().manual_seed(61)
    checked = 0
    for d, rows, terms, side, nparts in _panel_cases():
        parts = [_special_part(rows, d, g) * (1 if p == 0 else 0.5 + p) for p in range(nparts)]
        rs = [None if p % 2 == 0 else torch.rand(rows, generator=g) + 0.5 for p in range(nparts)]
        ps = PART_SCALE[:nparts]
        got = _panel_nan([x.to(device) for x in parts], side, terms, ps, [None if r is None else r.to(device) for r in rs]).data.cpu()
        want = R.panel_statement(parts, ps, rs, terms, side)
        assert got.shape == want.shape, (d, rows, terms, side, nparts, got.shape, want.shape)
        assert torch.equal(got.view(torch.int16), want.view(torch.int16)), (d, rows, terms, side, nparts, _first_mismatch(got, want))
        checked += 1
    _note("panels_bit_exact", checked)


def test_panel_subnormal_lo_is_kept(device):
    """v_cvt_pk_bf16_f32 on an fp32 subnormal: v = 2^-120 (1 + 2^-9 + 3 2^-14) splits into hi = 2^-120 and v - hi = 2^-129 + 3 2^-134,
    an fp32 subnormal; on bf16's subnormal grid (2^-133) that is 17.5 steps, a tie, so lo = 18 x 2^-133 (even).  v = 3 2^-132 is itself
    subnormal (hi = v, lo = 0); the scale 2^-60 applied to 2^-60 (1 + 2^-9 + 3 2^-14) in fp32 makes the same v through the multiply."""
    v = [2.0 ** -120 * (1 + 2.0 ** -9 + 3 * 2.0 ** -14), -2.0 ** -120 * (1 + 2.0 ** -9 + 3 * 2.0 ** -14), 3 * 2.0 ** -132, 1.5]
    src = torch.tensor([v], dtype=torch.float32)
    scaled = torch.tensor([[2.0 ** -60 * (1 + 2.0 ** -9 + 3 * 2.0 ** -14)] * 4], dtype=torch.float32)
    for parts, ps in (([src], [1.0]), ([scaled], [2.0 ** -60])):
        for side in (0, 1):
            got = _panel_nan([x.to(device) for x in parts], side, 3, ps).data.cpu()
            want = R.panel_statement(parts, ps, None, 3, side)
            assert torch.equal(got.view(torch.int16), want.view(torch.int16)), (ps, side, _first_mismatch(got, want))
    lo = want.double()[0, 128]
    assert lo == 2.0 ** -129 + 2.0 ** -132, lo                 # the statement's lo: kept and rounded on the subnormal grid
    _note("panel_subnormal_lo", "kept (not flushed)")


# ------------------------------------------------------------------------------------------------ scores
def _unit(n, d, g):
    return torch.nn.functional.normalize(torch.randn(n, d, generator=g), dim=-1)


def _score_case(kind, nq, ng, d, nparts, g):
    """(query parts, gallery parts, part_scale, query row_scale): unit embeddings (the retrieval panels), fusion-head-like rows
    (activations of a few units against nn.Linear weights of std in^-0.5, gated per row), or cancelling pairs (gallery row i made
    orthogonal to query row i in fp64, so |s_ii| << sum |q||g|)."""
    if kind == "fusion":
        qs = [torch.randn(nq, d, generator=g) * 3 for _ in range(nparts)]
        gs = [(torch.rand(ng, d, generator=g) * 2 - 1) * d ** -0.5 for _ in range(nparts)]
        return qs, gs, [0.5 + 0.25 * p for p in range(nparts)], [torch.rand(nq, generator=g) if p % 2 else None for p in range(nparts)]
    qs = [_unit(nq, d, g) for _ in range(nparts)]
    gs = [_unit(ng, d, g) for _ in range(nparts)]
    if kind == "cancel":
        m = min(nq, ng)
        for q, gg in zip(qs, gs):
            q64, g64 = q[:m].double(), gg[:m].double()
            gg[:m] = (g64 - (g64 * q64).sum(-1, keepdim=True) / (q64 * q64).sum(-1, keepdim=True) * q64).float()
    return qs, gs, [1.0 / nparts] * nparts, None


SCORE_CASES = [  # kind, nq, ng, d, nparts, terms
    ("unit", 1, 1, 64, 1, 1), ("unit", 127, 129, 768, 1, 1), ("unit", 129, 1000, 768, 1, 3), ("unit", 1000, 127, 768, 2, 3),
    ("unit", 129, 257, 384, 4, 3), ("unit", 127, 129, 65, 3, 3), ("cancel", 129, 129, 768, 1, 3), ("cancel", 127, 127, 768, 1, 1),
    ("fusion", 1000, 129, 512, 1, 3), ("fusion", 127, 1000, 768, 2, 3),
]


@pytest.mark.parametrize("kind,nq,ng,d,nparts,terms", SCORE_CASES)
def test_scores_against_panel_emulation(device, kind, nq, ng, d, nparts, terms):
    g = torch.Generator().manual_seed(nq * 7 + ng + d + nparts + terms)
    qs, gs, ps, rs = _score_case(kind, nq, ng, d, nparts, g)
    dv = lambda xs: None if xs is None else [None if x is None else x.to(device) for x in xs]      # noqa: E731
    qp = engine.build_panel(dv(qs), _lib.SIDE_QUERY, terms, part_scale=ps, row_scale=dv(rs))
    gp = engine.build_panel(dv(gs), _lib.SIDE_GALLERY, terms)
    what = f"{kind}_q{nq}_g{ng}_k{qp.kdim}_t{terms}"
    got = engine.scores_dense(qp, gp).cpu()
    ref, extra = R.panel_scores_emulation(qp.data, gp.data, KAPPA, nq, ng)
    top, _ = R.check_budget(got, ref, extra, fmt="fp32", what=what)
    kappa = float(((got.double() - ref).abs() / (extra / KAPPA)).nan_to_num(0.0, 0.0, 0.0).max())
    bias = R.relative_bias(got, ref)
    _note(f"scores_{what}_ratio_relbias_kappa", (round(top, 4), round(bias, 4), round(kappa, 4)))
    if kind != "cancel":                           # cancelling pairs: |s| << its error bar, so the relative bias is not defined there
        assert abs(bias) <= MAX_REL_BIAS, (what, bias)
    # the panels' cost against fp64 of the fp32 inputs, the kernel's accumulation on top
    rep, bound = R.panel_representation_bound(qs, gs, terms, q_part_scale=ps, q_row_scale=rs)
    worst = float(((got.double() - rep).abs() / (bound + extra)).max())
    _note(f"scores_{what}_representation_ratio", round(worst, 4))
    assert worst <= 1.0, (what, worst)
    # pair scores: the same operand roles and k order, bit for bit
    pq = torch.randint(0, nq, (min(4000, nq * ng),), generator=g, dtype=torch.int32)
    pg = torch.randint(0, ng, (pq.numel(),), generator=g, dtype=torch.int32)
    ps_got = engine.pair_scores(qp, gp, pq, pg).cpu()
    assert torch.equal(ps_got, got[pq.long(), pg.long()]), what
