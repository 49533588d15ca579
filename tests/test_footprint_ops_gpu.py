"""GPU: every op-level kernel held to its memory contract (DESIGN.md "Memory contracts"; helper and the three assertions:
tests/footprint.py).  Each case calls the entry point twice through raw pointers -- on tight, separately allocated tensors with zero
pad rows (the call the numerics tests hold to their fp64 budgets), and on windows: inputs in 0xff margins with 0xff pad rows, int
inputs in 0x7fffffff margins, outputs in 0xa5 margins -- and asserts
  A1  the same output bits, A2  every margin intact, A3  the bytes the header says a call leaves alone still 0xa5 (or what they held).
No tolerance anywhere: every assertion is an equality of bits or bytes.  Shapes are the smallest at which each path's ragged edge
exists (a last item's ragged key block and query tile, rows before row 0, pad rows up to ceil256, a d that is no multiple of 64)."""
import ctypes as C

import pytest
import torch

import footprint as F
from footprint import In, IntIn, Out
from knowledge_enhanced_multimodal_retrieval_amd import _lib, debug, engine

pytestmark = pytest.mark.gpu

BF16, F32, U8, FP8 = torch.bfloat16, torch.float32, torch.uint8, torch.float8_e4m3fn


def _both(device, name, specs, what):
    """The entry point `name` on the plain and on the contract arguments (the stream is appended), then A1 / A2 / A3."""
    fn = getattr(_lib.lib(), name)

    def run(*args):
        with torch.cuda.device(device):
            _lib.check(fn(*args, C.c_void_p(torch.cuda.current_stream(device).cuda_stream)), name)
    return F.run_both(run, specs, device, what=what)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _qkv(rows, width, seed, dtype=BF16, qscale=0.25):
    qkv = torch.randn(rows, 3 * width, generator=_gen(seed))
    qkv[:, :width] *= qscale                    # pre-scaled queries: logits of a few units
    return qkv.to(dtype)


# ------------------------------------------------------------------------------------------------ tile attention, heads of 64
# 289 and 321: the route boundaries (the streaming kernel from 289 tokens; its first ragged 64-key chunk and 33-row query block)
@pytest.mark.parametrize("t,causal,batch", [(1, 0, 3), (1, 1, 3), (17, 0, 3), (77, 1, 3), (257, 0, 2), (288, 0, 2), (289, 0, 2), (321, 0, 2)])
def test_attention_heads_of_64(device, t, causal, batch):
    width = 256
    _both(device, "kemr_op_attention", [In(_qkv(batch * t, width, t + causal)), Out((batch * t, width), BF16), batch, t, width, causal],
          f"attention t={t} causal={causal}")


# ------------------------------------------------------------------------------------------------ heads of 80
@pytest.mark.parametrize("batch", [3, 9])
@pytest.mark.parametrize("t", [1, 17, 257, 288])
def test_attention_heads_of_80(device, t, batch):
    width = 240
    specs = [In(_qkv(batch * t, width, 80 + t)), Out((batch * t, width), BF16), batch, t, width, 80, 0]
    outs = []
    for waves in ((0, 4) if t == 257 else (0,)):          # both instantiations of the 257-token shape
        with debug.override(attn80_waves=waves):
            outs.append(_both(device, "kemr_op_attention_hd", specs, f"attention80 t={t} b={batch} waves={waves}").win[1].view.clone())
    for o in outs[1:]:
        assert F.same_bits(o, outs[0])


@pytest.mark.parametrize("tokens", [50, 257, 288])
def test_pooled_row_attention_heads_of_80(device, tokens):
    items, width = 5, 240
    q = (torch.randn(items, width, generator=_gen(tokens)) * 0.25).to(BF16)
    _both(device, "kemr_debug_op_attention_pooled_hd",
          [In(q), In(_qkv(items * tokens, width, 81 + tokens)), Out((items, width), BF16), None, None, items, tokens, width, 80, 0, 0],
          f"pooled80 tokens={tokens}")


@pytest.mark.parametrize("t", [17, 257])
def test_attention_x3_heads_of_80(device, t):
    batch, width = 3, 240
    rows = batch * t
    _both(device, "kemr_op_attention_x3_hd",
          [In(_qkv(rows, width, 82 + t, F32)), Out((F.ceil256(rows), 3 * width), BF16, keep=lambda v: v[rows:]), None, batch, t, width, 80, 0],
          f"attention80_x3 t={t}")


# ------------------------------------------------------------------------------------------------ packed causal attention
def test_packed_causal_attention(device):
    width, lens = 256, [1, 16, 17, 77, 128]
    row_start = torch.tensor([0] + lens).cumsum(0).int()
    rows = int(row_start[-1])
    _both(device, "kemr_debug_op_attention_packed",
          [In(_qkv(rows, width, 5)), Out((rows, width), BF16), IntIn(row_start), len(lens), max(lens), width], "packed attention")


# ------------------------------------------------------------------------------------------------ pooled-row attention, heads of 64
@pytest.mark.parametrize("tokens,force_long,width", [(50, 0, 768), (257, 0, 768), (577, 0, 768), (257, 1, 768), (257, 0, 1024)])
def test_pooled_row_attention_vision(device, tokens, force_long, width):
    items = 3
    q = (torch.randn(items, width, generator=_gen(tokens)) * 0.25).to(BF16)
    _both(device, "kemr_debug_op_attention_pooled",
          [In(q), In(_qkv(items * tokens, width, tokens + width)), Out((items, width), BF16), None, None, items, tokens, width, 0, force_long],
          f"pooled vision tokens={tokens} long={force_long}")


@pytest.mark.parametrize("where", ["first", "last"])
def test_pooled_row_attention_text(device, where):
    """pool_idx at the item's first row (one key) and at its last (all of them, up to the next item's first row)."""
    width, lens = 512, [1, 9, 77]
    row_start = torch.tensor([0] + lens).cumsum(0).int()
    pool_idx = row_start[:-1].clone() if where == "first" else row_start[1:] - 1
    q = (torch.randn(len(lens), width, generator=_gen(3)) * 0.25).to(BF16)
    _both(device, "kemr_debug_op_attention_pooled",
          [In(q), In(_qkv(int(row_start[-1]), width, 44)), Out((len(lens), width), BF16), IntIn(pool_idx), IntIn(row_start), len(lens), 77,
           width, 1, 0], f"pooled text {where}")


# ------------------------------------------------------------------------------------------------ fp32x3 attention, heads of 64
@pytest.mark.parametrize("t,causal", [(17, 0), (17, 1), (257, 0)])
def test_attention_x3(device, t, causal):
    """The output panel has ceil256(rows) rows: those that hold no query keep 0xa5."""
    batch, width = 3, 256
    rows = batch * t
    _both(device, "kemr_op_attention_x3",
          [In(_qkv(rows, width, 30 + t, F32)), Out((F.ceil256(rows), 3 * width), BF16, keep=lambda v: v[rows:]), None, batch, t, width, causal],
          f"attention_x3 t={t} causal={causal}")


def test_attention_x3_packed(device):
    width, lens = 256, [1, 16, 17, 77]
    row_start = torch.tensor([0] + lens).cumsum(0).int()
    rows = int(row_start[-1])
    _both(device, "kemr_op_attention_x3",
          [In(_qkv(rows, width, 31, F32)), Out((F.ceil256(rows), 3 * width), BF16, keep=lambda v: v[rows:]), IntIn(row_start), len(lens), 77,
           width, 1], "attention_x3 packed")


# ------------------------------------------------------------------------------------------------ LayerNorm
def _ln_rows(kind, rows, width, seed):
    x = torch.randn(rows, width, generator=_gen(seed)) + 0.25
    if kind == "f32":
        return x, _lib.KEMR_F32
    if kind == "bf16":
        return x.to(BF16), _lib.KEMR_BF16
    return engine.pack_f24_rows(x), _lib.KEMR_F24          # uint8 [rows, 3 width]


def _ln_out(dtype_code, rows, width):
    if dtype_code == _lib.KEMR_F24:
        return (rows, 3 * width), U8
    return (rows, width), {_lib.KEMR_BF16: BF16, _lib.KEMR_F32: F32, _lib.KEMR_FP8: FP8}[dtype_code]


# Every form launch_layernorm accepts (csrc/layernorm.hip).  Left out because the launcher refuses them: a delta with an fp32 or a
# 24-bit output ("the residual forms write bf16 or fp8"), a second delta without the first or without write-back, and 24-bit output
# rows from bf16 or 24-bit input rows ("24-bit output rows need fp32 input rows").
LN_DELTAS = [("none", 0, 0, 0), ("delta_wb", 1, 0, 1), ("delta", 1, 0, 0), ("two_deltas", 1, 1, 1)]       # name, delta, delta2, writeback


@pytest.mark.parametrize("kind", ["f32", "bf16", "f24"])
@pytest.mark.parametrize("rows", [1, 5, 133])
@pytest.mark.parametrize("width", [256, 1280])
def test_layernorm_rows_every_form(device, width, rows, kind):
    g = _gen(width + rows)
    gamma, beta = 1 + 0.1 * torch.randn(width, generator=g), 0.1 * torch.randn(width, generator=g)
    d1 = (torch.randn(rows, width, generator=g) * 0.5).to(BF16)
    d2 = (torch.randn(rows, width, generator=g) * 0.5).to(BF16)
    x, x_code = _ln_rows(kind, rows, width, 7 * width + rows)
    forms = 0
    for name, use_d1, use_d2, wb in LN_DELTAS:
        outs = [_lib.KEMR_BF16, _lib.KEMR_FP8] if use_d1 else [_lib.KEMR_BF16, _lib.KEMR_F32, _lib.KEMR_FP8] + ([_lib.KEMR_F24] if kind == "f32" else [])
        for out_code in outs:
            # write-back forms: x is an output (0xa5 margins, its body the plain call's x); every other form: x keeps its input bits
            xs = Out(tuple(x.shape), x.dtype, init=x) if wb else In(x)
            shape, dt = _ln_out(out_code, rows, width)
            calls = _both(device, "kemr_op_layernorm_rows",
                          [xs, x_code, In(d1) if use_d1 else None, In(d2) if use_d2 else None, wb, In(gamma), In(beta), Out(shape, dt), rows,
                           width, out_code], f"layernorm {kind} {name} out={out_code} rows={rows} width={width}")
            if wb:
                assert not torch.equal(F.bits(calls.win[0].view).cpu(), F.bits(x))          # the sum did replace x
            forms += 1
    assert forms == (9 if kind != "f32" else 10)


@pytest.mark.parametrize("rows", [5, 133])
def test_layernorm_x3_zero_fills_its_pad_rows(device, rows):
    width = 256
    g = _gen(rows)
    x = torch.randn(rows, width, generator=g) + 0.25
    gamma, beta = 1 + 0.1 * torch.randn(width, generator=g), 0.1 * torch.randn(width, generator=g)
    calls = _both(device, "kemr_op_layernorm_x3", [In(x), In(gamma), In(beta), Out((F.ceil256(rows), 3 * width), BF16), rows, width],
                  f"layernorm_x3 rows={rows}")
    assert F.all_bytes(calls.win[3].view[rows:], 0)                 # include/kemr.h: pad rows zero-filled
    assert F.all_bytes(calls.plain[3][rows:], 0)


# ------------------------------------------------------------------------------------------------ GEMM
EPI_NAMES = {_lib.EPI_BIAS_BF16: "BIAS_BF16", _lib.EPI_BIAS_QGELU_BF16: "QGELU", _lib.EPI_BIAS_GELU_BF16: "GELU",
             _lib.EPI_BIAS_TGELU_BF16: "TGELU", _lib.EPI_BIAS_RESID_F32: "RESID_F32"}


def _gemm_operands(m, n, k, seed):
    g = _gen(seed)
    a = torch.zeros(F.ceil256(m), k)
    a[:m] = torch.randn(m, k, generator=g)
    w = torch.randn(n, k, generator=g) * k ** -0.5
    bias = torch.randn(n, generator=g)
    return a, w, bias


# At m = 300 every variant accepts the five epilogues below (csrc/gemm.hip launch_gemm: 1 = the 128 x 128 kernel, 2 and 7 = the
# 256 x 256 kernel -- the persistent one takes more than 512 rows only --, 8 = the skinny kernel for the bf16 stores, the 256 x 256
# kernel for RESID_F32).  RESADD_BF16 is refused at m = 300 by every variant ("the residual-add epilogue needs ... more than 512
# rows"): it runs at m = 600 below.
@pytest.mark.parametrize("epi", sorted(EPI_NAMES), ids=lambda e: EPI_NAMES[e])
@pytest.mark.parametrize("variant", [1, 2, 7, 8])
def test_gemm_operand_side(device, variant, epi):
    """A's pad rows 300 .. 511 are NaN, W and the bias sit in NaN margins, C has guard margins in front as well as behind.  bf16
    stores: rows < m have the plain call's bits (the pad rows of C may be written: include/kemr.h); RESID_F32 (read-modify-write, the
    tile kernels with row masks at m <= 512): C's pad rows keep their bytes."""
    m, n, k = 300, 768, 256
    a, w, bias = _gemm_operands(m, n, k, 1)
    if epi == _lib.EPI_BIAS_RESID_F32:
        c0 = torch.randn(F.ceil256(m), n, generator=_gen(2))
        c = Out((F.ceil256(m), n), F32, init=c0, keep=lambda v: v[m:])
    else:
        c = Out((F.ceil256(m), n), BF16, written=lambda v: v[:m])
    with debug.override(gemm_variant=variant):
        _both(device, "kemr_op_gemm", [In(a.to(BF16), valid_rows=m), In(w.to(BF16)), In(bias), c, m, n, k, epi],
              f"gemm variant={variant} epi={EPI_NAMES[epi]}")


def test_gemm_residual_add_bf16(device):
    """RESADD_BF16 (the persistent kernel, whole 256-row tiles: C's pad rows 600 .. 767 are scratch) at the smallest m it accepts a
    ragged tile at."""
    m, n, k = 600, 768, 256
    a, w, bias = _gemm_operands(m, n, k, 3)
    x0 = torch.randn(F.ceil256(m), n, generator=_gen(4)).to(BF16)
    _both(device, "kemr_op_gemm", [In(a.to(BF16), valid_rows=m), In(w.to(BF16)), In(bias), Out((F.ceil256(m), n), BF16, init=x0, written=lambda v: v[:m]),
                                   m, n, k, _lib.EPI_BIAS_RESADD_BF16], "gemm RESADD_BF16")


@pytest.mark.parametrize("epi", [_lib.EPI_BIAS_BF16, _lib.EPI_BIAS_QGELU_BF16, _lib.EPI_BIAS_GELU_BF16], ids=lambda e: EPI_NAMES[e])
def test_gemm_fp8_operand_side(device, epi):
    m, n, k = 300, 768, 256
    g = _gen(5)
    a = torch.zeros(F.ceil256(m), k)
    a[:m] = torch.randint(-8, 9, (m, k), generator=g).float()
    w = torch.randint(-8, 9, (n, k), generator=g).float()
    wscale = 2.0 ** torch.randint(-6, -2, (n,), generator=g).float()
    bias = torch.randn(n, generator=g)
    _both(device, "kemr_op_gemm_fp8", [In(a.to(FP8), valid_rows=m), In(w.to(FP8)), In(wscale), In(bias),
                                       Out((F.ceil256(m), n), BF16, written=lambda v: v[:m]), m, n, k, epi], f"gemm_fp8 epi={EPI_NAMES[epi]}")


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_gemm_x3(device, mode):
    """Modes 0 / 1: C is fp32 [m, n] with EXACTLY m rows -- the 0xa5 margin starts at row 300, inside the last 128-row tile.  Modes
    2 / 3: the triple [ceil256(m), 3 n]; rows m .. are not written."""
    m, n, k = 300, 256, 256
    g = _gen(6)
    a = engine.build_panel([torch.randn(m, k, generator=g).to(device)], _lib.SIDE_QUERY, 3).data.cpu()
    w = engine.build_panel([(torch.randn(n, k, generator=g) * k ** -0.5).to(device)], _lib.SIDE_GALLERY, 3).data.cpu()
    assert tuple(a.shape) == (F.ceil256(m), 3 * k) and tuple(w.shape) == (n, 3 * k) and float(a[m:].abs().max()) == 0
    bias = torch.randn(n, generator=g)
    if mode == 0:
        c = Out((m, n), F32)
    elif mode == 1:
        c = Out((m, n), F32, init=torch.randn(m, n, generator=g))
    else:
        c = Out((F.ceil256(m), 3 * n), BF16, keep=lambda v: v[m:])
    _both(device, "kemr_op_gemm_x3", [In(a, valid_rows=m), In(w), In(bias), c, m, n, 3 * k, mode], f"gemm_x3 mode={mode}")


# ------------------------------------------------------------------------------------------------ pooling tail
@pytest.mark.parametrize("form", ["cls", "argmax", "packed"])
@pytest.mark.parametrize("kind", ["f32", "bf16", "f24"])
def test_tail(device, kind, form):
    """d = 68: the second column block holds 4 of its 64 columns.  cls: the rows b * tokens; argmax: the first row maximum of ids,
    with both deltas; packed: inside row_start's rows, one item of length 1 (its pooled position clamps to that row)."""
    batch, tokens, width, d = 5, 16, 512, 68
    g = _gen(9)
    lens = [1, 5, 16, 3, 16]
    row_start = torch.tensor([0] + lens).cumsum(0).int()
    rows = int(row_start[-1]) if form == "packed" else batch * tokens
    x, code = _ln_rows(kind, rows, width, 10)
    d1 = (torch.randn(rows, width, generator=g) * 0.5).to(BF16)
    d2 = (torch.randn(rows, width, generator=g) * 0.5).to(BF16)
    gamma, beta = 1 + 0.1 * torch.randn(width, generator=g), 0.1 * torch.randn(width, generator=g)
    proj = torch.randn(width, d, generator=g) * width ** -0.5
    ids = torch.randint(0, 1000, (batch, tokens), generator=g, dtype=torch.int32)
    pos = torch.tensor([3, 4, 15, 0, 7])
    ids[torch.arange(batch), pos] = 5000
    ids[2, 15] = 0
    ids[2, 9] = 5000
    ids[2, 12] = 5000                                         # the maximum twice: the first position wins
    results = []
    for normalize in (0, 1):
        specs = [In(x), code, None if form == "cls" else In(d1), None if form == "cls" else In(d2), None if form == "cls" else IntIn(ids),
                 IntIn(row_start) if form == "packed" else None, batch, tokens, width, In(gamma), In(beta), In(proj), d, normalize,
                 Out((batch, d), F32)]
        results.append(_both(device, "kemr_debug_op_tail", specs, f"tail {kind} {form} normalize={normalize}").win[14].view.clone())
    assert bool(torch.isfinite(results[0]).all()) and not torch.equal(results[0], results[1])
