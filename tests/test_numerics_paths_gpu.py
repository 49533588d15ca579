"""GPU: the kernels a tower reaches only inside itself, held to fp64 statements of what they compute (oracle/rounding.py):

* the streaming attention of T > 288 (csrc/attention_stream.hip) against attention_long_emulation -- P rounded to bf16 against the
  running max of 64-key chunks -- at ragged lengths, through the rescale edge cases, per image and inside its output rows;
* the pooled-row attention of the last block (attention_pooled_kernel<320> / <1088>), vision and text (causal, packed) forms;
* the causal attention over packed texts (launch_attention_packed) against the per-item causal statement;
* the pooling tail (tail_proj_kernel + l2norm_rows_kernel) on every row format, pooling rule and width.
bf16 outputs: budget ratio <= 1 and |signed bias| <= 0.02 ulp over the outputs the final rounding dominates.  fp32 tail outputs:
budget ratio <= 1 (fp32 ulps) and |relative bias| <= TAIL_MAX_REL_BIAS.  The fp64 references run on the CPU.  Every measured
worst ratio / bias is printed (pytest -s)."""
import ctypes as C

import pytest
import torch

from knowledge_enhanced_multimodal_retrieval_amd import _lib, debug, engine
from oracle import rounding as R

pytestmark = pytest.mark.gpu

MAX_BIAS = 0.02
MAXK_LONG = 1088            # (KEMR_MAX_VISION_TOKENS + 63) / 64 * 64: the long instantiation of the pooled-row kernel
TAIL_KAPPA = 1              # projection accumulator: |acc - ref64| <= TAIL_KAPPA 2^-24 sum|y||P|; 2 x the worst measured (0.453), cap 16
LN_F32_FACTOR = 2.0 ** -21  # fp32 LayerNorm outputs within 2^-21 max|y| (tests/test_numerics_gpu.py)
TAIL_MAX_REL_BIAS = 4       # units of 2^-24 (rounding.relative_bias); outputs 2^-20 too large read 16


def _note(name, value):
    print(f"NUMERICS {name} {value}")


def _check(got, ref, extra, what, max_bias=MAX_BIAS, rounding_only=True):
    """rounding_only: the bias over the outputs whose extra is below a quarter ulp (rounding.signed_bias_ulps); attention_emulation's
    extra (the tile kernels) is above that almost everywhere, so its checks take every output, as tests/test_numerics_gpu.py does."""
    top, bias = R.check_budget(got.cpu(), ref, extra, max_bias=max_bias, what=what, bias_rounding_only=rounding_only)
    _note(f"{what}_ratio_bias", (round(top, 4), round(bias, 5)))
    return top, bias


def _qkv(rows, width, seed, qscale=0.25):
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(rows, 3 * width, generator=g)
    qkv[:, :width] *= qscale                    # pre-scaled queries: logits of a few units
    return qkv.to(torch.bfloat16)


# ------------------------------------------------------------------------------------------------ streaming attention
def _check_long(device, qkv_bf, batch, t, width, what):
    got = engine.op_attention(qkv_bf.to(device), batch, t, width, False)
    ref, extra = R.attention_long_emulation(qkv_bf, batch, t, width)
    _check(got, ref, extra, what)
    return got


# 385 = 3 x 128 + 1: the last query block holds one row; 320 / 1024: whole 64-key chunks; 321 / 577 / 1025: one key in the last
@pytest.mark.parametrize("t,batch,width", [(289, 3, 256), (320, 3, 256), (321, 3, 256), (385, 3, 256), (577, 3, 256), (600, 2, 256),
                                           (1024, 2, 256), (1025, 2, 256), (577, 1, 1024)])
def test_long_attention_against_chunked_emulation(device, t, batch, width):
    _check_long(device, _qkv(batch * t, width, 100 + t + width), batch, t, width, f"attn_long_t{t}_b{batch}_w{width}")


@pytest.mark.parametrize("case", ["spike_first_chunk", "spike_last_ragged_chunk", "max_moves_every_chunk", "max_creeps"])
def test_long_attention_online_rescale_against_chunked_emulation(device, case):
    """tests/test_attention_long_gpu.py::test_online_rescale's inputs.  Most outputs of a spike row sit just below a bf16 value (one
    key takes nearly all the weight), so their exact values do not spread over the ulp interval: the ratio bar only there."""
    t, batch, width = 577, 2, 256
    g = torch.Generator().manual_seed(11)
    qkv = torch.randn(batch * t, 3 * width, generator=g) * 0.1
    qkv[:, :width] *= 0.5
    for hd in range(width // 64):
        qkv[:, hd * 64] = 4.0
        if case == "max_moves_every_chunk":
            qkv[:, width + hd * 64] = torch.linspace(-8, 8, t).repeat(batch)
        elif case == "max_creeps":
            qkv[:, width + hd * 64] = torch.linspace(-2, 2, t).repeat(batch)
        else:
            spike = 5 if case == "spike_first_chunk" else t - 1
            for b in range(batch):
                qkv[b * t + spike, width + hd * 64] = 5.0
    qkv = qkv.to(torch.bfloat16)
    got = engine.op_attention(qkv.to(device), batch, t, width, False)
    ref, extra = R.attention_long_emulation(qkv, batch, t, width)
    _check(got, ref, extra, f"attn_long_{case}", max_bias=None if case.startswith("spike") else MAX_BIAS)


def test_long_attention_images_are_isolated(device):
    """Image 0's output does not depend on image 1's rows: bit-identical with image 1 all zeros or all +-1e4."""
    t, width = 577, 256
    qkv = _qkv(2 * t, width, 7)
    a, b = qkv.clone(), qkv.clone()
    a[t:] = 0
    g = torch.Generator().manual_seed(8)
    b[t:] = (torch.randint(0, 2, (t, 3 * width), generator=g) * 2 - 1).to(torch.bfloat16) * 1e4
    oa = engine.op_attention(a.to(device), 2, t, width, False).cpu()
    ob = engine.op_attention(b.to(device), 2, t, width, False).cpu()
    assert torch.isfinite(ob[:t].float()).all()
    assert torch.equal(oa[:t], ob[:t])
    assert torch.equal(oa[:t], engine.op_attention(qkv[:t].to(device), 1, t, width, False).cpu())


@pytest.mark.parametrize("t,batch", [(385, 2), (577, 1), (1025, 1)])
def test_long_attention_writes_only_its_rows(device, t, batch):
    """kemr_op_attention called on a window of a larger buffer: the guard rows around [B T, W] keep their sentinel."""
    width, guard = 256, 64
    qkv = _qkv(batch * t, width, 9).to(device)
    sentinel = torch.tensor(-12345.0, dtype=torch.bfloat16)
    buf = torch.full(((batch * t + 2 * guard), width), float(sentinel), dtype=torch.bfloat16, device=device)
    L = _lib.lib()
    with torch.cuda.device(device):
        _lib.check(L.kemr_op_attention(C.c_void_p(qkv.data_ptr()), C.c_void_p(buf.data_ptr() + guard * width * 2), batch, t, width, 0,
                                       C.c_void_p(torch.cuda.current_stream(device).cuda_stream)), "op_attention")
    torch.cuda.synchronize(device)
    buf = buf.cpu()
    assert bool((buf[:guard] == sentinel).all()) and bool((buf[guard + batch * t:] == sentinel).all())
    assert torch.equal(buf[guard:guard + batch * t], engine.op_attention(qkv, batch, t, width, False).cpu())


# ------------------------------------------------------------------------------------------------ pooled-row attention
def _pooled(device, q, qkv, pool_idx, row_start, tokens, causal, force_long=False):
    dv = lambda x: None if x is None else x.to(device)          # noqa: E731
    return debug.op_attention_pooled(q.to(device), qkv.to(device), dv(pool_idx), dv(row_start), tokens, causal, force_long).cpu()


@pytest.mark.parametrize("width", [768, 1024])
@pytest.mark.parametrize("tokens", [50, 257, 320, 321, 577, 1025])
def test_pooled_row_vision_against_fp64(device, tokens, width):
    items = 8
    qkv = _qkv(items * tokens, width, tokens + width)
    q = (torch.randn(items, width, generator=torch.Generator().manual_seed(tokens)) * 0.25).to(torch.bfloat16)
    maxk = 320 if tokens <= 320 else MAXK_LONG
    got = _pooled(device, q, qkv, None, None, tokens, False)
    ref, extra = R.attention_pooled_emulation(q, qkv, None, None, items, tokens, width, False, maxk)
    _check(got, ref, extra, f"pooled_vision_t{tokens}_w{width}")
    if tokens <= 320:            # the 1088-key instantiation gives the same bits where both apply (csrc/attention.hip)
        assert torch.equal(_pooled(device, q, qkv, None, None, tokens, False, force_long=True), got)


def _text_items(lens, positions, width, seed):
    g = torch.Generator().manual_seed(seed)
    lens = torch.tensor(lens, dtype=torch.int64)
    row_start = torch.cat([torch.zeros(1, dtype=torch.int64), lens.cumsum(0)]).int()
    qkv = _qkv(int(lens.sum()), width, seed)
    q = (torch.randn(len(lens), width, generator=g) * 0.25).to(torch.bfloat16)
    pool_idx = (row_start[:-1] + torch.tensor(positions, dtype=torch.int32)).int()
    return q, qkv, pool_idx, row_start


@pytest.mark.parametrize("force_long", [False, True])
def test_pooled_row_text_packed_against_fp64(device, force_long):
    """Causal form on packed texts of lengths 1 .. 77, pooled at the first, a middle and the last row; one more item whose pooled
    position lies before its first row (nk clamps to 1): its output is v[r0], bit for bit."""
    width = 512
    lens, pos = [], []
    for n in (1, 2, 7, 8, 9, 64, 65, 77):
        for p in sorted({0, n // 2, n - 1}):
            lens.append(n)
            pos.append(p)
    lens.append(5)
    pos.append(-3)
    q, qkv, pool_idx, row_start = _text_items(lens, pos, width, 41)
    items = len(lens)
    got = _pooled(device, q, qkv, pool_idx, row_start, 77, True, force_long)
    ref, extra = R.attention_pooled_emulation(q, qkv, pool_idx, row_start, items, 77, width, True, MAXK_LONG if force_long else 320)
    _check(got, ref, extra, f"pooled_text_packed{'_long' if force_long else ''}")
    assert torch.equal(got[-1], qkv[int(row_start[-2]), 2 * width:])
    if force_long:
        assert torch.equal(got, _pooled(device, q, qkv, pool_idx, row_start, 77, True))


def test_pooled_row_text_full_context_against_fp64(device):
    """Causal form without row_start (item b = rows b 77 ..), pooled at positions 0, 38 and 76; clamped item at the end."""
    width, ctx = 512, 77
    pos = [0, 38, 76] * 3 + [0, 76, 38]
    items = len(pos)
    qkv = _qkv(items * ctx, width, 43)
    q = (torch.randn(items, width, generator=torch.Generator().manual_seed(44)) * 0.25).to(torch.bfloat16)
    pool_idx = (torch.arange(items) * ctx + torch.tensor(pos)).int()
    pool_idx[-1] = (items - 1) * ctx - 10                              # before its first row: nk = 1
    got = _pooled(device, q, qkv, pool_idx, None, ctx, True)
    ref, extra = R.attention_pooled_emulation(q, qkv, pool_idx, None, items, ctx, width, True, 320)
    _check(got, ref, extra, "pooled_text_ctx77")
    assert torch.equal(got[-1], qkv[(items - 1) * ctx, 2 * width:])


# ------------------------------------------------------------------------------------------------ packed causal attention
def _packed_emulation(qkv, row_start, width):
    ref, extra = torch.empty(qkv.shape[0], width, dtype=torch.float64), torch.empty(qkv.shape[0], width, dtype=torch.float64)
    for b in range(len(row_start) - 1):
        a, e = int(row_start[b]), int(row_start[b + 1])
        ref[a:e], extra[a:e] = R.attention_emulation(qkv[a:e], 1, e - a, width, True)
    return ref, extra


def test_packed_causal_attention_against_per_item_emulation(device):
    """~300 texts of lengths 1 .. 77 packed behind one another (max_t = 77: the 4-wave run-time-T instantiation), and the same
    lengths at full context 77 (the 5-wave 77-token instantiation, which packed rows never take): both within the budget of the
    per-item causal statement."""
    width = 256
    g = torch.Generator().manual_seed(51)
    lens = [1, 16, 17, 32, 33, 76, 77] + torch.randint(1, 78, (293,), generator=g).tolist()
    row_start = torch.tensor([0] + lens).cumsum(0).int()
    qkv = _qkv(int(row_start[-1]), width, 52)
    got = debug.op_attention_packed(qkv.to(device), row_start.to(device), 77, width).cpu()
    ref, extra = _packed_emulation(qkv, row_start, width)
    _check(got, ref, extra, "packed_causal_300", rounding_only=False)
    starts = row_start[:-1].long()
    assert torch.equal(got[starts], qkv[starts, 2 * width:])          # row 0 of every text sees one key: its V row, exactly
    full = _qkv(40 * 77, width, 53)
    gotf = engine.op_attention(full.to(device), 40, 77, width, True)
    reff, extraf = R.attention_emulation(full, 40, 77, width, True)
    _check(gotf, reff, extraf, "causal_ctx77_5wave", rounding_only=False)


# ------------------------------------------------------------------------------------------------ pooling tail
def _rows(kind, x32):
    """The stored rows (device form) and the values the kernel reads from them, exactly."""
    if kind == "f32":
        return x32, x32, _lib.KEMR_F32
    if kind == "bf16":
        xb = x32.to(torch.bfloat16)
        return xb, xb.float(), _lib.KEMR_BF16
    x24 = engine.pack_f24_rows(x32)
    return x24, engine.unpack_f24_rows(x24, x32.shape[1]), _lib.KEMR_F24


def _tail_case(batch, tokens, width, d, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(batch * tokens, width, generator=g) + 0.25
    d1 = (torch.randn(batch * tokens, width, generator=g) * 0.5).to(torch.bfloat16)
    d2 = (torch.randn(batch * tokens, width, generator=g) * 0.5).to(torch.bfloat16)
    gamma = 1 + 0.1 * torch.randn(width, generator=g)
    beta = 0.1 * torch.randn(width, generator=g)
    proj = torch.randn(width, d, generator=g) * width ** -0.5
    return x, d1, d2, gamma, beta, proj


def _run_tail(device, xdev, dtype, d1, d2, ids, row_start, batch, tokens, width, gamma, beta, proj, normalize):
    dv = lambda t: None if t is None else t.to(device)          # noqa: E731
    return debug.op_tail(xdev.to(device), dtype, dv(d1), dv(d2), dv(ids), dv(row_start), batch, tokens, width, gamma.to(device),
                         beta.to(device), proj.to(device), normalize).cpu()


def _check_tail(device, what, xdev, dtype, xread, d1, d2, prow, ids, row_start, batch, tokens, width, gamma, beta, proj):
    """normalize = 0 against tail_emulation of the rows at prow; normalize = 1 against l2norm_emulation of that same output."""
    xs = xread[prow]
    if d1 is not None:
        xs = xs + d1.float()[prow]                           # (x + d1) + d2 in fp32, the kernel's order
    if d2 is not None:
        xs = xs + d2.float()[prow]
    got = _run_tail(device, xdev, dtype, d1, d2, ids, row_start, batch, tokens, width, gamma, beta, proj, False)
    ref, extra = R.tail_emulation(xs, gamma, beta, proj, TAIL_KAPPA, LN_F32_FACTOR)
    top, bias = R.check_budget(got, ref, extra, fmt="fp32", what=what)
    rel = R.relative_bias(got, ref)
    assert abs(rel) <= TAIL_MAX_REL_BIAS, (what, rel)
    _note(f"{what}_ratio_relbias", (round(top, 4), round(rel, 3)))
    gotn = _run_tail(device, xdev, dtype, d1, d2, ids, row_start, batch, tokens, width, gamma, beta, proj, True)
    refn, extran = R.l2norm_emulation(got)
    topn, _ = R.check_budget(gotn, refn, extran, fmt="fp32", what=f"{what}_l2")
    reln = R.relative_bias(gotn, refn)
    assert abs(reln) <= TAIL_MAX_REL_BIAS, (what, reln)
    _note(f"{what}_l2_ratio_relbias", (round(topn, 4), round(reln, 3)))


@pytest.mark.parametrize("width,d", [(512, 68), (768, 512), (1024, 768), (1280, 1024)])
def test_tail_projection_accumulator(device, width, d):
    """gamma = 0: the LayerNorm output is beta exactly, so what is measured is the projection's fp32 accumulator alone:
    |out - beta @ proj| / (2^-24 sum|beta||P|) = the kernel's kappa (0.385 .. 0.453 on the MI355X); TAIL_KAPPA is 2 x the worst."""
    batch = 32
    x, _, _, _, _, proj = _tail_case(batch, 1, width, d, width + d)
    beta = torch.randn(width, generator=torch.Generator().manual_seed(3))
    got = _run_tail(device, x, _lib.KEMR_F32, None, None, None, None, batch, 1, width, torch.zeros(width), beta, proj, False)
    b64, p64 = beta.double().expand(batch, -1), proj.double()
    kappa = float(((got.double() - b64 @ p64).abs() / (2.0 ** -24 * (b64.abs() @ p64.abs()))).max())
    _note(f"tail_kappa_w{width}_d{d}", round(kappa, 3))
    assert kappa <= TAIL_KAPPA, kappa


@pytest.mark.parametrize("kind", ["f32", "f24", "bf16"])
@pytest.mark.parametrize("deltas", [0, 1, 2])
def test_tail_cls_rows_against_fp64(device, kind, deltas):
    """CLS pooling (ids NULL): the compact form of the product (tokens = 1) and the full rows (tokens = T: row b T)."""
    width, d = 768, 512
    for batch, tokens in ((32, 1), (16, 50)):
        x, d1, d2, gamma, beta, proj = _tail_case(batch, tokens, width, d, 60 + deltas + tokens)
        xdev, xread, dt = _rows(kind, x)
        prow = torch.arange(batch) * tokens
        _check_tail(device, f"tail_cls_{kind}_d{deltas}_t{tokens}", xdev, dt, xread, d1 if deltas >= 1 else None,
                    d2 if deltas == 2 else None, prow, None, None, batch, tokens, width, gamma, beta, proj)


@pytest.mark.parametrize("width,d", [(512, 68), (640, 512), (1024, 768), (1280, 1024)])
def test_tail_eot_rows_against_fp64(device, width, d):
    """EOT pooling: the first position of the row maximum of the ids wins (the maximum repeated at later positions)."""
    batch, tokens = 24, 77
    x, d1, d2, gamma, beta, proj = _tail_case(batch, tokens, width, d, width + 7)
    g = torch.Generator().manual_seed(71)
    ids = torch.randint(0, 1000, (batch, tokens), generator=g, dtype=torch.int32)
    first = torch.randint(0, tokens, (batch,), generator=g)
    for b in range(batch):
        ids[b, first[b]:] = torch.where(torch.rand(tokens - first[b], generator=g) < 0.3, 5000, ids[b, first[b]:])
        ids[b, first[b]] = 5000
    assert torch.equal(ids.long().argmax(-1), first)
    xdev, xread, dt = _rows("f24", x)
    _check_tail(device, f"tail_eot_w{width}_d{d}", xdev, dt, xread, d1, d2, torch.arange(batch) * tokens + first, ids, None,
                batch, tokens, width, gamma, beta, proj)


def test_tail_packed_rows_clamp_to_the_last_row(device):
    """Packed rows (row_start): the pooled position inside the text's rows; one beyond the text's length reads its last row."""
    width, d, tokens = 512, 512, 77
    g = torch.Generator().manual_seed(81)
    lens = torch.randint(1, tokens + 1, (24,), generator=g)
    lens[:4] = torch.tensor([1, 5, 30, 70])
    batch = len(lens)
    row_start = torch.cat([torch.zeros(1, dtype=torch.int64), lens.cumsum(0)]).int()
    rows = int(row_start[-1])
    x, d1, d2, gamma, beta, proj = _tail_case(rows, 1, width, d, 82)
    ids = torch.randint(0, 1000, (batch, tokens), generator=g, dtype=torch.int32)
    pos = torch.randint(0, tokens, (batch,), generator=g)
    pos[:4] = lens[:4] + 3                                    # beyond the text: clamped
    pos[4] = lens[4] - 1
    ids[torch.arange(batch), pos] = 5000
    prow = row_start[:-1].long() + torch.minimum(pos, lens - 1)
    xdev, xread, dt = _rows("bf16", x)
    _check_tail(device, "tail_packed_clamp", xdev, dt, xread, d1, d2, prow, ids, row_start, batch, tokens, width, gamma, beta, proj)


def test_tail_refusals(device):
    width = 512
    x = torch.zeros(2, width, device=device)
    gamma, beta = torch.ones(width, device=device), torch.zeros(width, device=device)
    with pytest.raises(RuntimeError, match="multiple of 4"):
        debug.op_tail(x, _lib.KEMR_F32, None, None, None, None, 2, 1, width, gamma, beta, torch.zeros(width, 70, device=device), False)
    with pytest.raises(RuntimeError, match="65535"):
        debug.op_tail(x, _lib.KEMR_F32, None, None, None, None, 65536, 1, width, gamma, beta, torch.zeros(width, 64, device=device), False)
    with pytest.raises(RuntimeError, match="dtype"):
        debug.op_tail(x, _lib.KEMR_FP8, None, None, None, None, 2, 1, width, gamma, beta, torch.zeros(width, 64, device=device), False)
