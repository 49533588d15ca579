"""GPU: a 248-position CLIP text tower on the packed causal path (Long-CLIP; the tiny test architecture config.ARCHS["tiny-ctx248"],
random weights from the oracle's generator): kemr_encode_text_packed / _packed_pooled at ctx > 128 against the CPU oracle and against
the dense route, the workspace contract of the packed call, and what stays refused (fp32x3 packed above 128)."""
import ctypes as C

import pytest
import torch

import footprint as F
import longclip_ref as L
import test_footprint_towers_gpu as TOWERS
from footprint import IntIn, Out, SizeOf, Work
from knowledge_enhanced_multimodal_retrieval_amd import _lib, engine

pytestmark = pytest.mark.gpu

BAR = 1e-3                    # the project's bar on 1 - cos against the fp32 oracle (tests/test_encoder_gpu.py)
F32 = torch.float32


def _engine(device, precision, weights="plain"):
    eng = engine.ClipEngine(L.ARCH, device, precision=precision)
    eng.load_state_dict(L.state_dict(weights))
    return eng


def _stream(device):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _packed_call(eng, device, ids, lens, pooled=False):
    """kemr_encode_text_packed (or _packed_pooled) called directly: (status, out, message)."""
    lib = _lib.lib()
    n, rows = ids.shape[0], int(lens.sum())
    ids_d, lens_d = ids.to(device).contiguous(), lens.to(device=device, dtype=torch.int32).contiguous()
    out = torch.zeros((n, L.ARCH.t_width if pooled else L.ARCH.embed_dim), dtype=F32, device=device)
    ws = torch.empty(max(256, int(lib.kemr_text_packed_workspace_bytes(eng._h, rows, n)) + 4096), dtype=torch.uint8, device=device)
    head = (eng._h, C.c_void_p(ids_d.data_ptr()), C.c_void_p(lens_d.data_ptr()), rows, n, C.c_void_p(out.data_ptr()))
    tail = (C.c_void_p(ws.data_ptr()), ws.numel(), _stream(device))
    with torch.cuda.device(device):
        rc = lib.kemr_encode_text_packed_pooled(*head, *tail) if pooled else lib.kemr_encode_text_packed(*head, 0, *tail)
    torch.cuda.synchronize(device)
    return rc, out, (lib.kemr_last_error() or b"").decode()


def test_direct_packed_call_is_served_at_ctx_248(device):
    """The call the library refused before ("context length 248 > 128") returns 0 and gives the oracle's embeddings."""
    ids, ref = L.oracle_text("plain")
    lens = torch.tensor(L.TEXT_LENGTHS, dtype=torch.int32)
    eng = _engine(device, "bf16")
    assert int(_lib.lib().kemr_text_packed_workspace_bytes(eng._h, int(lens.sum()), len(lens))) > 0
    rc, out, msg = _packed_call(eng, device, ids, lens)
    assert rc == 0, (rc, msg)
    worst = float(L.one_minus_cos(out, ref).max())
    print(f"NUMERICS longclip_direct_packed_1_minus_cos {worst:.3e}")
    assert worst <= BAR


@pytest.mark.parametrize("weights", ["plain", "heavy"])
@pytest.mark.parametrize("precision", ["bf16-x24", "bf16"])
def test_packed_and_dense_routes_against_the_oracle(device, precision, weights):
    """Texts whose end-of-text tokens sit at positions 0 .. 247 (lengths 1 .. 248, both sides of every tile, chunk and query-block edge):
    the packed route (the default), the dense route (pack_text = False) and the two against each other, 1 - cos <= 1e-3 each."""
    ids, ref = L.oracle_text(weights)
    eng = _engine(device, precision, weights)
    assert eng.pack_text
    packed = eng.encode_text(ids)                       # host ids: the lengths are read from them
    eng.pack_text = False
    dense = eng.encode_text(ids)
    assert bool(torch.isfinite(packed).all()) and bool(torch.isfinite(dense).all())
    cp, cd, cm = (float(L.one_minus_cos(a, b).max()) for a, b in ((packed, ref), (dense, ref), (packed, dense)))
    print(f"NUMERICS longclip_tower_{precision}_{weights}_1_minus_cos packed {cp:.3e} dense {cd:.3e} packed_vs_dense {cm:.3e}")
    assert cp <= BAR and cd <= BAR and cm <= BAR, (cp, cd, cm)
    # the shuffled batch gives every text the bits it had: a text's embedding does not depend on what is packed around it
    perm = torch.randperm(len(L.TEXT_LENGTHS), generator=torch.Generator().manual_seed(5))
    eng.pack_text = True
    assert torch.equal(eng.encode_text(ids[perm]), packed[perm.to(device)])


def test_pooled_rows_packed_against_dense(device):
    """encode_text_pooled (the rows finetune.ProjectionHeads trains on): the packed route against the dense one, per row within the bar,
    and through ln_final + text_projection the embeddings of encode_text."""
    ids, _ = L.oracle_text("plain")
    eng = _engine(device, "bf16-x24")
    packed = eng.encode_text_pooled(ids)
    eng.pack_text = False
    dense = eng.encode_text_pooled(ids)
    assert tuple(packed.shape) == (len(L.TEXT_LENGTHS), L.ARCH.t_width) and bool(torch.isfinite(packed).all())
    worst = float(L.one_minus_cos(packed, dense).max())
    print(f"NUMERICS longclip_pooled_packed_vs_dense_1_minus_cos {worst:.3e}")
    assert worst <= BAR
    sd = L.state_dict("plain")
    head = torch.nn.functional.layer_norm(packed.cpu(), (L.ARCH.t_width,), sd["ln_final.weight"], sd["ln_final.bias"], 1e-5) @ sd["text_projection"]
    eng.pack_text = True
    assert float(L.one_minus_cos(head, eng.encode_text(ids)).max()) <= BAR


@pytest.mark.parametrize("precision", ["bf16-x24", "fp8"])
def test_packed_workspace_is_exactly_sufficient(device, precision):
    """tests/footprint.py on kemr_encode_text_packed at ctx 248: a workspace of exactly kemr_text_packed_workspace_bytes, every byte
    0xff inside guard margins, gives the roomy call's bits with every margin intact; 256 bytes fewer, or a pointer moved by 128 bytes,
    is KEMR_ERR_WORKSPACE with nothing launched.  (fp8: its text tower is the bf16 one.)"""
    lib = _lib.lib()
    eng = _engine(device, precision)
    lens = torch.tensor([1, 248, 129, 5], dtype=torch.int32)
    ids = L.ids_of_lengths(lens.tolist())
    rows, batch = int(lens.sum()), len(lens)
    need = int(lib.kemr_text_packed_workspace_bytes(eng._h, rows, batch))
    assert need > 0
    for pooled in (True, False):
        eng.set_last_block_pooled_row(pooled)
        calls = TOWERS._both(device, lib.kemr_encode_text_packed,
                             [eng._h, IntIn(ids), IntIn(lens), rows, batch, Out((batch, L.ARCH.embed_dim), F32), 1,
                              Work(need, need + (1 << 20), 48 * L.ARCH.t_width), SizeOf(7)], f"encode_text_packed ctx248 {precision} pooled={int(pooled)}")
        assert bool(torch.isfinite(calls.win[5].view).all())
        TOWERS._refusals(device, lib.kemr_encode_text_packed, calls, 7, 5, f"encode_text_packed ctx248 {precision}")


def test_fp32x3_stays_dense_above_128(device):
    """An fp32x3 model at ctx 248: the engine encodes through the dense call (and meets the oracle far inside the bar); the packed call
    is refused with a message that says so, nothing launched."""
    ids, ref = L.oracle_text("plain", [1, 17, 129, 248])
    eng = _engine(device, "fp32x3")
    assert eng.pack_text
    got = eng.encode_text(ids)
    worst = float(L.one_minus_cos(got, ref).max())
    print(f"NUMERICS longclip_fp32x3_dense_1_minus_cos {worst:.3e}")
    assert worst <= BAR
    rc, out, msg = _packed_call(eng, device, ids, torch.tensor([1, 17, 129, 248], dtype=torch.int32))
    assert rc == -1 and "248 > 128" in msg and "FP32X3" in msg, (rc, msg)
    assert not bool(out.any())
