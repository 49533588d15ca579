"""The bytes of the device arena, on the host: kemr_debug_pack_weights (the pack step of kemr_model_finalize, csrc/model.hip
pack_weights) against a numpy / torch statement of the layout and the arithmetic, byte for byte.  No GPU.

The statement, written here and not taken from the C++:

* placement: the required tensors in kemr_model_tensor_name order, every entry zero-padded to a multiple of 256 bytes; the per-row
  scales of an e4m3 matrix form an entry IN FRONT of the matrix, the pooling head's query an entry BEHIND the probe;
* vectors and tables are fp32 verbatim; matrices are bf16, round to nearest even (torch's bf16 cast); conv1 rows are zero-padded from
  3 p p to kpad = ceil64(3 p p) columns;
* the attention scale is multiplied into the query rows of every in_proj_weight and the first third of every in_proj_bias in fp32 BEFORE
  any rounding: 0.125, or the fp32 nearest to 1 / sqrt(80) in the vision tower at head dim 80.  The pooling head's in_proj takes it too
  (its query rows are never read: the head's query is the entry behind the probe);
* fp8 (vision tower only; QKV, and fc1 under fp8-mlp): per LayerNorm channel s_c = 2^clamp(ceil(log2 max(|gamma_c|, |beta_c|)), -12, 12)
  with the log in fp32 (1 where the maximum is 0), gamma and beta divided by s, the weight columns multiplied by s, then per row
  scale = amax / 448 (1 for an all-zero row) and e4m3(value / scale) (torch's float8_e4m3fn cast, which
  test_abi.py::test_host_e4m3_conversion_matches_torch ties to the library's);
* fp32x3: every matrix [N, K] as [N, 3K] = [hi | hi | lo], hi = bf16(v), lo = bf16(v - hi); conv1 over 3 kpad;
* SigLIP: visual.positional_embedding + visual.conv1.bias per row; the head's query bf16(((probe . Wq^T, accumulated in fp64 in column
  order, rounded to fp32) + bq) / 8);  BERT: positional_embedding + token_type_embedding[0] per row.

The weights make every branch matter (`weights`): block LayerNorm gains spread over eleven binades, exact powers of two, a channel whose
gain and bias are both 0, channels beyond both clamps, all-zero weight rows.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from knowledge_enhanced_multimodal_retrieval_amd import _lib
from knowledge_enhanced_multimodal_retrieval_amd.config import ARCHS, BERT_ARCHS, FAMILIES

# (fixture, precision, option residual_stream_24bit)
CASES = [("tiny", "bf16", 1), ("tiny", "bf16", 0), ("tiny", "bf16-res16", 1), ("tiny", "fp8", 1), ("tiny", "fp8-mlp", 1), ("tiny", "fp32x3", 1),
         ("tiny-h", "bf16", 1), ("tiny-h", "fp32x3", 1), ("tiny-siglip", "bf16", 1), ("tiny-bert", "bf16", 1)]


def arch_of(name):
    return BERT_ARCHS[name] if name in BERT_ARCHS else ARCHS[name]


def tensor_list(arch):
    """[(name, shape)] in placement order."""
    out = []

    def blocks(prefix, w, layers):
        for i in range(layers):
            b = f"{prefix}.resblocks.{i}"
            out.extend([(f"{b}.ln_1.weight", (w,)), (f"{b}.ln_1.bias", (w,)), (f"{b}.attn.in_proj_weight", (3 * w, w)),
                        (f"{b}.attn.in_proj_bias", (3 * w,)), (f"{b}.attn.out_proj.weight", (w, w)), (f"{b}.attn.out_proj.bias", (w,)),
                        (f"{b}.ln_2.weight", (w,)), (f"{b}.ln_2.bias", (w,)), (f"{b}.mlp.c_fc.weight", (4 * w, w)),
                        (f"{b}.mlp.c_fc.bias", (4 * w,)), (f"{b}.mlp.c_proj.weight", (w, 4 * w)), (f"{b}.mlp.c_proj.bias", (w,))])

    if arch.family == "bert":
        w = arch.width
        out.extend([("token_embedding.weight", (arch.vocab, w)), ("positional_embedding", (arch.ctx, w)), ("token_type_embedding", (2, w)),
                    ("ln_embed.weight", (w,)), ("ln_embed.bias", (w,))])
        blocks("transformer", w, arch.layers)
        return out
    sig = arch.family == "siglip"
    vw, tw, d, p = arch.v_width, arch.t_width, arch.embed_dim, arch.patch
    out.append(("visual.conv1.weight", (vw, 3, p, p)))
    out.append(("visual.conv1.bias", (vw,)) if sig else ("visual.class_embedding", (vw,)))
    out.append(("visual.positional_embedding", (arch.v_tokens, vw)))
    if not sig:
        out.extend([("visual.ln_pre.weight", (vw,)), ("visual.ln_pre.bias", (vw,))])
    blocks("visual.transformer", vw, arch.v_layers)
    out.extend([("visual.ln_post.weight", (vw,)), ("visual.ln_post.bias", (vw,))])
    if sig:
        h = "visual.attn_pool"
        out.extend([(f"{h}.probe", (vw,)), (f"{h}.in_proj_weight", (3 * vw, vw)), (f"{h}.in_proj_bias", (3 * vw,)),
                    (f"{h}.out_proj.weight", (vw, vw)), (f"{h}.out_proj.bias", (vw,)), (f"{h}.ln.weight", (vw,)), (f"{h}.ln.bias", (vw,)),
                    (f"{h}.mlp.c_fc.weight", (4 * vw, vw)), (f"{h}.mlp.c_fc.bias", (4 * vw,)), (f"{h}.mlp.c_proj.weight", (vw, 4 * vw)),
                    (f"{h}.mlp.c_proj.bias", (vw,))])
    else:
        out.append(("visual.proj", (vw, d)))
    out.extend([("token_embedding.weight", (arch.vocab, tw)), ("positional_embedding", (arch.ctx, tw))])
    blocks("transformer", tw, arch.t_layers)
    out.extend([("ln_final.weight", (tw,)), ("ln_final.bias", (tw,)), ("text_projection", (tw, d))])
    if sig:
        out.append(("text_projection_bias", (d,)))
    return out


def weights(arch, seed=0):
    """Seeded fp32 tensors.  Matrices N(0, 1 / fan_in), the rest N(0, 0.5^2).  Every block LayerNorm (ln_1 / ln_2, both towers): gains
    +-m 2^e with m in [1.05, 1.95] (never next to a power of two, where an fp32 log2 may land on the wrong side of the integer) and e in
    -5 .. 5; channels 0 .. 8 are the exact powers 2^-4 .. 2^4 with bias = gain / 2 (so the channel maximum IS the power of two);
    channel 9 has gain = bias = 0; channel 10 is 1.5 * 2^14 and channel 11 1.5 * 2^-15 with bias 0 (beyond the +-12 clamps).  Rows 3 and
    W + 7 of every in_proj_weight and row 5 of every c_fc.weight are all zero."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name, shape in tensor_list(arch):
        t = torch.randn(shape, generator=g, dtype=torch.float32)
        t = t * (math.prod(shape[1:]) ** -0.5 if len(shape) > 1 and "embedding" not in name else 0.5)
        if ".resblocks." in name and name.rsplit(".", 2)[-2] in ("ln_1", "ln_2"):
            n = shape[0]
            if name.endswith("weight"):
                m = 1.05 + 0.9 * torch.rand(n, generator=g)
                e = torch.randint(-5, 6, (n,), generator=g).float()
                sign = torch.where(torch.rand(n, generator=g) < 0.25, -1.0, 1.0)
                t = sign * m * torch.exp2(e)
                t[:9] = torch.exp2(torch.arange(-4, 5).float())
                t[9], t[10], t[11] = 0.0, 1.5 * 2.0 ** 14, 1.5 * 2.0 ** -15
            else:
                t = 0.1 * t
                t[:9] = 0.5 * sd[name[:-4] + "weight"][:9]
                t[9:12] = 0.0
        if name.endswith("in_proj_weight"):
            t[3] = 0.0
            t[shape[1] + 7] = 0.0
        if name.endswith("c_fc.weight"):
            t[5] = 0.0
        sd[name] = t.contiguous()
    return sd


# ------------------------------------------------------------------------------------------------ the statement
def _bf16(t):
    return t.to(torch.bfloat16).view(torch.int16).numpy().tobytes()


def _triple(t):
    hi = t.to(torch.bfloat16)
    lo = (t - hi.float()).to(torch.bfloat16)
    return torch.cat([hi, hi, lo], dim=1).contiguous().view(torch.int16).numpy().tobytes()


def _f32(t):
    return t.to(torch.float32).contiguous().numpy().tobytes()


def channel_scales(gamma, beta):
    a = np.maximum(np.abs(gamma.numpy()), np.abs(beta.numpy())).astype(np.float32)
    with np.errstate(divide="ignore"):
        e = np.clip(np.ceil(np.log2(a)), -12.0, 12.0)           # np.log2 of an fp32 array is an fp32 log2
    return torch.from_numpy(np.where(a > 0, np.exp2(e), 1.0).astype(np.float32))


def expected_arena(arch, sd, precision):
    """[(name, bytes)] entries in arena order, unpadded."""
    fp8 = {"fp8": 1, "fp8-res16": 1, "fp8-mlp": 3}.get(precision, 0)
    x3 = precision == "fp32x3"
    bert = arch.family == "bert"
    v_qs = torch.tensor(np.float32(1.0 / np.sqrt(80.0)) if getattr(arch, "v_head_dim", 64) == 80 else np.float32(0.125))
    entries = []
    for name, shape in tensor_list(arch):
        t = sd[name]
        vision_block = name.startswith("visual.transformer.")
        qs = v_qs if name.startswith("visual.") else torch.tensor(np.float32(0.125))
        matrix = lambda m: _triple(m) if x3 else _bf16(m)                          # noqa: E731
        if name == "visual.conv1.weight":
            kv = 3 * arch.patch * arch.patch
            padded = torch.zeros(shape[0], -(-kv // 64) * 64)
            padded[:, :kv] = t.reshape(shape[0], kv)
            entries.append((name, matrix(padded)))
        elif name.endswith("in_proj_weight") or name.endswith("c_fc.weight"):
            qkv = name.endswith("in_proj_weight")
            m = t.clone()
            if qkv:
                m[:shape[1]] = m[:shape[1]] * qs
            if vision_block and fp8 & (1 if qkv else 2):
                block = name[:name.index(".attn." if qkv else ".mlp.")]
                ln = f"{block}.{'ln_1' if qkv else 'ln_2'}"
                m = m * channel_scales(sd[ln + ".weight"], sd[ln + ".bias"])[None, :]
                amax = m.abs().amax(dim=1)
                scale = torch.where(amax > 0, amax / 448.0, torch.ones_like(amax))
                entries.append((name + " row scales", _f32(scale)))
                entries.append((name, (m / scale[:, None]).to(torch.float8_e4m3fn).view(torch.uint8).numpy().tobytes()))
            else:
                entries.append((name, matrix(m)))
        elif name.endswith("out_proj.weight") or name.endswith("c_proj.weight"):
            entries.append((name, matrix(t)))
        elif name.endswith("in_proj_bias"):
            b = t.clone()
            b[:shape[0] // 3] = b[:shape[0] // 3] * qs
            entries.append((name, _f32(b)))
        elif vision_block and name.rsplit(".", 2)[-2] in ("ln_1", "ln_2") and fp8 & (1 if ".ln_1." in name else 2):
            ln = name.rsplit(".", 1)[0]
            entries.append((name, _f32(t / channel_scales(sd[ln + ".weight"], sd[ln + ".bias"]))))
        elif name == "visual.positional_embedding" and arch.family == "siglip":
            entries.append((name, _f32(t + sd["visual.conv1.bias"][None, :])))
        elif name == "positional_embedding" and bert:
            entries.append((name, _f32(t + sd["token_type_embedding"][0][None, :])))
        elif name == "visual.attn_pool.probe":
            w = shape[0]
            wq = sd["visual.attn_pool.in_proj_weight"][:w].double().numpy()
            acc = np.cumsum(wq * t.double().numpy()[None, :], axis=1)[:, -1]       # exact products, summed in column order
            q = (torch.from_numpy(acc.astype(np.float32)) + sd["visual.attn_pool.in_proj_bias"][:w]) * torch.tensor(np.float32(0.125))
            entries.append((name, _f32(t)))
            entries.append((name + " query", _bf16(q)))
        else:
            entries.append((name, _f32(t)))
    return entries


# ------------------------------------------------------------------------------------------------ the library
def make_model(lib, arch, stream24=1):
    h = C.c_void_p()
    cfg = _lib.KemrCfg(**arch.cfg_dict())
    if arch.family == "bert":
        _lib.check(lib.kemr_model_create_family(C.byref(cfg), _lib.FAMILY_BERT, C.byref(h)), "model_create_family")
    else:
        _lib.check(lib.kemr_model_create(C.byref(cfg), C.byref(h)), "model_create")
        if arch.v_head_dim != 64:
            _lib.check(lib.kemr_model_set_option(h, b"vision_head_dim", arch.v_head_dim), "set_option")
        if arch.family != "clip":
            _lib.check(lib.kemr_model_set_option(h, b"family", FAMILIES[arch.family]), "set_option")
    _lib.check(lib.kemr_model_set_option(h, b"residual_stream_24bit", stream24), "set_option")
    return h


def load(lib, h, sd, skip=()):
    for name, t in sd.items():
        if name in skip:
            continue
        shape = (C.c_int64 * max(t.dim(), 1))(*t.shape)
        _lib.check(lib.kemr_model_load_tensor(h, name.encode(), C.c_void_p(t.data_ptr()), _lib.KEMR_F32, shape, t.dim()), f"load_tensor({name})")


def pack(lib, h, precision):
    """(status, arena bytes as a numpy uint8 array or None)."""
    n = C.c_size_t(0)
    rc = lib.kemr_debug_pack_weights(h, _lib.PRECISIONS[precision], None, 0, C.byref(n))
    if rc != 0:
        return rc, None
    buf = np.zeros(n.value, dtype=np.uint8)
    m = C.c_size_t(0)
    _lib.check(lib.kemr_debug_pack_weights(h, _lib.PRECISIONS[precision], C.c_void_p(buf.ctypes.data), buf.size, C.byref(m)), "debug_pack_weights")
    assert m.value == n.value, "the size-only call and the filling call disagree"
    return 0, buf


@pytest.mark.parametrize("fixture,precision,stream24", CASES, ids=[f"{f}-{p}-s24_{s}" for f, p, s in CASES])
def test_arena_bytes(fixture, precision, stream24):
    lib = _lib.lib()
    arch = arch_of(fixture)
    h = make_model(lib, arch, stream24)
    try:
        names = [lib.kemr_model_tensor_name(h, i).decode() for i in range(lib.kemr_model_num_tensors(h))]
        assert names == [n for n, _ in tensor_list(arch)]
        sd = weights(arch)
        load(lib, h, sd)
        rc, got = pack(lib, h, precision)
        assert rc == 0, lib.kemr_last_error()
        # too small a buffer is refused, the size still reported
        n = C.c_size_t(0)
        assert lib.kemr_debug_pack_weights(h, _lib.PRECISIONS[precision], C.c_void_p(got.ctypes.data), got.size - 1, C.byref(n)) == -1
        assert n.value == got.size
        off = 0
        for name, b in expected_arena(arch, sd, precision):
            assert off % 256 == 0
            want = np.frombuffer(b, dtype=np.uint8)
            padded = -(-want.size // 256) * 256
            assert off + padded <= got.size, f"{name}: the arena ends at {got.size}, the entry at {off + padded}"
            have = got[off:off + want.size]
            if not np.array_equal(have, want):
                first = int(np.flatnonzero(have != want)[0])
                pytest.fail(f"{name}: first differing byte at entry offset {first} (arena offset {off + first}): {have[first]:#04x} != {want[first]:#04x}")
            assert not got[off + want.size:off + padded].any(), f"{name}: the padding behind the entry is not zero"
            off += padded
        assert off == got.size, f"the arena has {got.size} bytes, the entries end at {off}"
    finally:
        lib.kemr_model_destroy(h)


def test_weights_exercise_every_branch():
    """What `weights` promises, on the tensors the fp8 cases quantise: scales over several binades, both clamps, a channel at scale 1
    because its gain and bias are 0, exact powers of two, an all-zero row."""
    arch = arch_of("tiny")
    sd = weights(arch)
    b = "visual.transformer.resblocks.0"
    s = channel_scales(sd[f"{b}.ln_1.weight"], sd[f"{b}.ln_1.bias"])
    assert len(set(s.tolist())) >= 8 and s.max() == 2.0 ** 12 and s.min() == 2.0 ** -12
    assert s[9] == 1.0 and sd[f"{b}.ln_1.weight"][9] == 0 and sd[f"{b}.ln_1.bias"][9] == 0
    assert torch.equal(s[:9], torch.exp2(torch.arange(-4, 5).float()))
    assert not sd[f"{b}.attn.in_proj_weight"][3].any() and not sd[f"{b}.mlp.c_fc.weight"][5].any()


def _both(lib, h, precision):
    """(code, message) of kemr_debug_pack_weights and of kemr_model_finalize, which must refuse alike."""
    n = C.c_size_t(0)
    a = (lib.kemr_debug_pack_weights(h, precision, None, 0, C.byref(n)), lib.kemr_last_error())
    b = (lib.kemr_model_finalize(h, precision), lib.kemr_last_error())
    return a, b


def test_refusals_are_finalize_s():
    lib = _lib.lib()
    sig, bert, clip = make_model(lib, arch_of("tiny-siglip")), make_model(lib, arch_of("tiny-bert")), make_model(lib, arch_of("tiny"))
    try:
        for h, prec, code, words in ((sig, _lib.PREC_FP8, -1, (b"fp8", b"family 1")), (sig, _lib.PREC_FP8_MLP, -1, (b"fp8", b"family 1")),
                                     (bert, _lib.PREC_FP8, -1, (b"fp8", b"family 2")), (bert, _lib.PREC_FP32X3, -1, (b"KEMR_PREC_FP32X3", b"family 2")),
                                     (clip, 0, -1, (b"unsupported precision",)), (clip, _lib.PREC_BF16, -2, (b"missing key 'visual.conv1.weight'",))):
            a, b = _both(lib, h, prec)
            assert a == b and a[0] == code and all(w in a[1] for w in words), (a, b)
        # one key short of complete: the last name is the one reported, by both
        arch = arch_of("tiny")
        sd = weights(arch)
        load(lib, clip, sd, skip=("text_projection",))
        a, b = _both(lib, clip, _lib.PREC_BF16)
        assert a == b and a[0] == -2 and b"missing key 'text_projection'" in a[1], (a, b)
        a, b = _both(lib, None, _lib.PREC_BF16)
        assert a == b and a[0] == -1 and b"null model" in a[1], (a, b)
    finally:
        for h in (sig, bert, clip):
            lib.kemr_model_destroy(h)
