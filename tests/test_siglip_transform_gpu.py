"""GPU: the SigLIP family's image transform on the device (KEMR_TRANSFORM_SIGLIP of kemr_transform_u8 / kemr_transform_u8_batch,
python: preprocess.SiglipPreprocessGPU) against the host class preprocess.SiglipPreprocess -- every comparison is an equality of bits --,
the images the library refuses for Pillow's pass order, kind 0 through the new entry points, the memory contract of the four launch
calls for both kinds (windows: tests/footprint.py), and the route end to end on a tiny SigLIP model."""
import ctypes as C
import functools
import json
import os
import warnings

import numpy as np
import pytest
import torch

import footprint as F
from footprint import In, Out, SizeOf, Work
from knowledge_enhanced_multimodal_retrieval_amd import _lib, clip_api, datasets, evaluators
from knowledge_enhanced_multimodal_retrieval_amd.config import ARCHS
from knowledge_enhanced_multimodal_retrieval_amd.preprocess import (ClipPreprocessGPU, PackedRaw, SiglipPreprocess, SiglipPreprocessGPU,
                                                                    pack_raw)

pytestmark = pytest.mark.gpu

CLIP, SIGLIP = _lib.TRANSFORM_CLIP, _lib.TRANSFORM_SIGLIP
ERR_INVALID, ERR_WORKSPACE = -1, -4
F32, U8 = torch.float32, torch.uint8
SINGLE = ([(64, h, w) for h, w in [(64, 64), (64, 300), (300, 64), (150, 291), (1, 1), (1, 500), (500, 1), (2, 3), (63, 65), (37, 1000),
                                   (1700, 17), (1080, 1920)]]
          + [(224, h, w) for h, w in [(150, 291), (224, 224), (225, 224), (2000, 1500)]] + [(384, 500, 333)])


def _image(h, w, seed):
    """Noise for even seeds, ramps for odd ones (the content of tests/test_preprocess.py)."""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if seed % 2:
        yy, xx = np.mgrid[0:h, 0:w]
        base = np.stack([(xx * 255 // max(w - 1, 1)), (yy * 255 // max(h - 1, 1)), ((xx + yy) % 256)], -1).astype(np.uint8)
    return base


@functools.lru_cache(maxsize=None)
def _case(n, h, w, seed):
    """(uint8 image tensor, the host class's pixels for it): computed once, shared, never modified."""
    from PIL import Image
    arr = _image(h, w, seed)
    return torch.from_numpy(arr), SiglipPreprocess(n)(Image.fromarray(arr))


def _ptr(a):
    return C.c_void_p(a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr())


def _stream(device):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


# ------------------------------------------------------------------------------------------------ one image per call
def test_single_image_is_the_host_transform(device):
    """PIL input and tensor input, one object per output size: its workspace is reused (and grows) across the sizes."""
    from PIL import Image
    pres = {}
    for i, (n, h, w) in enumerate(SINGLE):
        img, want = _case(n, h, w, h + 2 * w + i)
        pre = pres.setdefault(n, SiglipPreprocessGPU(n, device))
        got = pre(img)
        assert got.dtype == F32 and tuple(got.shape) == (3, n, n) and got.device == device
        assert torch.equal(got.cpu(), want), (n, h, w)
        assert torch.equal(pre(Image.fromarray(img.numpy())).cpu(), want), (n, h, w)
        assert torch.equal(pre(img.to(device)).cpu(), want), (n, h, w)
    assert float(pres[64](torch.zeros(0, 0, 3, dtype=U8)).abs().max()) == 0.0
    with pytest.raises(RuntimeError, match="uint8"):
        pres[64](torch.zeros(10, 10, 3))
    assert repr(pres[64]) == "SiglipPreprocessGPU(n_px=64)" and repr(ClipPreprocessGPU(224, device)) == "ClipPreprocessGPU(n_px=224)"


# ------------------------------------------------------------------------------------------------ the batch
def test_batch_is_the_stacked_host_transforms(device):
    n = 64
    pre = SiglipPreprocessGPU(n, device)
    empty = torch.zeros(0, 0, 3, dtype=U8)
    small = [(64, 64), (150, 291), (64, 300), None, (150, 291), (1, 500), (64, 64)]
    large = small + [(300, 64), (2, 3), (63, 65), (37, 1000), (500, 1), (1, 1), None, (1700, 17), (1080, 1920), (150, 291)]
    for sizes in (small, large):                   # the second, larger batch reuses and grows the workspace
        items = [None if s is None else _case(n, s[0], s[1], 5 * s[0] + s[1] + i) for i, s in enumerate(sizes)]
        want = torch.stack([torch.zeros(3, n, n) if it is None else it[1] for it in items])
        packed = pack_raw([empty if it is None else it[0] for it in items])
        before = None if pre._ws is None else pre._ws.numel()
        got = pre.batch(packed)
        got_pinned = pre.batch(packed.pin_memory())
        got_dev = pre.batch(packed.to(device))
        torch.cuda.synchronize(device)
        assert torch.equal(got.cpu(), want) and torch.equal(got_pinned.cpu(), want) and torch.equal(got_dev.cpu(), want)
        for i, it in enumerate(items):
            if it is None:
                assert F.all_bytes(got[i], 0)          # exact zeros: +0.0f
        assert before is None or pre._ws.numel() > before
    allbad = pre.batch(pack_raw([empty, empty, empty]))
    assert tuple(allbad.shape) == (3, 3, n, n) and F.all_bytes(allbad, 0)
    none = pre.batch(pack_raw([]))
    assert tuple(none.shape) == (0, 3, n, n) and none.dtype == F32


# ------------------------------------------------------------------------------------------------ the aspect-ratio path
def test_image_pillow_filters_vertically_first(device):
    """(1701, 17) -> 64: alone and inside a batch of five it is the host transform's bits (computed on the host, copied into its slot;
    the other four go through the kernels); the raw library call refuses it and leaves `out` alone."""
    n = 64
    pre = SiglipPreprocessGPU(n, device)
    tall, want_tall = _case(n, 1701, 17, 8)
    assert torch.equal(pre(tall).cpu(), want_tall) and torch.equal(pre(tall.to(device)).cpu(), want_tall)
    others = [_case(n, h, w, 3 * h + w) for h, w in [(150, 291), (64, 64), (1700, 17), (1, 500)]]
    items = others[:2] + [(tall, want_tall)] + others[2:]
    want = torch.stack([it[1] for it in items])
    packed = pack_raw([it[0] for it in items])
    for p in (packed, packed.to(device)):
        assert torch.equal(pre.batch(p).cpu(), want)
    assert packed.heights.tolist() == [150, 64, 1701, 1700, 1] and packed.widths.tolist() == [291, 64, 17, 17, 500]      # the batch keeps its sizes
    # the library itself: -1, the message, nothing written
    L = _lib.lib()
    out = torch.full((3, n, n), 7.25, device=device)
    ws = torch.zeros(1 << 20, dtype=U8, device=device)
    img = tall.to(device)
    with torch.cuda.device(device):
        rc = L.kemr_transform_u8(SIGLIP, _ptr(img), 1701, 17, n, _ptr(out), _ptr(ws), ws.numel(), _stream(device))
    msg = L.kemr_last_error()
    torch.cuda.synchronize(device)
    assert rc == ERR_INVALID and b"1701 x 17" in msg and b"vertically first" in msg
    assert bool((out == 7.25).all()) and F.all_bytes(ws, 0)
    out5 = torch.full((5, 3, n, n), 7.25, device=device)
    data, offs, hs, wd = packed.data.to(device), packed.offsets, packed.heights, packed.widths
    with torch.cuda.device(device):
        rc = L.kemr_transform_u8_batch(SIGLIP, _ptr(data), _ptr(offs), _ptr(hs), _ptr(wd), 5, n,
                                       _ptr(out5), _ptr(ws), ws.numel(), _stream(device))
    msg = L.kemr_last_error()
    torch.cuda.synchronize(device)
    assert rc == ERR_INVALID and b"image 2" in msg and b"1701 x 17" in msg and b"vertically first" in msg
    assert bool((out5 == 7.25).all()) and F.all_bytes(ws, 0)


# ------------------------------------------------------------------------------------------------ kind 0 through the new entry points
def test_kind_0_is_clip_preprocess_gpu(device):
    L = _lib.lib()
    n = 224
    sizes = [(300, 400), (999, 224), (225, 224)]
    clip = ClipPreprocessGPU(n, device)
    imgs = [torch.from_numpy(_image(h, w, h + w)) for h, w in sizes]
    want = torch.stack([clip(im) for im in imgs])
    ws = torch.empty(64 << 20, dtype=U8, device=device)
    for im, (h, w), ref in zip(imgs, sizes, want):
        out = torch.empty(3, n, n, device=device)
        d = im.to(device)
        with torch.cuda.device(device):
            _lib.check(L.kemr_transform_u8(CLIP, _ptr(d), h, w, n, _ptr(out), _ptr(ws), ws.numel(), _stream(device)), "transform_u8")
            old = torch.empty(3, n, n, device=device)
            _lib.check(L.kemr_preprocess_u8(_ptr(d), h, w, n, _ptr(old), _ptr(ws), ws.numel(), _stream(device)), "preprocess_u8")
        assert torch.equal(out, ref) and torch.equal(old, ref)
    packed = pack_raw(imgs)
    data, offs, hs, wd = packed.data.to(device), packed.offsets, packed.heights, packed.widths
    out = torch.empty(3, 3, n, n, device=device)
    with torch.cuda.device(device):
        _lib.check(L.kemr_transform_u8_batch(CLIP, _ptr(data), _ptr(offs), _ptr(hs), _ptr(wd), 3, n,
                                             _ptr(out), _ptr(ws), ws.numel(), _stream(device)), "transform_u8_batch")
    assert torch.equal(out, want) and torch.equal(clip.batch(packed), want)


# ------------------------------------------------------------------------------------------------ memory contract
def _refusals(device, fn, calls, i_ws, i_out, what):
    """The contract call with one byte too few, then with the pointer moved by 128 bytes: KEMR_ERR_WORKSPACE, nothing launched."""
    ws, out = calls.win[i_ws], calls.win[i_out]
    for shift, less in ((0, 1), (128, 0)):
        ws.refill_body(F.POISON)
        out.refill_body(F.GUARD)
        args = calls.args(True, lambda t: C.c_void_p(t.data_ptr()))
        args[i_ws] = C.c_void_p(ws.ptr + shift)
        args[i_ws + 1] = ws.nbytes - less
        with torch.cuda.device(device):
            rc = fn(*args, _stream(device))
        torch.cuda.synchronize(device)
        assert rc == ERR_WORKSPACE, (what, shift, less, rc, _lib.lib().kemr_last_error())
        assert F.all_bytes(out.view, F.GUARD) and F.all_bytes(ws.view, F.POISON), (what, shift, less)
        assert ws.margins_intact() and out.margins_intact()


def _both(device, fn, specs, what):
    def run(*args):
        with torch.cuda.device(device):
            _lib.check(fn(*args, _stream(device)), what)
    return F.run_both(run, specs, device, what=what)


@pytest.mark.parametrize("kind", [CLIP, SIGLIP])
def test_launch_calls_inside_their_windows(device, kind):
    """Plain call (tight tensors, roomy zeroed workspace) against contract call (exactly the stated workspace, every byte 0xff, 0xa5
    margins; the image bytes in 0xff margins; `out` all 0xa5 in 0xa5 margins): same bits, margins intact.  Then the packed buffer with
    0xff in front of, between and behind the images: same bits again."""
    L = _lib.lib()
    n = 64
    # ---- one image
    h, w = 63, 65
    img, host = _case(n, h, w, 21)
    need = int(L.kemr_transform_workspace_bytes(kind, h, w, n))
    assert need > 0
    calls = _both(device, L.kemr_transform_u8, [kind, In(img.reshape(-1)), h, w, n, Out((3, n, n), F32), Work(need, need + (1 << 20)), SizeOf(6)],
                  f"transform_u8 kind {kind}")
    if kind == SIGLIP:
        assert torch.equal(calls.win[5].view.cpu(), host)
    _refusals(device, L.kemr_transform_u8, calls, 6, 5, f"transform_u8 kind {kind}")
    # ---- the batch
    sizes = [(150, 291), (0, 0), (1, 500), (64, 64)]
    items = [(torch.zeros(0, 0, 3, dtype=U8), torch.zeros(3, n, n)) if hw == (0, 0) else _case(n, hw[0], hw[1], 31 + i) for i, hw in enumerate(sizes)]
    packed = pack_raw([it[0] for it in items])
    hs, ws, offs = packed.heights, packed.widths, packed.offsets
    b = len(sizes)
    need = int(L.kemr_transform_batch_workspace_bytes(kind, _ptr(hs), _ptr(ws), b, n))
    assert need > 0
    what = f"transform_u8_batch kind {kind}"
    calls = _both(device, L.kemr_transform_u8_batch,
                  [kind, In(packed.data), _ptr(offs), _ptr(hs), _ptr(ws), b, n, Out((b, 3, n, n), F32), Work(need, need + (1 << 20)), SizeOf(8)], what)
    tight = calls.plain[7].clone()
    assert F.all_bytes(tight[1], 0)
    if kind == SIGLIP:
        assert torch.equal(tight.cpu(), torch.stack([it[1] for it in items]))
    _refusals(device, L.kemr_transform_u8_batch, calls, 8, 7, what)
    # ---- 0xff between the images: image i starts 256 + 3 * i bytes behind the end of the one before it
    gaps, pos, chunks = np.zeros(b, dtype=np.int64), 0, []
    for i, it in enumerate(items):
        chunks.append(torch.full((256 + 3 * i,), F.POISON, dtype=U8))
        pos += 256 + 3 * i
        gaps[i] = pos
        chunks.append(it[0].reshape(-1))
        pos += it[0].numel()
    chunks.append(torch.full((1000,), F.POISON, dtype=U8))
    gapped = F.window((pos + 1000,), U8, device, F.POISON, body=torch.cat(chunks), what="gapped packed images")
    out = F.window((b, 3, n, n), F32, device, F.GUARD, what="out")
    work = F.window((need,), U8, device, F.GUARD, body=F.POISON, what="workspace")
    with torch.cuda.device(device):
        _lib.check(L.kemr_transform_u8_batch(kind, C.c_void_p(gapped.ptr), _ptr(gaps), _ptr(hs), _ptr(ws), b, n, C.c_void_p(out.ptr),
                                             C.c_void_p(work.ptr), need, _stream(device)), what)
    torch.cuda.synchronize(device)
    assert F.same_bits(out.view, tight) and out.margins_intact() and work.margins_intact() and gapped.margins_intact()


# ------------------------------------------------------------------------------------------------ end to end
def _tokenize(texts, ctx=ARCHS["tiny-siglip"].ctx, vocab=ARCHS["tiny-siglip"].vocab):
    """The test's own tokenizer: [B, ctx] ids of the tiny model's vocabulary, a function of the text alone."""
    out = torch.ones(len(texts), ctx, dtype=torch.int32)
    for i, t in enumerate(texts):
        ids = [2 + (sum(w.encode()) * 31 + len(w)) % (vocab - 2) for w in t.split()][:ctx]
        out[i, :len(ids)] = torch.tensor(ids, dtype=torch.int32)
    return out


def test_tiny_siglip_end_to_end(device, monkeypatch):
    from PIL import Image
    monkeypatch.setenv("KEMR_GPU_PREPROCESS", "1")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        model, pre = clip_api.load("tiny-siglip", device=device)
        monkeypatch.setenv("KEMR_GPU_PREPROCESS", "0")
        _, pre_off = clip_api.load("tiny-siglip", device=device)
    S = model.arch.image_size
    assert isinstance(pre, SiglipPreprocess) and pre.defer_to_gpu and pre.n_px == S == 64
    assert isinstance(pre_off, SiglipPreprocess) and not pre_off.defer_to_gpu
    sizes = [(150, 291), (64, 64), None, (300, 64), (1701, 17), (37, 1000), (150, 291), (63, 65)]
    arrs = [None if s is None else _image(s[0], s[1], 11 + i) for i, s in enumerate(sizes)]
    rows = [{"image": None if a is None else Image.fromarray(a), "query_text": f"vase {i} bronze", "target_text": f"bronze vase number {i}",
             "uuid": f"u{i}"} for i, a in enumerate(arrs)]
    gpu_ds = datasets.CLIPEvalDatasetHF(rows, pre)
    host_ds = datasets.CLIPEvalDatasetHF(rows, SiglipPreprocess(S))
    assert evaluators.image_transform_name(gpu_ds).startswith("gpu") and evaluators.image_transform_name(host_ds).startswith("host")
    gpu = evaluators.encode_dataset(model, gpu_ds, 3, 1, tokenize_fn=_tokenize)
    host = evaluators.encode_dataset(model, host_ds, 3, 1, tokenize_fn=_tokenize)
    assert torch.equal(gpu[0], host[0]) and torch.equal(gpu[1], host[1]) and torch.equal(gpu[2], host[2]) and gpu[3] == host[3]
    assert tuple(gpu[0].shape) == (len(rows), model.arch.embed_dim) and bool(torch.isfinite(gpu[0]).all())
    # the reference's loop shape: the packed batch moves with .to() and encode_image takes it
    raw = [gpu_ds[i][0] for i in range(len(rows))]
    packed = pack_raw(raw).to(device)
    assert isinstance(packed, PackedRaw)
    px = torch.stack([host_ds[i][0] for i in range(len(rows))])
    assert torch.equal(px[2], torch.zeros(3, S, S))
    assert torch.equal(model.encode_image(packed), model.encode_image(px.to(device)))


def test_cli_names_the_transform_in_its_results(device, tmp_path, monkeypatch):
    """The evaluator CLI on a SigLIP directory with camera-sized uint8 sources: the results JSON names where the transform ran, and the
    two routes give the same metrics."""
    import transformers
    import siglip_ref as SR
    from tokenizers import Tokenizer, models, pre_tokenizers
    from knowledge_enhanced_multimodal_retrieval_amd import hf_checkpoint
    arch = ARCHS["tiny-siglip"]
    d = str(tmp_path / "ckpt")
    hf = transformers.SiglipModel(transformers.SiglipConfig(**SR.hf_config_kwargs(arch), attn_implementation="eager")).eval()
    hf.load_state_dict(hf_checkpoint.to_siglip_state_dict(SR.weights(arch), arch), strict=False)
    hf.save_pretrained(d, safe_serialization=True)
    vocab = [("<pad>", 0.0), ("</s>", 0.0), ("<unk>", 0.0), ("▁", -6.0)] + [(c, -3.0) for c in "abcdefghijklmnopqrstuvwxyz0123456789"]
    tok = Tokenizer(models.Unigram(vocab, unk_id=2))
    tok.pre_tokenizer = pre_tokenizers.Metaspace()
    tok.save(os.path.join(d, "tokenizer.json"))
    runs = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("KEMR_GPU_PREPROCESS", mode)
        out = str(tmp_path / f"res{mode}" / "metrics.json")
        res = evaluators.main_evaluator(["--model_name", d, "--synthetic", "12", "--synthetic_images", "uint8", "--batch_size", "5",
                                         "--output_file", out, "--num_workers", "0", "--mrr_only"])
        with open(out) as f:
            saved = json.load(f)
        assert saved["image_transform"].startswith("gpu" if mode == "1" else "host (PIL"), saved["image_transform"]
        runs[mode] = res["metrics"]
    assert runs["1"] == runs["0"]
