"""CPU: the SigLIP family's image transform on its way to the device (kemr_transform_* in include/kemr.h) -- Pillow's pass order pinned
against the installed Pillow, the library's refusals and workspace sizes (host-only calls), and the Python plumbing that must not change
for a caller without a GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

from knowledge_enhanced_multimodal_retrieval_amd import _lib, clip_api, preprocess
from oracle import preprocess_ref

CLIP_SIZES = [(300, 400), (224, 500), (999, 224), (1080, 1920), (231, 229), (100, 80), (640, 480), (225, 224), (224, 224),
              (37, 1000), (2000, 1500)]           # SIZES of tests/test_preprocess.py


def _noise(h, w, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _pillow(arr, nw, nh):
    from PIL import Image
    return np.asarray(Image.fromarray(arr).resize((nw, nh), Image.BICUBIC))


def _horizontal_first(arr, nw, nh):
    return preprocess_ref.resize_bicubic_u8(arr, nw, nh)                     # the one-call form: what the kernels compute


def _vertical_first(arr, nw, nh):
    return preprocess_ref.resize_bicubic_u8(preprocess_ref.resize_bicubic_u8(arr, arr.shape[1], nh), nw, nh)


# ------------------------------------------------------------------------------------------------ Pillow's pass order
@pytest.mark.parametrize("h,w", [(1700, 17), (4000, 40)])
def test_pillow_filters_horizontally_first_up_to_100_to_1(h, w):
    arr = _noise(h, w, h)
    assert np.array_equal(_pillow(arr, 64, 64), _horizontal_first(arr, 64, 64))


@pytest.mark.parametrize("h,w", [(1701, 17), (4001, 40)])
def test_pillow_filters_vertically_first_beyond_100_to_1(h, w):
    """height > 100 x width and a lower output: the vertical pass runs first; the 8-bit intermediate makes that other bytes.  If a later
    Pillow moves this rule, the refusal in csrc/preprocess.hip (refuses()) and SiglipPreprocessGPU._on_host move with it."""
    arr = _noise(h, w, h)
    pil = _pillow(arr, 64, 64)
    assert np.array_equal(pil, _vertical_first(arr, 64, 64))
    assert not np.array_equal(pil, _horizontal_first(arr, 64, 64))


@pytest.mark.parametrize("h,w,nw,nh", [(1701, 17, 64, 1702),
                                       (1001, 10, 1024, 1024)])       # the largest n_px the library takes: the shape of the workspace test below
def test_pillow_stays_horizontal_first_when_the_vertical_pass_enlarges(h, w, nw, nh):
    arr = _noise(h, w, h)
    assert np.array_equal(_pillow(arr, nw, nh), _horizontal_first(arr, nw, nh))


def test_every_accepted_shape_around_the_boundary_is_horizontal_first():
    """Seeded shapes at and around height = 100 x width, squashed to n x n: whatever the library accepts, Pillow computes horizontally
    first (what it refuses is computed by Pillow itself, whichever order that is)."""
    lib = _lib.lib()
    rng = np.random.default_rng(0)
    accepted = 0
    for t in range(60):
        w = int(rng.integers(1, 9))
        h = max(1, 100 * w + int(rng.integers(-2, 3)) if t % 3 == 0 else int(rng.integers(1, 100 * w + 400)))
        n = int(rng.choice([1, 2, 7, 16, 64, 100])) if t % 5 else h + int(rng.integers(0, 2))
        if n > 1024:
            continue
        arr = _noise(h, w, t)
        if lib.kemr_transform_workspace_bytes(_lib.TRANSFORM_SIGLIP, h, w, n) == 0:
            assert h > 100 * w and h > n, (h, w, n)
            continue
        accepted += 1
        assert np.array_equal(_pillow(arr, n, n), _horizontal_first(arr, n, n)), (h, w, n)
    assert accepted >= 30


def test_the_python_rule_is_the_librarys_rule():
    """SiglipPreprocessGPU._on_host (which images the host computes) against kemr_transform_workspace_bytes (which the library refuses)."""
    lib = _lib.lib()
    pre = preprocess.SiglipPreprocessGPU.__new__(preprocess.SiglipPreprocessGPU)
    for n in (64, 384, 1024):
        pre.n_px = n
        for h, w in [(1700, 17), (1701, 17), (300, 3), (301, 3), (101, 1), (100, 1), (n, 1), (n + 1, 1), (500, 5), (501, 5),
                     (4001, 40), (5, 501), (2, 900), (150, 291), (1, 1), (32768, 327), (32768, 328)]:
            assert pre._on_host(h, w) == (lib.kemr_transform_workspace_bytes(_lib.TRANSFORM_SIGLIP, h, w, n) == 0), (h, w, n)


# ------------------------------------------------------------------------------------------------ the library, host-only calls
def _batch_bytes(lib, kind, sizes, n):
    hs = np.array([h for h, _ in sizes], dtype=np.int32)
    ws = np.array([w for _, w in sizes], dtype=np.int32)
    return int(lib.kemr_transform_batch_workspace_bytes(kind, C.c_void_p(hs.ctypes.data), C.c_void_p(ws.ctypes.data), len(sizes), n))


def test_kind_0_is_the_clip_entry_points():
    lib = _lib.lib()
    for h, w in CLIP_SIZES:
        want = lib.kemr_preprocess_workspace_bytes(h, w, 224)
        assert want > 0 and lib.kemr_transform_workspace_bytes(_lib.TRANSFORM_CLIP, h, w, 224) == want
    for sizes in (CLIP_SIZES, CLIP_SIZES[:5] + CLIP_SIZES[:2], [(0, 0)] + CLIP_SIZES[:3]):
        hs = np.array([h for h, _ in sizes], dtype=np.int32)
        ws = np.array([w for _, w in sizes], dtype=np.int32)
        want = lib.kemr_preprocess_batch_workspace_bytes(C.c_void_p(hs.ctypes.data), C.c_void_p(ws.ctypes.data), len(sizes), 224)
        assert want > 0 and _batch_bytes(lib, _lib.TRANSFORM_CLIP, sizes, 224) == want
    # CLIP's geometry keeps accepting what it always accepted, the tall image included (horizontal-first, as ever)
    assert lib.kemr_transform_workspace_bytes(_lib.TRANSFORM_CLIP, 1701, 17, 64) == lib.kemr_preprocess_workspace_bytes(1701, 17, 64) > 0


def test_kind_1_workspace_sizes_and_refusals():
    """Non-zero where the kernels' pass order is Pillow's, 0 where it is not, for an unknown kind and for an output size out of range.
    The accepted tall image whose vertical pass ENLARGES is (1001, 10) -> 1024 here: the (1701, 17) -> 2000 one could name is beyond the
    1 .. 1024 range of n_px that this same test holds the library to (n_px 1025 is 0), so it is asserted as that: 0, for its n_px."""
    lib = _lib.lib()
    S = _lib.TRANSFORM_SIGLIP
    for h, w, n in [(150, 291, 64), (1, 1, 64), (1700, 17, 64), (1001, 10, 1024)]:
        assert lib.kemr_transform_workspace_bytes(S, h, w, n) > 0, (h, w, n)
    assert lib.kemr_transform_workspace_bytes(S, 1701, 17, 64) == 0
    assert lib.kemr_transform_workspace_bytes(S, 1001, 10, 1000) == 0
    assert lib.kemr_transform_workspace_bytes(2, 150, 291, 64) == 0 and lib.kemr_transform_workspace_bytes(-1, 150, 291, 64) == 0
    assert lib.kemr_transform_workspace_bytes(S, 150, 291, 0) == 0 and lib.kemr_transform_workspace_bytes(S, 150, 291, 1025) == 0
    assert lib.kemr_transform_workspace_bytes(S, 1701, 17, 2000) == 0 and lib.kemr_transform_workspace_bytes(S, 150, 291, 2000) == 0
    # squash: both tables have n_px rows, all input rows are filtered when the height shrinks -- not CLIP's plan
    assert lib.kemr_transform_workspace_bytes(S, 150, 291, 64) != lib.kemr_transform_workspace_bytes(_lib.TRANSFORM_CLIP, 150, 291, 64)
    # the batch form: tables once per distinct size, 0 x 0 items cost a descriptor only, one refused image refuses the batch
    sizes = [(150, 291), (0, 0), (1, 500), (64, 64)]
    one = _batch_bytes(lib, S, sizes, 64)
    assert one > 0 and _batch_bytes(lib, 2, sizes, 64) == 0 and _batch_bytes(lib, S, sizes, 1025) == 0 and _batch_bytes(lib, S, sizes, 0) == 0
    assert _batch_bytes(lib, S, [(0, 0)] * 3, 64) == 256
    assert _batch_bytes(lib, S, sizes + [(1701, 17)], 64) == 0
    assert b"image 4" in lib.kemr_last_error() and b"1701 x 17" in lib.kemr_last_error() and b"vertically first" in lib.kemr_last_error()
    assert _batch_bytes(lib, S, sizes + [(1700, 17)], 64) > one
    assert _batch_bytes(lib, S, [(150, 291)] * 2, 64) < _batch_bytes(lib, S, [(150, 291), (150, 290)], 64)      # a repeat shares its tables


def test_launch_calls_refuse_on_the_host_before_anything_else():
    """Unknown kind, out-of-range sizes and the vertical-first image are KEMR_ERR_INVALID from host-side checks (no pointer is touched)."""
    lib = _lib.lib()
    S = _lib.TRANSFORM_SIGLIP
    bogus = C.c_void_p(256)
    assert lib.kemr_transform_u8(2, bogus, 10, 10, 64, bogus, bogus, 1 << 20, None) == -1 and b"kind" in lib.kemr_last_error()
    assert lib.kemr_transform_u8(S, bogus, 10, 10, 1025, bogus, bogus, 1 << 20, None) == -1
    assert lib.kemr_transform_u8(S, bogus, 1701, 17, 64, bogus, bogus, 1 << 30, None) == -1
    msg = lib.kemr_last_error()
    assert b"1701 x 17" in msg and b"vertically first" in msg and b"Pillow" in msg
    hs, ws = np.array([64, 1701], dtype=np.int32), np.array([64, 17], dtype=np.int32)
    offs = np.array([0, 64 * 64 * 3], dtype=np.int64)
    args = (bogus, C.c_void_p(offs.ctypes.data), C.c_void_p(hs.ctypes.data), C.c_void_p(ws.ctypes.data), 2, 64, bogus, bogus, 1 << 30, None)
    assert lib.kemr_transform_u8_batch(S, *args) == -1
    msg = lib.kemr_last_error()
    assert b"image 1" in msg and b"1701 x 17" in msg and b"vertically first" in msg
    assert lib.kemr_transform_u8_batch(2, *args) == -1 and b"kind" in lib.kemr_last_error()
    assert lib.kemr_transform_u8_batch(2, None, None, None, None, 0, 64, None, None, 0, None) == -1
    assert lib.kemr_transform_u8_batch(S, None, None, None, None, 0, 64, None, None, 0, None) == 0          # an empty batch of a known kind


# ------------------------------------------------------------------------------------------------ Python plumbing
def test_deferring_object_is_still_the_host_transform():
    from PIL import Image
    img = Image.fromarray(_noise(150, 291, 3))
    pre = preprocess.SiglipPreprocess(64, defer_to_gpu=True)
    assert pre.defer_to_gpu and pre.n_px == 64
    assert torch.equal(pre(img), preprocess.SiglipPreprocess(64)(img))
    assert not preprocess.SiglipPreprocess(64).defer_to_gpu
    with pytest.raises(RuntimeError, match="GPU"):
        preprocess.SiglipPreprocessGPU(64, "cpu")


def test_load_on_the_cpu_does_not_defer():
    clip_api.allow_random_weights(True)
    try:
        with pytest.warns(RuntimeWarning, match="RANDOM weights"):
            model, pre = clip_api.load("tiny-siglip", device="cpu")
    finally:
        clip_api.allow_random_weights(False)
    assert isinstance(pre, preprocess.SiglipPreprocess) and pre.n_px == 64 and not pre.defer_to_gpu


def test_undecodable_items_are_the_same_zeros_on_both_routes():
    """CLIPEvalDatasetHF with a SigLIP transform: the raw route hands out the empty item (zeros after the device transform), the host
    route zeros of the transform's own size, so that the item stacks with its batch."""
    from PIL import Image
    from knowledge_enhanced_multimodal_retrieval_amd import datasets
    rows = [{"image": Image.fromarray(_noise(30, 50, 1)), "query_text": "a", "target_text": "b", "uuid": "u0"},
            {"image": None, "query_text": "c", "target_text": "d", "uuid": "u1"}]
    raw = datasets.CLIPEvalDatasetHF(rows, preprocess.SiglipPreprocess(64, defer_to_gpu=True))
    host = datasets.CLIPEvalDatasetHF(rows, preprocess.SiglipPreprocess(64))
    assert tuple(raw[1][0].shape) == (0, 0, 3) and raw[0][0].dtype == torch.uint8 and tuple(raw[0][0].shape) == (30, 50, 3)
    assert torch.equal(host[1][0], torch.zeros(3, 64, 64)) and tuple(host[0][0].shape) == (3, 64, 64)
    images, *_ = datasets.collate_fn_eval([host[0], host[1]])
    assert tuple(images.shape) == (2, 3, 64, 64)
    packed, *_ = datasets.collate_fn_eval([raw[0], raw[1]])
    assert isinstance(packed, preprocess.PackedRaw) and packed.heights.tolist() == [30, 0]


def test_results_json_names_the_siglip_transforms():
    from knowledge_enhanced_multimodal_retrieval_amd import datasets, evaluators
    rows = [{"image": None, "query_text": "a", "target_text": "b", "uuid": "u0"}]
    assert evaluators.image_transform_name(datasets.CLIPEvalDatasetHF(rows, preprocess.SiglipPreprocess(64, defer_to_gpu=True))).startswith("gpu")
    assert evaluators.image_transform_name(datasets.CLIPEvalDatasetHF(rows, preprocess.SiglipPreprocess(64))).startswith("host (PIL")
    assert evaluators.image_transform_name(datasets.CLIPEvalDatasetHF(rows, preprocess.ClipPreprocess(64))).startswith("host (PIL")
    assert evaluators.image_transform_name(datasets.SyntheticRetrievalDataset(2, 64)).startswith("none")
