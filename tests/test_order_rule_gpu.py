"""GPU: the claim of csrc/rank_order.h -- on finite scores the order rule's two forms (the fp32 predicate of the k <= 32 routes, the
64-bit key of the deep routes) are one order, so on one adversarial input EVERY producer of a ranked list or an `ahead` count returns
the same bits: kemr_rank_dense, kemr_rank_dense_shard (whole, in 2 pieces through the wave merge, in 40 pieces through the block
merge), kemr_topk_merge, kemr_select_topk (offset ids and explicit ids) and kemr_list_fuse's place of the ground truth.

The input: fp32 [3, 1000], multiples of 1/8 in [-2, 2] (hundreds of exact ties per row), one row with several +0.0 AND -0.0, row
stride 1003 with +1e30 in the three columns behind each row (they would lead every list if they were read), the ground truth of each
row inside a run of ties with tied neighbours at id - 1 and id + 1.  The expected order is one numpy lexsort on (id, -score) with
-0.0 folded to +0.0 for the comparison only; output scores are compared as uint32 bits with the input's own.

Only finite values: where the two forms differ -- a NaN entry, a NaN ground truth -- and what the k <= 32 lists admit (-inf, NaN) is
covered by the per-kernel tests (test_rank_dense_shard_gpu.py, test_topk_deep*_gpu.py, test_list_fuse_gpu.py, test_sim_gpu.py)."""
import numpy as np
import pytest
import torch

from knowledge_enhanced_multimodal_retrieval_amd import engine

pytestmark = pytest.mark.gpu

NQ, NG, LD = 3, 1000, 1003
KS = (1, 10, 32)
FAR = 2 ** 31 - 1 - NG                           # the largest id offset that keeps every id an int32
GT = (123, 500, 998)                             # inside a piece, first column of a piece (2 and 40 pieces alike), next to the last column


def make_input():
    """(S [NQ, LD] with the columns behind the rows, expected order [NQ, NG], ground-truth columns [NQ])."""
    rng = np.random.default_rng(20260)
    S = (rng.integers(-16, 17, size=(NQ, LD)) / 8.0).astype(np.float32)
    S[:, NG:] = np.float32(1e30)
    zeros = np.flatnonzero(S[1, :NG] == 0)
    S[1, zeros[::2]] = np.float32(-0.0)          # about fifteen of each sign
    for q, g in enumerate(GT):
        S[q, g - 1:g + 2] = S[q, g]              # tied neighbours on both sides
    S[1, [GT[1] - 1, GT[1] + 1]] = np.float32(-0.0)
    S[1, GT[1]] = np.float32(0.0)                # ... of the other zero
    v = S[:, :NG]
    ids = np.arange(NG)
    order = np.stack([np.lexsort((ids, -np.where(v[q] == 0, np.float32(0), v[q]))) for q in range(NQ)])
    assert np.isfinite(v).all() and order.shape == (NQ, NG)          # the reference alone fills every list of k <= NG entries
    assert np.signbit(v[1][v[1] == 0]).sum() >= 3 and (~np.signbit(v[1][v[1] == 0])).sum() >= 3
    assert all(np.unique(v[q], return_counts=True)[1].max() >= 20 for q in range(NQ))
    return S, order, np.array(GT, np.int32)


@pytest.fixture(scope="module")
def data(device):
    S, order, gt = make_input()
    S_dev = torch.from_numpy(S).to(device)
    ahead = np.array([int(np.flatnonzero(order[q] == gt[q])[0]) for q in range(NQ)], np.int32)      # entries in front of the ground truth
    return dict(S=S, S_dev=S_dev, view=S_dev[:, :NG], order=order, gt=gt, ahead=ahead,
                gt_dev=torch.from_numpy(gt).to(device), sgt_dev=torch.from_numpy(S[np.arange(NQ), gt].copy()).to(device))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def check_lists(d, k, top_s, top_i, off=0, what=""):
    """the first k of the expected order: the ids (after the offset), and the scores as the input's own bits"""
    want_i = d["order"][:, :k]
    got_i = top_i.cpu().numpy().astype(np.int64) - off
    assert np.array_equal(got_i, want_i), f"{what} k={k}: ids"
    want_s = np.take_along_axis(d["S"][:, :NG], want_i, axis=1)
    assert np.array_equal(bits(top_s.cpu().numpy()), bits(want_s)), f"{what} k={k}: score bits"


def shard_route(d, pieces, k, off=0):
    """kemr_rank_dense_shard over `pieces` equal column pieces (views of the strided matrix), the lists merged by kemr_topk_merge"""
    step = NG // pieces
    ahead, ls, li = 0, [], []
    gt = d["gt_dev"] + off
    for lo in range(0, NG, step):
        a, s, i = engine.rank_dense_shard(d["S_dev"][:, lo:lo + step], id_offset=off + lo, gt_idx=gt, gt_score=d["sgt_dev"], k=k)
        ahead = ahead + a
        ls.append(s)
        li.append(i)
    if pieces == 1:
        return ahead, ls[0], li[0]
    s, i = engine.topk_merge(torch.stack(ls, dim=1), torch.stack(li, dim=1), k)
    return ahead, s, i


@pytest.mark.parametrize("k", KS)
def test_rank_dense(data, k):
    ahead, s, i = engine.rank_dense(data["view"], gt_idx=data["gt_dev"], k=k)
    check_lists(data, k, s, i, what="rank_dense")
    assert np.array_equal(ahead.cpu().numpy(), data["ahead"])


@pytest.mark.parametrize("off", [0, FAR])
@pytest.mark.parametrize("pieces", [1, 2])
@pytest.mark.parametrize("k", KS)
def test_rank_dense_shard_whole_and_two_pieces_wave_merge(data, k, pieces, off):
    assert pieces * k <= 256                     # kemr_topk_merge's wave kernel
    ahead, s, i = shard_route(data, pieces, k, off)
    check_lists(data, k, s, i, off, what=f"rank_dense_shard x{pieces}")
    assert np.array_equal(ahead.cpu().numpy(), data["ahead"])


@pytest.mark.parametrize("off", [0, FAR])
def test_rank_dense_shard_forty_pieces_block_merge(data, off):
    k, pieces = 10, 40
    assert pieces * k > 256 and NQ <= 64         # kemr_topk_merge's block kernel
    ahead, s, i = shard_route(data, pieces, k, off)
    check_lists(data, k, s, i, off, what="rank_dense_shard x40")
    assert np.array_equal(ahead.cpu().numpy(), data["ahead"])


@pytest.mark.parametrize("off", [0, FAR])
@pytest.mark.parametrize("k", KS + (33, NG))
def test_select_topk_offset_ids_and_explicit_ids(data, device, k, off):
    s, i = engine.select_topk(data["view"], k, id_offset=off)
    check_lists(data, k, s, i, off, what="select_topk(id_offset)")
    idx = torch.full((NQ, LD), -5, dtype=torch.int32, device=device)
    idx[:, :NG] = torch.arange(off, off + NG, dtype=torch.int64, device=device).to(torch.int32)
    s, i = engine.select_topk(data["view"], k, idx=idx[:, :NG])
    check_lists(data, k, s, i, off, what="select_topk(idx)")


def test_ahead_of_list_fuse_is_rank_dense_s(data, device):
    idx = torch.arange(NG, dtype=torch.int32, device=device).repeat(NQ, 1)
    fused, ahead, found, gt_score = engine.list_fuse(data["view"].contiguous(), idx, depth=NG, scale=1.0, bonus=None, gt_idx=data["gt_dev"])
    dense_ahead, _, _ = engine.rank_dense(data["view"], gt_idx=data["gt_dev"], k=0)
    assert np.array_equal(dense_ahead.cpu().numpy(), data["ahead"])
    assert np.array_equal(ahead.cpu().numpy(), dense_ahead.cpu().numpy())
    assert np.array_equal(found.cpu().numpy(), np.ones(NQ, np.int32))
    assert np.array_equal(bits(gt_score.cpu().numpy()), bits(data["S"][np.arange(NQ), data["gt"]]))
    assert np.array_equal(bits(fused.cpu().numpy()), bits(data["S"][:, :NG]))
