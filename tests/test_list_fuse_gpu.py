"""GPU: kemr_list_fuse -- scale, SPARQL bonus and the ground truth's place on a learned head's listed scores -- against the numpy
restatement of its contract (tests/list_fuse_ref.py), BIT FOR BIT: the kernel's arithmetic is fully specified (one fp32 multiply,
fp32 adds in list order) and its counts are integers, so no tolerance applies."""
import ctypes as C

import numpy as np
import pytest
import torch

import list_fuse_ref as ref
from knowledge_enhanced_multimodal_retrieval_amd import _lib, engine

pytestmark = pytest.mark.gpu

DEPTHS = [1, 31, 32, 33, 255, 256, 257, 1000, 1024]
SENTINEL = 7.0
BEYOND = 2 ** 31 - 2          # a bonus column beyond any gallery id


def make_case(nq, depth, seed=0):
    """Lists with everything the contract names.  Scores are multiples of 0.25 (many ties across ids on both sides of the ground
    truth, which survive a bonus of multiples of 0.25) with -0.0 / +0.0 / -inf mixed in; -1 ids in the middle of rows and at their
    ends, an all-padding row; the three extra columns hold valid-looking ids and scores that must never be read.  Bonus rows by
    (q + depth) % 4: empty / one listed column three times with an order-dependent sum + columns outside the list and beyond any
    id / a few hundred random entries / 5 000 entries (beyond what the kernel stages in LDS).  Ground truth by q % 3: slot 0, the
    last slot, absent (its id sits in an extra column)."""
    rng = np.random.default_rng(1000 * depth + 10 * nq + seed)
    ld, universe = depth + 3, 4 * depth + 8
    S = (rng.integers(-8, 9, (nq, ld)) * 0.25).astype(np.float32)
    special = rng.random((nq, ld))
    S[special < 0.05] = -0.0
    S[(special >= 0.05) & (special < 0.10)] = 0.0
    S[(special >= 0.10) & (special < 0.13)] = -np.inf
    I = np.stack([rng.permutation(universe)[:ld] for _ in range(nq)]).astype(np.int32)
    gt = np.zeros(nq, np.int32)
    for q in range(nq):
        kind = q % 3
        if depth > 4:
            I[q, rng.integers(1, depth - 1, max(1, depth // 16))] = -1                  # padding in the middle
            if kind != 1:
                I[q, depth - max(1, depth // 10):depth] = -1                            # ... and at the end
        gt[q] = I[q, 0] if kind == 0 else I[q, depth - 1] if kind == 1 else I[q, depth]  # absent: only in an extra column
        if kind != 2 and depth >= 8:                                                    # same score, lower and higher id than gt
            S[q, 0 if kind == 0 else depth - 1] = 0.5
            others = [j for j in range(1, depth - 1) if I[q, j] >= 0]
            lower = [j for j in others if I[q, j] < gt[q]][:2]
            higher = [j for j in others if I[q, j] > gt[q]][:2]
            S[q, lower + higher] = 0.5
    if nq >= 3:
        I[nq - 1, :depth] = -1                                                          # a row that is all padding
    ptr, cols, vals = [0], [], []
    for q in range(nq):
        kind = (q + depth) % 4
        entries = []
        listed = [int(c) for c in I[q, :depth] if c >= 0]
        if kind == 1:
            c = listed[len(listed) // 2] if listed else 3
            entries += [(c, 1e8), (c, -1e8), (c, 1.0)]                                  # in this order 1.0 survives; sorted, it does not
            entries += [(universe + 5, 0.5), (universe + 9, 0.25), (BEYOND, 0.75), (int(I[q, depth]), 2.0)]
            entries += [(x, 0.25) for x in listed[:3]]
        elif kind == 2:
            entries += [(int(x), float(v)) for x, v in zip(rng.integers(0, universe + 50, 300), rng.integers(1, 5, 300) * 0.25)]
        elif kind == 3:
            entries += [(int(x), float(v)) for x, v in zip(rng.integers(0, 2 * universe + 3000, 5000), rng.integers(1, 9, 5000) * 0.25)]
            entries += [(x, 0.5) for x in listed[::7]]
        entries.sort(key=lambda e: e[0])                                                # stable: a column's entries keep their order
        cols += [e[0] for e in entries]
        vals += [e[1] for e in entries]
        ptr.append(len(cols))
    bonus = (np.asarray(ptr, np.int32), np.asarray(cols, np.int32), np.asarray(vals, np.float32))
    return S, I, gt, bonus


def _same_bits(got, want, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.dtype == want.dtype and got.shape == want.shape, what
    if got.dtype == np.float32:
        assert np.array_equal(ref.bits(got), ref.bits(want)), what
    else:
        assert np.array_equal(got, want), what


def _run(S, I, depth, scale, bonus, gt, device, out=None):
    Sd, Id = torch.from_numpy(S).to(device), torch.from_numpy(I).to(device)
    if out is None:
        out = torch.full(S.shape, SENTINEL, dtype=torch.float32, device=device)
    return engine.list_fuse(Sd, Id, depth, scale, bonus, None if gt is None else torch.from_numpy(gt).to(device), out=out)


@pytest.mark.parametrize("nq", [1, 3, 70])
@pytest.mark.parametrize("depth", DEPTHS)
def test_list_fuse_matches_the_restatement_bit_for_bit(device, depth, nq):
    S, I, gt, bonus = make_case(nq, depth)
    sentinel = np.full(S.shape, SENTINEL, np.float32)
    scale = 0.75
    want = ref.list_fuse(S, I, depth, scale, bonus, gt, out=sentinel)
    got = _run(S, I, depth, scale, bonus, gt, device)
    for g, w, what in zip(got, want, ("fused", "ahead", "found", "gt_score")):
        _same_bits(g, w, what)
    assert (got[0].cpu().numpy()[:, depth:] == SENTINEL).all()                          # columns >= depth: not touched
    if nq >= 3:                                                                         # the ground-truth kinds and the padded row
        f = got[2].cpu().numpy()
        assert f[0] == 1 and f[1] == (1 if nq - 1 != 1 else 0) and f[2] == 0 and np.isneginf(got[3].cpu().numpy()[2])
        assert np.isneginf(got[0].cpu().numpy()[nq - 1, :depth]).all() and got[1].cpu().numpy()[nq - 1] == 0
    # a pure function of its input
    again = _run(S, I, depth, scale, bonus, gt, device)
    assert all(torch.equal(a, b) for a, b in zip(got, again))
    # out aliasing scores
    Sd, Id = torch.from_numpy(S).to(device), torch.from_numpy(I).to(device)
    alias = engine.list_fuse(Sd, Id, depth, scale, bonus, torch.from_numpy(gt).to(device), out=Sd)
    assert alias[0].data_ptr() == Sd.data_ptr()
    assert torch.equal(alias[0][:, :depth], got[0][:, :depth]) and np.array_equal(ref.bits(Sd[:, depth:].cpu().numpy()), ref.bits(S[:, depth:]))
    assert all(torch.equal(a, b) for a, b in zip(alias[1:], got[1:]))
    # each argument group on its own, and neither
    for b, g in ((None, gt), (bonus, None), (None, None)):
        want = ref.list_fuse(S, I, depth, scale, b, g, out=sentinel)
        got_g = _run(S, I, depth, scale, b, g, device)
        for a, w, what in zip(got_g, want, ("fused", "ahead", "found", "gt_score")):
            if w is None:
                assert a is None, what
            else:
                _same_bits(a, w, what)
    # scale == 1.0 keeps the bits of every listed score
    plain = _run(S, I, depth, 1.0, None, None, device)[0].cpu().numpy()
    real = np.zeros(S.shape, bool)
    real[:, :depth] = I[:, :depth] >= 0
    assert np.array_equal(ref.bits(plain)[real], ref.bits(S)[real]) and np.isneginf(plain[:, :depth][I[:, :depth] < 0]).all()
    # where the ground truth is listed, ahead + 1 is its position in the deep selection of the fused list
    fused, ahead, found, _ = got
    top_s, top_i = engine.select_topk(fused[:, :depth], depth, idx=torch.from_numpy(I).to(device)[:, :depth])
    top_i, ahead, found = top_i.cpu().numpy(), ahead.cpu().numpy(), found.cpu().numpy()
    for q in range(nq):
        where = np.flatnonzero(top_i[q] == gt[q])
        assert len(where) == found[q]
        if found[q]:
            assert where[0] == ahead[q], (q, where, ahead[q])
        else:
            assert ahead[q] == (I[q, :depth] >= 0).sum()
    want_s, want_i = ref.sorted_rows(fused.cpu().numpy()[:, :depth], I[:, :depth], depth)
    assert np.array_equal(top_i, want_i) and np.array_equal(ref.bits(top_s.cpu().numpy()), ref.bits(want_s))


def test_list_fuse_nan_scores_rank_behind_minus_inf(device):
    """NaN scores (and a NaN made by the bonus: -inf + inf) follow the order rule of kemr_select_topk: behind -inf, by id."""
    depth, nq = 40, 6
    S, I, gt, _ = make_case(nq, depth, seed=5)
    S[:, 3] = np.nan
    S[:, 7] = np.nan
    S[1, 0] = np.nan                                                                    # the ground truth itself (q % 3 == 0 is slot 0)
    S[0, 0] = np.nan
    S[3, 5] = -np.inf
    I[:, [3, 5, 7]] = [500, 501, 502]                                                   # listed for sure, ids of their own
    ptr = np.arange(nq + 1, dtype=np.int32)
    bonus = (ptr, I[:, 5].copy(), np.full(nq, np.inf, np.float32))                      # row 3: -inf + inf = NaN
    want = ref.list_fuse(S, I, depth, 1.0, bonus, gt)
    got = _run(S, I, depth, 1.0, bonus, gt, device)
    wf, gf = want[0][:, :depth], got[0].cpu().numpy()[:, :depth]
    assert np.array_equal(np.isnan(wf), np.isnan(gf)) and np.isnan(gf[3, 5])
    assert np.array_equal(ref.bits(np.nan_to_num(gf, nan=0.0)), ref.bits(np.nan_to_num(wf, nan=0.0)))
    assert np.array_equal(got[1].cpu().numpy(), want[1]) and np.array_equal(got[2].cpu().numpy(), want[2])
    top_i = engine.select_topk(got[0][:, :depth], depth, idx=torch.from_numpy(I).to(device)[:, :depth])[1].cpu().numpy()
    for q in range(nq):
        if want[2][q]:
            assert top_i[q, want[1][q]] == gt[q]


def test_list_fuse_argument_groups_and_wrapper(device):
    L = _lib.lib()
    S, I, gt, bonus = make_case(3, 33)
    dev = lambda a: torch.from_numpy(a).to(device)
    Sd, Id, gtd, (bp, bc, bv) = dev(S), dev(I), dev(gt), (dev(b) for b in bonus)
    out = torch.empty_like(Sd)
    i3, f3 = torch.empty(3, dtype=torch.int32, device=device), torch.empty(3, dtype=torch.float32, device=device)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream(device).cuda_stream)

    def call(b=(None, None, None), g=(None, None, None, None), depth=33, ld=36, nq=3):
        status = L.kemr_list_fuse(p(Sd), p(Id), nq, depth, ld, 1.0, p(b[0]), p(b[1]), p(b[2]), p(g[0]), p(g[1]), p(g[2]), p(g[3]), p(out), stream)
        return status, L.kemr_last_error().decode()

    full_b, full_g = (bp, bc, bv), (gtd, i3, i3.clone(), f3)
    assert call(full_b, full_g)[0] == 0 and call()[0] == 0
    for drop in range(3):
        status, msg = call(b=tuple(None if i == drop else t for i, t in enumerate(full_b)))
        assert status == -1 and "bonus CSR arrays must be given together" in msg
    for drop in range(4):
        status, msg = call(g=tuple(None if i == drop else t for i, t in enumerate(full_g)))
        assert status == -1 and "must be given together" in msg
    assert call(depth=0)[0] == -1 and call(depth=1025, ld=1025)[0] == -1 and call(depth=33, ld=32)[0] == -1
    assert call(nq=0)[0] == 0
    torch.cuda.synchronize(device)
    # the wrapper: a fresh tensor reads -inf beyond depth; an empty CSR is no bonus; shapes are checked before the launch
    fresh = engine.list_fuse(Sd, Id, 20, 0.5)[0]
    assert np.isneginf(fresh.cpu().numpy()[:, 20:]).all()
    empty = (np.zeros(4, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32))
    assert torch.equal(engine.list_fuse(Sd, Id, 20, 0.5, bonus=empty)[0], fresh)
    with pytest.raises(RuntimeError, match="nq \\+ 1"):
        engine.list_fuse(Sd, Id, 20, 0.5, bonus=(bonus[0][:-1], bonus[1], bonus[2]))
    with pytest.raises(RuntimeError, match="one entry per query"):
        engine.list_fuse(Sd, Id, 20, gt_idx=gtd[:2])
    with pytest.raises(RuntimeError, match="depth=37"):
        engine.list_fuse(Sd, Id, 37)
    with pytest.raises(RuntimeError, match="share one"):
        engine.list_fuse(Sd, Id[:, :30])
