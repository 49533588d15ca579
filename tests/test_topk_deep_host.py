"""No GPU: argument checks of the deep top-k entry points (they run before any HIP call) and the collective plumbing of
ShardedGallery.search_deep at world size 2 over gloo, with a numpy stand-in for the kernels (TEST ONLY)."""
import ctypes as C
import os
import sys

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from knowledge_enhanced_multimodal_retrieval_amd import _lib, retriever

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _err(L):
    return (L.kemr_last_error() or b"").decode()


def test_select_topk_argument_checks():
    L = _lib.lib()
    buf = (C.c_float * 64)()                               # host memory: every call below fails before a pointer is used
    p = C.c_void_p(C.addressof(buf))
    assert L.kemr_select_topk(None, None, 1, 8, 8, 0, 4, p, p, None) == -1
    assert L.kemr_select_topk(p, None, 1, 8, 8, 0, 4, None, p, None) == -1
    assert L.kemr_select_topk(p, None, 1, 8, 8, 0, 4, p, None, None) == -1
    assert L.kemr_select_topk(p, None, 1, 8, 8, 0, 1025, p, p, None) == -1 and "k=1025" in _err(L)
    assert L.kemr_select_topk(p, None, 1, 8, 8, 0, 0, p, p, None) == -1 and "k=0" in _err(L)
    assert L.kemr_select_topk(p, None, 1, 8, 7, 0, 4, p, p, None) == -1 and "ld=7" in _err(L)
    assert L.kemr_select_topk(p, None, 1, 8, 8, 2 ** 31 - 4, 4, p, p, None) == -1 and "int32" in _err(L)
    assert L.kemr_select_topk(p, None, 0, 8, 8, 0, 4, p, p, None) == 0          # no rows: nothing to do


def test_sim_topk_deep_argument_checks():
    L = _lib.lib()
    buf = (C.c_float * 64)()
    p = C.c_void_p(C.addressof(buf))
    assert L.kemr_sim_topk_deep(None, 4, p, 4, 64, 0, 4, p, p, p, 1 << 20, None) == -1
    assert L.kemr_sim_topk_deep(p, 4, None, 4, 64, 0, 4, p, p, p, 1 << 20, None) == -1
    assert L.kemr_sim_topk_deep(p, 4, p, 4, 64, 0, 4, None, p, p, 1 << 20, None) == -1
    assert L.kemr_sim_topk_deep(p, 4, p, 4, 64, 0, 4, p, None, p, 1 << 20, None) == -1
    assert L.kemr_sim_topk_deep(p, 4, p, 4, 64, 0, 1025, p, p, p, 1 << 20, None) == -1 and "k=1025" in _err(L)
    assert L.kemr_sim_topk_deep(p, 4, p, 4, 64, 0, 0, p, p, p, 1 << 20, None) == -1 and "k=0" in _err(L)
    assert L.kemr_sim_topk_deep(p, 4, p, 4, 64, 2 ** 31 - 2, 4, p, p, p, 1 << 20, None) == -1 and "int32" in _err(L)
    assert L.kemr_sim_topk_deep(p, 4, p, 4, 64, 0, 4, p, p, None, 1 << 20, None) == -4        # KEMR_ERR_WORKSPACE
    assert L.kemr_sim_topk_deep(p, 4, p, 4, 64, 0, 4, p, p, p, 127 * 4 * 4, None) == -4       # fewer than 128 rows of ceil4(4) floats


def test_workspace_size_and_limits():
    L = _lib.lib()
    full = L.kemr_sim_topk_deep_workspace_bytes(1024, 43000, 768, 100)
    assert full == 1024 * 43000 * 4 and full % 256 == 0
    assert L.kemr_sim_topk_deep_workspace_bytes(5000, 43000, 768, 100) == full                # never more than 1024 rows
    assert L.kemr_sim_topk_deep_workspace_bytes(1, 43001, 768, 1000) == 128 * 43004 * 4       # whole 128-row tiles of ceil4(ng) floats
    assert L.kemr_sim_topk_deep_workspace_bytes(0, 43000, 768, 100) == 0
    assert retriever.MAX_DEEP_TOP_K == 1024 == _lib.MAX_DEEP_K and retriever.MAX_TOP_K == 32


class DeepOracleOps:
    """numpy stand-in with the signatures of engine.build_panel / sim_topk_deep / select_topk."""

    class P:
        def __init__(self, mat):
            self.mat, self.rows, self.kdim, self.device = mat, mat.shape[0], mat.shape[1], torch.device("cpu")

    @staticmethod
    def build_panel(parts, side, terms=3, part_scale=None, row_scale=None):
        cols = []
        for p, t in enumerate(parts):
            x = t.double().numpy().copy()
            if part_scale is not None:
                x *= part_scale[p]
            cols.append(x)
        return DeepOracleOps.P(np.concatenate(cols, 1))

    @staticmethod
    def _take(s, i, k):
        nq = s.shape[0]
        out_s = np.full((nq, k), -np.inf, np.float32)
        out_i = np.full((nq, k), -1, np.int32)
        for r in range(nq):
            ok = i[r] >= 0
            o = np.lexsort((i[r][ok], -s[r][ok]))[:k]
            out_s[r, :len(o)], out_i[r, :len(o)] = s[r][ok][o], i[r][ok][o]
        return torch.from_numpy(out_s), torch.from_numpy(out_i)

    @staticmethod
    def sim_topk_deep(qp, gp, k, gallery_offset=0, query_block=None):
        S = (qp.mat @ gp.mat.T).astype(np.float32)
        ids = np.broadcast_to(np.arange(gp.rows, dtype=np.int32) + gallery_offset, S.shape)
        return DeepOracleOps._take(S, ids, k)

    @staticmethod
    def select_topk(scores, k, idx=None, id_offset=0):
        s = scores.numpy()
        i = idx.numpy() if idx is not None else np.broadcast_to(np.arange(s.shape[1], dtype=np.int32) + id_offset, s.shape)
        return DeepOracleOps._take(s, i, k)


def _worker(rank, world, port, n, nq, d, k, q_out):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from knowledge_enhanced_multimodal_retrieval_amd.dist import ShardedGallery, shard_bounds
    from oracle import metrics_ref
    img, q, t = metrics_ref.planted_embeddings(n, d, seed=3)
    lo, hi = shard_bounds(n, world, rank)
    gal = ShardedGallery([torch.from_numpy(img[lo:hi]), torch.from_numpy(t[lo:hi])], n, group=None, ops=DeepOracleOps)
    per = nq // world
    ql = torch.from_numpy(q[rank * per:(rank + 1) * per])
    s, i = gal.search_deep([ql, ql], weights=[0.3, 0.7], k=k)
    q_out.put((rank, s.numpy(), i.numpy()))
    dist.barrier()
    dist.destroy_process_group()


def test_sharded_search_deep_world2():
    """Both ranks end with the merged k = 100 lists of the WHOLE query batch against the WHOLE gallery (shards of 75 and 76
    rows: shorter than k, so the exchanged lists carry -inf / -1 padding that the merge skips)."""
    from oracle import metrics_ref
    world, n, nq, d, k = 2, 151, 16, 32, 100
    port = 29500 + (os.getpid() + 1231) % 2000
    ctx = mp.get_context("spawn")
    q_out = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, n, nq, d, k, q_out)) for r in range(world)]
    for p in procs:
        p.start()
    results = [q_out.get(timeout=180) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    img, q, t = metrics_ref.planted_embeddings(n, d, seed=3)
    S = (np.concatenate([0.3 * q[:nq].astype(np.float64), 0.7 * q[:nq].astype(np.float64)], 1)
         @ np.concatenate([img.astype(np.float64), t.astype(np.float64)], 1).T).astype(np.float32)
    ids = np.arange(n)
    for rank, s, i in results:
        assert s.shape == (nq, k) and i.shape == (nq, k)
        for r in range(nq):
            o = np.lexsort((ids, -S[r]))[:k]
            assert np.array_equal(i[r], ids[o]), (rank, r)
            assert np.array_equal(s[r], S[r, o]), (rank, r)
