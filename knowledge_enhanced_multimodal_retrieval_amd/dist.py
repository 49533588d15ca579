"""Gallery sharded over the GPUs of one node: one process per GPU, RCCL through ``torch.distributed``.

The reference's eval / search path is single-device; this is new design for BASELINE
config 4.  Gallery items are independent, so each rank encodes and keeps its own contiguous shard resident; a search
has exactly one exchange step:

1. ``all_gather`` of the query embeddings (each rank encoded 1/world of the query batch; 128 x 768 fp32 per rank at
   Q = 1024 -- KB-scale, latency-bound, the xGMI links are never the limit),
2. local fused similarity + top-k against the own shard with global candidate ids (``gallery_offset``),
3. ``all_gather`` of the per-shard candidates ([Q, k] scores + ids), merged by ``kemr_topk_merge`` on every rank.

Ranks of a ground truth add two tiny reductions: the owner shard computes the ground-truth score
(``kemr_pair_scores``; ``all_reduce(sum)`` with zeros elsewhere) and the per-shard ``ahead`` counts are summed.

Step 3 is issued asynchronously (``search_async`` / ``search_many``): the candidate all-gather runs on RCCL's stream while
the compute stream already encodes the NEXT query batch; the merge is queued when the result is asked for.  Every rank must
bring the same number of query rows (a fused all-gather needs equal shapes; unequal ones hang or corrupt under RCCL): that
is checked with one 2-element all-reduce per call and refused with a ValueError on every rank.

The compute calls are taken from an ``ops`` namespace (default: the HIP-backed ``engine`` module) so that the
collective plumbing can be exercised with gloo on CPU-only machines in tests; the product path always uses ``engine``.

The drop-in evaluators reach all this under ``torchrun`` through the last section of the module: ``init_from_env`` / ``finish``
(what a CLI calls first and last), ``active_shard`` (do the evaluators shard?), ``EvenRows`` (equal query rows when ``n`` does not
divide by the world) and ``sharded_ranks_dense`` (the dense learned heads: ``kemr_rank_dense_shard`` per shard + two reductions).
"""
from __future__ import annotations

import os
from typing import Callable, Iterable, Iterator, List, Optional, Sequence, Tuple

import torch
import torch.distributed as dist

from . import _lib, engine, ranking


def shard_bounds(n: int, world: int, rank: int) -> Tuple[int, int]:
    """Contiguous split: rank r owns global ids [lo, hi) with ceil(n / world) items per rank (the last may be short)."""
    per = (n + world - 1) // world
    lo = min(n, rank * per)
    return lo, min(n, lo + per)


def _world(group) -> Tuple[int, int]:
    if dist.is_available() and dist.is_initialized():
        return dist.get_world_size(group), dist.get_rank(group)
    return 1, 0


_FORCE = os.environ.get("KEMR_DIST_FORCE_COLLECTIVES", "") == "1"


def force_collectives(on: bool = True) -> None:
    """A world of ONE rank normally short-circuits every helper below (nothing to exchange).  With this switch on (or
    KEMR_DIST_FORCE_COLLECTIVES=1) and a process group initialised, the collectives are issued anyway -- so that the exact calls an
    8-GPU run makes (device-tensor all_gather_into_tensor, the device branch of require_equal_rows, async work.wait() stream
    ordering, all_reduce, the candidate merge over [world, Q, k]) can be executed through RCCL on a one-GPU box
    (tests/test_dist_rccl_world1.py).  Results are unchanged: gathering one rank's rows is the identity."""
    global _FORCE
    _FORCE = bool(on)


def _skip(world: int) -> bool:
    """True when a helper may return without a collective: one rank and nobody asked for the collectives to run anyway."""
    return world == 1 and not (_FORCE and dist.is_available() and dist.is_initialized())


def _host_staged(x: torch.Tensor, group) -> bool:
    """gloo moves device tensors through the host itself only for some collectives; the rehearsal of the N > 1 path on one GPU
    (KEMR_DIST_BACKEND=gloo, bench.py) stages them explicitly.  RCCL ("nccl") never takes this branch."""
    return x.is_cuda and dist.get_backend(group) == "gloo"


def all_gather_rows(x: torch.Tensor, group=None) -> torch.Tensor:
    """Concatenate equally shaped per-rank tensors along dim 0 (single fused all-gather)."""
    world, _ = _world(group)
    if _skip(world):
        return x
    x = x.contiguous()
    if _host_staged(x, group):
        xc = x.cpu()
        oc = torch.empty((world * xc.shape[0],) + tuple(xc.shape[1:]), dtype=xc.dtype)
        dist.all_gather_into_tensor(oc, xc, group=group)
        return oc.to(x.device)
    out = torch.empty((world * x.shape[0],) + tuple(x.shape[1:]), dtype=x.dtype, device=x.device)
    dist.all_gather_into_tensor(out, x, group=group)
    return out


def all_gather_rows_async(x: torch.Tensor, group=None):
    """As :func:`all_gather_rows`, not waited for: returns (out, work); ``work.wait()`` orders the current stream after it."""
    world, _ = _world(group)
    if _skip(world):
        return x, None
    x = x.contiguous()
    if _host_staged(x, group):
        return all_gather_rows(x, group), None
    out = torch.empty((world * x.shape[0],) + tuple(x.shape[1:]), dtype=x.dtype, device=x.device)
    return out, dist.all_gather_into_tensor(out, x, group=group, async_op=True)


def all_reduce_sum(x: torch.Tensor, group=None) -> torch.Tensor:
    """In-place sum over the ranks (device tensors staged through the host under gloo, see :func:`_host_staged`)."""
    world, _ = _world(group)
    if _skip(world):
        return x
    if _host_staged(x, group):
        xc = x.cpu()
        dist.all_reduce(xc, group=group)
        x.copy_(xc)
        return x
    dist.all_reduce(x, group=group)
    return x


def require_equal_rows(n_local: int, device, group=None, what: str = "query rows") -> None:
    """Refuse, on every rank, a call in which the ranks bring different row counts."""
    world, rank = _world(group)
    if _skip(world):
        return
    t = torch.tensor([n_local, -n_local], dtype=torch.int64)      # host tensor under gloo, device tensor under RCCL
    if dist.get_backend(group) != "gloo":
        t = t.to(device)
    dist.all_reduce(t, op=dist.ReduceOp.MAX, group=group)
    hi, lo = int(t[0]), -int(t[1])
    if hi != lo:
        raise ValueError(f"sharded search: every rank must pass the same number of {what}; rank {rank} has {n_local}, "
                         f"the group has between {lo} and {hi} (pad the last batch or split it evenly)")


class PendingSearch:
    """A search whose candidate exchange is in flight; ``result()`` queues the merge behind it."""

    def __init__(self, merge: Callable, works, tensors):
        self._merge, self._works, self._tensors, self._out = merge, works, tensors, None

    def result(self):
        if self._out is None:
            for w in self._works:
                if w is not None:
                    w.wait()
            self._out = self._merge(*self._tensors)
            self._tensors = None
        return self._out


def _exchange(s, i, k, world, group, ops) -> PendingSearch:
    """Per-shard candidate lists ([Q, k] scores + GLOBAL ids) of all shards -> every rank, not waited for; ``result()`` merges them
    (``kemr_topk_merge``)."""
    if _skip(world):
        return PendingSearch(lambda a, b: (a, b), [], (s, i))
    ss, w1 = all_gather_rows_async(s.unsqueeze(0), group)          # [world, Q, k]
    ii, w2 = all_gather_rows_async(i.unsqueeze(0), group)
    merge = lambda a, b: ops.topk_merge(a.permute(1, 0, 2).contiguous(), b.permute(1, 0, 2).contiguous(), k)
    return PendingSearch(merge, [w1, w2], (ss, ii))


class ShardedGallery:
    """This rank's shard of the gallery, packed for the fused similarity kernel."""

    def __init__(self, local_parts: Sequence[torch.Tensor], n_total: int, precision: str = "fp32x3", group=None, ops=engine):
        self.group, self.ops = group, ops
        # one 2-element all-reduce + host read per call, the only host synchronisation of search / ranks: a caller that guarantees
        # equal batches (a fixed batch size, as bench.py's) clears it for THIS gallery and the whole call is asynchronous
        self.check_rows = True
        self.world, self.rank = _world(group)
        self.n_total = n_total
        self.lo, self.hi = shard_bounds(n_total, self.world, self.rank)
        if local_parts[0].shape[0] != self.hi - self.lo:
            raise ValueError(f"rank {self.rank} owns ids [{self.lo}, {self.hi}) but got {local_parts[0].shape[0]} rows")
        self.terms = ranking.PRECISION_TERMS[precision]
        self.nparts = len(local_parts)
        self.panel = ops.build_panel(list(local_parts), _lib.SIDE_GALLERY, self.terms) if self.hi > self.lo else None

    def _query_panel(self, local_query_parts, weights, row_gate):
        if self.check_rows:
            require_equal_rows(int(local_query_parts[0].shape[0]), local_query_parts[0].device, self.group)
        qs = [all_gather_rows(q, self.group) for q in local_query_parts]
        gates = None
        if row_gate is not None:
            gates = [None if g is None else all_gather_rows(g.reshape(-1, 1), self.group).reshape(-1) for g in row_gate]
        return self.ops.build_panel(qs, _lib.SIDE_QUERY, self.terms, part_scale=weights, row_scale=gates), qs[0].shape[0]

    def _local_topk(self, qp, nq, k, dev, *rank_args, bonus=None):
        if self.panel is not None:
            if bonus is None:
                return self.ops.sim_topk(qp, self.panel, k, self.lo, *rank_args)
            return self.ops.sim_topk(qp, self.panel, k, self.lo, *rank_args, bonus=bonus)
        return (torch.full((nq, k), float("-inf"), dtype=torch.float32, device=dev),
                torch.full((nq, k), -1, dtype=torch.int32, device=dev))

    def _exchange(self, s, i, k) -> PendingSearch:
        """Candidates of all shards -> every rank, not waited for."""
        return _exchange(s, i, k, self.world, self.group, self.ops)

    def search_async(self, local_query_parts: Sequence[torch.Tensor], weights: Optional[Sequence[float]] = None, k: int = 10,
                     row_gate=None, bonus=None) -> PendingSearch:
        """``search`` with the candidate exchange left in flight: encode the next query batch, then call ``result()``."""
        qp, nq = self._query_panel(local_query_parts, weights, row_gate)
        s, i = self._local_topk(qp, nq, k, local_query_parts[0].device, bonus=bonus)
        return self._exchange(s, i, k)

    def search(self, local_query_parts: Sequence[torch.Tensor], weights: Optional[Sequence[float]] = None, k: int = 10,
               row_gate=None, bonus=None) -> Tuple[torch.Tensor, torch.Tensor]:
        """Every rank passes its slice of the query batch (same row count on all ranks) and receives the merged
        top-k of the WHOLE batch against the WHOLE gallery: (scores [Q, k], global ids [Q, k]).
        ``bonus``: a CSR ``(rowptr, col, val)`` over the WHOLE gathered query batch with GLOBAL column ids, the same on every rank;
        each shard adds the entries that fall into its own id range (``kemr_sim_topk``) and the lists hold fused scores."""
        return self.search_async(local_query_parts, weights, k, row_gate, bonus).result()

    def search_deep(self, local_query_parts: Sequence[torch.Tensor], weights: Optional[Sequence[float]] = None, k: int = 100,
                    row_gate=None, bonus=None) -> Tuple[torch.Tensor, torch.Tensor]:
        """``search`` for lists of up to 1024 candidates (``kemr_sim_topk_deep``): every shard's k best of the whole query batch are
        all-gathered as in ``search`` and the [Q, world * k] concatenation is merged by ``select_topk`` with explicit ids.
        ``bonus``: a CSR ``(rowptr, col, val)`` over the WHOLE gathered query batch with GLOBAL column ids, the same on every rank;
        each shard adds the entries that fall into its own id range (``kemr_sim_topk_deep_fused``) and the lists hold fused scores."""
        qp, nq = self._query_panel(local_query_parts, weights, row_gate)
        dev = local_query_parts[0].device
        if self.panel is not None:
            if bonus is None:
                s, i = self.ops.sim_topk_deep(qp, self.panel, k, self.lo)
            else:
                s, i = self.ops.sim_topk_deep(qp, self.panel, k, self.lo, bonus=bonus)
        else:
            s = torch.full((nq, k), float("-inf"), dtype=torch.float32, device=dev)
            i = torch.full((nq, k), -1, dtype=torch.int32, device=dev)
        if _skip(self.world):
            return s, i
        ss, w1 = all_gather_rows_async(s.unsqueeze(0), self.group)          # [world, Q, k]
        ii, w2 = all_gather_rows_async(i.unsqueeze(0), self.group)
        merge = lambda a, b: self.ops.select_topk(a.permute(1, 0, 2).reshape(nq, -1), k, idx=b.permute(1, 0, 2).reshape(nq, -1))
        return PendingSearch(merge, [w1, w2], (ss, ii)).result()

    def search_many(self, batches: Iterable[Sequence[torch.Tensor]], weights: Optional[Sequence[float]] = None, k: int = 10
                    ) -> Iterator[Tuple[torch.Tensor, torch.Tensor]]:
        """A stream of query batches with one batch of lookahead.  ``batches`` is consumed lazily: if producing an element
        encodes the texts (a generator around ``model.encode_text``), the encoder of batch b+1 is queued on the compute
        stream while the candidate all-gather of batch b is still on the wire.  Yields the merged results in order."""
        prev = None
        for parts in batches:
            cur = self.search_async(parts, weights, k)
            if prev is not None:
                yield prev.result()
            prev = cur
        if prev is not None:
            yield prev.result()

    def ranks(self, local_query_parts: Sequence[torch.Tensor], local_gt: torch.Tensor,
              weights: Optional[Sequence[float]] = None, k: int = 10, row_gate=None, bonus=None
              ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """As ``search`` plus the 1-based rank of each query's ground-truth candidate (GLOBAL id in ``local_gt``).  With ``bonus``
        (as in ``search``) the rank is counted on the fused scores: the ground-truth pair's own bonus is added to its score."""
        qp, nq = self._query_panel(local_query_parts, weights, row_gate)
        dev = local_query_parts[0].device
        gt = all_gather_rows(local_gt.to(device=dev, dtype=torch.int32).reshape(-1, 1), self.group).reshape(-1)
        # the ground-truth score of EVERY query against this shard with the local row clamped into it, masked to the queries whose
        # ground truth lives here: no data-dependent shape, no host read (round 2 tested `mine.any()` on the host and gathered rows)
        sgt = torch.zeros(nq, dtype=torch.float32, device=dev)
        if self.panel is not None:
            mine = (gt >= self.lo) & (gt < self.hi)
            local = (gt - self.lo).clamp(0, self.hi - self.lo - 1).to(torch.int32)
            every = self.ops.pair_scores(qp, self.panel, torch.arange(nq, dtype=torch.int32, device=dev), local)
            sgt = torch.where(mine, every, sgt)
        all_reduce_sum(sgt, self.group)                            # exactly one rank contributed a non-zero per query
        if bonus is not None:                                      # the ground-truth pair's own bonus, the same on every rank
            sgt = sgt + ranking._bonus_of_pairs(bonus, gt, dev)
        ahead = torch.zeros(nq, dtype=torch.int32, device=dev)
        s, i = self._local_topk(qp, nq, k, dev, gt, sgt, ahead, bonus=bonus)
        pending = self._exchange(s, i, k) if k > 0 else None       # k == 0: ranks only (what Recall@K / MRR need), nothing to merge
        all_reduce_sum(ahead, self.group)                          # rides while the candidates are gathered
        if pending is not None:
            s, i = pending.result()
        return ahead.long() + 1, s, i

    def rerank(self, fusion_model, local_head_gallery, local_query_embed: torch.Tensor, depth: int = 200, k: int = 10,
               local_gt: Optional[torch.Tensor] = None, bonus=None, head_weight: float = 1.0, shortlist_weights=(0.5, 0.5),
               score_lists: Optional[Callable] = None):
        """``FusionModel.rerank`` over a gallery sharded as ``[image, target]`` parts, with or without the knowledge side.

        1. ``search_deep(k=depth, bonus=...)`` gives every rank the same global shortlist (ids [Q, depth], -1 padded);
        2. every rank scores, against its LOCAL ``HeadGallery`` (``fusion_model.prepare_gallery`` of this rank's shard), only the slots
           whose id lies in its own ``[lo, hi)``; the other slots are handed to the head as -1, which scores -inf;
        3. the non-owners contribute 0 and ONE ``all_reduce_sum`` assembles the list: exactly one rank owns a slot (the trick
           ``ranks`` uses for the ground-truth score), so a score arrives with its own bits (a head score of -0.0 as +0.0, which
           ties with it).  No folded projection and no key row crosses the wire: depth floats per query do;
        4. ``ops.list_fuse`` (``head_weight * head + bonus``, the ground truth's place, ``found``) and ``ops.select_topk`` run on every
           rank on identical inputs, so every rank ends with the same answer.

        ``local_gt``: this rank's queries' GLOBAL ground-truth ids, or None.  ``bonus``: CSR over the WHOLE gathered query batch, GLOBAL
        column ids, the same on every rank.  ``score_lists(q, local_head_gallery, local_idx) -> fp32 [Q, depth]`` defaults to
        ``fusion_model.list_scores`` (the gloo rehearsal substitutes an oracle).  Returns the 5-tuple of ``FusionModel.rerank`` with
        GLOBAL ids; at world size 1 it has that call's bits."""
        depth, k = int(depth), int(k)
        if self.nparts != 2:
            raise ValueError(f"ShardedGallery.rerank: the gallery must be built from [image, target] parts, this one has {self.nparts}")
        if not 1 <= depth <= _lib.MAX_DEEP_K:
            raise ValueError(f"ShardedGallery.rerank: depth={depth} not in 1..{_lib.MAX_DEEP_K}")
        if not 1 <= k <= depth:
            raise ValueError(f"ShardedGallery.rerank: k={k} not in 1..depth={depth}")
        if bonus is None and float(head_weight) != 1.0:
            raise ValueError("ShardedGallery.rerank: head_weight scales the head against a bonus; without bonus it must stay 1.0")
        if self.panel is not None and (local_head_gallery is None or len(local_head_gallery) != self.hi - self.lo):
            raise ValueError(f"ShardedGallery.rerank: rank {self.rank} needs the HeadGallery of its own {self.hi - self.lo} candidates")
        if score_lists is None:
            score_lists = fusion_model.list_scores
        q_local = local_query_embed
        dev = q_local.device
        if bonus is not None and len(bonus[0]) != q_local.shape[0] * self.world + 1:      # every rank brings the same number of rows
            raise ValueError(f"ShardedGallery.rerank: the bonus row pointer must have {q_local.shape[0] * self.world + 1} entries "
                             f"(one row per query of the whole batch), got {len(bonus[0])}")
        _, gi = self.search_deep([q_local, q_local], list(shortlist_weights), depth, bonus=bonus)
        q = all_gather_rows(q_local, self.group)
        nq = q.shape[0]
        lists = torch.zeros((nq, depth), dtype=torch.float32, device=dev)
        if self.panel is not None:
            mine = (gi >= self.lo) & (gi < self.hi)
            local_idx = torch.where(mine, gi - self.lo, torch.full_like(gi, -1)).to(torch.int32).contiguous()
            lists = torch.where(mine, score_lists(q, local_head_gallery, local_idx), lists).contiguous()
        all_reduce_sum(lists, self.group)                          # exactly one rank contributed a non-zero per listed slot
        gt = None
        if local_gt is not None:
            gt = all_gather_rows(local_gt.to(device=dev, dtype=torch.int32).reshape(-1, 1), self.group).reshape(-1)
        fused, ahead, found, gt_score = self.ops.list_fuse(lists, gi, depth, float(head_weight), bonus, gt, out=lists)
        top_s, top_i = self.ops.select_topk(fused, k, idx=gi)
        if gt is None:
            return None, top_s, top_i, fused, gi
        present = found != 0
        ranking._require_finite(gt_score[present], "fused scores at the ground truth")
        ranks = torch.where(present, ahead.long() + 1, torch.full_like(ahead, depth + 1, dtype=torch.int64))
        return ranks, top_s, top_i, fused, gi


# ------------------------------------------------------------------------------------------------ the drop-in evaluators under torchrun
def _torchrun_env() -> Optional[Tuple[int, int, int]]:
    """(world, rank, local_rank) of a torchrun environment with more than one rank, else None: neither RANK nor WORLD_SIZE set, or
    WORLD_SIZE=1, is "no process group" -- the evaluators then run exactly as they do without this module."""
    if "RANK" not in os.environ or "WORLD_SIZE" not in os.environ:
        return None
    world = int(os.environ["WORLD_SIZE"])
    if world <= 1:
        return None
    return world, int(os.environ["RANK"]), int(os.environ.get("LOCAL_RANK", "0"))


def eval_sharded_enabled() -> bool:
    """KEMR_EVAL_SHARDED=0 is the opt-out: under torchrun every rank then encodes and ranks everything alone, as before."""
    return os.environ.get("KEMR_EVAL_SHARDED", "1") != "0"


_OWN_GROUP = False

# The compute namespace of the sharded evaluators (evaluators._ShardedEmbeddings): always the HIP-backed engine in the product; the
# gloo tests on CPU-only machines put a numpy stand-in here, as they pass ``ops=`` to ShardedGallery.
eval_ops = engine


def init_from_env() -> Tuple[int, int, torch.device]:
    """What an evaluator CLI calls first: (world, rank, device) of this process.  Under torchrun (RANK / WORLD_SIZE / LOCAL_RANK)
    it picks ``cuda:{KEMR_LOCAL_DEVICE or LOCAL_RANK}`` and initialises "nccl" (RCCL) with ``device_id=`` BEFORE anything else
    touches the GPU; KEMR_DIST_BACKEND=gloo initialises gloo instead (several ranks on ONE GPU with KEMR_LOCAL_DEVICE=0: the
    rehearsal of the N > 1 path; RCCL refuses two ranks on a device).  Without a torchrun environment, or with
    KEMR_EVAL_SHARDED=0, it does nothing and returns (1, 0, ``cuda`` or ``cpu``)."""
    global _OWN_GROUP
    env = _torchrun_env()
    if env is None or not eval_sharded_enabled():
        return 1, 0, torch.device("cuda" if torch.cuda.is_available() else "cpu")      # (no index: the GPU is not touched here)
    world, rank, local_rank = env
    dev = torch.device("cpu")
    if torch.cuda.is_available():
        dev = torch.device("cuda", int(os.environ.get("KEMR_LOCAL_DEVICE", local_rank)))
        torch.cuda.set_device(dev)
    if not dist.is_initialized():
        backend = os.environ.get("KEMR_DIST_BACKEND", "nccl")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(backend)
        _OWN_GROUP = True
    return dist.get_world_size(), dist.get_rank(), dev


def finish() -> None:
    """The counterpart of :func:`init_from_env`: a barrier and the end of the process group it created (nothing otherwise)."""
    global _OWN_GROUP
    if _OWN_GROUP and dist.is_available() and dist.is_initialized():
        dist.barrier()
        dist.destroy_process_group()
    _OWN_GROUP = False


def active_shard(group=None) -> Optional[Tuple[int, int]]:
    """(rank, world) when the evaluators shard their work: a process group is initialised, it has more than one rank (or the
    collectives are forced, see :func:`force_collectives`) and KEMR_EVAL_SHARDED is not 0.  None: the single-process code runs."""
    if not (dist.is_available() and dist.is_initialized()) or not eval_sharded_enabled():
        return None
    world, rank = _world(group)
    return None if _skip(world) else (rank, world)


def is_writer(group=None) -> bool:
    """True on the one rank that creates output directories, log files and result files (rank 0; every rank without a group)."""
    return _world(group)[1] == 0


def all_gather_list(items: list, group=None) -> list:
    """The ranks' python lists concatenated in rank order (``all_gather_object``; used ONCE per evaluation, for the uuids)."""
    world, _ = _world(group)
    if _skip(world):
        return list(items)
    parts: List[Optional[list]] = [None] * world
    dist.all_gather_object(parts, list(items), group=group)
    return [x for part in parts for x in part]


class EvenRows:
    """Equal-rows padding of a contiguous split.  ``ShardedGallery`` refuses unequal query rows and ``n`` need not divide by the
    world, so every rank brings ``per = ceil(n / world)`` query rows: its own ``hi - lo`` and zero vectors with ground truth 0 behind
    them.  ``shard_bounds`` fills the ranks front to back, so the gathered row r * per + j IS the global item r * per + j and the
    pad rows are exactly the gathered rows >= n: ``real()`` drops them before any metric sees them."""

    def __init__(self, n: int, group=None):
        self.n, self.group = int(n), group
        self.world, self.rank = _world(group)
        self.per = (self.n + self.world - 1) // self.world
        self.lo, self.hi = shard_bounds(self.n, self.world, self.rank)
        self.rows = self.per * self.world

    def pad(self, x: torch.Tensor) -> torch.Tensor:
        """[hi - lo, ...] -> [per, ...], zeros behind the own rows."""
        if x.shape[0] != self.hi - self.lo:
            raise ValueError(f"rank {self.rank} owns items [{self.lo}, {self.hi}) but got {x.shape[0]} rows")
        if x.shape[0] == self.per:
            return x
        return torch.cat([x, torch.zeros((self.per - x.shape[0],) + tuple(x.shape[1:]), dtype=x.dtype, device=x.device)])

    def local_gt(self, device) -> torch.Tensor:
        """The padded rows' GLOBAL ground-truth ids (query lo + j <-> candidate lo + j; pad rows: 0), int32 [per]."""
        return self.pad(torch.arange(self.lo, self.hi, dtype=torch.int32, device=device))

    def all_gt(self, device) -> torch.Tensor:
        """``local_gt`` of every rank, as the gathered rows carry it: int32 [world * per]."""
        g = torch.arange(self.rows, dtype=torch.int32, device=device)
        return torch.where(g < self.n, g, torch.zeros_like(g))

    def pad_bonus(self, bonus):
        """A CSR over the n real queries -> one over all gathered rows (the pad rows hold no entry)."""
        import numpy as np
        ptr = np.asarray(bonus[0])
        if len(ptr) != self.n + 1:
            raise ValueError(f"the bonus row pointer must have {self.n + 1} entries, got {len(ptr)}")
        return np.concatenate([ptr, np.full(self.rows - self.n, ptr[-1], ptr.dtype)]), bonus[1], bonus[2]

    def real(self, gathered: torch.Tensor) -> torch.Tensor:
        if gathered.shape[0] != self.rows:
            raise ValueError(f"expected {self.rows} gathered rows, got {gathered.shape[0]}")
        return gathered[: self.n]


def sharded_ranks_dense(local_scores: torch.Tensor, lo: int, gt_global: torch.Tensor, k: int = 0, group=None, ops=engine
                        ) -> Tuple[torch.Tensor, Optional[torch.Tensor], Optional[torch.Tensor]]:
    """Ranks (and top-k) of a dense score matrix whose COLUMNS are sharded: ``local_scores`` fp32 [Q_all, n_local] holds every query's
    scores against this rank's candidates, GLOBAL ids ``lo .. lo + n_local - 1`` (the dense learned heads: ``forward(all_q, local_img,
    local_tgt)``); ``gt_global`` [Q_all] GLOBAL ground-truth ids, the same on every rank.

    1. the owner reads the ground-truth score ``S[q, gt - lo]`` (masked and clamped: no data-dependent shape, no host read; zeros on
       the other ranks) and ONE ``all_reduce_sum`` hands it to everybody -- 4 * Q_all bytes;
    2. a non-finite ground-truth score is refused (``ranking._require_finite``);
    3. ``ops.rank_dense_shard`` counts this shard's columns ahead of it and lists its k best with GLOBAL ids;
    4. ``all_reduce_sum(ahead)`` -- 4 * Q_all bytes -- and, for k > 0, the candidate exchange + merge of ``ShardedGallery.search``.
    Returns (ranks int64 [Q_all] 1-based, top scores, top ids), the same on every rank."""
    world, _ = _world(group)
    dev = local_scores.device
    nq, nl = local_scores.shape
    gt = gt_global.to(device=dev, dtype=torch.int32).reshape(-1)
    if gt.numel() != nq:
        raise ValueError(f"sharded_ranks_dense: {nq} score rows but {gt.numel()} ground-truth ids")
    sgt = torch.zeros(nq, dtype=torch.float32, device=dev)
    if nl > 0:
        mine = (gt >= lo) & (gt < lo + nl)
        local = (gt.long() - lo).clamp(0, nl - 1)
        sgt = torch.where(mine, local_scores.gather(1, local.view(-1, 1)).reshape(-1).float(), sgt)
    all_reduce_sum(sgt, group)                                     # exactly one rank contributed a non-zero per query
    ranking._require_finite(sgt, "ground-truth scores")
    ahead, s, i = ops.rank_dense_shard(local_scores, lo, gt, sgt, k)
    pending = _exchange(s, i, k, world, group, ops) if k > 0 else None
    all_reduce_sum(ahead, group)
    if pending is not None:
        s, i = pending.result()
    return ahead.long() + 1, s, i
