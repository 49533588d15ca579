"""Evaluation loops and CLIs of the reference, device-resident.

Counterparts of /root/reference/src/clip/eval/evaluator.py (``evaluate_clip_model`` :53-221,
``evaluate_clip_model_for_training`` :224-257, ``main`` :260-390) and evaluator_baseline.py (``evaluate_clip_model``
:38-146, ``main`` :150-274), with the defects listed in SURVEY.md section 3.5 routed around (4-tuple batches,
``--splits_file`` accepted, ``val`` -> ``validation``, import-time side effects made lazy).

What changes on the hot path: the reference copies every batch of embeddings back to the host
(``.cpu().numpy()``, evaluator.py:123,129,135) and ranks with numpy; here the three embedding sets stay in HBM and go
straight into the fused similarity / rank kernels, L2 normalisation is fused into the encoder tail.
"""
from __future__ import annotations

import argparse
import logging
import os
import random
from pathlib import Path
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
from torch.utils.data import DataLoader

from . import _lib
from . import dist as KD
from . import engine
from . import metrics as M
from . import sparql_fusion as SF
from .datasets import TextOnlyDatasetHF, collate_fn_eval_texts
from .datasets import CLIPEvalDatasetHF, CollateAndTokenize, SyntheticHFSplit, SyntheticRawImageDataset, SyntheticRetrievalDataset, collate_fn_eval
from .preprocess import ClipPreprocessGPU, PackedRaw, gpu_preprocess_for
from .logging_utils import save_metrics_to_json, setup_logger

logger = logging.getLogger(__name__)

TEXT2SPARQL_DIR = "experiments/text2sparql/results"
ALPHAS = [0.9, 0.8, 0.7, 0.6, 0.5, 0.4, 0.3, 0.2, 0.1]


def seed_worker(worker_id):
    worker_seed = torch.initial_seed() % 2 ** 32
    np.random.seed(worker_seed)
    random.seed(worker_seed)


def load_text2sparql_results(directory: str = TEXT2SPARQL_DIR) -> Dict[str, List[str]]:
    """uuid -> list of artefact URIs, one file per query (reference evaluator.py:43-50, but lazy and tolerant)."""
    out: Dict[str, List[str]] = {}
    if not os.path.isdir(directory):
        return out
    for fn in os.listdir(directory):
        with open(os.path.join(directory, fn), "r") as f:
            out[fn.split(".")[0]] = [line.strip() for line in f.readlines()]
    return out


def default_tokenize(texts: Sequence[str]) -> torch.Tensor:
    from .tokenizer import tokenize
    return tokenize(list(texts), truncate=True)


def model_tokenize(model) -> Callable:
    """The tokenize callable that goes with `model` when the caller names none: CLIP's BPE (`default_tokenize`), or, for a SigLIP
    model, `tokenizer.siglip_tokenizer` on the directory its `tokenizer_dir` attribute names (`clip.load(<dir>)` sets it to the
    checkpoint directory; `--tokenizer_dir` / an assignment set it otherwise).  A SigLIP model without one cannot be tokenised for --
    CLIP's ids are [B, 77] of another vocabulary -- so that is an error here, before any data is read.
    A CLIP-family model with a longer text tower than CLIP's 77 positions (Long-CLIP: 248) gets CLIP's BPE cut at ITS context length,
    `tokenizer.ClipTokenize(arch.ctx)` -> [B, arch.ctx] ids, picklable for the loader workers; at 77 -- and for the shorter test
    shapes, as before -- it is `default_tokenize` itself (`model_tokenizer_name` compares by identity)."""
    arch = getattr(model, "arch", None)
    if arch is None or getattr(arch, "family", "clip") != "siglip":
        if arch is not None and getattr(arch, "family", "clip") == "clip" and int(getattr(arch, "ctx", 77)) > 77:
            from .tokenizer import ClipTokenize
            return ClipTokenize(arch.ctx)
        return default_tokenize
    directory = getattr(model, "tokenizer_dir", None)
    if not directory:
        raise RuntimeError("a SigLIP model needs its own tokenizer and this one names none: it was not loaded from a directory that holds "
                           "a tokenizer.json.  Set model.tokenizer_dir (evaluator CLIs: --tokenizer_dir DIR) to a directory with the "
                           "checkpoint's tokenizer.json, or pass tokenize_fn= (pre-tokenised ids [B, %d] always work)" % arch.ctx)
    from .tokenizer import siglip_tokenizer
    return siglip_tokenizer(directory, arch.ctx)


def model_tokenizer_name(model) -> str:
    """What the results JSON records under "tokenizer"."""
    from . import tokenizer
    fn = model_tokenize(model)
    if fn is default_tokenize:
        return tokenizer.tokenizer_name()
    if isinstance(fn, tokenizer.ClipTokenize):
        return f"{tokenizer.tokenizer_name()} context_length={fn.context_length}"
    return f"siglip tokenizers ({fn.path})"


ENCODE_ITEMS = 255          # items per encoder call in encode_dataset (see there)


def default_loader_workers() -> int:
    """Loader processes of the drop-in CLIs (the reference's scripts leave the DataLoader at 4, evaluator_baseline.py:83-92, or at
    0, evaluator.py:97-106): KEMR_LOADER_WORKERS, else min(12, half the cores this process may use).  With the image transform on
    the GPU a worker only decodes and tokenises; 12 of them deliver 17 k items/s, 0 leaves 1.5 k on the consumer."""
    v = os.environ.get("KEMR_LOADER_WORKERS", "")
    if v.strip():
        return max(0, int(v))
    try:
        cores = len(os.sched_getaffinity(0))
    except AttributeError:
        cores = os.cpu_count() or 1
    return max(0, min(12, cores // 2))


_FORKSERVER_PRELOAD = ["torch", "numpy", "PIL.Image", "knowledge_enhanced_multimodal_retrieval_amd.datasets",
                       "knowledge_enhanced_multimodal_retrieval_amd.preprocess", "knowledge_enhanced_multimodal_retrieval_amd.tokenizer",
                       "knowledge_enhanced_multimodal_retrieval_amd.evaluators"]


def loader_context():
    """Start method of the loader processes: "forkserver" (KEMR_LOADER_CONTEXT overrides: fork | spawn | forkserver).
    The evaluators' process has an initialised HIP context, GPU-mapped pinned buffers and gigabytes of weights by the time the
    loader starts; workers forked from IT share all of that copy-on-write.  Measured (round 3, tools/probe_pipeline_state.py, same
    box, same 4 080 items): 4.2 k items/s when the loader forks right after clip.load, 1.2-1.6 k with one more piece of state in
    front of the fork, 0.5 k after an encoder engine has run -- the consumer then blocks ~300 ms per loader batch inside its
    launches although the device work of the call takes 0.9 ms.  Workers forked from a clean fork server (torch and this package
    pre-imported, no HIP state -- the library makes no HIP call at load time) do not touch the GPU process's address space."""
    import multiprocessing as mp
    method = os.environ.get("KEMR_LOADER_CONTEXT", "forkserver")
    ctx = mp.get_context(method)
    if method == "forkserver":
        ctx.set_forkserver_preload(_FORKSERVER_PRELOAD)          # takes effect when the server starts (first use in this process)
    return ctx


def _local_world_size() -> int:
    for key in ("LOCAL_WORLD_SIZE", "WORLD_SIZE"):
        v = os.environ.get(key, "")
        if v.strip().isdigit() and int(v) > 0:
            return int(v)
    return 1


def usable_loader_workers(dataset, collate, num_workers: int) -> int:
    """Worker processes the loader can actually be given.  They come from a fork server (loader_context), which PICKLES the
    dataset and the collate object; the reference's loaders fork (evaluator_baseline.py:83-92) and therefore accept lambdas,
    closures and in-memory objects.  A caller who passes such a dataset / tokenize_fn gets num_workers = 0 and a warning
    instead of a crash inside DataLoader; under torchrun the count is divided by the local world size."""
    if num_workers <= 0:
        return 0
    num_workers = max(1, num_workers // _local_world_size())
    if os.environ.get("KEMR_LOADER_CONTEXT", "forkserver") == "fork":
        return num_workers
    import pickle

    class _Discard:                                            # a big in-memory split is serialised once here (as it will be once per
        def write(self, b):                                    # worker by the loader), but never held: the bytes are dropped
            return len(b)

    try:
        pickle.Pickler(_Discard(), protocol=pickle.HIGHEST_PROTOCOL).dump((collate, dataset))
    except Exception as e:                                     # noqa: BLE001 - anything that cannot cross to a fresh process
        logger.warning(f"loader workers need a picklable dataset / tokenize_fn ({type(e).__name__}: {e}); using num_workers=0")
        return 0
    return num_workers


def eval_loader(dataset, batch_size: int, seed: int, num_workers: int, tokenize_fn: Callable, pin: bool) -> DataLoader:
    """The evaluation DataLoader (evaluator.py:96-105: no shuffle, seeded workers), with tokenisation and the packing of raw
    images into one buffer moved INTO the loader (its worker processes when there are any); the pin thread pins both.
    What is left on the consumer's thread per loader batch: three asynchronous copies and the kernel launches."""
    g = torch.Generator()
    g.manual_seed(seed)
    num_workers = usable_loader_workers(dataset, CollateAndTokenize(tokenize_fn), num_workers)
    return DataLoader(dataset, batch_size=batch_size, shuffle=False, num_workers=num_workers, pin_memory=pin,
                      collate_fn=CollateAndTokenize(tokenize_fn), worker_init_fn=seed_worker if num_workers else None,
                      generator=g, prefetch_factor=4 if num_workers else None,
                      multiprocessing_context=loader_context() if num_workers else None)


def model_name_arg(value: str) -> str:
    """`--model_name`: a served model name (clip.available_models()) or a Hugging Face save_pretrained directory on the local disk."""
    from . import clip_api, hf_checkpoint
    if value in clip_api.available_models() or hf_checkpoint.is_hf_directory(value):
        return value
    raise argparse.ArgumentTypeError(f"{value!r} is neither one of {clip_api.available_models()} nor a directory with a config.json")


def image_transform_name(dataset) -> str:
    """What the results JSON records under ``image_transform``: where the dataset's image transform runs."""
    return {"RawRGB": "gpu (batched kernels, bit-identical to the host transform)", "ClipPreprocess": "host (PIL, per sample)",
            "SiglipPreprocess": "host (PIL, per sample)"}.get(type(getattr(dataset, "preprocessor", None)).__name__,
                                                              "none (pre-normalised tensors)")


@torch.no_grad()
def encode_dataset(model, dataset, batch_size: int = 64, seed: int = 42, num_workers: Optional[int] = 0,
                   tokenize_fn: Optional[Callable] = None, shard: Optional[Tuple[int, int]] = None
                   ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, List[str]]:
    """Hot loop A: (image, query, target) -> three L2-normalised embedding sets that stay on the GPU.
    num_workers None = default_loader_workers().
    ``shard=(rank, world)``: only the items ``dist.shard_bounds(len(dataset), world, rank)`` are read and encoded (a ``Subset``); the
    embeddings and uuids returned are that contiguous part's.  A rank whose part is empty encodes nothing and returns [0, D] tensors
    whose width comes from the model.  None: the whole dataset, as before."""
    if num_workers is None:
        num_workers = default_loader_workers()
    model.eval()
    device = next(model.parameters()).device
    if shard is not None:
        lo, hi = KD.shard_bounds(len(dataset), int(shard[1]), int(shard[0]))
        if hi == lo:
            empty = torch.zeros((0, model_embed_dim(model)), dtype=torch.float32, device=device)
            return empty, empty.clone(), empty.clone(), []
        dataset = torch.utils.data.Subset(dataset, range(lo, hi))
    tokenize_fn = tokenize_fn or model_tokenize(model)
    loader = eval_loader(dataset, batch_size, seed, num_workers, tokenize_fn, pin=device.type == "cuda")
    img, qry, tgt, uuids = [], [], [], []
    logger.info(f"Computing embeddings for {len(dataset)} samples...")
    # The loader's batch size is the host pipeline's business (the reference scripts pass 64); the encoders are fed the number
    # of items per call that fills the persistent GEMM's rounds (engine.tile_friendly_batch), whatever it is: 255 images of
    # ViT-L/14 are 65 535 token rows = 256 row tiles, while e.g. 64 images are 65 row tiles -> 260 tiles on 256 CUs, a second
    # round for 4 tiles; texts go 850 to a call (queries and targets of 425 items together: 256 row tiles, whole rounds in every
    # GEMM; 255 texts leave 10 % of the out-proj round empty).  Rows are independent, so the embeddings do
    # not depend on the grouping.
    arch = getattr(model, "arch", None)
    # (towers of more than 288 tokens -- ViT-L/14@336px -- take the engine's own call size, about ENCODE_ITEMS * 257 token rows)
    n_img = ENCODE_ITEMS if arch is None else (
        engine.tile_friendly_batch(arch.v_tokens, arch.v_width, ENCODE_ITEMS // 2, ENCODE_ITEMS) if arch.v_tokens <= 288
        else engine.image_call_items(arch))
    n_txt = ENCODE_ITEMS if arch is None else max(1, engine.tile_friendly_batch(arch.ctx, arch.t_width, ENCODE_ITEMS, engine.MAX_TEXT_BATCH) // 2)
    pend_i, pend_q, pend_t, pend_ql, pend_tl = [], [], [], [], []
    count = {"i": 0, "t": 0, "rows": 0}
    # (Round 4 measured the text calls on a SIDE stream beside the image calls -- tools/bench_two_streams.py, profiles/r04_two_streams.txt:
    # +3.2 % items/s when every image call has a text call beside it, +0.7 % in the bench's mix of one text call per three image calls,
    # consecutive image calls on two streams +1.4 % -- and left it out: the persistent GEMM takes every CU's LDS, so only the HBM-bound
    # kernels of the other tower fit beside it, and a gain of that size does not pay for two-stream bookkeeping in every caller.)
    # Packed text calls (engine.ClipEngine.encode_text: a text is computed up to its end-of-text token only): the tokenizer-side
    # lengths travel with the ids, and a call takes as many (query, target) pairs as fill engine.TEXT_ROW_BUDGET token rows.
    # (every context the library takes, Long-CLIP's 248 included; an fp32x3 engine above 128 positions ignores the lengths and runs dense)
    by_rows = bool(getattr(model, "accepts_text_lengths", False)) and arch is not None and \
        os.environ.get("KEMR_TEXT_PACKED", "1") != "0"

    def flush_images(final: bool):
        take = count["i"] if final else (count["i"] // n_img) * n_img              # whole encoder calls; the rest waits
        if take <= 0:
            return
        ci = torch.cat(pend_i)
        img.append(model.encode_image(ci[:take], normalize=True))
        pend_i[:] = [ci[take:]]
        count["i"] -= take

    def flush_texts(final: bool):
        if by_rows:
            if count["t"] <= 0:
                return
            cq, ct, lq, lt = torch.cat(pend_q), torch.cat(pend_t), torch.cat(pend_ql), torch.cat(pend_tl)
            pair_rows = torch.cumsum((lq + lt).to(torch.int64), 0)
            s0, base = 0, 0
            while s0 < count["t"]:
                s1 = s0 + max(1, int((pair_rows[s0:] - base <= engine.TEXT_ROW_BUDGET).sum()))
                if s1 >= count["t"] and not final:
                    break                                                          # not a whole call yet: wait for more
                both = model.encode_text(torch.cat([cq[s0:s1], ct[s0:s1]]), normalize=True, lens=torch.cat([lq[s0:s1], lt[s0:s1]]))
                qry.append(both[: s1 - s0])
                tgt.append(both[s1 - s0:])
                base, s0 = int(pair_rows[s1 - 1]), s1
            pend_q[:], pend_t[:], pend_ql[:], pend_tl[:] = [cq[s0:]], [ct[s0:]], [lq[s0:]], [lt[s0:]]
            count["t"] -= s0
            count["rows"] = int(pair_rows[-1]) - base if s0 < pair_rows.numel() else 0
            return
        take = count["t"] if final else (count["t"] // n_txt) * n_txt
        if take <= 0:
            return
        cq, ct = torch.cat(pend_q), torch.cat(pend_t)
        for s0 in range(0, take, n_txt):                                           # queries and targets of n_txt items in ONE call
            s1 = min(take, s0 + n_txt)
            both = model.encode_text(torch.cat([cq[s0:s1], ct[s0:s1]]), normalize=True)
            qry.append(both[: s1 - s0])
            tgt.append(both[s1 - s0:])
        pend_q[:], pend_t[:] = [cq[take:]], [ct[take:]]
        count["t"] -= take

    gpu_pre = None
    for images, q_ids, t_ids, ids in loader:
        if isinstance(images, PackedRaw):      # raw uint8 images (preprocess.RawRGB): the model family's transform on the device,
            if gpu_pre is None:                # one launch pair per loader batch
                gpu_pre = gpu_preprocess_for(model, device)
            images = gpu_pre.batch(images)
        pend_i.append(images.to(device, non_blocking=True))
        if by_rows:                            # lengths from the host copy, before the upload
            lq_, lt_ = engine.text_lengths(q_ids.cpu()), engine.text_lengths(t_ids.cpu())
            pend_ql.append(lq_)
            pend_tl.append(lt_)
            count["rows"] += int(lq_.sum()) + int(lt_.sum())
        pend_q.append(q_ids.to(device, non_blocking=True))
        pend_t.append(t_ids.to(device, non_blocking=True))
        count["i"] += int(images.shape[0])
        count["t"] += int(images.shape[0])
        uuids.extend(ids)
        if count["i"] >= n_img:
            flush_images(False)
        if (count["rows"] > engine.TEXT_ROW_BUDGET) if by_rows else (count["t"] >= n_txt):
            flush_texts(False)
    flush_images(True)
    flush_texts(True)
    return torch.cat(img), torch.cat(qry), torch.cat(tgt), uuids


def model_embed_dim(model) -> int:
    """The width of a model's embeddings from the model itself (what a rank with an empty shard has instead of a tensor)."""
    arch = getattr(model, "arch", None)
    if arch is not None and hasattr(arch, "embed_dim"):
        return int(arch.embed_dim)
    if hasattr(model, "get_sentence_embedding_dimension"):
        return int(model.get_sentence_embedding_dimension())
    if hasattr(model, "embed_dim"):
        return int(model.embed_dim)
    raise RuntimeError(f"{type(model).__name__} states no embedding width (arch.embed_dim / get_sentence_embedding_dimension / embed_dim)")


class _ShardedEmbeddings:
    """One evaluation's embeddings sharded over the ranks of the process group (``dist.active_shard``): this rank's contiguous part,
    padded to equal query rows (``dist.EvenRows``), and the ``ShardedGallery`` of each candidate set, built on first use.  Every
    ``ranks`` / ``metrics`` call is collective and returns the same values on every rank; pad rows never reach a metric."""

    def __init__(self, n: int, image: Optional[torch.Tensor], query: torch.Tensor, target: torch.Tensor, ops=None):
        self.ops = ops if ops is not None else KD.eval_ops
        self.even = KD.EvenRows(n)
        self.device = query.device
        self.local = {"image": image, "query": query, "target": target}
        self.padded = {name: None if x is None else self.even.pad(x.float()) for name, x in self.local.items()}
        self._galleries: Dict[Tuple[str, ...], KD.ShardedGallery] = {}

    def gallery(self, *names: str, precision: str = "fp32x3") -> "KD.ShardedGallery":
        key = names + (precision,)
        if key not in self._galleries:
            self._galleries[key] = KD.ShardedGallery([self.local[n].float() for n in names], self.even.n, precision=precision, ops=self.ops)
        return self._galleries[key]

    def ranks(self, query_names: Sequence[str], gallery_names: Sequence[str], weights=None, row_gate=None, bonus=None,
              precision: str = "fp32x3") -> torch.Tensor:
        if bonus is not None:
            bonus = None if len(bonus[1]) == 0 else self.even.pad_bonus(bonus)
        r = self.gallery(*gallery_names, precision=precision).ranks(
            [self.padded[n] for n in query_names], self.even.local_gt(self.device), weights=weights, k=0, row_gate=row_gate, bonus=bonus)[0]
        return self.even.real(r)

    def metrics(self, query_names, gallery_names, prefix: str = "", k_values=M.DEFAULT_K, compute_recall: bool = True,
                compute_mrr: bool = True, **kw) -> Dict[str, float]:
        return M._metrics_of_ranks(self.ranks(query_names, gallery_names, **kw), prefix, k_values, compute_recall, compute_mrr)


def _encode_sharded(model, dataset, batch_size, seed, num_workers, tokenize_fn, shard) -> Tuple[_ShardedEmbeddings, List[str]]:
    image, query, target, uuids = encode_dataset(model, dataset, batch_size, seed, num_workers, tokenize_fn, shard=shard)
    logger.info(f"rank {shard[0]} of {shard[1]}: {len(uuids)} of {len(dataset)} items encoded")
    return _ShardedEmbeddings(len(dataset), image, query, target), uuids


def _sparql_sweep_sharded(emb: _ShardedEmbeddings, uuids, text2sparql_results, t2i_weight, t2t_weight) -> Dict[str, Dict[str, float]]:
    """``sparql_sweep`` over sharded embeddings: ``uuids`` are those of ALL items (gathered once by the caller), so the bonus CSR covers
    every gathered query with GLOBAL columns and is the same on every rank; each shard adds the entries of its own id range."""
    fused = (["query", "query"], ["image", "target"])
    out = {"T2I": emb.metrics(["query"], ["image"]), "T2T": emb.metrics(["query"], ["target"]),
           "Fused": emb.metrics(*fused, weights=[t2i_weight, t2t_weight])}
    for alpha in ALPHAS:
        scale, bonus = SF.sparql_bonus(text2sparql_results, uuids, uuids, "weighted", {"alpha": alpha, "sparql_weight": 1 - alpha})
        out[f"weighted_alpha={alpha}"] = emb.metrics(*fused, weights=[scale * t2i_weight, scale * t2t_weight], bonus=bonus)
    return out


def sparql_sweep(query, target, image, uuids, text2sparql_results, t2i_weight, t2t_weight) -> Dict[str, Dict[str, float]]:
    """T2I / T2T / fused metrics + the 9-alpha weighted SPARQL fusion of evaluator.py:164-218, every variant one fused
    kernel pass (no N x N matrix, no dense 0/1 hit matrix)."""
    out = {"T2I": M.compute_retrieval_metrics(query, image), "T2T": M.compute_retrieval_metrics(query, target),
           "Fused": M.compute_retrieval_metrics_final(query, target, image, t2i_weight=t2i_weight, t2t_weight=t2t_weight)}
    for alpha in ALPHAS:
        out[f"weighted_alpha={alpha}"] = SF.fused_metrics(
            [query, query], [image, target], [t2i_weight, t2t_weight], text2sparql_results, uuids, uuids, "weighted",
            {"alpha": alpha, "sparql_weight": 1 - alpha})
    return out


@torch.no_grad()
def evaluate_clip_model(model, dataset, batch_size: int = 64, device: str = "cuda", seed: int = 42,
                        tasks: List[str] = ("T2I", "I2T", "T2T"), compute_recall: bool = True, compute_mrr: bool = True,
                        tokenize_fn: Optional[Callable] = None, num_workers: Optional[int] = 0,
                        text2sparql_results: Optional[Dict[str, List[str]]] = None, analysis: bool = True
                        ) -> Dict[str, float]:
    """evaluator.py semantics: per-task metrics are returned; the fused / SPARQL-sweep analysis is logged and kept in
    ``evaluate_clip_model.last_analysis``.  ``num_workers`` defaults to the reference's 0 (evaluator.py:101); the CLIs opt into
    ``default_loader_workers()``, a library caller passes a number (None = that default).
    With a process group of more than one rank (``dist.active_shard``) every rank encodes its contiguous part of the dataset, ranks
    against its own shard and receives the same dict (``dist.ShardedGallery``)."""
    shard = KD.active_shard()
    if shard is not None:
        emb, uuids = _encode_sharded(model, dataset, batch_size, seed, num_workers, tokenize_fn, shard)
        pairs = {"T2I": ("query", "image"), "I2T": ("image", "target"), "T2T": ("query", "target")}
        result = {}
        for task in ("T2I", "I2T", "T2T"):
            if task in tasks:
                result.update(emb.metrics([pairs[task][0]], [pairs[task][1]], task, compute_recall=compute_recall, compute_mrr=compute_mrr))
        evaluate_clip_model.last_analysis = {}
        if analysis and compute_recall:
            results = load_text2sparql_results() if text2sparql_results is None else text2sparql_results
            all_uuids = KD.all_gather_list(uuids)                 # the one object exchange of an evaluation
            for wi, wt in ((0.5, 0.5), (0.1, 0.9)):
                sweep = _sparql_sweep_sharded(emb, all_uuids, results, wi, wt)
                evaluate_clip_model.last_analysis[f"{wi}_{wt}"] = sweep
                for name, m in sweep.items():
                    logger.info(f"[t2i={wi} t2t={wt}] {name}: " + ", ".join(f"{k}={v:.2f}" for k, v in m.items()))
        return result
    image, query, target, uuids = encode_dataset(model, dataset, batch_size, seed, num_workers, tokenize_fn)
    logger.info(f"Image embeddings: {tuple(image.shape)}")
    logger.info(f"Query embeddings: {tuple(query.shape)}")
    logger.info(f"Target embeddings: {tuple(target.shape)}")
    result = M.compute_all_retrieval_metrics(query, target, image, tasks=tasks, compute_recall=compute_recall,
                                             compute_mrr=compute_mrr)
    evaluate_clip_model.last_analysis = {}
    if analysis and compute_recall:
        results = load_text2sparql_results() if text2sparql_results is None else text2sparql_results
        for wi, wt in ((0.5, 0.5), (0.1, 0.9)):
            sweep = sparql_sweep(query, target, image, uuids, results, wi, wt)
            evaluate_clip_model.last_analysis[f"{wi}_{wt}"] = sweep
            for name, m in sweep.items():
                logger.info(f"[t2i={wi} t2t={wt}] {name}: " + ", ".join(f"{k}={v:.2f}" for k, v in m.items()))
    return result


evaluate_clip_model.last_analysis = {}


@torch.no_grad()
def evaluate_clip_model_for_training(model, dataset, batch_size: int = 64, device: str = "cuda", seed: int = 42,
                                     tasks: List[str] = ("T2I", "I2T", "T2T"), **kw) -> Dict[str, float]:
    return evaluate_clip_model(model, dataset, batch_size, device, seed, tasks, compute_recall=False, compute_mrr=True, **kw)


@torch.no_grad()
def evaluate_clip_model_baseline(model, dataset, batch_size: int = 64, device: str = "cuda", seed: int = 42,
                                 tasks: List[str] = ("T2I", "I2T", "T2T"), compute_recall: bool = True,
                                 compute_mrr: bool = True, t2i_weight: float = 0.5, t2t_weight: float = 0.5,
                                 tokenize_fn: Optional[Callable] = None, num_workers: Optional[int] = 4) -> Dict[str, float]:
    """evaluator_baseline.py semantics: metrics of the fused score w_i * T2I + w_t * T2T (un-prefixed keys); 4 loader workers
    as there (evaluator_baseline.py:87).  Sharded over the ranks of a process group like ``evaluate_clip_model``."""
    shard = KD.active_shard()
    if shard is not None:
        emb, _ = _encode_sharded(model, dataset, batch_size, seed, num_workers, tokenize_fn, shard)
        return emb.metrics(["query", "query"], ["image", "target"], compute_recall=compute_recall, compute_mrr=compute_mrr,
                           weights=[t2i_weight, t2t_weight])
    image, query, target, _ = encode_dataset(model, dataset, batch_size, seed, num_workers, tokenize_fn)
    return M.compute_retrieval_metrics_final(query, target, image, compute_recall=compute_recall, compute_mrr=compute_mrr,
                                             t2i_weight=t2i_weight, t2t_weight=t2t_weight)


# ------------------------------------------------------------------------------------------------ CLIs
def _common_args(parser, baseline: bool):
    parser.add_argument("--model_name", type=model_name_arg, default="ViT-L/14",
                        help="a served model name (clip.available_models(): the CLIP and ViT-*-SigLIP* names), or a Hugging Face "
                             "save_pretrained directory (CLIP or SigLIP)")
    parser.add_argument("--tokenizer_dir", type=str, default=None, metavar="DIR",
                        help="SigLIP models only: the directory whose tokenizer.json tokenises the texts (default: the --model_name "
                             "directory; a bare ViT-*-SigLIP* name has none and needs this flag)")
    parser.add_argument("--checkpoint", type=str, help="Path to checkpoint, if None uses pretrained model")
    parser.add_argument("--images_dir", type=str, default=None)
    parser.add_argument("--texts_dir", type=str, default=None, help="Directory containing query-target JSON files")
    parser.add_argument("--split", type=str, default="test", choices=["train", "val", "test"])
    parser.add_argument("--splits_file", type=str, default=None, help="accepted for the shipped scripts; unused")
    parser.add_argument("--tasks", type=str, nargs="+", default=["T2I", "I2T", "T2T"], choices=["T2I", "I2T", "T2T"])
    parser.add_argument("--mrr_only", action="store_true", help="Only compute MRR (faster, for training validation)")
    parser.add_argument("--batch_size", type=int, default=32)
    parser.add_argument("--device", type=str, default="cuda")
    parser.add_argument("--output_file", type=str, required=True)
    parser.add_argument("--seed", type=int, default=42)
    parser.add_argument("--synthetic", type=int, default=0, metavar="N",
                        help="evaluate on N seeded synthetic items instead of the HuggingFace dataset (offline)")
    parser.add_argument("--synthetic_images", type=str, default="float", choices=["float", "uint8"],
                        help="synthetic items: 'float' = already normalised pixel tensors; 'uint8' = camera-sized PIL images through "
                             "CLIPEvalDatasetHF(split, preprocess), the reference's own dataset call (image transform on the GPU "
                             "unless KEMR_GPU_PREPROCESS=0)")
    parser.add_argument("--num_workers", type=int, default=-1, help="DataLoader workers (-1: KEMR_LOADER_WORKERS or min(12, cores / 2))")
    parser.add_argument("--dataset", type=str, default="xuemduan/reevaluate-image-text-pairs")
    if baseline:
        parser.add_argument("--t2i_weight", type=float, default=0.5)
        parser.add_argument("--t2t_weight", type=float, default=0.5)


def _bind_tokenizer(model, args) -> None:
    """--tokenizer_dir onto the model, then the model's tokenize callable built once: a SigLIP model without a tokenizer.json fails
    here, before the dataset is opened; the flag on a CLIP model is an error, not a silent no-op."""
    if getattr(args, "tokenizer_dir", None):
        if model.arch.family != "siglip":
            raise ValueError(f"--tokenizer_dir is for SigLIP models; {args.model_name!r} is a CLIP model (its BPE vocabulary is built in)")
        model.tokenizer_dir = args.tokenizer_dir
    model_tokenize(model)


def _open_outputs(output_file: str, log_name: str) -> logging.Logger:
    """The output directory and ``evaluation.log`` beside the results file: created by the writer rank only (``dist.is_writer``:
    rank 0 of a process group, or the only process); the other ranks log to stderr."""
    out_dir = Path(output_file).parent
    if KD.is_writer():
        out_dir.mkdir(parents=True, exist_ok=True)
        setup_logger(log_name, str(out_dir / "evaluation.log"))
    else:
        setup_logger(log_name)
    return logging.getLogger(log_name)


def _sharding_record(n: int) -> Dict[str, object]:
    """``world_size`` / ``items_per_rank`` of the results JSON (a sharded run only)."""
    shard = KD.active_shard()
    if shard is None:
        return {}
    return {"world_size": shard[1], "items_per_rank": [hi - lo for lo, hi in (KD.shard_bounds(n, shard[1], r) for r in range(shard[1]))]}


def _save_results(results: dict, output_file: str) -> None:
    """The results JSON, written by the writer rank only (every rank holds the same dict)."""
    if KD.is_writer():
        save_metrics_to_json(results, output_file)


def _in_process_group(fn: Callable) -> Callable:
    """A CLI body between ``dist.init_from_env()`` (first: RCCL is initialised before anything else touches the GPU) and
    ``dist.finish()`` (last).  Under torchrun ``--device cuda`` means this rank's own device.  A rank that fails does not wait in
    ``finish()``'s barrier for ranks that wait for it in a collective: the exception leaves the process and the launcher ends the rest."""
    import functools

    @functools.wraps(fn)
    def wrapped(argv=None):
        KD.init_from_env()
        out = fn(argv)
        KD.finish()
        return out
    return wrapped


def _device_of(args) -> str:
    """``--device``: under a process group a bare ``cuda`` is this rank's current device (set by ``dist.init_from_env``)."""
    device = args.device if args.device.startswith("cuda") else "cuda"
    if device == "cuda" and KD.active_shard() is not None and torch.cuda.is_available():
        device = f"cuda:{torch.cuda.current_device()}"
    return device


def _run(args, baseline: bool, log_name: str):
    torch.manual_seed(args.seed)
    np.random.seed(args.seed)
    random.seed(args.seed)
    log = _open_outputs(args.output_file, log_name)
    log.info("=" * 80)
    log.info("CLIP Model Evaluation (MI355X HIP engine)")
    log.info(f"Model: {args.model_name}  Checkpoint: {args.checkpoint}  Split: {args.split}  Tasks: {args.tasks}  "
             f"MRR only: {args.mrr_only}  Seed: {args.seed}")
    if not torch.cuda.is_available():
        raise RuntimeError("no GPU visible: the encoders and the ranking run only in the HIP kernels (no CPU fallback)")
    device = _device_of(args)
    from . import clip_api, tokenizer
    from .clip_model import load_clip_model
    if args.synthetic > 0:           # synthetic data: seeded random weights / hash token ids are acceptable, and recorded below
        clip_api.allow_random_weights(True)
        tokenizer.allow_hash_tokenizer(True)
    model, preprocess = load_clip_model(model_name=args.model_name, checkpoint_path=args.checkpoint, device=device)
    _bind_tokenizer(model, args)
    if args.synthetic > 0 and args.synthetic_images == "float":
        dataset = SyntheticRetrievalDataset(args.synthetic, model.arch.image_size, args.seed)
    elif args.synthetic > 0:
        dataset = CLIPEvalDatasetHF(hf_dataset=SyntheticHFSplit(args.synthetic, args.seed), preprocessor=preprocess)
    else:
        from datasets import load_dataset
        ds = load_dataset(args.dataset)
        split = {"val": "validation"}.get(args.split, args.split)
        dataset = CLIPEvalDatasetHF(hf_dataset=ds[split], preprocessor=preprocess)        # the reference's call (evaluator.py:330-333)
    workers = default_loader_workers() if args.num_workers < 0 else args.num_workers
    log.info(f"Image transform: {'GPU (batched, bit-identical)' if getattr(preprocess, 'defer_to_gpu', False) else 'host (PIL, per sample)'}; loader workers: {workers}")
    if baseline:
        metrics = evaluate_clip_model_baseline(model, dataset, args.batch_size, device, args.seed, args.tasks,
                                               compute_recall=not args.mrr_only, compute_mrr=True,
                                               t2i_weight=args.t2i_weight, t2t_weight=args.t2t_weight, num_workers=workers)
    else:
        metrics = evaluate_clip_model(model, dataset, args.batch_size, device, args.seed, args.tasks,
                                      compute_recall=not args.mrr_only, compute_mrr=True, num_workers=workers)
    log.info("EVALUATION RESULTS")
    for name, value in sorted(metrics.items()):
        log.info(f"{name}: {value:.2f}" + ("" if "Mean_Rank" in name else "%"))
    results = {"model_name": args.model_name, "checkpoint": args.checkpoint, "split": args.split,
               "num_samples": len(dataset), "seed": args.seed, "metrics": metrics,
               # provenance (not in the reference's file): what the numbers were computed with
               "weights_source": getattr(model, "weights_source", "unknown"), "tokenizer": model_tokenizer_name(model),
               "precision": _lib.env_precision(), "data": "synthetic" if args.synthetic > 0 else args.dataset,
               "image_transform": image_transform_name(dataset),
               "loader_workers": workers, **_sharding_record(len(dataset))}
    if not baseline:
        results["tasks"] = list(args.tasks)
    _save_results(results, args.output_file)
    log.info(f"Results saved to {args.output_file}")
    return results


@_in_process_group
def main_evaluator(argv=None):
    parser = argparse.ArgumentParser(description="Evaluate CLIP model")
    _common_args(parser, baseline=False)
    return _run(parser.parse_args(argv), baseline=False, log_name="src.clip.eval.evaluator")


@_in_process_group
def main_baseline(argv=None):
    parser = argparse.ArgumentParser(description="Evaluate CLIP model (fused T2I + T2T score)")
    _common_args(parser, baseline=True)
    return _run(parser.parse_args(argv), baseline=True, log_name="src.clip.eval.evaluator_baseline")


# ------------------------------------------------------------------------------------------------ learned fusion heads
RERANK_DEPTH_MIN = 20       # every reported Recall@K has K <= 20: with at least 20 listed candidates each is exact for the two-stage route


_SPARQL_NEEDS_RERANK = ("the SPARQL bonus of the learned heads is applied to the reranked shortlist (FusionModel.rerank(bonus=...), "
                        "kemr_list_fuse): the dense route scores every pair with the head and has no bonus stage -- give a "
                        "rerank depth as well (rerank_depth / --rerank_depth N)")


def _check_rerank_depth(fusion_type: str, rerank_depth: int) -> None:
    if not RERANK_DEPTH_MIN <= rerank_depth <= _lib.MAX_DEEP_K:
        raise ValueError(f"rerank_depth={rerank_depth} not in {RERANK_DEPTH_MIN}..{_lib.MAX_DEEP_K}")
    if fusion_type not in ("linear", "cross_attention"):
        raise ValueError(f"rerank_depth is for the linear and cross_attention heads; the {fusion_type!r} head ranks the whole "
                         "gallery in one fused pass already (FusionModel.rank)")


@torch.no_grad()
def evaluate_fusion_model(fusion_model, dataset, batch_size: int = 64, device: str = "cuda", seed: int = 42,
                          tokenize_fn: Optional[Callable] = None, num_workers: Optional[int] = 4,
                          rerank_depth: Optional[int] = None, text2sparql_results: Optional[Dict[str, List[str]]] = None,
                          fusion_strategy: str = "weighted", fusion_params: Optional[dict] = None) -> Dict[str, float]:
    """Counterpart of /root/reference/src/clip/eval/evaluator_fusion.py:28-144 (4 loader workers as at :42).  The reference fills an N x N numpy
    matrix in 50 x 500 blocks with an H2D/D2H round trip and ``empty_cache()`` per block (:76-121); here the head's
    score is one fused kernel pass over resident embeddings (``FusionModel.rank``).

    ``rerank_depth`` (None = the above, unchanged; else 20..1024, linear / cross_attention heads only): retrieve-then-rerank
    (``FusionModel.rerank``) -- every query's ``rerank_depth`` best candidates by 0.5 * T2I + 0.5 * T2T are scored with the head and
    the metrics come from the ground truth's position in that reranked list, ``rerank_depth + 1`` where it was not shortlisted.
    Recall@K (K <= 20 <= rerank_depth) is exact for the two-stage pipeline.  Two keys are added: ``Shortlist_Recall`` (percent of
    queries whose ground truth reached the list) and ``Rerank_Depth``.  Unless ``Shortlist_Recall`` is 100, ``MRR`` is an UPPER and
    ``Mean_Rank`` a LOWER bound of the pipeline's value: a query whose ground truth missed the list counts with rank
    ``rerank_depth + 1``, the best it could have.

    ``text2sparql_results`` (query uuid -> listed URIs, with ``rerank_depth``): the knowledge-fused rerank.  The bonus comes from
    ``sparql_fusion.sparql_bonus(text2sparql_results, uuids, uuids, fusion_strategy, fusion_params)``; its ``clip_scale`` becomes
    the ``head_weight`` of ``FusionModel.rerank(bonus=...)``: hits join the shortlist wherever CLIP ranks them and the list is
    ranked by ``head_weight * head + bonus``.  ``Head_Weight`` and ``SPARQL_Strategy`` are added to the result."""
    if text2sparql_results is not None and rerank_depth is None:
        raise ValueError(_SPARQL_NEEDS_RERANK)
    if rerank_depth is not None:
        _check_rerank_depth(fusion_model.fusion_type, int(rerank_depth))
    fusion_model.eval()
    from . import ranking
    shard = KD.active_shard()
    if shard is not None:
        result = _evaluate_fusion_sharded(fusion_model, dataset, batch_size, seed, tokenize_fn, num_workers, rerank_depth,
                                          text2sparql_results, fusion_strategy, fusion_params, shard)
        return _log_fusion_result(result)
    image, query, target, uuids = encode_dataset(fusion_model.clip_model, dataset, batch_size, seed, num_workers, tokenize_fn)
    if rerank_depth is None:
        ranks, _, _ = fusion_model.rank(query, image, target, k=0)
        result = ranking.metrics_from_ranks(ranks, [1, 5, 10, 20])
    else:
        depth = int(rerank_depth)
        fused = {}
        if text2sparql_results is not None:
            from . import sparql_fusion
            head_weight, bonus = sparql_fusion.sparql_bonus(text2sparql_results, uuids, uuids, fusion_strategy, fusion_params)
            fused = {"bonus": bonus, "head_weight": head_weight}
        ranks = fusion_model.rerank(query, fusion_model.prepare_gallery(image, target), depth=depth, k=1, gt_idx="diag", **fused)[0]
        result = ranking.metrics_from_ranks(ranks, [1, 5, 10, 20])
        result["Shortlist_Recall"] = float((ranks <= depth).double().mean().item() * 100.0)
        result["Rerank_Depth"] = depth
        if fused:
            result["Head_Weight"] = float(fused["head_weight"])
            result["SPARQL_Strategy"] = fusion_strategy
    return _log_fusion_result(result)


def _log_fusion_result(result):
    logger.info("Fusion Model Evaluation Results")
    for k, v in result.items():
        logger.info(f"{k}: {v}" if isinstance(v, str) else f"{k}: {v:.2f}" + ("%" if ("R@" in k or "MRR" in k or "Recall" in k) else ""))
    return result


def _evaluate_fusion_sharded(fusion_model, dataset, batch_size, seed, tokenize_fn, num_workers, rerank_depth, text2sparql_results,
                             fusion_strategy, fusion_params, shard) -> Dict[str, float]:
    """``evaluate_fusion_model`` over a process group, one route per head family:
    gated family and bilinear: the head folds into the fused contraction (``FusionModel._parts`` of the padded local queries; a gate is a
        function of its own query row) -> ``ShardedGallery.ranks(row_gate=...)``;
    ``rerank_depth``: ``ShardedGallery.rerank`` against this rank's ``HeadGallery``, with or without the SPARQL bonus;
    dense linear / cross_attention: all-gather the query embeddings (4 * D bytes per item), the head on (all queries) x (local
        candidates), then ``dist.sharded_ranks_dense``."""
    from . import ranking
    emb, uuids = _encode_sharded(fusion_model.clip_model, dataset, batch_size, seed, num_workers, tokenize_fn, shard)
    even, image, target, q_pad = emb.even, emb.local["image"], emb.local["target"], emb.padded["query"]
    if rerank_depth is not None:
        depth = int(rerank_depth)
        fused = {}
        if text2sparql_results is not None:
            all_uuids = KD.all_gather_list(uuids)
            head_weight, bonus = SF.sparql_bonus(text2sparql_results, all_uuids, all_uuids, fusion_strategy, fusion_params)
            fused = {"bonus": even.pad_bonus(bonus), "head_weight": head_weight}
        head_gallery = fusion_model.prepare_gallery(image, target) if even.hi > even.lo else None
        ranks = emb.gallery("image", "target").rerank(fusion_model, head_gallery, q_pad, depth=depth, k=1,
                                                      local_gt=even.local_gt(emb.device), **fused)[0]
        ranks = even.real(ranks)
        result = ranking.metrics_from_ranks(ranks, [1, 5, 10, 20])
        result["Shortlist_Recall"] = float((ranks <= depth).double().mean().item() * 100.0)
        result["Rerank_Depth"] = depth
        if fused:
            result["Head_Weight"] = float(fused["head_weight"])
            result["SPARQL_Strategy"] = fusion_strategy
        return result
    if fusion_model.fusion_type in ("linear", "cross_attention"):
        all_q = KD.all_gather_rows(q_pad)
        if even.hi > even.lo:
            scores = fusion_model.forward(all_q, image, target)
        else:
            scores = torch.zeros((all_q.shape[0], 0), dtype=torch.float32, device=emb.device)
        ranks = KD.sharded_ranks_dense(scores, even.lo, even.all_gt(emb.device), k=0, ops=emb.ops)[0]
        return ranking.metrics_from_ranks(even.real(ranks), [1, 5, 10, 20])
    qs, _, weights, gates = fusion_model._parts(q_pad, image, target)     # the query side: (transformed) rows, weights, per-row gates
    ranks = emb.gallery("image", "target").ranks(qs, even.local_gt(emb.device), weights=weights, k=0, row_gate=gates)[0]
    return ranking.metrics_from_ranks(even.real(ranks), [1, 5, 10, 20])


def _rerank_depth_arg(text: str) -> int:
    try:
        value = int(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f"{text!r} is not an integer")
    if not RERANK_DEPTH_MIN <= value <= _lib.MAX_DEEP_K:
        raise argparse.ArgumentTypeError(f"{value} not in {RERANK_DEPTH_MIN}..{_lib.MAX_DEEP_K}")
    return value


def fusion_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(description="Evaluate Fusion Model")
    parser.add_argument("--model_name", type=str, default="ViT-L/14")
    parser.add_argument("--tokenizer_dir", type=str, default=None, metavar="DIR", help="SigLIP models only: directory of the tokenizer.json")
    parser.add_argument("--clip_checkpoint", type=str, default=None)
    parser.add_argument("--fusion_checkpoint", type=str, default=None)
    parser.add_argument("--fusion_type", type=str, required=True,
                        choices=["linear", "cross_attention", "gated", "simple_gated", "simple_gated_with_bias", "bilinear"])
    parser.add_argument("--images_dir", type=str, default=None)
    parser.add_argument("--texts_dir", type=str, default=None)
    parser.add_argument("--splits_file", type=str, default=None)
    parser.add_argument("--split", type=str, default="test", choices=["train", "val", "test"])
    parser.add_argument("--max_text_length", type=int, default=150)
    parser.add_argument("--batch_size", type=int, default=64)
    parser.add_argument("--device", type=str, default="cuda")
    parser.add_argument("--output_file", type=str, default=None)
    parser.add_argument("--synthetic", type=int, default=0, metavar="N")
    parser.add_argument("--dataset", type=str, default="xuemduan/reevaluate-image-text-pairs")
    parser.add_argument("--rerank_depth", type=_rerank_depth_arg, default=None, metavar="N",
                        help=f"linear / cross_attention heads: retrieve-then-rerank over every query's N ({RERANK_DEPTH_MIN}..{_lib.MAX_DEEP_K}) "
                             "best candidates by the fused T2I + T2T score instead of the head on every pair")
    parser.add_argument("--sparql_results", type=str, default=None, metavar="DIR",
                        help="with --rerank_depth: directory of Text2SPARQL result files (load_text2sparql_results); the hits join the "
                             "shortlist and the list is ranked by head_weight * head + bonus")
    parser.add_argument("--sparql_strategy", type=str, default="weighted", choices=["weighted", "additive", "adaptive"],
                        help="how --sparql_results become a bonus (sparql_fusion.sparql_bonus); its clip_scale is the head's weight")
    return parser


@_in_process_group
def main_fusion(argv=None):
    import json
    parser = fusion_parser()
    args = parser.parse_args(argv)
    if args.rerank_depth is not None and args.fusion_type not in ("linear", "cross_attention"):
        parser.error(f"--rerank_depth is for the linear and cross_attention heads; the {args.fusion_type} head ranks the whole "
                     "gallery in one fused pass already")
    if args.sparql_results is not None:
        if args.fusion_type not in ("linear", "cross_attention"):
            parser.error(f"--sparql_results is for the linear and cross_attention heads (with --rerank_depth); the {args.fusion_type} head "
                         "folds into the fused similarity pass: fuse its ranking with sparql_fusion.fused_ranks")
        if args.rerank_depth is None:
            parser.error("--sparql_results needs --rerank_depth: " + _SPARQL_NEEDS_RERANK)
    elif args.sparql_strategy != "weighted":
        parser.error("--sparql_strategy has no effect without --sparql_results DIR")
    logging.basicConfig(level=logging.INFO, format="%(asctime)s - %(levelname)s - %(message)s")
    from . import clip_api, tokenizer
    from .clip_model import load_clip_model
    from .fusion_model import FusionModel
    if args.synthetic > 0:
        clip_api.allow_random_weights(True)
        tokenizer.allow_hash_tokenizer(True)
    if KD.active_shard() is not None:
        args.device = _device_of(args)
    clip_model, preprocess = load_clip_model(model_name=args.model_name, checkpoint_path=args.clip_checkpoint, device=args.device)
    _bind_tokenizer(clip_model, args)
    embed_dim = clip_model.arch.embed_dim                 # 768 (ViT-L/14), 512 (ViT-B), 1024 (ViT-H-14); a directory states its own
    fusion_model = FusionModel(clip_model=clip_model, fusion_type=args.fusion_type, embed_dim=embed_dim).to(args.device)
    if args.fusion_checkpoint:
        ckpt = torch.load(args.fusion_checkpoint, map_location="cpu", weights_only=True)
        fusion_model.fusion_head.load_state_dict(ckpt["fusion_head_state_dict"])
    if args.synthetic > 0:
        dataset = SyntheticRetrievalDataset(args.synthetic, clip_model.arch.image_size)
    else:
        from datasets import load_dataset
        ds = load_dataset(args.dataset)
        dataset = CLIPEvalDatasetHF(ds[{"val": "validation"}.get(args.split, args.split)], preprocess, args.max_text_length)
    t2s = load_text2sparql_results(args.sparql_results) if args.sparql_results is not None else None
    result = evaluate_fusion_model(fusion_model, dataset, args.batch_size, args.device, rerank_depth=args.rerank_depth,
                                   text2sparql_results=t2s, fusion_strategy=args.sparql_strategy)
    results = {"model_name": args.model_name, "clip_checkpoint": args.clip_checkpoint,
               "fusion_checkpoint": args.fusion_checkpoint, "fusion_type": args.fusion_type, "split": args.split,
               "num_samples": len(dataset), "metrics": result,
               "weights_source": getattr(clip_model, "weights_source", "unknown"), "tokenizer": model_tokenizer_name(clip_model),
               "precision": _lib.env_precision(), "data": "synthetic" if args.synthetic > 0 else args.dataset,
               **_sharding_record(len(dataset))}
    if not KD.is_writer():
        return results
    if args.output_file:
        Path(args.output_file).parent.mkdir(parents=True, exist_ok=True)
        with open(args.output_file, "w") as f:
            json.dump(results, f, indent=2)
    else:
        print(json.dumps(results, indent=2))
    return results


# ------------------------------------------------------------------------------------------------ sentence encoders (text-to-text baselines)
def _text_loader(dataset, batch_size: int, seed: int, collate, shuffle: bool = False, num_workers: int = 0) -> DataLoader:
    g = torch.Generator()
    g.manual_seed(seed)
    return DataLoader(dataset, batch_size=batch_size, shuffle=shuffle, num_workers=num_workers, collate_fn=collate,
                      worker_init_fn=seed_worker if num_workers else None, generator=g)


@torch.no_grad()
def evaluate_text_model(model, dataset, batch_size: int = 32, device: str = "cuda", seed: int = 42, compute_recall: bool = True,
                        compute_mrr: bool = True, num_workers: int = 0) -> Dict[str, float]:
    """Text-to-text retrieval of a sentence encoder, query -> target (reference: src/clip/eval/evaluator_lm.py:40-135; same signature,
    same ``T2T_*`` keys).  `model`: a ``sentence_model.SentenceEncoder`` (or anything with ``SentenceTransformer.encode``'s contract);
    `dataset`: samples ``(query, target_text)``.  The embeddings stay on the GPU and go into the fused rank kernel
    (``metrics.compute_retrieval_metrics``) instead of back to the host and through two ``np.argsort`` passes; `device` is accepted and
    must be the model's.  `num_workers`: the texts are strings in memory, 0 (the default here; the reference forks 4) loses nothing."""
    model = model.to(device)
    model.eval()
    shard = KD.active_shard()
    if shard is not None:                      # this rank's contiguous part of the pairs; ranked against the sharded targets
        n = len(dataset)
        lo, hi = KD.shard_bounds(n, shard[1], shard[0])
        queries, targets = [], []
        logger.info(f"rank {shard[0]} of {shard[1]}: encoding texts for {hi - lo} of {n} samples...")
        if hi > lo:
            for q, t in _text_loader(torch.utils.data.Subset(dataset, range(lo, hi)), batch_size, seed, collate_fn_eval_texts,
                                     num_workers=num_workers):
                queries.append(model.encode(q, convert_to_tensor=True, device=device, show_progress_bar=False, normalize_embeddings=True))
                targets.append(model.encode(t, convert_to_tensor=True, device=device, show_progress_bar=False, normalize_embeddings=True))
            query, target = torch.cat(queries), torch.cat(targets)
        else:
            query = torch.zeros((0, model_embed_dim(model)), dtype=torch.float32, device=device)
            target = query.clone()
        return _ShardedEmbeddings(n, None, query, target).metrics(["query"], ["target"], "T2T", compute_recall=compute_recall,
                                                                  compute_mrr=compute_mrr)
    queries, targets = [], []
    logger.info(f"Encoding texts for {len(dataset)} samples...")
    for q, t in _text_loader(dataset, batch_size, seed, collate_fn_eval_texts, num_workers=num_workers):
        queries.append(model.encode(q, convert_to_tensor=True, device=device, show_progress_bar=False, normalize_embeddings=True))
        targets.append(model.encode(t, convert_to_tensor=True, device=device, show_progress_bar=False, normalize_embeddings=True))
    query, target = torch.cat(queries), torch.cat(targets)
    logger.info(f"Query embeddings: {tuple(query.shape)}")
    logger.info(f"Target embeddings: {tuple(target.shape)}")
    return M.compute_retrieval_metrics(query, target, prefix="T2T", compute_recall=compute_recall, compute_mrr=compute_mrr)


@torch.no_grad()
def evaluate_text_model_for_training(model, dataset, batch_size: int = 32, device: str = "cuda", seed: int = 42) -> Dict[str, float]:
    """MRR / Mean_Rank only (reference: evaluator_lm.py:138-170)."""
    return evaluate_text_model(model, dataset, batch_size, device, seed, compute_recall=False, compute_mrr=True)


def _load_sentence_encoder(model_name: str, device: str):
    from .sentence_model import SentenceEncoder
    if not os.path.isdir(model_name):
        raise RuntimeError(f"--model_name {model_name!r} is not a directory: the sentence encoders are loaded from a local checkpoint "
                           "directory (config.json, weights, tokenizer.json), e.g. a download of sentence-transformers/all-mpnet-base-v2, "
                           "intfloat/e5-base-v2 or thenlper/gte-large; "
                           "nothing here contacts a model hub")
    return SentenceEncoder.from_pretrained(model_name, device=device, precision=_lib.env_precision())


def text_lm_parser() -> argparse.ArgumentParser:
    """The arguments of the reference's src/clip/eval/evaluator_lm.py:173-201 (+ --dataset / --synthetic, as the other CLIs have)."""
    p = argparse.ArgumentParser(description="Evaluate text-only models")
    p.add_argument("--model_name", type=str, required=True, help="local directory of a sentence encoder (all-mpnet-base-v2, E5, GTE)")
    p.add_argument("--texts_dir", type=str, required=True, help="accepted for the reference's command lines; not read")
    p.add_argument("--images_dir", type=str, required=True, help="accepted for the reference's command lines; not read")
    p.add_argument("--split", type=str, default="test", choices=["train", "val", "test"])
    p.add_argument("--mrr_only", action="store_true")
    p.add_argument("--batch_size", type=int, default=32)
    p.add_argument("--device", type=str, default="cuda")
    p.add_argument("--output_file", type=str, required=True)
    p.add_argument("--seed", type=int, default=42)
    p.add_argument("--dataset", type=str, default="xuemduan/reevaluate-image-text-pairs")
    p.add_argument("--synthetic", type=int, default=0, help="N > 0: N synthetic (query, target) pairs instead of the dataset")
    return p


class _SyntheticTextSplit:
    def __init__(self, n: int, seed: int):
        self._raw = SyntheticRawImageDataset(n, seed)

    def __len__(self):
        return len(self._raw)

    def __getitem__(self, idx):
        _, query, target, _ = self._raw[idx]
        return {"query_text": query, "target_text": target}


def _seed_all(seed: int) -> None:
    torch.manual_seed(seed)
    np.random.seed(seed)
    random.seed(seed)


def _save_text_results(log, args, dataset, metrics, extra) -> dict:
    log.info("EVALUATION RESULTS (T2T Only)")
    for name, value in sorted(metrics.items()):
        log.info(f"{name}: {value:.2f}" + ("" if "Mean_Rank" in name else "%"))
    results = {"model_name": args.model_name, "split": args.split, "num_samples": len(dataset), "seed": args.seed, "metrics": metrics,
               "precision": _lib.env_precision(), **extra}
    _save_results(results, args.output_file)
    log.info(f"Results saved to {args.output_file}")
    return results


@_in_process_group
def main_text_lm(argv=None):
    args = text_lm_parser().parse_args(argv)
    _seed_all(args.seed)
    name = "src.clip.eval.evaluator_lm"
    log = _open_outputs(args.output_file, name)
    log.info(f"Text-Only Model Evaluation (T2T only, MI355X HIP engine)  Model: {args.model_name}  Split: {args.split}  MRR only: {args.mrr_only}  Seed: {args.seed}")
    if not torch.cuda.is_available():
        raise RuntimeError("no GPU visible: the encoder and the ranking run only in the HIP kernels (no CPU fallback)")
    device = _device_of(args)
    model = _load_sentence_encoder(args.model_name, device)
    if args.synthetic > 0:
        dataset = TextOnlyDatasetHF(_SyntheticTextSplit(args.synthetic, args.seed))
    else:
        from datasets import load_dataset
        dataset = TextOnlyDatasetHF(load_dataset(args.dataset)[{"val": "validation"}.get(args.split, args.split)])
    fn = evaluate_text_model_for_training if args.mrr_only else evaluate_text_model
    metrics = fn(model, dataset, batch_size=args.batch_size, device=device, seed=args.seed)
    return _save_text_results(log, args, dataset, metrics, {"data": "synthetic" if args.synthetic > 0 else args.dataset,
                                                            **_sharding_record(len(dataset))})


# ---- the legacy five-variant script (reference: baselines/evaluate_text_models.py)
class TextVariantsDataset(torch.utils.data.Dataset):
    """One artifact per sample: the five description variants of ``<text_folder>/<uuid>.json`` (missing ones are "")."""
    KEYS = {"content": "content_descriptions", "metadata": "metadata_descriptions", "hybrid_o1": "hybrid_descriptions",
            "hybrid_o2": "hybrid_descriptions"}

    def __init__(self, uuids: Sequence[str], text_folder: str, description_type: str, random_seed: int = 42, num_variants: int = 5):
        self.uuids, self.text_folder, self.num_variants = list(uuids), Path(text_folder), num_variants
        self.key = self.KEYS[description_type]

    def __len__(self):
        return len(self.uuids)

    def __getitem__(self, idx):
        import json
        try:
            with open(self.text_folder / f"{self.uuids[idx]}.json", "r", encoding="utf-8") as f:
                found = json.load(f).get(self.key, [])
        except Exception as e:          # noqa: BLE001 - the reference substitutes empty texts as well
            logger.error(f"Error loading text for {self.uuids[idx]}: {e}")
            found = []
        texts = [d if isinstance(d, str) and d.strip() else "" for d in found[: self.num_variants]]
        return texts + [""] * (self.num_variants - len(texts))


def variant_metrics(embeddings_by_variant: Sequence[torch.Tensor], mode: str = "multi", k_values: Sequence[int] = (1, 5, 10, 20)) -> Dict[str, float]:
    """The single / multi metrics of the legacy script from the per-variant embeddings ([N, D] each, L2-normalised): for a query
    variant v the candidates are the other variants of every artifact, artifact-major (candidate id = artifact * 4 + slot), and a
    query's rank is that of the FIRST candidate of its own artifact (``ranking.ranks_of_groups``).  single: variant 0 queries;
    multi: every variant queries, all 5 N ranks averaged."""
    if mode not in ("single", "multi"):
        raise ValueError(f"mode {mode!r}: 'single' or 'multi'")
    from . import ranking
    nv = len(embeddings_by_variant)
    n = embeddings_by_variant[0].shape[0]
    ranks = []
    for qv in ([0] if mode == "single" else range(nv)):
        others = [v for v in range(nv) if v != qv]
        cand = torch.stack([embeddings_by_variant[v] for v in others], dim=1).reshape(n * len(others), -1)
        own = torch.arange(n).unsqueeze(1) * len(others) + torch.arange(len(others)).unsqueeze(0)
        ranks.append(ranking.ranks_of_groups(embeddings_by_variant[qv], cand, own))
    return {f"T2T_{k}": v for k, v in ranking.metrics_from_ranks(torch.cat(ranks), list(k_values)).items()}


@torch.no_grad()
def evaluate_text_model_variants(model, dataset, batch_size: int = 32, device: str = "cuda", mode: str = "multi", seed: int = 42,
                                 num_workers: int = 0) -> Dict[str, float]:
    """``evaluate_text_model`` of the legacy script (reference: baselines/evaluate_text_models.py:96-263; same signature).  The loader
    shuffles with the seeded generator as there; the metrics do not depend on the order of the artifacts."""
    model = model.to(device)
    model.eval()
    per = [[] for _ in range(5)]
    for batch in _text_loader(dataset, batch_size, seed, list, shuffle=True, num_workers=num_workers):
        for v in range(5):
            per[v].append(model.encode([b[v] for b in batch], convert_to_tensor=True, device=device, show_progress_bar=False,
                                       normalize_embeddings=True))
    return variant_metrics([torch.cat(p) for p in per], mode)


def text_variants_parser() -> argparse.ArgumentParser:
    """The arguments of the reference's baselines/evaluate_text_models.py:268-299."""
    p = argparse.ArgumentParser(description="Evaluate text-only models")
    p.add_argument("--model_name", type=str, required=True, help="local directory of a sentence encoder (all-mpnet-base-v2, E5, GTE)")
    p.add_argument("--texts_dir", type=str, required=True)
    p.add_argument("--description_type", type=str, required=True, choices=["content", "metadata", "hybrid_o1", "hybrid_o2"])
    p.add_argument("--images_dir", type=str, required=True, help="accepted for the reference's command lines; not read")
    p.add_argument("--splits_file", type=str, default=None)
    p.add_argument("--split", type=str, default="test", choices=["train", "val", "test"])
    p.add_argument("--eval_mode", type=str, default="multi", choices=["single", "multi"])
    p.add_argument("--batch_size", type=int, default=32)
    p.add_argument("--device", type=str, default="cuda")
    p.add_argument("--output_file", type=str, required=True)
    p.add_argument("--seed", type=int, default=42)
    return p


def main_text_variants(argv=None):
    import json
    args = text_variants_parser().parse_args(argv)
    _seed_all(args.seed)
    out_dir = Path(args.output_file).parent
    out_dir.mkdir(parents=True, exist_ok=True)
    name = "baselines.evaluate_text_models"
    setup_logger(name, str(out_dir / "evaluation.log"))
    log = logging.getLogger(name)
    if not args.splits_file or not Path(args.splits_file).exists():
        # the reference generates splits from `list(set(uuids))`, whose order follows Python's per-process string hashing: its own
        # runs do not reproduce them.  The file its save_splits_to_json writes is the one stable statement of a split.
        raise RuntimeError("--splits_file is required here: a JSON with the lists 'train', 'val' and 'test' (what the reference's "
                           "save_splits_to_json writes); the reference's on-the-fly splits depend on set iteration order")
    with open(args.splits_file, "r", encoding="utf-8") as f:
        uuids = json.load(f)[args.split]
    log.info(f"Text-Only Model Evaluation (T2T only, MI355X HIP engine)  Model: {args.model_name}  Description type: {args.description_type}  "
             f"Split: {args.split} ({len(uuids)} samples)  Mode: {args.eval_mode}  Seed: {args.seed}")
    if not torch.cuda.is_available():
        raise RuntimeError("no GPU visible: the encoder and the ranking run only in the HIP kernels (no CPU fallback)")
    device = args.device if args.device.startswith("cuda") else "cuda"
    model = _load_sentence_encoder(args.model_name, device)
    dataset = TextVariantsDataset(uuids, args.texts_dir, args.description_type, args.seed)
    metrics = evaluate_text_model_variants(model, dataset, args.batch_size, device, args.eval_mode, args.seed)
    return _save_text_results(log, args, dataset, metrics, {"description_type": args.description_type, "eval_mode": args.eval_mode})
