"""Online retrieval: resident gallery embeddings + single-query search, and the reference's ``RetrievalEngine`` API.

Reference call stack: ``RetrievalEngine.retrieve_text`` (/root/reference/src/retrieval.py:79-95)
-> ``CLIPRetrieval.retrieval`` (src/clip/clip_retrieval.py:39-40) -> ``retriever.search(query, alpha)`` of a
``CLIPRetriever`` whose source the reference downloads from the HF Hub and ``exec``s
(clip_retrieval.py:15-37) -- that file is not in the reference checkout, so ``search``'s exact semantics are
UNPINNED.  This build's local ``CLIPRetriever`` takes the documented argument names at face value:
``score = alpha * <q, image_i> + (1 - alpha) * <q, target_text_i>`` over gallery embeddings precomputed under
``data/embeddings`` (the reference's ``local_embeddings_dir``), best ``top_k`` first.

Store format (this build's definition): ``<dir>/image_embeddings.npy`` and ``<dir>/text_embeddings.npy``
(float32 [N, D], L2-normalised rows) + ``<dir>/uuids.json`` (list of N strings).  ``EmbeddingStore.load`` puts both
sets into HBM as one bf16 split panel ([image ; text] along k), built once; a query is one fused kernel pass.

The SPARQL side (Mistral + GraphDB over HTTP, src/text2sparql/*) is out of scope; ``RetrievalEngine`` takes any object
with ``retrieval(query) -> List[uuid]`` and defaults to one that returns no hits.
"""
from __future__ import annotations

import json
import os
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _lib, engine, ranking
from .sparql_fusion import _uri_tail

MAX_TOP_K = 32
MAX_DEEP_TOP_K = 1024        # search_deep / retrieve_text_deep: kemr_sim_topk_deep (selection + sort instead of register lists)


def hits_to_csr(hits_per_query: Sequence[Sequence[str]], row_of: Dict[str, int], value: float):
    """SPARQL hit lists (uuids or URIs, one list per query) -> the one-value bonus CSR ``(rowptr int32 [Q + 1], col int32, val fp32)``
    of ``engine.sim_topk_deep``: a URI counts by its tail after the last ``/`` (``sparql_fusion._uri_tail``), ids that ``row_of``
    (uuid -> gallery row) does not hold are ignored, an id listed twice counts once (the reference tests
    ``uuid in set(sparql_results)``), columns ascend within a row."""
    rowptr = np.zeros(len(hits_per_query) + 1, np.int32)
    cols: List[int] = []
    for r, hits in enumerate(hits_per_query):
        cols.extend(sorted({row_of[t] for t in map(_uri_tail, hits) if t in row_of}))
        rowptr[r + 1] = len(cols)
    return rowptr, np.asarray(cols, np.int32), np.full(len(cols), value, np.float32)


class EmbeddingStore:
    """Gallery embeddings resident in HBM, ready for the fused similarity kernel."""

    def __init__(self, image_embeddings, text_embeddings, uuids: Sequence[str], device=None, precision: str = "fp32x3"):
        self.uuids = list(uuids)
        self.image = ranking.to_device_f32(image_embeddings, device)
        self.text = ranking.to_device_f32(text_embeddings, self.image.device)
        if self.image.shape != self.text.shape or self.image.shape[0] != len(self.uuids):
            raise ValueError("image / text embeddings and uuids must describe the same N items")
        self.precision = precision
        self._row_of: Optional[Dict[str, int]] = None
        self.panel = engine.build_panel([self.image, self.text], _lib.SIDE_GALLERY, ranking.PRECISION_TERMS[precision])

    def __len__(self):
        return len(self.uuids)

    @property
    def row_of(self) -> Dict[str, int]:
        """uuid -> gallery row, built on first use (a uuid stored twice: its first row, as ``list.index`` would say)."""
        if self._row_of is None:
            rows: Dict[str, int] = {}
            for i, u in enumerate(self.uuids):
                rows.setdefault(u, i)
            self._row_of = rows
        return self._row_of

    def hits_csr(self, hits_per_query: Sequence[Sequence[str]], value: float):
        """``hits_to_csr`` against this store's rows."""
        return hits_to_csr(hits_per_query, self.row_of, value)

    @property
    def dim(self) -> int:
        return self.image.shape[1]

    def save(self, directory: str) -> None:
        os.makedirs(directory, exist_ok=True)
        np.save(os.path.join(directory, "image_embeddings.npy"), self.image.cpu().numpy())
        np.save(os.path.join(directory, "text_embeddings.npy"), self.text.cpu().numpy())
        with open(os.path.join(directory, "uuids.json"), "w") as f:
            json.dump(self.uuids, f)

    @classmethod
    def load(cls, directory: str, device=None, precision: str = "fp32x3") -> "EmbeddingStore":
        img = np.load(os.path.join(directory, "image_embeddings.npy"), allow_pickle=False)
        txt = np.load(os.path.join(directory, "text_embeddings.npy"), allow_pickle=False)
        with open(os.path.join(directory, "uuids.json")) as f:
            uuids = json.load(f)
        return cls(img, txt, uuids, device, precision)

    @classmethod
    def build(cls, model, dataset, batch_size: int = 64, tokenize_fn=None, precision: str = "fp32x3") -> "EmbeddingStore":
        """Encode a dataset of (image, query, target, uuid) once; the gallery keeps image and TARGET-text embeddings."""
        from .evaluators import encode_dataset
        image, _, target, uuids = encode_dataset(model, dataset, batch_size, tokenize_fn=tokenize_fn)
        return cls(image, target, uuids, image.device, precision)


class CLIPRetriever:
    """Local counterpart of the reference's remote ``CLIPRetriever`` (see module docstring: semantics unpinned)."""

    def __init__(self, model, store: EmbeddingStore, tokenize_fn=None):
        self.model, self.store = model, store
        if tokenize_fn is None:
            from .evaluators import model_tokenize
            tokenize_fn = model_tokenize(model)          # CLIP's BPE, or a SigLIP model's own tokenizer.json (model.tokenizer_dir)
        self.tokenize_fn = tokenize_fn

    @classmethod
    def from_pretrained(cls, repo_id: str = "xuemduan/reevaluate-clip-retriever", local_embeddings_dir: str = "data/embeddings",
                        model_name: Optional[str] = None, token: Optional[str] = None, device: str = "cuda", **_):
        """Nothing is fetched: ``repo_id`` / ``token`` are accepted for signature compatibility; weights come from
        ``clip.load`` (see clip_api.py) and the gallery from ``local_embeddings_dir``."""
        from . import clip_api
        model, _ = clip_api.load(model_name or "ViT-L/14", device=device)
        return cls(model, EmbeddingStore.load(local_embeddings_dir, device))

    @torch.no_grad()
    def search_batch(self, queries: Sequence[str], alpha: float = 0.5, top_k: int = 10):
        if not 1 <= top_k <= MAX_TOP_K:
            raise ValueError(f"top_k must be in 1..{MAX_TOP_K}")
        ids = self.tokenize_fn(list(queries))          # host ids: the engine takes the text lengths from them before the upload (no device sync)
        q = self.model.encode_text(ids, normalize=True)
        qp = engine.build_panel([q, q], _lib.SIDE_QUERY, ranking.PRECISION_TERMS[self.store.precision],
                                part_scale=[alpha, 1.0 - alpha])
        return engine.sim_topk(qp, self.store.panel, min(top_k, len(self.store)))

    def search(self, query: str, alpha: float = 0.5, top_k: int = 10) -> List[Dict]:
        scores, idx = self.search_batch([query], alpha, top_k)
        scores, idx = scores[0].cpu().tolist(), idx[0].cpu().tolist()
        return [{"uuid": self.store.uuids[i], "score": float(s)} for s, i in zip(scores, idx) if i >= 0]

    @torch.no_grad()
    def search_batch_deep(self, queries: Sequence[str], alpha: float = 0.5, top_k: int = 200):
        """``search_batch`` for lists of up to MAX_DEEP_TOP_K candidates: the same scores and order, by ``engine.sim_topk_deep``."""
        if not 1 <= top_k <= MAX_DEEP_TOP_K:
            raise ValueError(f"top_k must be in 1..{MAX_DEEP_TOP_K}")
        ids = self.tokenize_fn(list(queries))
        q = self.model.encode_text(ids, normalize=True)
        qp = engine.build_panel([q, q], _lib.SIDE_QUERY, ranking.PRECISION_TERMS[self.store.precision],
                                part_scale=[alpha, 1.0 - alpha])
        return engine.sim_topk_deep(qp, self.store.panel, min(top_k, len(self.store)))

    def search_deep(self, query: str, alpha: float = 0.5, top_k: int = 200) -> List[Dict]:
        scores, idx = self.search_batch_deep([query], alpha, top_k)
        scores, idx = scores[0].cpu().tolist(), idx[0].cpu().tolist()
        return [{"uuid": self.store.uuids[i], "score": float(s)} for s, i in zip(scores, idx) if i >= 0]


    @torch.no_grad()
    def search_batch_fused(self, queries: Sequence[str], hits_per_query: Sequence[Sequence[str]], alpha: float = 0.5,
                           clip_weight: float = 1.0, hit_bonus: float = 0.2, top_k: int = 200):
        """The ``top_k`` best of the WHOLE gallery by
        ``clip_weight * (alpha * <q, image_i> + (1 - alpha) * <q, text_i>) + hit_bonus * [uuid_i in hits]``: one pass of
        ``engine.sim_topk_deep`` with ``clip_weight`` folded into the query panel and the hits as a bonus list (``hits_csr``), so a
        hit receives its bonus wherever CLIP alone would rank it."""
        if not 1 <= top_k <= MAX_DEEP_TOP_K:
            raise ValueError(f"top_k must be in 1..{MAX_DEEP_TOP_K}")
        if len(hits_per_query) != len(queries):
            raise ValueError("search_batch_fused: one hit list per query")
        ids = self.tokenize_fn(list(queries))
        q = self.model.encode_text(ids, normalize=True)
        qp = engine.build_panel([q, q], _lib.SIDE_QUERY, ranking.PRECISION_TERMS[self.store.precision],
                                part_scale=[clip_weight * alpha, clip_weight * (1.0 - alpha)])
        return engine.sim_topk_deep(qp, self.store.panel, min(top_k, len(self.store)),
                                    bonus=self.store.hits_csr(hits_per_query, hit_bonus))

    def search_fused(self, query: str, hits: Sequence[str], alpha: float = 0.5, clip_weight: float = 1.0, hit_bonus: float = 0.2,
                     top_k: int = 200) -> List[Dict]:
        scores, idx = self.search_batch_fused([query], [hits], alpha, clip_weight, hit_bonus, top_k)
        scores, idx = scores[0].cpu().tolist(), idx[0].cpu().tolist()
        return [{"uuid": self.store.uuids[i], "score": float(s)} for s, i in zip(scores, idx) if i >= 0]

    @torch.no_grad()
    def search_batch_reranked(self, queries: Sequence[str], fusion_model, gallery, depth: int = 200, top_k: int = 10):
        """The online route of a trained ``linear`` / ``cross_attention`` head (``FusionModel.rerank``): text tower -> the ``depth``
        best of the store's fused panel by 0.5 * <q, image_i> + 0.5 * <q, text_i> -> the head on those pairs -> its ``top_k`` best,
        ``(scores [Q, top_k], ids [Q, top_k])`` with the HEAD's scores (score descending, then lower row; -inf / -1 padding).
        ``gallery``: ``fusion_model.prepare_gallery(store.image, store.text)``, built once.  ``top_k`` may exceed MAX_TOP_K, up to
        ``depth`` <= MAX_DEEP_TOP_K: the list goes through the deep route."""
        if not 1 <= depth <= MAX_DEEP_TOP_K:
            raise ValueError(f"depth must be in 1..{MAX_DEEP_TOP_K}")
        if not 1 <= top_k <= depth:
            raise ValueError(f"top_k must be in 1..depth={depth}")
        fusion_model._require_rerank_head("search_batch_reranked")
        if len(gallery) != len(self.store):
            raise ValueError(f"the prepared gallery has {len(gallery)} candidates, the store {len(self.store)}")
        ids = self.tokenize_fn(list(queries))
        q = self.model.encode_text(ids, normalize=True)
        list_idx = fusion_model.shortlist(q, self.store.panel, depth)
        _, top_s, top_i, _, _ = fusion_model._rerank_lists(q, gallery, list_idx, top_k, None)
        return top_s, top_i

    def search_reranked(self, query: str, fusion_model, gallery, depth: int = 200, top_k: int = 10) -> List[Dict]:
        scores, idx = self.search_batch_reranked([query], fusion_model, gallery, depth, top_k)
        scores, idx = scores[0].cpu().tolist(), idx[0].cpu().tolist()
        return [{"uuid": self.store.uuids[i], "score": float(s)} for s, i in zip(scores, idx) if i >= 0]

    @torch.no_grad()
    def search_batch_reranked_fused(self, queries: Sequence[str], hits_per_query: Sequence[Sequence[str]], fusion_model, gallery,
                                    depth: int = 200, top_k: int = 10, head_weight: float = 0.8, hit_bonus: float = 0.2):
        """``search_batch_reranked`` with the knowledge graph kept (``FusionModel.rerank(bonus=...)``): text tower -> the ``depth``
        best of the store's fused panel by 0.5 * <q, image_i> + 0.5 * <q, text_i> + hit_bonus * [uuid_i in hits], so a hit reaches
        the list wherever CLIP ranks it -> the head on those pairs -> ``head_weight * head + hit_bonus * [uuid_i in hits]``
        (``engine.list_fuse``) -> its ``top_k`` best, ``(scores [Q, top_k], ids [Q, top_k])`` with the fused scores."""
        if not 1 <= depth <= MAX_DEEP_TOP_K:
            raise ValueError(f"depth must be in 1..{MAX_DEEP_TOP_K}")
        if not 1 <= top_k <= depth:
            raise ValueError(f"top_k must be in 1..depth={depth}")
        if len(hits_per_query) != len(queries):
            raise ValueError("search_batch_reranked_fused: one hit list per query")
        fusion_model._require_rerank_head("search_batch_reranked_fused")
        if len(gallery) != len(self.store):
            raise ValueError(f"the prepared gallery has {len(gallery)} candidates, the store {len(self.store)}")
        bonus = self.store.hits_csr(hits_per_query, hit_bonus)
        ids = self.tokenize_fn(list(queries))
        q = self.model.encode_text(ids, normalize=True)
        list_idx = fusion_model.shortlist(q, self.store.panel, depth, bonus=bonus)
        _, top_s, top_i, _, _ = fusion_model._rerank_lists_fused(q, gallery, list_idx, top_k, None, bonus, float(head_weight))
        return top_s, top_i

    def search_reranked_fused(self, query: str, hits: Sequence[str], fusion_model, gallery, depth: int = 200, top_k: int = 10,
                              head_weight: float = 0.8, hit_bonus: float = 0.2) -> List[Dict]:
        scores, idx = self.search_batch_reranked_fused([query], [hits], fusion_model, gallery, depth, top_k, head_weight, hit_bonus)
        scores, idx = scores[0].cpu().tolist(), idx[0].cpu().tolist()
        return [{"uuid": self.store.uuids[i], "score": float(s)} for s, i in zip(scores, idx) if i >= 0]


class CLIPRetrieval:
    """``CLIPRetrieval(model_name=None).retrieval(query, alpha=0.5)`` (reference src/clip/clip_retrieval.py:10-40),
    without the hub download / ``exec`` / ``login``."""

    def __init__(self, model_name=None, retriever: Optional[CLIPRetriever] = None, embeddings_dir: str = "data/embeddings"):
        self.retriever = retriever or CLIPRetriever.from_pretrained(
            "xuemduan/reevaluate-clip-retriever", local_embeddings_dir=embeddings_dir, model_name=model_name)

    def retrieval(self, query: str, alpha: float = 0.5):
        return self.retriever.search(query, alpha=alpha)

    def retrieval_deep(self, query: str, alpha: float = 0.5, depth: int = 200):
        """The ``depth`` best instead of the ten of ``retrieval`` (this build's addition: candidates for the SPARQL fusion)."""
        return self.retriever.search_deep(query, alpha=alpha, top_k=depth)

    def retrieval_fused(self, query: str, hits: Sequence[str], alpha: float = 0.5, clip_weight: float = 1.0, hit_bonus: float = 0.2,
                        depth: int = 200):
        """The ``depth`` best by the fused score ``clip_weight * clip + hit_bonus * [uuid in hits]`` over the whole gallery."""
        return self.retriever.search_fused(query, hits, alpha=alpha, clip_weight=clip_weight, hit_bonus=hit_bonus, top_k=depth)

    def retrieval_reranked_fused(self, query: str, hits: Sequence[str], fusion_model, gallery, head_weight: float = 0.8,
                                 hit_bonus: float = 0.2, depth: int = 200):
        """The ``depth`` best by ``head_weight * head + hit_bonus * [uuid in hits]``, the trained head scored on a shortlist that
        the hits are part of (``CLIPRetriever.search_reranked_fused``)."""
        return self.retriever.search_reranked_fused(query, hits, fusion_model, gallery, depth=depth, top_k=depth,
                                                    head_weight=head_weight, hit_bonus=hit_bonus)


class NoText2SPARQL:
    """Placeholder for the out-of-scope LLM + SPARQL retriever: never any hit."""

    def retrieval(self, query: str) -> List[str]:
        return []


class RetrievalEngine:
    """Same public methods as the reference (src/retrieval.py:11-107); both retrievers are injectable."""

    def __init__(self, clip_retriever=None, t2s_retriever=None):
        self.clip_retriever = clip_retriever or CLIPRetrieval()
        self.t2s_retriever = t2s_retriever or NoText2SPARQL()
        self.cir_endpoint = os.getenv("CIR_ENDPOINT")
        self.cir_headers = {"accept": "application/json", "X-API-Key": os.getenv("CIR_ENDPOINT_KEY")}

    def _fuse_clip_sparql_linear(self, clip_results: List[Dict], sparql_results: List[str], alpha: float = 0.8,
                                 beta: float = 0.2) -> List[Dict]:
        """score = round(alpha * clip + beta * [uuid in sparql], 4), best first (stable), no normalisation."""
        if not clip_results:
            return []
        hits = set(sparql_results)
        fused = [{"uuid": it["uuid"], "score": round(alpha * it["score"] + beta * (1.0 if it["uuid"] in hits else 0.0), 4)}
                 for it in clip_results]
        fused.sort(key=lambda x: x["score"], reverse=True)
        return fused

    def retrieve_text(self, query: str, alpha: float = 0.8, beta: float = 0.2, alpha_clip: float = 0.5, threshold: float = 0):
        clip_results = self.clip_retriever.retrieval(query, alpha=alpha_clip)
        t2s_results = self.t2s_retriever.retrieval(query)
        fused = self._fuse_clip_sparql_linear(clip_results=clip_results, sparql_results=t2s_results, alpha=alpha, beta=beta)
        return [{"uuid": it["uuid"], "score": it["score"]} for it in fused if it.get("score", 0) >= threshold]

    def retrieve_text_deep(self, query: str, alpha: float = 0.8, beta: float = 0.2, alpha_clip: float = 0.5, threshold: float = 0,
                           depth: int = 200):
        """``retrieve_text`` over the ``depth`` best CLIP candidates instead of CLIP's own ten: the same linear fusion, so a SPARQL
        hit that CLIP ranks anywhere among them receives ``beta`` and can be lifted, and ``threshold`` selects from a list long
        enough to mean "everything that scores at least t".  (This build's addition; the reference has no counterpart.)"""
        clip_results = self.clip_retriever.retrieval_deep(query, alpha=alpha_clip, depth=depth)
        t2s_results = self.t2s_retriever.retrieval(query)
        fused = self._fuse_clip_sparql_linear(clip_results=clip_results, sparql_results=t2s_results, alpha=alpha, beta=beta)
        return [{"uuid": it["uuid"], "score": it["score"]} for it in fused if it.get("score", 0) >= threshold]

    def retrieve_text_fused(self, query: str, alpha: float = 0.8, beta: float = 0.2, alpha_clip: float = 0.5, threshold: float = 0,
                            depth: int = 200):
        """The reference's fusion formula (``src/retrieval.py:63-64``: ``alpha * clip + beta * [uuid in sparql]``) applied to EVERY
        gallery item instead of to CLIP's own list: the SPARQL retriever is asked first, then one fused search scores the whole
        gallery and returns its ``depth`` best, so a hit lands where its fused score puts it however low CLIP alone ranks it, and the
        head of the list does not change with ``depth``.  ``{"uuid", "score": round(score, 4)}`` in the kernel's order (score
        descending, then gallery row), cut at ``threshold``.  (This build's addition; the reference has no counterpart.)"""
        t2s_results = self.t2s_retriever.retrieval(query)
        fused = self.clip_retriever.retrieval_fused(query, t2s_results, alpha=alpha_clip, clip_weight=alpha, hit_bonus=beta, depth=depth)
        return [{"uuid": it["uuid"], "score": round(it["score"], 4)} for it in fused if round(it["score"], 4) >= threshold]

    def retrieve_text_reranked(self, query: str, fusion_model, gallery, alpha: float = 0.8, beta: float = 0.2, threshold: float = 0,
                               depth: int = 200):
        """``retrieve_text_fused`` with a trained ``linear`` / ``cross_attention`` head in CLIP's place: the SPARQL retriever is
        asked first, its hits join the ``depth``-deep shortlist wherever CLIP ranks them, the head scores the listed pairs and the
        list is ordered by ``alpha * head + beta * [uuid in sparql]``.  ``gallery``: ``fusion_model.prepare_gallery(store.image,
        store.text)``.  ``{"uuid", "score": round(score, 4)}`` in the kernel's order, cut at ``threshold``.  (This build's
        addition; the reference has no counterpart.)"""
        t2s_results = self.t2s_retriever.retrieval(query)
        fused = self.clip_retriever.retrieval_reranked_fused(query, t2s_results, fusion_model, gallery, head_weight=alpha,
                                                             hit_bonus=beta, depth=depth)
        return [{"uuid": it["uuid"], "score": round(it["score"], 4)} for it in fused if round(it["score"], 4) >= threshold]

    def retrieve_text_noknowledge(self, query: str, alpha: float = 0.8, beta: float = 0.2, alpha_clip: float = 0.5,
                                  threshold: float = 0):
        results = self.clip_retriever.retrieval(query, alpha=alpha_clip)
        return [{"uuid": it["uuid"], "score": it["score"]} for it in results if it.get("score", 0) >= threshold]
