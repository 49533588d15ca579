"""Child process of tests/test_sharded_eval_gpu.py (not collected by pytest): the drop-in evaluators over a process group on one GPU.

    python tests/sharded_eval_child.py world1 OUT.json       one rank through RCCL ("nccl") with the collectives forced on
    python -m torch.distributed.run --standalone --nproc-per-node 2 tests/sharded_eval_child.py ranks OUT_DIR
                                                              (KEMR_DIST_BACKEND=gloo KEMR_LOCAL_DEVICE=0: two ranks on the one GPU)
Each mode writes a JSON report (rank<r>.json in OUT_DIR) of what the parent asserts; exit code 0 = the child itself saw no error."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, MODEL = 37, "ViT-B/32"


def _setup(device):
    import torch
    from knowledge_enhanced_multimodal_retrieval_amd import clip_api, tokenizer
    from knowledge_enhanced_multimodal_retrieval_amd.clip_model import load_clip_model
    from knowledge_enhanced_multimodal_retrieval_amd.datasets import SyntheticRetrievalDataset
    from knowledge_enhanced_multimodal_retrieval_amd.fusion_model import FusionModel
    clip_api.allow_random_weights(True)
    tokenizer.allow_hash_tokenizer(True)
    torch.manual_seed(0)
    model, _ = load_clip_model(model_name=MODEL, checkpoint_path=None, device=str(device))
    fusion = FusionModel(clip_model=model, fusion_type="linear", embed_dim=model.arch.embed_dim).to(device)
    return model, fusion, SyntheticRetrievalDataset(N, model.arch.image_size, 42)


def _bits_equal(a, b):
    import torch
    return a.shape == b.shape and bool(torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)))


def world1(out_path):
    """The same calls without a process group and through RCCL at world size 1: metrics and the embeddings' bits."""
    import torch
    import torch.distributed as dist
    from knowledge_enhanced_multimodal_retrieval_amd import dist as KD, evaluators as E
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", str(29500 + os.getpid() % 2000))
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)          # before anything else touches the GPU
    model, fusion, ds = _setup(dev)

    def run():
        return {"clip": E.evaluate_clip_model(model, ds, 16, str(dev), num_workers=0, text2sparql_results={}),
                "analysis": E.evaluate_clip_model.last_analysis,
                "fusion": E.evaluate_fusion_model(fusion, ds, 16, str(dev), num_workers=0),
                "emb": E.encode_dataset(model, ds, 16, 42, 0, shard=KD.active_shard())}
    assert KD.active_shard() is None                                              # one rank: everything short-circuits
    plain = run()
    KD.force_collectives(True)
    assert KD.active_shard() == (0, 1)
    calls = {"all_gather_into_tensor": 0, "all_reduce": 0, "all_gather_object": 0}
    for name in calls:
        orig = getattr(dist, name)

        def wrap(*a, _orig=orig, _name=name, **kw):
            calls[_name] += 1
            return _orig(*a, **kw)
        setattr(dist, name, wrap)
    forced = run()
    torch.cuda.synchronize()
    report = {"backend": dist.get_backend(), "calls": calls,
              "metrics_equal": {k: plain[k] == forced[k] for k in ("clip", "analysis", "fusion")},
              "emb_bits_equal": [_bits_equal(a, b) for a, b in zip(plain["emb"][:3], forced["emb"][:3])],
              "uuids_equal": plain["emb"][3] == forced["emb"][3], "clip": forced["clip"], "fusion": forced["fusion"]}
    dist.barrier()
    dist.destroy_process_group()
    with open(out_path, "w") as f:
        json.dump(report, f)
    return 0


def ranks(out_dir):
    """Two (or more) ranks on one GPU over gloo: the sharded metrics against the single-process functions on the gathered embeddings."""
    import torch
    import torch.nn.functional as Fn
    from knowledge_enhanced_multimodal_retrieval_amd import dist as KD, evaluators as E, metrics as M, ranking
    world, rank, dev = KD.init_from_env()
    model, fusion, ds = _setup(dev)
    shard = KD.active_shard()
    assert shard == (rank, world)
    clip = E.evaluate_clip_model(model, ds, 16, str(dev), num_workers=0, analysis=False)
    base = E.evaluate_clip_model_baseline(model, ds, 16, str(dev), num_workers=0, t2i_weight=0.3, t2t_weight=0.7)
    fus = E.evaluate_fusion_model(fusion, ds, 16, str(dev), num_workers=0)
    from knowledge_enhanced_multimodal_retrieval_amd.fusion_model import FusionModel
    torch.manual_seed(1)
    gated = FusionModel(clip_model=model, fusion_type="simple_gated_with_bias", embed_dim=model.arch.embed_dim).to(dev)
    fus_gated = E.evaluate_fusion_model(gated, ds, 16, str(dev), num_workers=0)
    fus_rerank = E.evaluate_fusion_model(fusion, ds, 16, str(dev), num_workers=0, rerank_depth=20)
    image, query, target, uuids = E.encode_dataset(model, ds, 16, 42, 0, shard=shard)
    even = KD.EvenRows(N)
    g_img, g_qry, g_tgt = (even.real(KD.all_gather_rows(even.pad(x))) for x in (image, query, target))
    report = {"rank": rank, "world": world, "uuids": uuids, "lo_hi": [even.lo, even.hi], "clip": clip, "baseline": base, "fusion": fus,
              "fusion_gated": fus_gated, "fusion_rerank": fus_rerank}
    # one process, the same rows: the whole dataset in one encode_dataset call
    w_img, w_qry, w_tgt, w_uuids = E.encode_dataset(model, ds, 16, 42, 0)
    sl = slice(even.lo, even.hi)
    report["bits_equal"] = [_bits_equal(a, b[sl]) for a, b in ((image, w_img), (query, w_qry), (target, w_tgt))]
    report["max_1mcos"] = [float((1 - Fn.cosine_similarity(a.double(), b[sl].double())).max()) if a.shape[0] else 0.0
                           for a, b in ((image, w_img), (query, w_qry), (target, w_tgt))]
    report["whole_uuids"] = w_uuids
    if rank == 0:                               # the single-process functions on the GATHERED embeddings (no collective in here)
        os.environ["KEMR_EVAL_SHARDED"] = "0"
        assert KD.active_shard() is None
        report["want_clip"] = M.compute_all_retrieval_metrics(g_qry, g_tgt, g_img)
        report["want_baseline"] = M.compute_retrieval_metrics_final(g_qry, g_tgt, g_img, t2i_weight=0.3, t2t_weight=0.7)
        report["want_fusion"] = ranking.metrics_from_ranks(fusion.rank(g_qry, g_img, g_tgt, k=0)[0], [1, 5, 10, 20])
        report["want_fusion_gated"] = ranking.metrics_from_ranks(gated.rank(g_qry, g_img, g_tgt, k=0)[0], [1, 5, 10, 20])
        r = fusion.rerank(g_qry, fusion.prepare_gallery(g_img, g_tgt), depth=20, k=1, gt_idx="diag")[0]
        report["want_fusion_rerank"] = {**ranking.metrics_from_ranks(r, [1, 5, 10, 20]),
                                        "Shortlist_Recall": float((r <= 20).double().mean().item() * 100.0), "Rerank_Depth": 20}
        os.environ.pop("KEMR_EVAL_SHARDED")
    torch.cuda.synchronize()
    with open(os.path.join(out_dir, f"rank{rank}.json"), "w") as f:
        json.dump(report, f)
    KD.finish()
    return 0


if __name__ == "__main__":
    sys.exit({"world1": world1, "ranks": ranks}[sys.argv[1]](sys.argv[2]))
