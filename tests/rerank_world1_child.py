"""Child process of tests/test_dist_rerank_world1.py (not collected by pytest): ShardedGallery.rerank and the k <= 32 bonus of
ShardedGallery.search / ranks through RCCL with a process group of ONE rank on the one GPU of the box, compared bit for bit with
FusionModel.rerank / ranking.ranks_and_topk on the same inputs.  Prints one JSON line; exit code 0 = all equal."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main() -> int:
    import numpy as np
    import torch
    import torch.distributed as dist
    from knowledge_enhanced_multimodal_retrieval_amd import dist as kd, ranking
    from knowledge_enhanced_multimodal_retrieval_amd.fusion_model import FusionModel

    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(7)
    n, d, nq, depth, k = 2000, 128, 64, 100, 10
    unit = lambda x: x / x.norm(dim=1, keepdim=True)
    img = unit(torch.randn(n, d, generator=g)).to(dev)
    txt = unit(img.cpu() + 0.5 * unit(torch.randn(n, d, generator=g))).to(dev)
    q = unit(img[:nq].cpu() + 0.8 * unit(torch.randn(nq, d, generator=g))).to(dev)
    gt = torch.arange(nq, dtype=torch.int32, device=dev)
    rng = np.random.default_rng(7)
    cols = np.sort(rng.integers(0, n, (nq, 12)), axis=1).astype(np.int32)
    bonus = (np.arange(0, 12 * nq + 1, 12, dtype=np.int32), cols.reshape(-1), np.full(12 * nq, 0.2, np.float32))

    heads = {}
    for ft in ("linear", "cross_attention"):
        fm = FusionModel(torch.nn.Linear(1, 1), fusion_type=ft, embed_dim=d)
        with torch.no_grad():
            for p_ in fm.fusion_head.parameters():
                p_.copy_(torch.randn(p_.shape, generator=g) * (0.1 if ft == "cross_attention" else 0.4))
        fm = fm.to(dev)
        heads[ft] = (fm, fm.prepare_gallery(img, txt))

    want = {}
    for ft, (fm, gal) in heads.items():                                        # the single-GPU route, no process group
        want[ft + "/fused"] = fm.rerank(q, gal, depth=depth, k=k, gt_idx=gt, bonus=bonus, head_weight=0.8)
        want[ft + "/plain"] = fm.rerank(q, gal, depth=depth, k=k, gt_idx=gt)
        want[ft + "/lists"] = fm.rerank(q, gal, depth=depth, k=k, bonus=bonus, head_weight=0.8)
    want["ranks"] = ranking.ranks_and_topk([q, q], [img, txt], weights=[0.5, 0.5], k=k, gt_idx=gt, bonus=bonus)
    torch.cuda.synchronize()

    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", str(29500 + os.getpid() % 2000))
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    kd.force_collectives(True)
    counted = {}
    for name in ("all_gather_into_tensor", "all_reduce"):                      # count what really reaches torch.distributed
        orig = getattr(dist, name)

        def wrap(*a, _orig=orig, _name=name, **kw):
            counted.setdefault(_name, {"n": 0, "cuda": 0})
            counted[_name]["n"] += 1
            counted[_name]["cuda"] += int(a[0].is_cuda)
            return _orig(*a, **kw)
        setattr(dist, name, wrap)
    sharded = kd.ShardedGallery([img, txt], n)
    got = {}
    for ft, (fm, gal) in heads.items():
        got[ft + "/fused"] = sharded.rerank(fm, gal, q, depth=depth, k=k, local_gt=gt, bonus=bonus, head_weight=0.8)
        got[ft + "/plain"] = sharded.rerank(fm, gal, q, depth=depth, k=k, local_gt=gt)
        got[ft + "/lists"] = sharded.rerank(fm, gal, q, depth=depth, k=k, bonus=bonus, head_weight=0.8)
    got["ranks"] = sharded.ranks([q, q], gt, [0.5, 0.5], k=k, bonus=bonus)
    search = sharded.search([q, q], [0.5, 0.5], k=k, bonus=bonus)
    torch.cuda.synchronize()

    def same(a, b):
        if a is None or b is None:
            return a is None and b is None
        if isinstance(a, (tuple, list)):
            return len(a) == len(b) and all(same(u, v) for u, v in zip(a, b))
        return a.dtype == b.dtype and torch.equal(a, b)
    report = {"backend": dist.get_backend(), "world": dist.get_world_size(), "calls": counted,
              "equal": {key: bool(same(want[key], got[key])) for key in want}}
    report["equal"]["search"] = bool(same(tuple(want["ranks"][1:]), tuple(search)))
    fused, plain = got["linear/fused"], got["linear/plain"]
    report["bonus_moves_the_list"] = bool((fused[2] != plain[2]).any())
    report["listed"] = float((fused[0] <= depth).float().mean())
    dist.barrier()
    dist.destroy_process_group()
    print(json.dumps(report))
    return 0 if all(report["equal"].values()) else 1


if __name__ == "__main__":
    sys.exit(main())
