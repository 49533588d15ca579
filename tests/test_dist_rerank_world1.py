"""GPU: ShardedGallery.rerank and the k <= 32 bonus of ShardedGallery.search / ranks with the collectives executed through RCCL, in
a process group of one rank (the pattern of tests/test_dist_rccl_world1.py: a fresh child process that initialises backend "nccl").
At world size 1 the sharded rerank must return the bits of FusionModel.rerank -- with and without bonus, with and without ground
truth, for both pair heads -- and the sharded fused search the bits of ranking.ranks_and_topk."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_sharded_rerank_through_rccl_at_world_size_one(device):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"), MASTER_ADDR="127.0.0.1")
    env.pop("KEMR_DIST_BACKEND", None)
    proc = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "rerank_world1_child.py")], capture_output=True, text=True,
                          timeout=600, env=env, cwd=ROOT)
    assert proc.returncode == 0, (proc.returncode, proc.stdout[-2000:], proc.stderr[-4000:])
    report = json.loads([l for l in proc.stdout.splitlines() if l.startswith("{")][-1])
    assert report["backend"] == "nccl" and report["world"] == 1
    assert set(report["equal"]) == {"linear/fused", "linear/plain", "linear/lists", "cross_attention/fused", "cross_attention/plain",
                                    "cross_attention/lists", "ranks", "search"}
    assert all(report["equal"].values()), report
    calls = report["calls"]
    # every collective ran on DEVICE tensors: per rerank the query and candidate gathers of the shortlist and ONE list all-reduce
    assert calls["all_gather_into_tensor"]["n"] >= 20 and calls["all_gather_into_tensor"]["cuda"] == calls["all_gather_into_tensor"]["n"]
    assert calls["all_reduce"]["n"] >= 8 and calls["all_reduce"]["cuda"] == calls["all_reduce"]["n"]
    assert report["bonus_moves_the_list"] and report["listed"] > 0.9
