"""GPU: the drop-in evaluators over a process group, on the one GPU of the box.  Every test starts fresh child processes
(tests/sharded_eval_child.py, or the CLIs under `python -m torch.distributed.run`) with a time limit; a child that fails ends the test.

  world 1 through RCCL   dist.force_collectives(): the exact collectives of an N-GPU run on device tensors; metrics and the
                         embeddings' bits equal the same calls without a process group;
  two ranks over gloo    KEMR_DIST_BACKEND=gloo, KEMR_LOCAL_DEVICE=0 (RCCL refuses two ranks on one device): the sharded metrics equal
                         the single-process functions on the gathered embeddings, exactly; the uuids partition the dataset in order;
                         each rank's embeddings against one whole-dataset encode_dataset call of the same rows;
  the CLIs               evaluator and evaluator_baseline under torchrun with two ranks: one results file, one log.

No N > 1 RCCL run is made here (one GPU)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "sharded_eval_child.py")
N = 37

pytestmark = pytest.mark.gpu


def _env(**extra):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"), MASTER_ADDR="127.0.0.1")
    for key in ("KEMR_DIST_BACKEND", "KEMR_LOCAL_DEVICE", "KEMR_EVAL_SHARDED", "KEMR_DIST_FORCE_COLLECTIVES", "RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(key, None)
    env.update(extra)
    return env


def _run(cmd, env, timeout=300):
    proc = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, env=env, cwd=ROOT)
    assert proc.returncode == 0, (proc.returncode, proc.stdout[-2000:], proc.stderr[-4000:])
    return proc


def _torchrun(nproc, *rest):
    return [sys.executable, "-m", "torch.distributed.run", "--standalone", "--nproc-per-node", str(nproc), *rest]


GLOO_ONE_GPU = dict(KEMR_DIST_BACKEND="gloo", KEMR_LOCAL_DEVICE="0")


def test_world_one_through_rccl_equals_no_process_group(device, tmp_path):
    out = tmp_path / "world1.json"
    _run([sys.executable, CHILD, "world1", str(out)], _env())
    report = json.loads(out.read_text())
    assert report["backend"] == "nccl"
    assert all(report["metrics_equal"].values()), report["metrics_equal"]
    assert report["emb_bits_equal"] == [True, True, True] and report["uuids_equal"]
    # the collectives did run: the query gathers and the two reductions of every ranks() call, the uuids once per evaluation
    assert report["calls"]["all_gather_into_tensor"] >= 20 and report["calls"]["all_reduce"] >= 40, report["calls"]
    assert report["calls"]["all_gather_object"] == 1
    assert set(report["fusion"]) == {"R@1", "R@5", "R@10", "R@20", "MRR", "Mean_Rank"} and len(report["clip"]) == 18


def test_two_ranks_on_one_gpu_equal_the_gathered_single_process_metrics(device, tmp_path):
    """Ranks are a pure function of the embeddings' bits and per-pair score bits do not depend on the shard (include/kemr.h), so
    the sharded metrics EQUAL metrics.compute_all_retrieval_metrics of the gathered embeddings.  First measurement (one MI355X): each
    rank's embeddings (19 / 18 items per call) have the bits of the whole-dataset call's rows (37 items per call) in all three sets,
    max 1 - cos 3.3e-16 in float64 -- bit equality is what is asserted; no cosine bound was needed."""
    _run(_torchrun(2, CHILD, "ranks", str(tmp_path)), _env(**GLOO_ONE_GPU))
    reports = [json.loads((tmp_path / f"rank{r}.json").read_text()) for r in range(2)]
    r0 = reports[0]
    for rep in reports:
        assert rep["world"] == 2
        assert rep["clip"] == r0["want_clip"], (rep["rank"], rep["clip"], r0["want_clip"])
        assert rep["baseline"] == r0["want_baseline"], rep["rank"]
        assert rep["fusion"] == r0["want_fusion"], rep["rank"]                        # dense linear head: kemr_rank_dense_shard per shard
        assert rep["fusion_gated"] == r0["want_fusion_gated"], rep["rank"]            # gates of the padded local rows, all-gathered
        assert rep["fusion_rerank"] == r0["want_fusion_rerank"], rep["rank"]          # ShardedGallery.rerank, one pad row on rank 1
        lo, hi = rep["lo_hi"]
        assert rep["uuids"] == rep["whole_uuids"][lo:hi]
        print(f"rank {rep['rank']}: bits equal (image, query, target) {rep['bits_equal']}, max 1 - cos {rep['max_1mcos']}")
        # each rank's embeddings are the rows of one whole-dataset call, bit for bit (evaluators.encode_dataset: "Rows are
        # independent, so the embeddings do not depend on the grouping")
        assert rep["bits_equal"] == [True, True, True], (rep["rank"], rep["bits_equal"], rep["max_1mcos"])
    assert [r["lo_hi"] for r in reports] == [[0, 19], [19, 37]]
    assert reports[0]["uuids"] + reports[1]["uuids"] == r0["whole_uuids"] and len(r0["whole_uuids"]) == N
    assert len(r0["want_clip"]) == 18


@pytest.mark.parametrize("module", ["src.clip.eval.evaluator", "src.clip.eval.evaluator_baseline"])
def test_cli_under_torchrun_writes_one_results_file(device, tmp_path, module):
    args = ["--model_name", "ViT-B/32", "--synthetic", str(N), "--num_workers", "0", "--batch_size", "16"]
    single, sharded = tmp_path / "single", tmp_path / "sharded"
    import importlib
    importlib.import_module(module).main([*args, "--output_file", str(single / "results.json")])      # no process group: in this process
    _run(_torchrun(2, "-m", module, *args, "--output_file", str(sharded / "results.json")), _env(**GLOO_ONE_GPU))
    assert sorted(os.listdir(sharded)) == ["evaluation.log", "results.json"]              # exactly one results file and one log
    one, two = json.loads((single / "results.json").read_text()), json.loads((sharded / "results.json").read_text())
    assert two["world_size"] == 2 and two["items_per_rank"] == [19, 18] and two["num_samples"] == N
    assert "world_size" not in one and one["num_samples"] == N
    assert sorted(two["metrics"]) == sorted(one["metrics"])
    m = two["metrics"]
    prefixes = [""] if module.endswith("baseline") else ["T2I_", "I2T_", "T2T_"]
    for p in prefixes:
        recalls = [m[f"{p}R@{k}"] for k in (1, 5, 10, 20)]
        assert recalls == sorted(recalls) and 0.0 <= recalls[0] and recalls[-1] <= 100.0    # Recall@K is monotone in K
        assert 1.0 <= m[f"{p}Mean_Rank"] <= N
    log = (sharded / "evaluation.log").read_text()
    assert "EVALUATION RESULTS" in log and "Results saved" in log
