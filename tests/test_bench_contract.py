"""bench.py's output contract (the driver parses the last stdout line): one JSON object with the agreed keys; with --full
also the roofline and cpu_baseline objects, and the BASELINE config in `config`; --dump-outputs writes the last timed step's
embeddings."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE_KEYS = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                 "dtype", "data", "config"}
KEYS = HEADLINE_KEYS | {"roofline", "cpu_baseline"}
DUMPS = ("image_embeddings", "text_embeddings")


def _bench(*args):
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "1"] + list(args),
                         capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-2000:]
    return json.loads(res.stdout.strip().splitlines()[-1])


def test_bench_cli_declares_the_contract_flags():
    src = open(os.path.join(ROOT, "bench.py")).read()
    for flag in ("--gpus", "--steps", "--warmup", "--full", "--dump-outputs"):
        assert flag in src


def test_dump_outputs_writes_float32_and_samples_the_same_rows_under_the_limit(tmp_path):
    import bench
    a = torch.arange(400 * 8, dtype=torch.float64).reshape(400, 8)
    b = -torch.arange(400 * 16, dtype=torch.bfloat16).reshape(400, 16)
    bench.dump_outputs(str(tmp_path / "all"), {"a": a, "b": b})
    ga, gb = np.load(tmp_path / "all" / "a.npy"), np.load(tmp_path / "all" / "b.npy")
    assert ga.dtype == np.float32 and gb.dtype == np.float32 and ga.shape == (400, 8) and gb.shape == (400, 16)
    assert np.array_equal(ga, a.float().numpy()) and np.array_equal(gb, b.float().numpy())
    limit = 4096 * 2 + 4 * 24 * 100                                    # room for 100 of the 400 rows of both
    for run in ("s1", "s2"):
        bench.dump_outputs(str(tmp_path / run), {"a": a, "b": b}, limit=limit)
    sa, sb = np.load(tmp_path / "s1" / "a.npy"), np.load(tmp_path / "s1" / "b.npy")
    assert sa.shape == (100, 8) and sb.shape == (100, 16)
    assert sum(os.path.getsize(tmp_path / "s1" / f) for f in ("a.npy", "b.npy")) <= limit
    rows = (sa[:, 0] / 8).astype(np.int64)                              # a's row i starts with 8 i
    assert np.all(np.diff(rows) > 0) and np.array_equal(sb, b.float().numpy()[rows])      # sorted, and the same rows in every array
    assert np.array_equal(sa, np.load(tmp_path / "s2" / "a.npy"))     # seeded: the same sample every run


@pytest.fixture(scope="module")
def full_run(device, tmp_path_factory):
    out = tmp_path_factory.mktemp("bench_full")
    return _bench("--full", "--no-extras", "--dump-outputs", str(out)), out


@pytest.mark.gpu
def test_bench_line_contract(full_run):
    d, _ = full_run
    assert KEYS <= set(d), KEYS - set(d)
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1 and d["higher_is_better"] is True
    assert d["scaling"] == "weak" and d["vs_baseline"] is None and d["dtype"] == "bf16" and d["data"] == "synthetic"
    assert d["unit"] == "items/s" and d["value"] > 1000 and d["ms_per_step"] > 0
    assert "workload" in d["config"] and "ViT-L/14" in d["config"]["workload"]
    r = d["roofline"]
    assert set(r) >= {"bound", "achieved", "peak", "unit", "frac", "traffic"} and r["bound"] == "mfma" and r["unit"] == "TFLOP/s"
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9 and 0.2 < r["frac"] < 1.0
    assert "traffic_source" in r and (r["traffic"] is None or r["traffic_source"]["commit"])
    c = d["cpu_baseline"]
    assert set(c) >= {"value", "unit", "cores", "kind", "sample"} and c["kind"] == "port" and c["value"] > 0 and c["cores"] >= 1
    # the bench checks its own outputs against the oracle: images AND texts, rows from the start, middle and end of the batch
    assert c["gpu_vs_oracle_min_cosine_images"] > 1 - 1e-3 and c["gpu_vs_oracle_min_cosine_texts"] > 1 - 1e-3
    rs = d["roofline_sim"]
    assert rs["bound"] == "mfma" and abs(rs["frac"] - rs["achieved"] / rs["peak"]) < 1e-9 and rs["ms"] > 0
    assert {"q1024_bf16", "q43000_bf16", "q43000_bf16_rank_only", "q43000_bf16_c3_fused_t2i_t2t"} <= set(d["sim_top10"])
    assert d["config"]["rccl_ranks"] == 1 and d["config"]["shard_bounds"] == [[0, 43000]] and d["config"]["items_timed"] == 2 * 765
    # images + texts of all ranks / time: 255 gallery items per step = 255 images + 510 texts
    assert abs(d["value"] - 765 / (d["ms_per_step"] / 1e3)) / d["value"] < 1e-6
    assert abs(d["value"] - (d["images_per_s"] + d["texts_per_s"])) / d["value"] < 1e-9


@pytest.mark.gpu
def test_plain_bench_line_and_dumped_outputs(full_run, tmp_path):
    """A plain run times the headline steps only; what it dumps is what the same steps of a --full run computed."""
    d = _bench("--dump-outputs", str(tmp_path))
    assert HEADLINE_KEYS <= set(d), HEADLINE_KEYS - set(d)
    assert not {"roofline", "cpu_baseline", "sim_top10", "pipeline", "reference_arithmetic"} & set(d)
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1 and d["higher_is_better"] is True and d["dtype"] == "bf16"
    assert d["unit"] == "items/s" and d["value"] > 1000 and abs(d["value"] - 765 / (d["ms_per_step"] / 1e3)) / d["value"] < 1e-6
    full_dir = full_run[1]
    assert sum(os.path.getsize(tmp_path / f"{n}.npy") for n in DUMPS) <= 64 << 20
    for n in DUMPS:
        got, ref = np.load(tmp_path / f"{n}.npy"), np.load(full_dir / f"{n}.npy")
        assert got.dtype == np.float32 and got.ndim == 2 and got.shape[1] == 768 and np.isfinite(got).all(), n
        assert np.allclose(np.linalg.norm(got, axis=1), 1.0, atol=1e-3), n                # L2-normalised embeddings
        assert got.shape == ref.shape and np.abs(got - ref).max() <= 1e-6, n
    assert np.load(tmp_path / "image_embeddings.npy").shape[0] == 255
