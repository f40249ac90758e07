"""bench.py's launch contract: a rank count that was not run never produces a line."""

import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def run_bench(args, env_extra=None, timeout=600):
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    env.update(env_extra or {})
    return subprocess.run([sys.executable, BENCH] + args, env=env, capture_output=True, text=True, timeout=timeout)


def test_more_gpus_than_the_node_has_is_an_error_not_a_one_gpu_line():
    """`python bench.py --gpus 64` outside a launcher starts the ranks itself -- after checking that the
    node has that many GPUs.  Round 1 printed an n_gpus = 1 line here."""
    r = run_bench(["--gpus", "64", "--steps", "1", "--warmup", "0"])
    assert r.returncode != 0
    assert "--gpus 64" in r.stderr and "GPU(s)" in r.stderr
    assert r.stdout.strip() == ""


def test_rank_count_from_the_launcher_must_match():
    r = run_bench(["--gpus", "2", "--steps", "1", "--warmup", "0"], {"WORLD_SIZE": "1", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode != 0
    assert "--gpus 2 but 1 rank(s)" in r.stderr
    assert r.stdout.strip() == ""


@pytest.mark.gpu
def test_two_ranks_on_a_one_gpu_box_fail_loudly():
    import torch

    if torch.cuda.device_count() >= 2:
        pytest.skip("this box has two GPUs")
    r = run_bench(["--gpus", "2", "--steps", "1", "--warmup", "0"])
    assert r.returncode != 0 and r.stdout.strip() == ""


@pytest.mark.gpu
def test_default_line_is_strong_scaling_and_verified():
    """A small matrix through the default workload: the line names the whole-matrix (strong) split and carries
    the self-check of the last step's results."""
    r = run_bench(["--variants", "20000", "--samples", "50000", "--steps", "2", "--warmup", "1", "--cpu-seconds", "0",
                   "--full"])
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["n_gpus"] == 1 and line["scaling"] == "strong" and line["verified"] is True
    assert line["roofline"]["bound"] == "hbm" and line["roofline"]["frac"] > 0


@pytest.mark.gpu
def test_all_configs_ride_the_default_line():
    """--configs all on a small matrix: BASELINE configs 2-5 next to the freq headline, each verified, and the
    table-function section."""
    r = run_bench(["--variants", "30000", "--samples", "20000", "--steps", "2", "--warmup", "1", "--cpu-seconds", "0",
                   "--configs", "all", "--config-steps", "1", "--full"])
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["metric"] == "plink_freq genotypes/s" and line["verified"] is True
    cfg = line["configs"]
    assert set(cfg) == {"fused", "unpack", "score16", "score1", "pca"}
    assert all(c["verified"] is True and c["frac"] > 0 and c["kernel_ms_avg"] > 0 for c in cfg.values())
    assert cfg["unpack"]["roofline"]["store_ceiling"]["GB/s"] > 0
    assert "algorithmic_flops_frac_of_fp64_peak" in cfg["score16"]["roofline"]
    sql = line["sql"]
    assert sql.pop("verified") is True
    assert len(sql) == 4 and all(v["rows"] in (30000, 20000) and v["scan_ms"] > 0 for v in sql.values())


@pytest.mark.gpu
@pytest.mark.parametrize("workload", ["freq", "score", "pca"])
def test_two_rank_run_rehearsed_on_one_gpu(workload):
    """The N-rank logic of bench.py (shard ranges, the reduction of per-sample partials, max-over-ranks timing, the
    verification vote, rank 0's line) under the driver's own launcher with two ranks -- both on GPU 0 and over gloo,
    since this box has one GPU and RCCL refuses two ranks on one device.  The line says it is a rehearsal."""
    import socket

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, PGH_BENCH_ONE_GPU_REHEARSAL="1")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    shape = {"freq": ["--variants", "40000", "--samples", "30000"],
             "score": ["--workload", "score", "--variants", "20000", "--samples", "20000"],
             "pca": ["--workload", "pca", "--variants", "6000", "--samples", "5000"]}[workload]
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", str(port), BENCH, "--gpus", "2", "--steps", "2",
                        "--warmup", "1", "--cpu-seconds", "0", "--full"] + shape, env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1  # rank 0 alone prints
    line = json.loads(lines[0])
    assert line["n_gpus"] == 2 and line["verified"] is True and line["value"] > 0
    assert "REHEARSAL" in line["config"]["workload"]
    assert line["cpu_baseline"] is None and "configs" not in line  # N = 1 only


def test_configs_all_without_full_is_an_error():
    """The extra configs are part of --full: asking for them in a plain run is refused before any GPU work."""
    r = run_bench(["--configs", "all", "--steps", "1", "--warmup", "0"])
    assert r.returncode != 0 and "--full" in r.stderr and r.stdout.strip() == ""
    r = run_bench(["--steps", "0"])
    assert r.returncode != 0 and "--steps" in r.stderr and r.stdout.strip() == ""


def test_dumped_outputs_are_float_and_stay_under_64_mb(tmp_path):
    """--dump-outputs' writer: integers exact in float32 are written as float32, others as float64; over the cap every
    output keeps the same fixed, seeded sample of its rows, and the indices of those rows are written next to it."""
    import numpy as np

    import bench  # the repository root is on sys.path (conftest.py)

    n = 500_000
    rng = np.random.default_rng(1)
    outs = {"score_sum": rng.standard_normal((n, 16)), "allele_ct": np.full(n, 2_000_000, dtype=np.int32),
            "dosage_sum": rng.standard_normal(n), "wide": np.array([1 << 40, 3], dtype=np.uint64)}
    limit = 64 << 20
    for d in ("a", "b"):
        bench.dump_outputs(np, str(tmp_path / d), outs, limit)
    files = sorted(os.listdir(tmp_path / "a"))
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= limit
    for f in files:
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b)
    rows = np.load(tmp_path / "a" / "score_sum.rows.npy").astype(np.int64)
    assert 0 < len(rows) < n and np.array_equal(np.load(tmp_path / "a" / "score_sum.npy"), outs["score_sum"][rows])
    assert np.load(tmp_path / "a" / "allele_ct.npy").dtype == np.float32
    assert np.load(tmp_path / "a" / "wide.npy").dtype == np.float64

    bench.dump_outputs(np, str(tmp_path / "small"), {"counts": np.arange(12, dtype=np.int32).reshape(3, 4)}, limit)
    assert sorted(os.listdir(tmp_path / "small")) == ["counts.npy"]
    assert np.array_equal(np.load(tmp_path / "small" / "counts.npy"), np.arange(12).reshape(3, 4))


DUMP_SHAPES = {
    "freq": ["--variants", "6000", "--samples", "5000"],
    "fused": ["--variants", "6000", "--samples", "5000"],
    "unpack": ["--variants", "6000", "--samples", "5000"],
    "score": ["--variants", "6000", "--samples", "5000", "--score-cols", "4"],
    "pca": ["--variants", "6000", "--samples", "5000"],
    "ld": ["--variants", "6000", "--samples", "5000", "--ld-variants", "2000"],
    "samplecounts": ["--variants", "6000", "--samples", "5000"],
    "missingsample": ["--variants", "6000", "--samples", "5000"],
    "dosagefreq": ["--variants", "6000", "--samples", "5000"],
    "dosagescore": ["--variants", "6000", "--samples", "5000"],
}
DUMP_NAMES = {
    "freq": {"counts", "alt_freq", "obs_ct"},
    "fused": {"counts", "alt_freq", "obs_ct", "hwe_lnp", "sample_missing"},
    "unpack": {"genotypes", "valid", "variant"},
    "score": {"score_sum", "dosage_sum", "allele_ct"},
    "pca": {"eigenvalues", "eigenvectors"},
    "ld": {"pair_sums"},
    "samplecounts": {"sample_class_counts"},
    "missingsample": {"sample_missing"},
    "dosagefreq": {"dosage_sums"},
    "dosagescore": {"score_sum", "dosage_sum", "allele_ct"},
}


@pytest.mark.gpu
@pytest.mark.parametrize("workload", sorted(DUMP_SHAPES))
def test_plain_run_is_lean_and_dumps_its_last_step(workload, tmp_path):
    """A plain run (no --full) times and reports, nothing more: no checks, no CPU baseline, no extra configs; with
    --dump-outputs it writes every result the workload hands its caller."""
    import numpy as np

    out = tmp_path / "out"
    r = run_bench(["--workload", workload, "--steps", "2", "--warmup", "1", "--dump-outputs", str(out)]
                  + DUMP_SHAPES[workload])
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["full"] is False and line["verified"] is None and line["cpu_baseline"] is None
    assert "configs" not in line and "sql" not in line and "store_ceiling" not in line["roofline"]
    assert line["steps"] == 2 and line["ms_per_step"] > 0 and line["value"] > 0
    got = {f[:-len(".npy")]: np.load(out / f) for f in os.listdir(out)}
    assert set(got) == DUMP_NAMES[workload]
    assert all(a.dtype in (np.float32, np.float64) and a.size > 0 for a in got.values())
    if workload == "freq":
        n = 5000
        c = got["counts"].astype(np.int64)
        assert c.shape == (6000, 4) and (c.sum(axis=1) == n).all()
        assert np.array_equal(got["obs_ct"], 2 * c[:, :3].sum(axis=1))
        assert np.array_equal(got["alt_freq"], (c[:, 1] + 2 * c[:, 2]) / (2.0 * c[:, :3].sum(axis=1)))


@pytest.mark.gpu
def test_dumped_outputs_repeat_from_run_to_run(tmp_path):
    """The same arguments give the same inputs and so the same outputs: what lets two builds be compared."""
    import numpy as np

    for d in ("a", "b"):
        r = run_bench(["--steps", "1", "--warmup", "0", "--dump-outputs", str(tmp_path / d), "--variants", "20000",
                       "--samples", "30000"])
        assert r.returncode == 0, r.stderr[-2000:]
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b")) == ["alt_freq.npy", "counts.npy", "obs_ct.npy"]
    assert all(np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)) for f in names)
