"""bench.py's contract on the GPU (the driver parses its one JSON line every round): the
default workload at a reduced row count, configs[0] through the parquet store (`--config c1`)
and the N > 1 path (`--gpus 2 --comm host`: spawn, sharding, the library's exchange and the
root merge, the spot-check over the whole corpus) with two rank processes on the one GPU.
Those runs are `--full` ones (the side measurements and checks they read); the plain run, the
headline line alone, and `--dump-outputs` are checked against them.
Each run is a child process; nothing here re-executes a GPU-initialised process."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAIN = ["--steps", "3", "--warmup", "1", "--settle-ms", "0"]
# (the side measurements and checks these tests read run under --full)
QUICK = [*PLAIN, "--full", "--p50-iters", "2", "--no-cpu-baseline"]
SMALL = ["--rows", "300000"]  # the default workload at a reduced row count (plain and --full runs)


def _bench(*args, timeout=240):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], cwd=ROOT, capture_output=True,
                       text=True, timeout=timeout)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout  # exactly one JSON line on stdout
    return json.loads(lines[0])


def _common(d, n_gpus, steps=3):
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
                "scaling", "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert key in d, key
    assert d["n_gpus"] == n_gpus and d["steps"] == steps and d["warmup"] == 1
    assert d["value"] > 0 and d["ms_per_step"] > 0 and d["higher_is_better"] is True
    assert d["unit"] == "queries/s" and d["dtype"] == "f32" and d["scaling"] in ("strong", "weak")
    assert "workload" in d["config"]


def _dump(path):
    return {n: np.load(os.path.join(path, n + ".npy")) for n in ("indices", "distances", "counts")}


@pytest.fixture(scope="module")
def full_small(gpu, tmp_path_factory):
    """One --full run of the reduced default workload, its outputs dumped (shared, read-only)."""
    out = str(tmp_path_factory.mktemp("bench_full") / "out")
    d = _bench(*SMALL, "--no-configs1", "--verify", "2", "--dump-outputs", out, *QUICK)
    return d, _dump(out)


def test_bench_default_workload_small(full_small):
    d, _ = full_small
    _common(d, 1)
    assert d["full"] is True
    rf = d["roofline"]
    assert rf["bound"] == "mfma" and rf["unit"] == "TOP/s" and rf["peak"] == 5000.0
    assert 0 < rf["frac"] < 1 and abs(rf["achieved"] / rf["peak"] - rf["frac"]) < 1e-3
    assert rf["algorithmic_ops_per_launch"] == 2 * 1000 * 300000 * 768
    assert d["cpu_baseline"] is None  # --no-cpu-baseline
    sc = d["parity_spot_check"]
    assert sc["indices_equal"] and sc["distance_bits_equal"]
    assert d["fallback_queries_per_step_rank0"] == 0
    assert d["self_query_rank1"] is True


def test_bench_plain_run_headline_and_outputs(full_small, tmp_path):
    """A plain run (no --full) times the steps and prints the headline line alone: none of the side
    measurements or checks.  --dump-outputs writes the last timed step's lists as float .npy files,
    and the plain and the --full run of the same arguments compute the same outputs, bit for bit
    (the --full run's are spot-checked against the oracle)."""
    out = str(tmp_path / "out")
    d = _bench(*SMALL, "--dump-outputs", out, *PLAIN)
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in d, key
    assert d["steps"] == 3 and d["warmup"] == 1 and d["full"] is False
    assert d["value"] > 0 and d["ms_per_step"] > 0 and d["unit"] == "queries/s" and d["dtype"] == "f32"
    assert abs(d["value"] - 1000 / (d["ms_per_step"] * 1e-3)) <= 1e-3 * d["value"]
    for key in ("roofline", "cpu_baseline", "parity_spot_check", "p50_ms", "configs1", "kernels_ms_per_step_rank0",
                "local_search_ms_per_step", "roofline_p50"):
        assert key not in d, key
    assert sorted(os.listdir(out)) == ["counts.npy", "distances.npy", "indices.npy"]
    got, (dfull, want) = _dump(out), full_small
    assert got["indices"].dtype == np.float64 and got["indices"].shape == (1000, 10)
    assert got["distances"].dtype == np.float32 and got["distances"].shape == (1000, 10)
    assert got["counts"].dtype == np.float64 and np.array_equal(got["counts"], np.full(1000, 10.0))
    assert got["indices"][0, 0] == 0 and got["distances"][0, 0] == 0.0  # the self-query
    assert np.all(np.diff(got["distances"], axis=1) >= 0)
    assert np.all((got["indices"] >= 0) & (got["indices"] < 300000))
    assert d["config"] == dfull["config"] and d["metric"] == dfull["metric"]
    for n in got:
        assert got[n].tobytes() == want[n].tobytes(), n


def test_bench_configs0_plain_run(gpu, tmp_path):
    out = str(tmp_path / "out")
    d = _bench("--config", "c1", "--dump-outputs", out, *PLAIN)
    assert d["value"] > 0 and d["ms_per_step"] > 0 and d["steps"] == 3 and d["full"] is False
    assert "parity_all_queries" not in d and "cpu_baseline" not in d and "p50_ms" not in d
    got = _dump(out)
    assert got["indices"].shape == (32, 10) and got["distances"].dtype == np.float32
    assert got["indices"][0, 0] == 0 and got["distances"][0, 0] == 0.0


def test_bench_configs0_parquet_store(gpu):
    d = _bench("--config", "c1", *QUICK)
    _common(d, 1)
    p = d["parity_all_queries"]
    assert p["queries"] == 32 and p["indices_equal"] and p["distance_bits_equal"]
    assert d["parquet_load_ms"] > 0


def test_bench_two_ranks_host_transport(gpu):
    d = _bench("--gpus", "2", "--comm", "host", "--rows", "200000", "--verify", "2", *QUICK)
    _common(d, 2)
    assert "HOST all-gather" in d["config"]["parallelism"]
    assert d["exchange_ms_per_step"] is not None
    sc = d["parity_spot_check"]
    assert sc["indices_equal"] and sc["distance_bits_equal"]


def test_bench_loopback_rank_step(gpu):
    """bench.py --comm loopback --gpus 4: a recorded 4-rank host-transport run of the batch, then ONE
    process timing rank 0's step with every all-gather emulated on the device and replayed from
    that recording; its result is the 4-rank run's global top-k (spot-checked over the whole
    corpus), every all-gather of the timed searches replayed."""
    d = _bench("--comm", "loopback", "--gpus", "4", "--rows", "400000", "--verify", "2", *QUICK)
    _common(d, 1)
    lb = d["loopback"]
    assert lb["ranks"] == 4 and lb["recorded_calls_per_search"] == 3
    assert lb["missed_allgathers"] == 0 and lb["replayed_allgathers"] >= 3 * 3
    assert d["config"]["rows_per_gpu_rank0"] == 100000 and "loopback" in d["config"]["parallelism"]
    assert d["candidates_per_query"] == 0  # the global-threshold path
    sc = d["parity_spot_check"]
    assert sc["rows"] == 400000 and sc["indices_equal"] and sc["distance_bits_equal"]


def _failing_run(extra=(), timeout=60):
    """bench.py --gpus 2 with rank 1 failing on purpose (BSR_BENCH_FAIL_RANK): the launcher must
    end rank 0 -- blocked in a collective with the dead rank -- and report, within the time."""
    import time
    env = dict(os.environ, BSR_BENCH_FAIL_RANK="1")
    t0 = time.monotonic()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--comm", "host",
                        "--rows", "200000", *QUICK, *extra], cwd=ROOT, capture_output=True, text=True,
                       timeout=timeout, env=env)
    dt = time.monotonic() - t0
    assert r.returncode != 0 and dt < timeout, (r.returncode, dt)
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    d = json.loads(lines[-1])
    assert d["value"] is None and d["failed_rank"] == 1 and "rank 1 exited with status 3" in d["error"]
    assert "BSR_BENCH_FAIL_RANK" in d["stderr_tail"]
    return d


def test_bench_failing_rank_fails_fast(gpu):
    _failing_run()


def _two_gpus():
    try:
        import torch  # (counting devices does not initialise the GPU)
        return torch.cuda.device_count() >= 2
    except Exception:
        return False


# The RCCL transport needs one device per rank (RCCL refuses two ranks on one device): these run
# on a box with two or more GPUs and are skipped on the one-GPU box (the driver's 8-GPU scale run
# exercises the same path through bench.py --gpus N).
@pytest.mark.skipif(not _two_gpus(), reason="RCCL: one device per rank, needs >= 2 GPUs")
def test_bench_two_ranks_rccl(gpu):
    d = _bench("--gpus", "2", "--rows", "200000", "--verify", "2", *QUICK)
    _common(d, 2)
    assert "HOST" not in d["config"]["parallelism"]
    sc = d["parity_spot_check"]
    assert sc["indices_equal"] and sc["distance_bits_equal"]


@pytest.mark.skipif(not _two_gpus(), reason="RCCL: one device per rank, needs >= 2 GPUs")
def test_bench_failing_rank_fails_fast_rccl(gpu):
    import time
    env = dict(os.environ, BSR_BENCH_FAIL_RANK="1")
    t0 = time.monotonic()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--rows", "200000", *QUICK],
                       cwd=ROOT, capture_output=True, text=True, timeout=90, env=env)
    assert r.returncode != 0 and time.monotonic() - t0 < 90
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.strip()][-1])
    assert d["value"] is None and d["failed_rank"] == 1
