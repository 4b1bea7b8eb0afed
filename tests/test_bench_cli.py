"""bench.py's command line on the CPU: a plain run times the steps and prints
the headline line only, --full adds the checks, and --dump-outputs writes the
last step's outputs reproducibly.  One rank of bench.py runs on CPU tensors
with the oracle standing in for the HIP codec (tests/bench_cpu_rank.py); the
GPU path of the same code is tests/test_gpu_multirank.py."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import bench
import fsg

REPO = Path(__file__).resolve().parents[1]
N_MSGS = 300


def _run(extra):
    argv = ["--device", "cpu", "--gpus", "1", "--steps", "3", "--warmup", "1", "--workload", "cm-decompress",
            "--n-msgs", str(N_MSGS), *extra]
    r = subprocess.run([sys.executable, str(REPO / "tests" / "bench_cpu_rank.py"), *argv],
                       capture_output=True, text=True, timeout=120, cwd=REPO)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.fixture(scope="module")
def dumps(tmp_path_factory):
    out = []
    for k in range(2):
        d = tmp_path_factory.mktemp(f"dump{k}")
        out.append((_run(["--dump-outputs", str(d)]), d))
    return out


def test_plain_run_reports_the_timed_steps_only(dumps):
    line, _ = dumps[0]
    assert line["steps"] == 3 and line["warmup"] == 1 and line["full"] is False
    assert line["ms_per_step"] > 0 and line["value"] > 0
    assert line["unit"].startswith("GiB/s") and line["higher_is_better"] is True and line["dtype"] == "u8"
    raw = int(fsg.mixed_sizes(N_MSGS).astype(np.uint64).sum())
    assert line["config"]["raw_bytes_all_ranks"] == raw
    # value is uncompressed GiB per second of one timed step
    assert line["value"] == pytest.approx(raw / (line["ms_per_step"] / 1e3) / (1 << 30), rel=1e-2, abs=2e-3)
    for moved in ("correct", "roofline", "cpu_baseline", "encode", "end_to_end", "multi_gpu"):
        assert line[moved] is None, moved


def test_full_run_keeps_the_checks():
    line = _run(["--full", "--no-cpu-baseline", "--verify-sample", "8"])
    assert line["full"] is True
    assert line["correct"] == {"status_errors": 0, "roundtrip_ok": True, "oracle_sample_ok": True}
    assert line["roofline"]["avg_kernel_ms"] > 0


def test_dump_outputs_match_the_batch_and_repeat(dumps):
    (_, d0), (_, d1) = dumps
    names = sorted(p.name for p in d0.iterdir())
    assert names == ["out_block_sums.npy", "out_bytes.npy", "out_len.npy", "status.npy"]
    a = {n: np.load(d0 / n) for n in names}
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    sizes = fsg.mixed_sizes(N_MSGS)
    batch = fsg.make_batch(fsg.KIND_MIXED, sizes)
    assert np.array_equal(a["out_len.npy"], sizes.astype(np.float64))
    assert not a["status.npy"].any()
    # the decoded bytes are the batch's bodies: block sums over the dense output
    blk = bench.DUMP_BLOCK
    nb = batch.total // blk
    want = batch.data[:nb * blk].reshape(nb, blk).sum(axis=1, dtype=np.int64).astype(np.float64)
    assert np.array_equal(a["out_block_sums.npy"][:nb], want)
    assert a["out_block_sums.npy"].sum() == float(batch.data[:batch.total].sum(dtype=np.int64))
    k = bench.DUMP_SAMPLE
    rng = np.random.default_rng(bench.DUMP_SEED)
    pos = np.sort(rng.integers(0, batch.total, size=k)) if batch.total > k else np.arange(batch.total)
    assert np.array_equal(a["out_bytes.npy"], batch.data[pos].astype(np.float32))
    # the same arguments give the same arrays
    for n in names:
        assert np.array_equal(a[n], np.load(d1 / n)), n
