"""The handler's packed compress path (flare-cpp_amd/host/gpu_codec.cc):
tests/cpp/test_pack_output.cc run with packing forced on, forced on with the
chunked pipeline, and forced off -- byte-identical outputs every way."""
import os
import subprocess
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parents[1]
BIN = REPO / "build" / "test_pack_output"
NEVER = str((1 << 64) - 1)


def _binary():
    if not BIN.exists():
        subprocess.run(["make", "-C", str(REPO), "cpptests"], check=True, capture_output=True, timeout=600)
    return BIN


def test_stats_and_threshold_parsing_cpu():
    r = subprocess.run([str(_binary()), "--cpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failures" in r.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("pack_min,chunk_bytes", [("0", None), ("0", "4096"), (NEVER, None)])
def test_packed_output_path_gpu(pack_min, chunk_bytes):
    env = dict(os.environ)
    env["FLARE_SNAPPY_GPU_PACK_MIN_BYTES"] = pack_min
    env.pop("FLARE_SNAPPY_GPU_CHUNK_BYTES", None)
    if chunk_bytes:
        env["FLARE_SNAPPY_GPU_CHUNK_BYTES"] = chunk_bytes
    r = subprocess.run([str(_binary()), "--gpu"], capture_output=True, text=True, timeout=300, env=env)
    print(r.stdout)
    print(r.stderr[-3000:])
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failures" in r.stdout
