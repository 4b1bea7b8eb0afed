"""The host runtime's device-path counters (fsh_device_path_stats,
flare-cpp_amd/host/gpu_codec.cc): tests/cpp/test_path_report.cc on the host
alone, and on the GPU with a batch on the fast path and one forced into the
encoder's whole-message fallback."""
import subprocess
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parents[1]
BIN = REPO / "build" / "test_path_report"


def _binary():
    if not BIN.exists():
        subprocess.run(["make", "-C", str(REPO), "cpptests"], check=True, capture_output=True, timeout=600)
    return BIN


def test_device_path_stats_cpu():
    r = subprocess.run([str(_binary()), "--cpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failures" in r.stdout


@pytest.mark.gpu
def test_device_path_stats_gpu():
    r = subprocess.run([str(_binary()), "--gpu"], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    print(r.stderr[-3000:])
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failures" in r.stdout
