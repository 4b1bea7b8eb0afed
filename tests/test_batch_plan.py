"""The host runtime's batch plan (host/batch_plan.h: which bodies a device
batch takes, the slot layout, the chunk cuts, which chunks pack, the D2H
target, a packed chunk's offsets, the column views and the split of an
explicit batch across devices) on the CPU.  tests/cpp/test_batch_plan.cc
includes only that header; it is built as a stand-alone program with
AddressSanitizer and UBSan and run as a subprocess."""
import shutil
import subprocess
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module")
def plan_test(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "g++ not found"
    exe = tmp_path_factory.mktemp("batch_plan") / "test_batch_plan"
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-I", str(REPO / "flare-cpp_amd" / "host"),
                        str(REPO / "tests" / "cpp" / "test_batch_plan.cc"), "-o", str(exe)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return exe


def _run(exe, part):
    r = subprocess.run([str(exe), part], capture_output=True, text=True, timeout=300,
                       env={"ASAN_OPTIONS": "detect_leaks=0"})
    print(r.stdout[-4000:])
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])


def test_plan_matches_recorded_values(plan_test):
    """Fixed batches of all three kinds (empty bodies, header verdicts, bodies
    beyond the u32 formats, one body, every body skipped) against the values
    of Device::run's planning expressions before they moved into plan_batch."""
    _run(plan_test, "table")


def test_plan_properties_over_a_sweep(plan_test):
    """A fixed-seed sweep of batches, chunk sizes, pack thresholds and kinds
    against a brute-force restatement: disjoint aligned slots, chunks that
    partition the batch, the D2H target's tiling, the reserve sizes."""
    _run(plan_test, "properties")


def test_packed_layout_offsets(plan_test):
    _run(plan_test, "packed_layout")


def test_byte_balanced_cuts_match_shard(plan_test):
    """The split of an explicit batch across devices gives shard.py's
    byte_balanced_ranges on the size lists test_distributed.py balances."""
    _run(plan_test, "balanced")
