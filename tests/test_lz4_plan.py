"""The launch arithmetic of the LZ4 block codec and of LZ4 frames
(csrc/lz4_plan.h, csrc/lz4_frame_plan.h: workspace layouts, capacities,
routes, thresholds, grid sizes) on the CPU.  tests/cpp/test_lz4_plan.cc
includes only those headers and its recorded table; it is built as a
stand-alone program with AddressSanitizer and UBSan and run as a subprocess."""
import shutil
import subprocess
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module")
def plan_test(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "g++ not found"
    exe = tmp_path_factory.mktemp("lz4_plan") / "test_lz4_plan"
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-I", str(REPO / "flare-cpp_amd" / "csrc"),
                        str(REPO / "tests" / "cpp" / "test_lz4_plan.cc"), "-o", str(exe)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return exe


def _run(exe, part):
    r = subprocess.run([str(exe), part], capture_output=True, text=True, timeout=300,
                       env={"ASAN_OPTIONS": "detect_leaks=0"})
    print(r.stdout[-4000:])
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])


def test_plans_match_recorded_values(plan_test):
    """Workspace sizes, capacities, routes and wave thresholds against what
    the C ABI answered before the arithmetic moved into the plan headers
    (tests/cpp/lz4_plan_golden.inc, recorded by tools/lz4_plan_golden.py)."""
    _run(plan_test, "table")


def test_plan_regions_are_ascending_disjoint_and_aligned(plan_test):
    _run(plan_test, "layout")


def test_workspace_sized_for_a_total_holds_it(plan_test):
    _run(plan_test, "sizing")


def test_frame_plans_fit_the_block_codec(plan_test):
    """A frame's inner workspace is one the block decoder accepts and the
    block encoder routes as 0."""
    _run(plan_test, "contracts")


def test_plan_rules_and_grids(plan_test):
    _run(plan_test, "rules")
