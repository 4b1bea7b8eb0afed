"""The Snappy encoder's launch arithmetic (csrc/encode_v3_plan.h: the route,
workspace regions, the wave encoder's threshold and geometry, the lanes
launched, grid sizes and the option range checks) on the CPU.
tests/cpp/test_encode_plan.cc includes only that header; it is built as a
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
    exe = tmp_path_factory.mktemp("encode_plan") / "test_encode_plan"
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-I", str(REPO / "flare-cpp_amd" / "csrc"),
                        str(REPO / "tests" / "cpp" / "test_encode_plan.cc"), "-o", str(exe)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return exe


def _run(exe, part):
    r = subprocess.run([str(exe), part], capture_output=True, text=True, timeout=300,
                       env={"ASAN_OPTIONS": "detect_leaks=0"})
    print(r.stdout[-4000:])
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])


def test_plan_matches_recorded_values(plan_test):
    """Fourteen (n, max_in_len, workspace) points at default options against
    the values of the batch call's and the launch's expressions before they
    moved into encode_v3_plan."""
    _run(plan_test, "table")


def test_plan_regions_are_disjoint_aligned_and_grids_nonempty(plan_test):
    _run(plan_test, "layout")


def test_plan_option_range_checks(plan_test):
    _run(plan_test, "options")
