"""The execution pass's two instances as csrc/decode_v4_plan.h sizes them (the
folded one: 16-bit tag ring and 4 KiB window; the general one: 32-bit ring and
3 KiB window): each instance's kept history over option exec_keep's whole
range, and the LDS arithmetic -- 5 KiB + 32 per wave either way, and per block
no more than before.  tests/cpp/test_decode_plan_windows.cc includes only that
header; it is built as a stand-alone program with AddressSanitizer and UBSan
and run as a subprocess."""
import shutil
import subprocess
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module")
def windows_test(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "g++ not found"
    exe = tmp_path_factory.mktemp("decode_plan_windows") / "test_decode_plan_windows"
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-I", str(REPO / "flare-cpp_amd" / "csrc"),
                        str(REPO / "tests" / "cpp" / "test_decode_plan_windows.cc"), "-o", str(exe)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return exe


def _run(exe, part):
    r = subprocess.run([str(exe), part], capture_output=True, text=True, timeout=300,
                       env={"ASAN_OPTIONS": "detect_leaks=0"})
    print(r.stdout[-4000:])
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])


def test_kept_history_per_instance_over_the_option_range(windows_test):
    _run(windows_test, "keep")


def test_lds_per_wave_and_per_block(windows_test):
    _run(windows_test, "lds")
