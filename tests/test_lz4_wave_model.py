"""The CPU model of the LZ4 wave encoder (tools/l4wenc_model.cc: the greedy
parse run 64 probes at a time, which csrc/lz4_encode_wave.hip is written
from) against oracle/lz4_oracle.c, block for block.  The model is built as a
stand-alone program with AddressSanitizer and UBSan and run as a subprocess."""
import json
import shutil
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

from bind import Lz4Oracle
from gen_inputs import build_input
from lz4_wave_cases import boundary_family

REPO = Path(__file__).resolve().parents[1]
VEC = json.loads((REPO / "tests" / "golden" / "lz4_vectors.json").read_text())


@pytest.fixture(scope="module")
def o():
    return Lz4Oracle()


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "g++ not found"
    exe = tmp_path_factory.mktemp("l4wenc") / "l4wenc_model"
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        str(REPO / "tools" / "l4wenc_model.cc"), "-o", str(exe)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return exe


def _run(exe, xs, tmp_path, tag):
    fin, fout = tmp_path / f"{tag}.in", tmp_path / f"{tag}.out"
    fin.write_bytes(b"".join(struct.pack("<I", len(x)) + x for x in xs))
    r = subprocess.run([str(exe), str(fin), str(fout)], capture_output=True, text=True, timeout=600,
                       env={"ASAN_OPTIONS": "detect_leaks=0"})
    assert r.returncode == 0, r.stderr[-3000:]
    out = fout.read_bytes()
    blocks, p = [], 0
    for _ in xs:
        (n,) = struct.unpack_from("<I", out, p)
        blocks.append(out[p + 4:p + 4 + n])
        p += 4 + n
    assert p == len(out)
    return blocks


def test_model_equals_oracle_on_fixtures_and_random(model, o, tmp_path):
    names = [v["name"] for v in VEC["compress"] if v["input_len"] <= 300000]
    xs = [build_input(v) for v in VEC["compress"] if v["input_len"] <= 300000]
    rng = np.random.default_rng(29)
    for t in range(150):  # sizes and alphabets of test_gpu_block_codec_on_host_asan
        n = int(rng.choice([rng.integers(0, 40), rng.integers(0, 5000), rng.integers(60000, 70000)]))
        xs.append(rng.integers(0, int(rng.choice([1, 2, 4, 256])), n, dtype=np.uint8).tobytes())
        names.append(f"random-{t}")
    for name, x, b in zip(names, xs, _run(model, xs, tmp_path, "a")):
        assert b == o.compress_block(x), (name, len(x))


def test_model_equals_oracle_on_boundary_family(model, o, tmp_path):
    fam = boundary_family()
    xs = [x for _, x in fam]
    for (name, x), b in zip(fam, _run(model, xs, tmp_path, "b")):
        assert b == o.compress_block(x), (name, len(x))
