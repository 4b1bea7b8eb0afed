"""CPU tests for LZ4 frames without a content size: the frame builder of
tests/lz4f_nosize_cases.py against liblz4, the host codec's FrameDecodedLength
(host/lz4_cpu.cc, exported as fsh_cpu_lz4f_decoded_length) against the frame
oracle on every frame the GPU tests use, the host handler on such a frame, the
mutated set's composition, and FrameDecodedLength under AddressSanitizer and
UBSan in a stand-alone program (tests/cpp/lz4f_length_check.cc)."""
import ctypes
import shutil
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

import lz4f_nosize_cases as C
import lz4f_ref as R
import lz4f_sys
from bind import Lz4Oracle
from lz4f_cases import load

REPO = Path(__file__).resolve().parent.parent
VEC = load()


@pytest.fixture(scope="module")
def o():
    return Lz4Oracle()


@pytest.fixture(scope="module")
def host():
    lib = REPO / "flare-cpp_amd" / "lib" / "libflare_rpc_snappy.so"
    if not lib.exists():
        subprocess.run(["make", "-C", str(REPO), "host"], check=True, capture_output=True)
    L = ctypes.CDLL(str(lib))
    L.fsh_cpu_lz4f_decoded_length.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_int)]
    L.fsh_cpu_lz4f_decoded_length.restype = ctypes.c_uint64
    return L


def host_length(L, f: bytes):
    st = ctypes.c_int(-9)
    n = L.fsh_cpu_lz4f_decoded_length(ctypes.create_string_buffer(f, max(len(f), 1)), len(f), ctypes.byref(st))
    return st.value, n


@pytest.fixture(scope="module")
def all_frames(o):
    """Every frame of GPU tests 1 to 4, the mixed batch and the liblz4 fixtures."""
    frames = [f for _, f, _ in C.routing_edges(o)] + [f for _, f, _ in C.free_form(o)]
    frames += [f for _, f, _ in C.one_block_frames(o, 300)]
    frames += [C.block_frame(b, bid) for b, bid in C.hard_blocks()]
    frames += C.mutated(o)[0][::3]
    frames += [f for f, _, _ in C.mixed(o)] + [bytes.fromhex(d["hex"]) for d in VEC["decode_ok"]]
    return frames


def test_builder_equals_liblz4_without_a_content_size(o):
    L = lz4f_sys.load()
    if L is None:
        pytest.skip("no system liblz4")
    z = lz4f_sys.SysLz4F(L)
    rng = np.random.default_rng(3)
    xs = [C.text(n) for n in (1, 13, 65536, 65537, 200000)] + [rng.integers(0, 256, 70000, dtype=np.uint8).tobytes()]
    for x in xs:
        for bid, cs in ((4, False), (4, True), (5, True), (7, False)):
            assert C.nosize_frame(o, x, bid, cs) == z.compress_frame(x, bid, cs, size=False), (len(x), bid, cs)
    # flushed pieces: a block ends where a piece does
    pieces = [xs[4][:1], xs[4][1:71], xs[4][71:30071], xs[5][:5000]]
    assert C.frame_of_pieces(o, pieces, 4, True) == z.compress_pieces(pieces, 4, checksum=True)


def test_built_frames_decode_to_their_inputs(o):
    for x, f, nb in C.routing_edges(o) + C.free_form(o) + C.one_block_frames(o, 300):
        if len(x) < C.BIG or not f[4] & R.F_CSUM:
            assert R.decode_frame(o, f, len(x)) == (R.OK, len(x), x)
        assert len(C.blocks_in(f)[2]) == nb and R.parse_header(f)[4] is R.NO_SIZE


def test_host_decoded_length_equals_the_oracle(host, all_frames):
    seen = set()
    for i, f in enumerate(all_frames):
        want = C.decoded_length(f)
        assert host_length(host, f) == want, i
        seen.add(want[0])
    assert seen == {R.OK, R.CORRUPT, R.BAD_HEADER}
    assert host_length(host, b"") == (R.BAD_HEADER, 0)


def test_mutated_set_composition(o):
    """The counts GPU test 4 relies on, by the oracle alone."""
    frames, caps, _ = C.mutated(o)
    assert len(frames) == 3 * C.MUT_COUNT
    accepted, undecodable, no_length = C.mutated_classes(o, frames, caps)
    assert accepted >= 20 and undecodable >= 20 and no_length >= 20, (accepted, undecodable, no_length)
    assert {R.decode_frame(o, f, c)[0] for f, c in zip(frames, caps)} >= {R.OK, R.CORRUPT}


def test_frame_handler_reads_a_frame_without_a_content_size(o, tmp_path):
    """policy::Lz4FrameDecompress (tests/cpp/test_lz4_frame_handler.cc reads
    the frame it is given through the handler) on a flushed-pieces frame: the
    slot is sized by FrameDecodedLength."""
    exe = REPO / "build" / "test_lz4_frame_handler"
    if not exe.exists():
        subprocess.run(["make", "-C", str(REPO), "build/test_lz4_frame_handler"], check=True, capture_output=True,
                       timeout=600)
    x, f, _ = C.free_form(o)[0]
    fin, fout = tmp_path / "frame.in", tmp_path / "raw.out"
    fin.write_bytes(f)
    r = subprocess.run([str(exe), str(fin), str(fout)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "0 failures" in r.stdout, r.stdout + r.stderr
    assert fout.read_bytes() == x


def test_host_decoded_length_sanitized(o, all_frames, tmp_path):
    """FrameDecodedLength in a stand-alone program under AddressSanitizer and
    UBSan, each frame in a heap buffer of exactly its length."""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("g++ not available")
    exe = tmp_path / "lz4f_length_check"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I", str(REPO / "flare-cpp_amd" / "host"), str(REPO / "tests" / "cpp" / "lz4f_length_check.cc"),
                        str(REPO / "flare-cpp_amd" / "host" / "lz4_cpu.cc"), "-o", str(exe)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    cases = [f for f in all_frames if len(f) < 300000]
    cases += [f[:len(f) // 2] for f in cases[::5]] + [b""]
    fin, fout = tmp_path / "f.in", tmp_path / "f.out"
    fin.write_bytes(b"".join(struct.pack("<I", len(f)) + f for f in cases))
    r = subprocess.run([str(exe), str(fin), str(fout)], capture_output=True, text=True, timeout=300,
                       env={"ASAN_OPTIONS": "detect_leaks=0"})
    assert r.returncode == 0, r.stderr[-3000:]
    out = fout.read_bytes()
    assert len(out) == 12 * len(cases)
    for i, f in enumerate(cases):
        st, ln = struct.unpack_from("<iQ", out, 12 * i)
        assert (st, ln) == C.decoded_length(f), i
