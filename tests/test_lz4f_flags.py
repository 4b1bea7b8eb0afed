"""The compress flags of the LZ4 frame calls on the CPU (include/flare_lz4_gpu.h,
"The compressor writes ..."): content checksum, block checksums, no content
size.  The host codec (host/lz4_cpu.cc: CompressFrame with a flags word, through
fsh_cpu_lz4f_compress_flags) against the liblz4 1.9.3 fixture
tests/golden/lz4f_flags_vectors.json (make_lz4f_flags_golden.py) and, where the
image has it, the system liblz4 live; the frame oracle and the host decoder read
the frames back; and the shared frame writer (csrc/lz4_frame_format.h) under
AddressSanitizer and UBSan in a stand-alone program."""
import ctypes
import shutil
import subprocess
from pathlib import Path

import pytest

import lz4f_flags_cases as C
import lz4f_ref as R
from bind import Lz4Oracle

REPO = Path(__file__).resolve().parents[1]
VEC = C.load()


@pytest.fixture(scope="module")
def o():
    return Lz4Oracle()


@pytest.fixture(scope="module")
def host():
    lib = REPO / "flare-cpp_amd" / "lib" / "libflare_rpc_snappy.so"
    if not lib.exists():
        subprocess.run(["make", "-C", str(REPO), "host"], check=True, capture_output=True)
    L = ctypes.CDLL(str(lib))
    L.fsh_lz4f_max_frame_length.argtypes = [ctypes.c_size_t, ctypes.c_int]
    L.fsh_lz4f_max_frame_length.restype = ctypes.c_size_t
    L.fsh_lz4f_max_frame_length_flags.argtypes = [ctypes.c_size_t, ctypes.c_int, ctypes.c_uint32]
    L.fsh_lz4f_max_frame_length_flags.restype = ctypes.c_size_t
    L.fsh_cpu_lz4f_compress.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    L.fsh_cpu_lz4f_compress.restype = ctypes.c_size_t
    L.fsh_cpu_lz4f_compress_flags.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int,
                                              ctypes.c_uint32]
    L.fsh_cpu_lz4f_compress_flags.restype = ctypes.c_size_t
    L.fsh_cpu_lz4f_uncompress.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t,
                                          ctypes.POINTER(ctypes.c_uint32)]
    return L


def host_compress(L, x: bytes, bid: int, flags: int) -> bytes:
    cap = L.fsh_lz4f_max_frame_length_flags(len(x), bid, flags)
    out = ctypes.create_string_buffer(cap + 1)
    n = L.fsh_cpu_lz4f_compress_flags(ctypes.create_string_buffer(x, max(len(x), 1)), len(x), out, bid, flags)
    assert n <= cap
    return out.raw[:n]


def host_uncompress(L, f: bytes, cap: int):
    out = ctypes.create_string_buffer(max(cap, 1))
    ln = ctypes.c_uint32(0)
    r = L.fsh_cpu_lz4f_uncompress(ctypes.create_string_buffer(f, max(len(f), 1)), len(f), out, cap, ctypes.byref(ln))
    return {1: R.OK, 0: R.CORRUPT, -1: R.BAD_HEADER, -2: R.SLOT_TOO_SMALL}[r], ln.value, \
        (out.raw[:ln.value] if r == 1 else None)


@pytest.fixture(scope="module")
def frames(host):
    """The host codec's frame of every fixture key, made once."""
    xs = C.inputs()
    return {k: host_compress(host, xs[k[0]], k[1], k[2]) for k in C.keys()}


def test_fixture_shape():
    assert len(VEC) == 160 and len(C.inputs()) == 10
    # what the flags change, in lengths: 4 for the content checksum, 4 per block, 8 for the size
    for i, x in enumerate(C.inputs()):
        for bid in C.IDS:
            nb = -(-len(x) // R.block_bytes(bid))
            base = VEC[(i, bid, 0)][0]
            for fl in C.ALL_FLAGS:
                want = base + (4 if fl & C.CSUM else 0) + (4 * nb if fl & C.BSUM else 0) - \
                    (8 if fl & C.NOSIZE and x else 0)
                assert VEC[(i, bid, fl)][0] == want, (i, bid, fl)


def test_host_codec_frames_equal_the_liblz4_fixture(frames):
    for k, f in frames.items():
        assert (len(f), C.fnv(f)) == VEC[k], k


def test_host_codec_descriptor_and_raw_block_checksum(frames, o):
    xs = C.inputs()
    for (i, bid, fl), f in frames.items():
        st, hl, bmax, flg, size = R.parse_header(f)
        assert st == R.OK
        assert bool(flg & R.F_CSUM) == bool(fl & C.CSUM) and bool(flg & R.F_BSUM) == bool(fl & C.BSUM)
        assert size == (len(xs[i]) if xs[i] and not fl & C.NOSIZE else R.NO_SIZE)
        assert bmax == R.block_bytes(R.frame_block_id(len(xs[i]), bid))   # the smallest-id rule, size or not
    # the raw middle block at id 4: its checksum is over the raw bytes
    x = xs[-1]
    f = frames[(len(xs) - 1, 4, C.BSUM)]
    blocks = R.blocks_of(o, x, 4)
    assert [raw for _, raw in blocks] == [False, True, False, False]
    at = 15 + 4 + len(blocks[0][0]) + 4
    assert int.from_bytes(f[at:at + 4], "little") == 65536 | R.RAW
    assert f[at + 4:at + 4 + 65536] == x[65536:131072]
    assert int.from_bytes(f[at + 4 + 65536:at + 8 + 65536], "little") == R.xxh32(x[65536:131072])


def test_bool_and_flags_entry_points_agree(host):
    x = C.inputs()[5]
    for cs in (0, 1):
        cap = host.fsh_lz4f_max_frame_length(len(x), 4)
        out = ctypes.create_string_buffer(cap)
        n = host.fsh_cpu_lz4f_compress(ctypes.create_string_buffer(x), len(x), out, 4, cs)
        assert out.raw[:n] == host_compress(host, x, 4, cs)
    assert host_compress(host, x, 4, 8 | 3) == b"" and host.fsh_lz4f_max_frame_length_flags(10, 4, 8) == 0   # undefined bits
    for n in (0, 1, 65536, 65537, 300000):
        for bid in (4, 5, 7):
            for fl in C.ALL_FLAGS:
                assert host.fsh_lz4f_max_frame_length_flags(n, bid, fl) == C.max_frame_length_flags(n, bid, fl)
            assert host.fsh_lz4f_max_frame_length_flags(n, bid, 5) == host.fsh_lz4f_max_frame_length(n, bid)
    assert host.fsh_lz4f_max_frame_length_flags(10, 3, 2) == 0 and host.fsh_lz4f_max_frame_length_flags(10, 8, 2) == 0


def test_frames_decode_back_by_oracle_and_host_decoder(frames, host, o):
    xs = C.inputs()
    for (i, bid, fl), f in frames.items():
        x = xs[i]
        if bid == 4 or len(x) > 65536:   # (at most 64 KiB the id-5 frame is the id-4 frame: same BD, same blocks)
            assert R.decode_frame(o, f, len(x)) == (R.OK, len(x), x), (i, bid, fl)
        else:
            assert f == frames[(i, 4, fl)]
        assert host_uncompress(host, f, len(x)) == (R.OK, len(x), x), (i, bid, fl)


def test_host_codec_against_system_liblz4_live(frames):
    from lz4f_sys import SysLz4F, load
    L = load()
    if L is None:
        pytest.skip("no system liblz4 with the frame API in this image")
    z = SysLz4F(L)
    xs = C.inputs()
    for (i, bid, fl), f in frames.items():
        assert f == z.compress_frame(xs[i], bid, bool(fl & C.CSUM), bsum=bool(fl & C.BSUM),
                                     size=not fl & C.NOSIZE), (i, bid, fl)


# ---- the shared frame writer under AddressSanitizer and UBSan: a stand-alone program

def test_frame_writer_sanitized_bound_is_kept_and_tight(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = tmp_path / "lz4f_flags_check"
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-I", str(REPO / "flare-cpp_amd" / "host"),
                        str(REPO / "tests" / "cpp" / "lz4f_flags_check.cc"),
                        str(REPO / "flare-cpp_amd" / "host" / "lz4_cpu.cc"), "-o", str(exe)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300,
                       env={"ASAN_OPTIONS": "detect_leaks=0"})
    assert r.returncode == 0 and r.stdout.startswith("ok 1248"), r.stdout[-2000:] + r.stderr[-3000:]
