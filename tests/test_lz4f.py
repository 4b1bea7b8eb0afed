"""LZ4 frames on the CPU (include/flare_lz4_gpu.h, "LZ4 frames"): the frame
oracle (tests/lz4f_ref.py) against the liblz4 1.9.3 fixtures in
tests/golden/lz4f_vectors.json (make_lz4f_golden.py) and, where the image has
it, the system liblz4 live; the product's host codec (host/lz4_cpu.cc) against
the oracle; and the GPU kernels' serial frame decoder, run on the CPU under
AddressSanitizer and UBSan by a stand-alone program."""
import ctypes
import json
import shutil
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

import fsg
import lz4f_ref as R
from bind import Lz4Oracle
from lz4f_cases import base_frame, build, fnv, load, mutate, oracle_frame

REPO = Path(__file__).resolve().parents[1]
GOLDEN = REPO / "tests" / "golden"
VEC = load()


@pytest.fixture(scope="module")
def o():
    return Lz4Oracle()


def test_xxh32_known_values():
    assert R.xxh32(b"") == 0x02CC5D05
    assert R.xxh32(b"a") == 0x550D7456
    assert R.xxh32(b"abc") == 0x32D153FF
    assert R.xxh32(b"Nobody inspects the spammish repetition") == 0xE2293B2F
    assert R.xxh32(b"abc", 1) != R.xxh32(b"abc")


def test_oracle_frames_equal_liblz4_fixtures(o):
    flagged = 0
    for e in VEC["compress"]:
        x = build(e["input"])
        f = oracle_frame(o, e, x)
        assert R.max_frame_length(len(x), e["bid"]) >= len(f)
        if e.get("differs_from_size_rule"):
            flagged += 1  # liblz4 stored a block otherwise than the size rule says: both frames are valid
            continue
        assert len(f) == e["frame_len"] and fnv(f) == e["frame_fnv"], e
        blocks = R.blocks_of(o, x, e["bid"])
        assert len(blocks) == e["blocks"] and sum(r for _, r in blocks) == e["raw_blocks"]
    assert flagged == 0  # none seen with liblz4 1.9.3; DESIGN.md section 4 says what to do if one appears
    assert R.compress_frame(o, b"", 4, False) == bytes.fromhex("04224d186040820000" "0000")
    assert len(R.compress_frame(o, b"", 7, True)) == 15


def test_oracle_reads_foreign_frames(o):
    for d in VEC["decode_ok"]:
        f = bytes.fromhex(d["hex"])
        for oo in (o, None):
            st, ln, y = R.decode_frame(oo, f, d["out_len"])
            assert st == R.OK and ln == d["out_len"] and fnv(y) == d["out_fnv"], d["name"]
        assert R.decode_frame(o, f, d["out_len"] - 1)[0] in (R.SLOT_TOO_SMALL, R.CORRUPT), d["name"]
        assert R.decode_frame(o, f + b"\0", d["out_len"])[0] == R.CORRUPT
        assert R.decode_frame(o, f[:-1], d["out_len"])[0] == R.CORRUPT


def test_oracle_verdicts_on_mutated_frames_and_one_way_relation(o):
    """Every frame the oracle accepts liblz4 accepted with the same bytes;
    frames liblz4 alone accepts are flagged, at most 1 % of the file."""
    n_ok = flagged = 0
    for i, c in enumerate(VEC["decode"]):
        x = build(VEC["decode_sources"][c["src"]])
        f = mutate(base_frame(o, c), c)
        st, ln, y = R.decode_frame(o, f, len(x))
        assert st == c["oracle"] and ln == c["out_len"], i
        if st == R.OK:
            n_ok += 1
            assert c["liblz4_ok"] and fnv(y) == c["out_fnv"], i
        elif c["liblz4_ok"]:
            assert c.get("liblz4_only"), i
            flagged += 1
    assert n_ok >= 50 and flagged * 100 <= len(VEC["decode"])
    assert {c["oracle"] for c in VEC["decode"]} == {R.OK, R.CORRUPT, R.BAD_HEADER, R.SLOT_TOO_SMALL}


def test_header_rules(o):
    x = b"hello hello hello hello hello hello"
    f = R.compress_frame(o, x, 4, True)
    assert R.decode_frame(o, f, len(x)) == (R.OK, len(x), x)
    assert R.decode_frame(o, f, len(x) - 1) == (R.SLOT_TOO_SMALL, len(x), None)

    def redo(g):  # a descriptor change with HC made right again
        g = bytearray(g)
        hl = 15 if g[4] & R.F_SIZE else 7
        g[hl - 1] = (R.xxh32(bytes(g[4:hl - 1])) >> 8) & 0xFF
        return bytes(g)

    for magic in (0x184D2A50, 0x184C2102, 0x184D2205):  # skippable, legacy, wrong
        assert R.decode_frame(o, struct.pack("<I", magic) + f[4:], 100)[0] == R.BAD_HEADER
    for at, val in ((4, f[4] & 0x3F), (4, f[4] | 0x80), (4, f[4] | R.F_RESERVED), (4, f[4] | R.F_DICT),
                    (5, 0x30), (5, f[5] | 0x80), (5, f[5] | 0x01)):
        g = bytearray(f)
        g[at] = val
        assert R.decode_frame(o, redo(g), 100)[0] == R.BAD_HEADER, (at, val)
    g = bytearray(f)
    g[14] ^= 1
    assert R.decode_frame(o, bytes(g), 100)[0] == R.BAD_HEADER          # HC
    assert all(R.decode_frame(o, f[:k], 100)[0] == R.BAD_HEADER for k in range(15))
    assert all(R.decode_frame(o, f[:k], 100)[0] == R.CORRUPT for k in range(15, len(f)))
    g = bytearray(f)
    g[10:14] = b"\xff\xff\xff\xff"                                       # content size 2^64 - 2^32 + ...
    assert R.decode_frame(o, redo(g), 100)[:2] == (R.SLOT_TOO_SMALL, 0xFFFFFFFF)
    big = R.header(None, 4, False) + struct.pack("<I", 65537 | R.RAW) + bytes(65537) + bytes(4)
    assert R.decode_frame(o, big, 1 << 20)[0] == R.CORRUPT               # size word above the block maximum
    nosize = R.header(None, 4, False) + struct.pack("<I", 5 | R.RAW) + b"abcde" + bytes(4)
    assert R.decode_frame(o, nosize, 5) == (R.OK, 5, b"abcde")
    assert R.decode_frame(o, nosize, 4)[0] == R.CORRUPT                  # past the capacity, no content size


def test_python_block_decoder_equals_oracle_on_mutated_blocks(o):
    cases = json.loads((GOLDEN / "lz4_vectors.json").read_text())["decode"]
    assert len(cases) == 600
    n_ok = 0
    for d in cases:
        b = bytes.fromhex(d["hex"])
        ok, y = o.decompress_block(b, d["ulen"])
        assert R.decode_block(b, d["ulen"]) == (y if ok else None)
        ln = R.block_length(b, 1 << 30)
        if ok:
            n_ok += 1
            assert ln == d["ulen"]
        elif ln is not None:  # judged with capacity equal to its own decoded length
            ok2, y2 = o.decompress_block(b, ln)
            assert R.decode_block(b, ln) == (y2 if ok2 else None)
    assert n_ok > 100


def test_oracle_against_system_liblz4_live(o):
    from lz4f_sys import LINKED, SysLz4F, load
    L = load()
    if L is None:
        pytest.skip("no system liblz4 with the frame API in this image")
    z = SysLz4F(L)
    rng = np.random.default_rng(12)
    for t in range(120):
        n = int(rng.choice([rng.integers(0, 40), rng.integers(0, 3000), rng.integers(60000, 70000),
                            rng.integers(0, 300000)]))
        alpha = int(rng.choice([1, 2, 4, 16, 256]))
        x = rng.integers(0, alpha, n, dtype=np.uint8).tobytes()
        bid, cs = int(rng.integers(4, 8)), bool(rng.integers(2))
        f = z.compress_frame(x, bid, cs)
        if n <= 70000 or not cs:
            assert R.compress_frame(o, x, bid, cs) == f, (n, alpha, bid, cs)
        assert len(f) <= R.max_frame_length(n, bid) <= z.bound(n, bid)
        g = z.compress_frame(x, bid, mode=LINKED if t % 2 else 1, bsum=bool(t % 3 == 0), size=bool(t % 5))
        st, ln, y = R.decode_frame(o, g, n)
        assert st == R.OK and y == x, (n, alpha, t)


# ---- the product host codec (host/lz4_cpu.cc through include/flare_snappy_host.h)

@pytest.fixture(scope="module")
def host():
    lib = REPO / "flare-cpp_amd" / "lib" / "libflare_rpc_snappy.so"
    if not lib.exists():
        subprocess.run(["make", "-C", str(REPO), "host"], check=True, capture_output=True)
    L = ctypes.CDLL(str(lib))
    L.fsh_lz4f_max_frame_length.argtypes = [ctypes.c_size_t, ctypes.c_int]
    L.fsh_lz4f_max_frame_length.restype = ctypes.c_size_t
    L.fsh_cpu_lz4f_compress.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    L.fsh_cpu_lz4f_compress.restype = ctypes.c_size_t
    L.fsh_cpu_lz4f_uncompress.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t,
                                          ctypes.POINTER(ctypes.c_uint32)]
    return L


def _host_compress(L, x: bytes, bid: int, cs: int) -> bytes:
    cap = L.fsh_lz4f_max_frame_length(len(x), bid)
    out = ctypes.create_string_buffer(cap + 1)
    n = L.fsh_cpu_lz4f_compress(ctypes.create_string_buffer(x, max(len(x), 1)), len(x), out, bid, cs)
    assert n <= cap
    return out.raw[:n]


_HOST_ST = {1: R.OK, 0: R.CORRUPT, -1: R.BAD_HEADER, -2: R.SLOT_TOO_SMALL}


def _host_uncompress(L, f: bytes, cap: int):
    out = ctypes.create_string_buffer(max(cap, 1))
    ln = ctypes.c_uint32(0)
    r = L.fsh_cpu_lz4f_uncompress(ctypes.create_string_buffer(f, max(len(f), 1)), len(f), out, cap, ctypes.byref(ln))
    return _HOST_ST[r], ln.value, (out.raw[:ln.value] if r == 1 else None)


def test_host_codec_frames_equal_fixtures_and_oracle(host, o):
    for e in VEC["compress"]:
        x = build(e["input"])
        f = _host_compress(host, x, e["bid"], e["checksum"])
        assert f == oracle_frame(o, e, x), e
        if not e.get("differs_from_size_rule"):
            assert len(f) == e["frame_len"] and fnv(f) == e["frame_fnv"], e
        assert _host_uncompress(host, f, len(x)) == (R.OK, len(x), x)
    assert host.fsh_lz4f_max_frame_length(10, 3) == 0 and host.fsh_lz4f_max_frame_length(10, 8) == 0
    assert host.fsh_lz4f_max_frame_length(65537, 4) == R.max_frame_length(65537, 4)


def test_host_codec_verdicts_equal_oracle(host, o):
    for d in VEC["decode_ok"]:
        f = bytes.fromhex(d["hex"])
        for cap in (d["out_len"], d["out_len"] - 1, 0):
            assert _host_uncompress(host, f, cap) == R.decode_frame(o, f, cap), (d["name"], cap)
    for i, c in enumerate(VEC["decode"]):
        x = build(VEC["decode_sources"][c["src"]])
        f = mutate(base_frame(o, c), c)
        got = _host_uncompress(host, f, len(x))
        assert got[0] == c["oracle"] and got[1] == c["out_len"], i
        if got[0] == R.OK:
            assert fnv(got[2]) == c["out_fnv"], i
        if i % 10 == 0:
            for cap in (0, max(len(x) - 1, 0)):
                assert _host_uncompress(host, f, cap) == R.decode_frame(o, f, cap), (i, cap)


# ---- the GPU kernels' serial frame decoder on the CPU under AddressSanitizer
# and UBSan (tests/cpp/lz4f_host_check.hip includes csrc/lz4_frame_format.h,
# whose functions are __host__ __device__): a stand-alone program.

@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not Path(hipcc).exists():
        pytest.skip("hipcc not available")
    exe = tmp_path_factory.mktemp("lz4fhc") / "lz4f_host_check"
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
                        "-Xarch_host", "-fno-sanitize-recover=undefined",
                        str(REPO / "tests" / "cpp" / "lz4f_host_check.hip"), "-o", str(exe)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return exe


def test_gpu_serial_frame_decoder_on_host_sanitized(host_check, o, tmp_path):
    cases = []
    for d in VEC["decode_ok"]:
        f = bytes.fromhex(d["hex"])
        cases += [(f, d["out_len"]), (f, d["out_len"] - 1), (f, 0), (f[:len(f) // 2], d["out_len"])]
    for c in VEC["decode"]:
        x = build(VEC["decode_sources"][c["src"]])
        f = mutate(base_frame(o, c), c)
        cases.append((f, len(x)))
        if len(cases) % 7 == 0:
            cases += [(f, 0), (f, max(len(x) - 1, 0))]
    cases.append((b"", 10))
    fin, fout = tmp_path / "f.in", tmp_path / "f.out"
    fin.write_bytes(b"".join(struct.pack("<II", cap, len(f)) + f for f, cap in cases))
    r = subprocess.run([str(host_check), str(fin), str(fout)], capture_output=True, text=True, timeout=300,
                       env={"ASAN_OPTIONS": "detect_leaks=0"})
    assert r.returncode == 0, r.stderr[-3000:]
    out = fout.read_bytes()
    p = 0
    for i, (f, cap) in enumerate(cases):
        st, ln = struct.unpack_from("<iI", out, p)
        p += 8
        want = R.decode_frame(o, f, cap)
        assert (st, ln) == want[:2], (i, cap)
        if st == 0:
            assert out[p:p + ln] == want[2], i
            p += ln
    assert p == len(out)


# ---- the frame CompressHandler of the host layer (host/lz4_compress.h)

def test_frame_handler_registers_and_interoperates(o, tmp_path):
    """tests/cpp/test_lz4_frame_handler.cc: GlobalInitializeLz4Frame at type 4,
    bodies and a message through policy::Lz4FrameCompress / Lz4FrameDecompress;
    its frame of the reference tests' 200-byte text equals the oracle's (and so
    liblz4's), and it reads a liblz4 frame with linked blocks and checksums."""
    exe = REPO / "build" / "test_lz4_frame_handler"
    if not exe.exists():
        subprocess.run(["make", "-C", str(REPO), "build/test_lz4_frame_handler"], check=True, capture_output=True,
                       timeout=600)
    d = next(d for d in VEC["decode_ok"] if d["name"] == "linked_checksums_no_size")
    fin, fout = tmp_path / "frame.in", tmp_path / "raw.out"
    fin.write_bytes(bytes.fromhex(d["hex"]))
    r = subprocess.run([str(exe), str(fin), str(fout)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "0 failures" in r.stdout, r.stdout + r.stderr
    text = (b"abcdefghijklmnopqrstuvwxyz0123456789" * 6)[:200]
    assert "frame " + R.compress_frame(o, text, 4).hex() in r.stdout
    assert fnv(fout.read_bytes()) == d["out_fnv"]
