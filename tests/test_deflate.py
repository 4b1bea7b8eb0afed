"""Deflate compress on the CPU (include/flare_deflate_compress_gpu.h): the host
model (host/deflate_cpu.cc over csrc/deflate_format.h, the text the device
encoder shares) judged by Python's zlib -- every body of tests/deflate_cases.py
in the three formats inflates to its input with the stream ended and nothing
left over -- the wrapper bytes, the block choice, the match limits read from
the model's tokens, the size condition against zlib level 1, then the model and
a 64-lane emulation of the wide functions under AddressSanitizer and UBSan in
a stand-alone program, the new symbols and argument checks, and the gzip /
zlib CompressHandler's C++ test."""
import ctypes
import shutil
import struct
import subprocess
import zlib
from pathlib import Path

import pytest

import deflate_cases as C
import deflate_streams as D
import fsg

REPO = Path(__file__).resolve().parents[1]
FORMATS = [C.RAW, C.ZLIB, C.GZIP]


def zlib_inflate(fmt, body):
    d = zlib.decompressobj(C.WBITS[fmt])
    out = d.decompress(body)
    assert d.eof and not d.unused_data and not d.unconsumed_tail
    return out


@pytest.mark.parametrize("fmt", FORMATS)
def test_family_is_read_by_zlib_and_by_the_host_inflate(fmt):
    L = C.host()
    for name, x in C.cases():
        body = C.model(fmt, x)
        assert zlib_inflate(fmt, body) == x, name
        out = ctypes.create_string_buffer(len(x) + 1)
        ln = ctypes.c_uint64()
        assert L.fsh_cpu_inflate(fmt, body, len(body), out, len(x), ctypes.byref(ln)) == D.OK, name
        assert ln.value == len(x) and out.raw[:len(x)] == x, name
        bound = L.fsh_cpu_deflate_bound(len(x), fmt)
        assert bound == C.bound(len(x), fmt) and len(body) <= bound, name
        n = len(body)
        st, ln, buf = C.deflate_into(fmt, x, bound)   # a second call: equal bytes, nothing past the length
        assert (st, ln) == (D.OK, n) and buf[:n] == body and buf[n:] == b"\xa5" * (bound - n), name
        st, ln, buf = C.deflate_into(fmt, x, n - 1)   # one byte short: refused, nothing written
        assert (st, ln) == (D.SLOT_TOO_SMALL, 0) and buf == b"\xa5" * (n - 1), name


def test_bound_formula_and_unknown_format():
    L = C.host()
    for n in (0, 1, C.U - 1, C.U, C.U + 1, 2 * C.U, 2 * C.U + 1, 10 ** 9, 2 ** 32 - 1):
        for fmt in FORMATS:
            assert L.fsh_cpu_deflate_bound(n, fmt) == C.bound(n, fmt)
    assert L.fsh_cpu_deflate_bound(100, 3) == 0
    assert C.deflate_into(3, b"abc", 64)[:2] == (D.CORRUPT, 0)
    # the bound is met: a body of stored units
    x = D.noise(2 * C.U, 4)
    assert len(C.model(C.GZIP, x)) == C.bound(len(x), C.GZIP)


def test_exact_capacity_is_enough():
    for name in ("text_300000", "noise_65", "fibonacci", "text_0", "block_choice"):
        x = C.by_name(name)
        for fmt in FORMATS:
            body = C.model(fmt, x)
            assert C.deflate_into(fmt, x, len(body)) == (D.OK, len(body), body), name


def test_wrappers():
    for x in (b"", b"a", D.text(5000, 3), D.text(2 * C.U + 1, 1)):
        raw, z, g = (C.model(f, x) for f in FORMATS)
        assert z[:2] == b"\x78\x01" and int.from_bytes(z[:2], "big") % 31 == 0 and not z[1] & 0x20
        assert z[2:-4] == raw and z[-4:] == struct.pack(">I", zlib.adler32(x))
        assert g[:10] == bytes.fromhex("1f8b0800000000000003")
        assert g[10:-8] == raw and g[-8:] == struct.pack("<II", zlib.crc32(x), len(x) & 0xFFFFFFFF)


def test_block_types_and_markers():
    btype = lambda raw: (raw[0] >> 1) & 3
    assert btype(C.model(C.RAW, D.text(5000))) == 2
    assert btype(C.model(C.RAW, D.noise(5000))) == 0
    assert btype(C.model(C.RAW, b"hello")) == 1
    assert C.unit_types(D.text(5000)) == (0, 0, 1) and C.unit_types(D.noise(5000)) == (1, 0, 0)
    assert C.unit_types(b"hello") == (0, 1, 0) and C.unit_types(b"") == (0, 1, 0) and C.unit_types(b"\x00") == (0, 1, 0)
    assert C.unit_types(C.block_choice()) == (1, 0, 2)
    # 2U + 1 text bytes: three units, an empty stored block behind the first two, each where its unit ends
    x = D.text(2 * C.U + 1, 1)
    raw = C.model(C.RAW, x)
    assert raw.count(b"\x00\x00\xff\xff") == 2
    at = 0
    for k in (1, 2):  # the bytes up to a marker's end are the first k units, flushed
        at = raw.index(b"\x00\x00\xff\xff", at) + 4
        assert zlib.decompressobj(-15).decompress(raw[:at]) == x[:k * C.U]
    assert raw[0] & 1 == 0 and zlib_inflate(C.RAW, raw) == x


def test_match_limits_from_the_tokens():
    def matches(data):
        toks = C.tokens(data)
        assert sum(1 if t[0] == "lit" else t[1] for t in toks) == len(data)
        return [t for t in toks if t[0] == "match"]
    # the 258 cap and the split
    for r in (257, 258, 259, 260, 516, 517):
        for pre in (b"", b"xyz"):
            ms = matches(pre + b"z" * r)
            assert ms and all(4 <= m[1] <= 258 and 1 <= m[2] <= 64 for m in ms), (r, pre)
    assert max(m[1] for m in matches(b"z" * 517)) == 258
    # distances: found up to 32,768, never beyond
    for d in (64, 65, 32767, 32768):
        assert any(m[2] == d and m[1] >= 90 for m in matches(C.repeat_at(d))), d
    assert not any(m[2] > 64 for m in matches(C.repeat_at(32769)))  # the zeros match at 1 .. 64, the string does not
    for d in (1, 3, 4, 63, 64, 65, 32767, 32768, 32769):
        assert all(m[2] <= 32768 for m in matches(C.repeat_at(d)))
    assert matches(C.by_name("literals_only")) == [] and matches(C.by_name("all_256_once")) == []
    assert matches(C.by_name("one_distance")) == [("match", 10, 64)]


def test_units_are_independent():
    """The last unit's bytes are those of the same input compressed alone, so
    nothing of it refers to the unit before (zlib would decode such a match
    all the same: its window spans blocks)."""
    x = C.straddle()
    assert len(x) > C.U + 300
    raw = C.model(C.RAW, x)
    alone = C.model(C.RAW, x[C.U:])
    assert raw.endswith(alone) and zlib_inflate(C.RAW, raw) == x
    # and the repeat is found where it may be: inside unit 2
    assert any(t[0] == "match" and t[2] == 200 for t in C.tokens(x[C.U:]))


def test_code_construction():
    L = C.host()
    deep = C.by_name("fibonacci_deep")                              # deflate_cases.deep_body says why not "fibonacci"
    assert L.fsh_cpu_deflate_limited(deep, len(deep)) >= 1         # the 15-bit limit was met
    assert C.unit_types(deep) == (0, 0, 1)                         # and the limited code is the one written
    assert L.fsh_cpu_deflate_limited(D.text(5000), 5000) == 0
    eq = C.by_name("all_256_equally")
    assert abs(len(C.model(C.RAW, eq)) - len(eq)) < 200            # 8-bit codes: no gain, or stored
    for name in ("all_256_once", "literals_only", "one_distance", "one_byte", "alphabet1_1000", "alphabet2_1000"):
        assert zlib_inflate(C.RAW, C.model(C.RAW, C.by_name(name))) == C.by_name(name)


def test_size_condition_against_zlib_level_1():
    """No longer than 1.15 x zlib level 1 on the same bytes (measured: 1.031
    and 1.055; a stored-only writer is at 2.6)."""
    for n in (70000, 300000):
        x = D.text(n)
        ours, ref = len(C.model(C.ZLIB, x)), len(zlib.compress(x, 1))
        print(f"text({n}): {ours} bytes, zlib level 1 {ref}, level 6 {len(zlib.compress(x, 6))}, ratio {ours / ref:.4f}")
        assert ours <= 1.15 * ref, (n, ours, ref)


def test_host_model_and_lanes_sanitized(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = tmp_path / "deflate_check"
    host = REPO / "flare-cpp_amd" / "host"
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-pthread", "-I", str(host), str(REPO / "tests" / "cpp" / "deflate_check.cc"),
                        str(host / "deflate_cpu.cc"), str(host / "inflate_cpu.cc"), "-o", str(exe)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lanes = {"text_5", "text_129", "noise_129", "text_65473", "fibonacci", "fibonacci_deep", "one_byte", "text_0", "one_distance",
             "all_256_equally", "alphabet2_1000", "xyz_run_517", "repeat_at_32768", "literals_only", "block_choice"}
    rec = units = 0
    with open(tmp_path / "vectors.bin", "wb") as f:
        for name, x in C.cases():
            for fmt in FORMATS:
                body = C.model(fmt, x)
                flags = (1 if name == "fibonacci_deep" else 0) | (2 if name in lanes and fmt == C.RAW else 0)
                f.write(struct.pack("<4I", fmt, len(x), len(body), flags) + x + body)
                rec += 1
                units += max(1, -(-len(x) // C.U)) if flags & 2 else 0
    r = subprocess.run([str(exe), str(tmp_path / "vectors.bin")], capture_output=True, text=True, timeout=900,
                       env={"ASAN_OPTIONS": "detect_leaks=0"})
    assert r.returncode == 0 and r.stdout.strip() == f"ok {rec} {units}", r.stdout[-2000:] + r.stderr[-3000:]


# ---- the public header and the argument checks, no GPU

NEW = ["fsg_deflate_batch", "fsg_deflate_max_length", "fsg_deflate_report", "fsg_deflate_workspace_bytes"]


def test_new_symbols_exported_and_bound():
    assert fsg.header_symbols(REPO / "include" / "flare_deflate_compress_gpu.h") == NEW
    assert '#include "flare_deflate_compress_gpu.h"' in (REPO / "include" / "flare_deflate_gpu.h").read_text()
    lib = fsg.load_gpu_lib()
    assert all(hasattr(lib, s) for s in NEW) and set(NEW) <= set(fsg.header_symbols()) and set(NEW) <= set(fsg._SIGS)
    for m in ("deflate", "deflate_max_length", "deflate_workspace_bytes", "deflate_report"):
        assert callable(getattr(fsg.SnappyGPU, m))
    for n in (0, 1, C.U, C.U + 1, 300000, 2 ** 32 - 1):
        for fmt in FORMATS:
            assert lib.fsg_deflate_max_length(n, fmt) == C.bound(n, fmt)
    assert lib.fsg_deflate_max_length(100, 3) == 0
    # the workspace grows with the batch and with its bytes, and is enough for what it says
    w = lib.fsg_deflate_workspace_bytes
    assert w(1, 0) < w(2, 0) < w(2, C.U) < w(2, 10 * C.U) and w(4, C.U - 1) == w(4, 0)


def test_invalid_arguments_rejected_without_gpu():
    lib = fsg.load_gpu_lib()
    one = 16  # any non-null, aligned value: rejected before it is looked at
    big = 1 << 40
    call = lib.fsg_deflate_batch
    assert call(None, None, None, 5, None, None, None, None, C.ZLIB, None, 0, None) == -1
    for hole in range(7):  # each NULL column
        a = [one] * 7
        a[hole] = None
        a.insert(3, 5)
        assert call(*a, C.ZLIB, one, big, None) == -1, hole
    for fmt in (3, 7, 0xFFFFFFFF):  # an unknown format, whatever the pointers and the count
        assert call(one, one, one, 5, one, one, one, one, fmt, one, big, None) == -1
        assert call(None, None, None, 0, None, None, None, None, fmt, None, 0, None) == -1
    need = lib.fsg_deflate_workspace_bytes(5, 0)
    assert call(one, one, one, 5, one, one, one, one, C.GZIP, one, need - 1, None) == -1  # one byte too small
    assert call(one, one, one, 5, one, one, one, one, C.GZIP, None, need, None) == -1     # no workspace
    assert call(one, one, one, 5, one, one, one, one, C.GZIP, one + 4, need, None) == -1  # misaligned
    assert call(None, None, None, 0, None, None, None, None, C.RAW, None, 0, None) == 0   # an empty batch
    rep = fsg.DeflateReport()
    head = ctypes.create_string_buffer(256)
    assert lib.fsg_deflate_report(None, 5, need, ctypes.byref(rep)) == -1
    assert lib.fsg_deflate_report(head, 5, need - 1, ctypes.byref(rep)) == -1
    assert lib.fsg_deflate_report(head, 5, need, ctypes.byref(rep)) == 0 and rep.unit_entries == 5
    assert lib.fsg_deflate_report(head, 5, lib.fsg_deflate_workspace_bytes(5, 3 * C.U), ctypes.byref(rep)) == 0
    assert rep.unit_entries == 8


# ---- the gzip / zlib CompressHandlers of the host layer (host/gzip_compress.h)

def test_gzip_handler_registers_and_interoperates(tmp_path):
    """tests/cpp/test_gzip_handler.cc: GlobalInitializeGzipZlib at types 2 and
    3, cord_buf bodies and a message through the four functions, a gzip body
    spelled out byte by byte, corrupt bodies refused; it reads a body Python's
    gzip wrote, and Python's zlib reads the body it writes."""
    import gzip
    subprocess.run(["make", "-C", str(REPO), "build/test_gzip_handler"], check=True, capture_output=True, timeout=600)
    x = D.text(100000, 5)
    fin, fout, zout = tmp_path / "body.gz", tmp_path / "raw.out", tmp_path / "body.z"
    fin.write_bytes(gzip.compress(x, 6))
    r = subprocess.run([str(REPO / "build" / "test_gzip_handler"), str(fin), str(fout), str(zout)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "0 failures" in r.stdout, r.stdout + r.stderr
    assert fout.read_bytes() == x
    assert zlib_inflate(C.ZLIB, zout.read_bytes()) == x and zout.read_bytes() == C.model(C.ZLIB, x)
