"""Inflate on the CPU (include/flare_deflate_gpu.h): the host model
(host/inflate_cpu.cc over csrc/inflate_format.h, the text the device decoder
shares) against Python's zlib -- bodies zlib's compressor writes, hand-built
streams from tests/deflate_streams.py, one rejected stream per cause with the
exact status and zlib's refusal beside it, 2,000 single-bit flips per format
-- then the same vectors under AddressSanitizer and UBSan in a stand-alone
program, and the new header's symbols and argument checks.  The seeded family
of tests/deflate_random.py (random hand-built streams and the worst-case code
tables) runs through the same checks, with floors on what it covers."""
import ctypes
import hashlib
import shutil
import struct
import subprocess
import zlib
from pathlib import Path

import pytest

import deflate_random as R
import deflate_streams as D
import fsg

REPO = Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module")
def host():
    lib = REPO / "flare-cpp_amd" / "lib" / "libflare_rpc_snappy.so"
    if not lib.exists():
        subprocess.run(["make", "-C", str(REPO), "host"], check=True, capture_output=True)
    L = ctypes.CDLL(str(lib))
    L.fsh_cpu_inflate.argtypes = [ctypes.c_uint32, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t,
                                  ctypes.POINTER(ctypes.c_uint64)]
    L.fsh_cpu_inflate_length.argtypes = [ctypes.c_uint32, ctypes.c_char_p, ctypes.c_size_t,
                                         ctypes.POINTER(ctypes.c_uint64)]
    L.fsh_cpu_crc32.argtypes = L.fsh_cpu_adler32.argtypes = [ctypes.c_char_p, ctypes.c_size_t]
    L.fsh_cpu_crc32.restype = L.fsh_cpu_adler32.restype = ctypes.c_uint32
    return L


GUARD = b"\xa5" * 32


def inflate(L, fmt, body, cap):
    """(status, length, bytes or None); the bytes past the capacity must stay as they were."""
    out = ctypes.create_string_buffer((GUARD * (cap // 32 + 2))[:cap + 32], cap + 32)
    ln = ctypes.c_uint64(99)
    st = L.fsh_cpu_inflate(fmt, body, len(body), out, cap, ctypes.byref(ln))
    assert out.raw[cap:] == GUARD, "the host model wrote past the capacity"
    return st, ln.value, out.raw[:ln.value] if st == D.OK else None


def length(L, fmt, body):
    ln = ctypes.c_uint64(99)
    return L.fsh_cpu_inflate_length(fmt, body, len(body), ctypes.byref(ln)), ln.value


def test_vector_shapes():
    """What the issue's table relies on: which block types the bodies hold."""
    btype = lambda raw: (raw[0] >> 1) & 3
    assert btype(D.compress(D.RAW, D.text(10), 6)) == 1
    for n in (100, 1000, 5000, 70000, 300000):
        assert btype(D.compress(D.RAW, D.text(n), 6)) == 2, n
    assert D.compress(D.RAW, D.text(300000), 6)[0] & 1 == 0  # a non-final first block
    assert btype(D.compress(D.RAW, D.text(1000), 0)) == 0 and btype(D.compress(D.RAW, D.noise(5000), 6)) == 0
    assert btype(D.compress(D.RAW, D.text(1000), 6, zlib.Z_FIXED)) == 1
    sync = D.compress(D.RAW, D.text(20000, 6), 6, flush_every=700)
    assert sync.count(b"\x00\x00\xff\xff") >= 28  # an empty stored block at every flush
    assert len(D.accept_vectors()) > 300 and len(D.reject_streams()) > 50


def test_accepted_vectors_match_zlib(host):
    exp = D.expected()
    for name, fmt, body in D.accept_vectors():
        want = exp[name]
        assert want is not None, name
        assert inflate(host, fmt, body, len(want)) == (D.OK, len(want), want), name
        assert length(host, fmt, body) == (D.OK, len(want)), name
    for name, fmt, body in D.accept_vectors()[::7]:  # a larger slot changes nothing
        want = exp[name]
        assert inflate(host, fmt, body, len(want) + 100) == (D.OK, len(want), want), name


def test_every_rejection_cause(host):
    for name, fmt, body, status in D.reject_streams():
        assert D.zlib_verdict(fmt, body) is None, f"zlib accepts {name}: the case is wrong, not the codec"
        assert inflate(host, fmt, body, 1 << 16) == (status, 0, None), name
    # a zlib header that declares a window below 32 KiB is accepted (and the 512-byte one decodes)
    small = dict((n, b) for n, f, b in D.accept_vectors())["zlib_window_512"]
    assert small[0] >> 4 == 1 and inflate(host, D.ZLIB, small, 5000)[0] == D.OK


def test_slot_too_small(host):
    exp = D.expected()
    picked = [v for v in D.accept_vectors() if v[0] in ("text_5000_l6_f1", "random_1000_l6_f0", "text_70000_l9_f2",
                                                       "fixed_every_length_f1", "sync_flush_f2")]
    assert len(picked) == 5
    for name, fmt, body in picked:
        n = len(exp[name])
        for cap in (0, 1, n - 1):
            assert inflate(host, fmt, body, cap) == (D.SLOT_TOO_SMALL, n, None), (name, cap)
        assert inflate(host, fmt, body, n) == (D.OK, n, exp[name]), name


def test_lengths_call_does_not_judge_the_checksum(host):
    data = D.text(4000, 21)
    raw = D.compress(D.RAW, data)
    for fmt, body in ((D.ZLIB, D.wrap(D.ZLIB, raw, data, adler=1)), (D.GZIP, D.wrap(D.GZIP, raw, data, crc=7)),
                      (D.GZIP, D.wrap(D.GZIP, raw, data, isize=3))):
        assert D.zlib_verdict(fmt, body) is None
        assert length(host, fmt, body) == (D.OK, len(data))
        assert inflate(host, fmt, body, len(data)) == (D.CORRUPT, 0, None)
    # everything else is judged alike by both calls
    for name, fmt, body, status in D.reject_streams():
        if name in ("zlib_adler", "gzip_crc", "gzip_isize"):
            assert length(host, fmt, body) == (D.OK, 2000), name
        else:
            assert length(host, fmt, body) == (status, 0), name


@pytest.mark.parametrize("fmt", [D.RAW, D.ZLIB, D.GZIP])
def test_bit_flips_match_zlib(host, fmt):
    accepted = 0
    for body, want in D.mutation_set(fmt):
        cap = len(want) if want is not None else 8192
        st, ln, got = inflate(host, fmt, body, cap)
        assert (st == D.OK) == (want is not None), (fmt, body.hex())
        if want is not None:
            assert got == want
            accepted += 1
    if fmt == D.RAW:  # neither side of the comparison is empty
        assert 200 <= accepted <= 1800, accepted


def test_serial_checksums(host):
    for n in (0, 1, 15, 16, 17, 5551, 5552, 5553, 70000):
        x = D.noise(n, 3)
        assert host.fsh_cpu_crc32(x, n) == zlib.crc32(x) and host.fsh_cpu_adler32(x, n) == zlib.adler32(x), n
    x = b"\xff" * 200000  # the largest sums
    assert host.fsh_cpu_adler32(x, len(x)) == zlib.adler32(x)


def check_vectors():
    """Every vector with its expected verdict at a few capacities, for the stand-alone program."""
    exp = D.expected()
    rec = []
    for name, fmt, body in D.accept_vectors():
        want = exp[name]
        rec.append((fmt, body, len(want), D.OK, want))
        if len(want) > 1:
            rec.append((fmt, body, len(want) - 1, D.SLOT_TOO_SMALL, want))
            rec.append((fmt, body, 0, D.SLOT_TOO_SMALL, want))
    for name, fmt, body, status in D.reject_streams():
        rec.append((fmt, body, 4096, status, b""))
        if name not in ("zlib_adler", "gzip_crc", "gzip_isize"):  # a checksum is judged only on a body that fits
            rec.append((fmt, body, 0, status, b""))
    for fmt in (D.RAW, D.ZLIB, D.GZIP):
        for body, want in D.mutation_set(fmt)[:300]:
            if want is not None:
                rec.append((fmt, body, len(want), D.OK, want))
    fam = R.random_family()
    for k, s in enumerate(fam[:8] + fam[8::10]):  # the worst-case tables and every tenth random stream
        fmt = k % 3
        n = len(s.expected)
        rec.append((fmt, s.body(fmt), n, D.OK, s.expected))
        cap = R.inner_capacity(s, fmt)[0]
        if cap is not None:
            rec.append((fmt, s.body(fmt), cap, D.SLOT_TOO_SMALL, s.expected))
    return rec


def test_host_model_sanitized(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = tmp_path / "inflate_check"
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-I", str(REPO / "flare-cpp_amd" / "host"),
                        str(REPO / "tests" / "cpp" / "inflate_check.cc"),
                        str(REPO / "flare-cpp_amd" / "host" / "inflate_cpu.cc"), "-o", str(exe)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    rec = check_vectors()
    with open(tmp_path / "vectors.bin", "wb") as f:
        for fmt, body, cap, status, want in rec:
            ln = len(want) if status in (D.OK, D.SLOT_TOO_SMALL) else 0
            f.write(struct.pack("<5I", fmt, len(body), cap, status, ln) + body + (want if status == D.OK else b""))
    r = subprocess.run([str(exe), str(tmp_path / "vectors.bin")], capture_output=True, text=True, timeout=600,
                       env={"ASAN_OPTIONS": "detect_leaks=0"})
    assert r.returncode == 0 and r.stdout.strip() == f"ok {len(rec)}", r.stdout[-2000:] + r.stderr[-3000:]


# ---- the seeded family of tests/deflate_random.py

def vector_digest(vectors):
    h = hashlib.sha256()
    for v in vectors:
        for x in v:
            x = x if isinstance(x, bytes) else str(x).encode()
            h.update(len(x).to_bytes(4, "little") + x)
    return h.hexdigest()


def test_writer_changes_keep_the_old_vectors():
    """The digests were taken before Deflate.dynamic got hclen and Bits.code
    stopped putting bit by bit.  The hand-built streams depend on the writer
    alone; the whole sets also hold zlib 1.2.11's compressor output."""
    assert vector_digest(D.accept_streams()) == "813e0aa3c80aa4a5ff9d1309823bb15385341149fc2082a421a09ab15cf2bc08"
    assert vector_digest(D.accept_vectors()) == "4fe8f586d18e5f8b26a431ec65eaeaafd6a34ae0450e7d0faab87b0d2484a0f6"
    assert vector_digest(D.reject_streams()) == "75219d17b9ff4a37893b34185dc302a6258055bf819c759ffc63ded5a50e36c0"


FORMATS = [D.RAW, D.ZLIB, D.GZIP]


@pytest.mark.parametrize("fmt", FORMATS)
def test_random_family_is_valid_for_zlib(fmt):
    """A generator bug fails here, not on the GPU."""
    for s in R.random_family():
        got = D.zlib_verdict(fmt, s.body(fmt))
        assert got is not None, s.name
        assert got == s.expected, s.name


@pytest.mark.parametrize("fmt", FORMATS)
def test_random_family_host_model(host, fmt):
    for s in R.random_family():
        body, n = s.body(fmt), len(s.expected)
        assert inflate(host, fmt, body, n) == (D.OK, n, s.expected), s.name
        assert length(host, fmt, body) == (D.OK, n), s.name
        for cap in sorted({0, n - 1, R.inner_capacity(s, fmt)[0]} - {None, -1, n}):
            assert inflate(host, fmt, body, cap) == (D.SLOT_TOO_SMALL, n, None), (s.name, cap)


def test_random_family_coverage():
    """Floors on what the generator places; table_entries restates the
    decoder's sizing rule and only measures the family."""
    fam = R.random_family()
    assert len(fam) == 308 and sum(len(s.raw) for s in fam) < 1_500_000
    assert R.table_entries([0] * 30, 6) == 2 and R.table_entries([0, 1], 6) == 2
    assert R.table_entries(D.FIXED_LL, 9) == 512 and R.table_entries(D.FIXED_D, 6) == 32
    staircase = list(range(1, 15)) + [15, 15]  # dynamic_15_bit_codes: 512 + 64
    assert R.table_entries(staircase, 9) == 576
    for s in fam[:8]:
        ll, dd = s.stats["ll_lens"], s.stats["d_lens"]
        assert R.table_entries(ll, 9) == 852 and R.table_entries(dd, 6) == 592, s.name
        assert all(ll) and all(dd) and len(ll) == 286 and len(dd) == 30  # every symbol is coded and used
        assert s.stats["used_ll"] == set(range(286)) and s.stats["used_d"] == set(range(30)), s.name
    for s in fam[:2]:  # the 48-bit symbol (15 + 5 + 15 + 13 bits) at the phases of the 32-bit refill
        ll, dd = s.stats["ll_lens"], s.stats["d_lens"]
        assert sorted(i for i, n in enumerate(ll) if n == 15)[0] >= 281 and ll[285] != 15
        assert dd[28] == dd[29] == 15
        marks = s.stats["long_marks"]
        assert s.stats["longest_run"] >= 40 and len({m % 32 for m in marks}) >= 16
    total, hclens = R.family_totals()
    assert total["ll_15_bit"] >= 50 and total["d_15_bit"] >= 50
    for kind in ("stored", "fixed", "dynamic"):
        assert total[kind] >= 200, kind
    assert total["stored_len_0"] >= 1 and total["stored_len_65535"] >= 1 and total["stored_misaligned"] >= 100
    assert total["no_distance_code"] >= 5 and total["single_distance_code"] >= 5
    assert total["boundary_repeat_headers"] >= 30
    assert len(hclens) >= 8
    assert total["cl_7_bit"] >= 20
    for cls in R.DIST_CLASSES:
        assert total["d_" + cls] >= 500, cls
    assert total["groups64_over_12000"] >= 20
    assert total["groups64_all_258"] >= 1
    assert total["chains_over_24"] >= 20 and total["max_chain"] >= 36  # resolution through dozens of records
    for fmt in FORMATS:  # what the device's count-only test relies on
        inside = [R.inner_capacity(s, fmt)[1] for s in fam]
        assert inside.count("copy") >= 100 and inside.count("stored") >= 20, fmt


def test_hand_built_unit_bodies(host):
    """The indexed gzip bodies of the device's units test: zlib's bytes are
    the generator's, the unit slices inflate alone where no unit reaches below
    its first byte, and the host model's route says so."""
    import gzip_index_cases as G
    cases = R.unit_bodies()
    assert len(cases) == 40 and sum(not p for _, _, p in cases) == 5
    for body, data, parallel in cases:
        assert D.zlib_verdict(D.GZIP, body) == data
        assert inflate(host, D.GZIP, body, len(data)) == (D.OK, len(data), data)
        route, units = G.route(body, len(data))
        assert 2 <= units <= 6
        if parallel:
            assert route == G.PARALLEL and G.slices(body) == data
        else:
            assert route == G.MISMATCH and G.slices(body) is None


@pytest.mark.parametrize("fmt", FORMATS)
def test_hand_built_flips_match_zlib(host, fmt):
    accepted = 0
    flips = R.hand_flip_set(fmt)
    for body, want in flips:
        cap = len(want) if want is not None else 8192
        st, ln, got = inflate(host, fmt, body, cap)
        assert (st == D.OK) == (want is not None), (fmt, body.hex())
        if want is not None:
            assert got == want
            accepted += 1
    if fmt == D.RAW:  # neither side of the comparison is empty
        assert 0.05 * len(flips) <= accepted <= 0.95 * len(flips), accepted


# ---- the public header and the argument checks, no GPU

def test_header_symbols_exported():
    names = fsg.header_symbols(REPO / "include" / "flare_deflate_gpu.h")
    assert names == ["fsg_adler32_batch", "fsg_crc32_batch", "fsg_inflate_batch", "fsg_inflate_lengths_batch"]
    lib = fsg.load_gpu_lib()
    assert all(hasattr(lib, s) for s in names) and set(names) <= set(fsg.header_symbols())


def test_invalid_arguments_rejected_without_gpu():
    lib = fsg.load_gpu_lib()
    one = ctypes.c_uint64(1).value  # any non-null value: rejected before it is looked at
    assert lib.fsg_inflate_batch(None, None, None, 5, None, None, None, None, None, D.ZLIB, None) == -1
    assert lib.fsg_inflate_lengths_batch(None, None, None, 5, None, None, D.RAW, None) == -1
    assert lib.fsg_crc32_batch(None, None, None, 5, None, None) == -1
    assert lib.fsg_adler32_batch(None, None, None, 5, None, None) == -1
    for fmt in (3, 7, 0xFFFFFFFF):  # an unknown format, whatever the pointers and the count
        assert lib.fsg_inflate_batch(one, one, one, 5, one, one, one, one, one, fmt, None) == -1
        assert lib.fsg_inflate_batch(None, None, None, 0, None, None, None, None, None, fmt, None) == -1
        assert lib.fsg_inflate_lengths_batch(one, one, one, 5, one, one, fmt, None) == -1
    # an empty batch succeeds and launches nothing
    assert lib.fsg_inflate_batch(None, None, None, 0, None, None, None, None, None, D.GZIP, None) == 0
    assert lib.fsg_inflate_lengths_batch(None, None, None, 0, None, None, D.ZLIB, None) == 0
    assert lib.fsg_crc32_batch(None, None, None, 0, None, None) == 0
    assert lib.fsg_adler32_batch(None, None, None, 0, None, None) == 0
