"""The unit index of gzip bodies on the host (csrc/gzip_index.h,
host/gzip_index_cpu.cc, fsh_cpu_deflate_flags in host/deflate_cpu.cc): the
flagged writer, the index parse, the route model of fsg_inflate_units_batch,
and both under a sanitizer.  No GPU.  Python's zlib is the judge."""
import shutil
import struct
import subprocess
import zlib
from pathlib import Path

import pytest

import deflate_level_cases as V
import deflate_streams as D
import fsg
import gzip_index_cases as G

REPO = Path(__file__).resolve().parents[1]
U = G.U


# ---- the flagged writer

@pytest.mark.parametrize("level", [0, 1, 2])
@pytest.mark.parametrize("n", G.OWN_SIZES)
def test_flagged_host_bodies(n, level):
    data = D.text(n, 3)
    body = G.own(data, level)
    units = max(1, -(-n // U))
    head = 22 + 2 * units
    assert D.zlib_verdict(G.GZIP, body) == data
    assert body[:4] == b"\x1f\x8b\x08\x04" and body[10:22] == struct.pack("<H2sHHHH", 10 + 2 * units, b"RA",
                                                                          6 + 2 * units, 1, U, units)
    assert body[head:] == V.model(G.GZIP, level, data)[10:]  # the same stream and trailer
    st, chlen, chcnt, starts = G.index(body)
    assert (st, chlen, chcnt, starts[0]) == (G.INDEX_USABLE, U, units, head)
    ends = starts[1:] + [len(body) - 8]
    assert [b - a for a, b in zip(starts, ends)] == list(struct.unpack(f"<{units}H", body[22:head]))
    for k, (a, b) in enumerate(zip(starts, ends)):  # each slice alone
        d = zlib.decompressobj(-15)
        assert d.decompress(body[a:b]) == data[k * U:(k + 1) * U] and d.eof == (k + 1 == units) and not d.unused_data
    assert G.slices(body) == data
    assert len(body) <= G.host().fsh_cpu_deflate_bound_flags(n, G.GZIP, G.FLAG) == G.bound(n)
    if level == 0:
        assert len(body) == G.bound(n)


def test_flags_refused_and_unflagged_unchanged():
    import ctypes
    L = G.host()
    x = D.text(1000, 1)
    out = ctypes.create_string_buffer(4096)
    ln = ctypes.c_uint64(5)
    for fmt, flags in ((D.RAW, 1), (D.ZLIB, 1), (D.GZIP, 2), (D.GZIP, 3)):
        assert L.fsh_cpu_deflate_flags(fmt, 1, flags, x, len(x), out, 4096, ctypes.byref(ln)) == G.CORRUPT
        assert ln.value == 0 and L.fsh_cpu_deflate_bound_flags(len(x), fmt, flags) == 0
    for fmt in (D.RAW, D.ZLIB, D.GZIP):
        assert G.own(x, 1, 0, fmt) == V.model(fmt, 1, x)
        assert L.fsh_cpu_deflate_bound_flags(len(x), fmt, 0) == L.fsh_cpu_deflate_bound(len(x), fmt)
    cap = len(G.own(x)) - 1  # one byte short
    assert L.fsh_cpu_deflate_flags(D.GZIP, 1, 1, x, len(x), out, cap, ctypes.byref(ln)) == G.SLOT_TOO_SMALL


# ---- the index and the route model

@pytest.mark.parametrize("name", [n for n, _, _ in G.parallel_bodies()])
def test_parallel_bodies(name):
    body, data = next((b, d) for n, b, d in G.parallel_bodies() if n == name)
    assert D.zlib_verdict(G.GZIP, body) == data
    st, chlen, chcnt, starts = G.index(body)
    assert st == G.INDEX_USABLE and chcnt == max(1, -(-len(data) // chlen))
    assert G.route(body) == (G.PARALLEL, chcnt)
    assert G.route(body, store=False, cap=0) == (G.PARALLEL, chcnt)
    assert G.slices(body) == data  # the independent judge
    assert G.route(body, cap=len(data)) == (G.PARALLEL, chcnt)
    if data:
        assert G.route(body, cap=len(data) - 1) == (G.MISMATCH, chcnt)  # the serial walk says SLOT_TOO_SMALL
    assert G.host_inflate(body, len(data)) == (G.OK, len(data), data)


def test_chcnt_cases_are_covered():
    names = [n for n, _, _ in G.parallel_bodies()]
    assert all(any(n.startswith(f"foreign_{c}x") for n in names) for c in G.CHCNTS)


@pytest.mark.parametrize("name", [n for n, _ in G.mismatch_bodies()])
def test_mismatch_bodies(name):
    body = dict(G.mismatch_bodies())[name]
    st, chlen, chcnt, _ = G.index(body)
    assert st == G.INDEX_USABLE
    assert G.route(body) == (G.MISMATCH, chcnt)
    assert G.route(body, store=False) == (G.MISMATCH, chcnt)
    assert G.slices(body) is None  # zlib, slice by slice, agrees
    want = D.zlib_verdict(G.GZIP, body)  # and the serial verdict is zlib's, index or not
    assert (want is None) == (name == "bfinal_mid")
    st, ln, out = G.host_inflate(body, 30000)
    assert (st, out) == ((G.OK, want) if want is not None else (G.CORRUPT, b""))


def test_sync_flush_units_depend_on_their_predecessors():
    body = dict(G.mismatch_bodies())["sync_flush"]
    _, chlen, chcnt, starts = G.index(body)
    ends = starts[1:] + [len(body) - 8]
    alone = 0
    for a, b in zip(starts, ends):
        try:
            zlib.decompressobj(-15).decompress(body[a:b])
            alone += 1
        except zlib.error:
            pass
    assert chcnt == 20 and alone < 20


@pytest.mark.parametrize("name", [n for n, _ in G.unusable_bodies()])
def test_unusable_bodies(name):
    body = dict(G.unusable_bodies())[name]
    assert D.zlib_verdict(G.GZIP, body) == G.TEXT5K  # zlib ignores the field
    if name == "chain_cut":  # broken behind the index: still the first RA of a chain well-formed up to it
        assert G.index(body)[0] == G.INDEX_USABLE and G.route(body) == (G.PARALLEL, 5)
        return
    assert G.index(body)[0] == G.INDEX_UNUSABLE
    assert G.route(body) == (G.UNUSABLE, 1)
    assert G.host_inflate(body, 5000) == (G.OK, 5000, G.TEXT5K)


def test_plain_wrapper_decided_and_other_formats():
    for name, body in G.plain_bodies():
        assert G.index(body)[0] == G.INDEX_NONE and G.route(body) == (G.NO_INDEX, 1), name
    indexed = G.foreign(G.TEXT5K, 1000)
    for bad in (b"", b"\x1f", b"\x1f\x8b\x07" + indexed[3:], indexed[:20]):
        assert G.index(bad)[0] == G.INDEX_NONE and G.route(bad) == (G.NO_INDEX, 0)
    assert G.route(D.compress(D.ZLIB, G.TEXT5K), fmt=D.ZLIB) == (G.NO_INDEX, 1)
    assert G.route(indexed, fmt=D.RAW) == (G.NO_INDEX, 1)  # raw: the bytes are a (corrupt) stream, one walk
    assert G.route(b"", fmt=D.RAW) == (G.NO_INDEX, 0)


def test_fhcrc_is_checked_alongside_the_index():
    body = dict((n, b) for n, b, _ in G.parallel_bodies())["fhcrc"]
    assert body[3] == 6
    bent = bytearray(body)
    bent[8] ^= 1  # XFL: the header CRC no longer holds
    assert D.zlib_verdict(G.GZIP, bytes(bent)) is None
    assert G.route(bytes(bent)) == (G.NO_INDEX, 0) and G.host_inflate(bytes(bent), 5000)[0] == G.BAD_HEADER


def test_every_truncation_of_an_indexed_body_keeps_the_serial_verdict():
    body = G.foreign(G.TEXT5K, 1000)
    for n in range(len(body)):
        cut = body[:n]
        r, units = G.route(cut)
        assert r != G.PARALLEL, n
        st, ln, out = G.host_inflate(cut, 5000)
        assert st in (G.CORRUPT, G.BAD_HEADER) and ln == 0, n


# ---- the model under a sanitizer

def test_index_and_route_model_sanitized(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = tmp_path / "gzip_index_check"
    host = REPO / "flare-cpp_amd" / "host"
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", str(host), str(REPO / "tests" / "cpp" / "gzip_index_check.cc"),
                        str(host / "gzip_index_cpu.cc"), str(host / "deflate_cpu.cc"), str(host / "inflate_cpu.cc"),
                        "-o", str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    # records: u32 expected route, u32 expected units, u32 length, the body
    rec = 0
    with open(tmp_path / "vectors.bin", "wb") as f:
        for name, body, want in G.fixtures():
            f.write(struct.pack("<III", want, G.route(body)[1], len(body)) + body)
            rec += 1
    whole = G.foreign(G.TEXT5K[:2500], 500, fhcrc=True)  # every truncation of it
    (tmp_path / "trunc.bin").write_bytes(whole)
    r = subprocess.run([str(exe), str(tmp_path / "vectors.bin"), str(tmp_path / "trunc.bin")], capture_output=True,
                       text=True, timeout=900, env={"ASAN_OPTIONS": "detect_leaks=0"})
    assert r.returncode == 0 and r.stdout.strip() == f"ok {rec} {len(whole)}", r.stdout[-2000:] + r.stderr[-3000:]


# ---- GzipCompress with GzipCompressOptions::unit_index (host/gzip_compress.h)

def test_gzip_options_unit_index(tmp_path):
    """tests/cpp/test_gzip_unit_index.cc: the option at compression_level 0, 1
    and -1; Python's zlib reads every body, and the bytes are the host model's
    flagged ones for the mapped level (0 -> 0, 1 -> 1, -1 -> 2)."""
    subprocess.run(["make", "-C", str(REPO), "build/test_gzip_unit_index"], check=True, capture_output=True,
                   timeout=600)
    x = D.text(150000, 5)
    fin = tmp_path / "raw.in"
    fin.write_bytes(x)
    r = subprocess.run([str(REPO / "build" / "test_gzip_unit_index"), str(fin), str(tmp_path)], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0 and "0 failures" in r.stdout, r.stdout + r.stderr
    for name, level in (("0", 0), ("1", 1), ("m1", 2)):
        body = (tmp_path / f"index_{name}.bin").read_bytes()
        assert D.zlib_verdict(G.GZIP, body) == x
        assert body == G.own(x, level)
        assert G.route(body) == (G.PARALLEL, 3)


# ---- the public header and the argument checks, no GPU

def test_new_symbols_exported_and_declared():
    want = ["fsg_deflate_batch_flags", "fsg_deflate_max_length_flags", "fsg_inflate_units_batch",
            "fsg_inflate_units_lengths_batch", "fsg_inflate_units_report", "fsg_inflate_units_workspace_bytes"]
    assert fsg.header_symbols(REPO / "include" / "flare_deflate_index_gpu.h") == want
    lib = fsg.load_gpu_lib()
    assert all(hasattr(lib, s) for s in want)
    for n in (0, 1, U, U + 1, 5 * U):
        assert lib.fsg_deflate_max_length_flags(n, 2, 1) == G.bound(n)
        assert lib.fsg_deflate_max_length_flags(n, 2, 0) == lib.fsg_deflate_max_length(n, 2)
    assert lib.fsg_deflate_max_length_flags(32762 * U, 2, 1) == G.bound(32762 * U)
    assert lib.fsg_deflate_max_length_flags(32762 * U + 1, 2, 1) == lib.fsg_deflate_max_length(32762 * U + 1, 2)
    for fmt, flags in ((0, 1), (1, 1), (2, 2), (3, 0)):
        assert lib.fsg_deflate_max_length_flags(100, fmt, flags) == 0


def test_invalid_arguments_rejected_without_gpu():
    lib = fsg.load_gpu_lib()
    one, big = 16, 1 << 40
    inval = -1  # FSG_ERR_INVALID_ARG
    ok_ws = lib.fsg_deflate_workspace_bytes(1, 100)
    deflate = lambda fmt, level, flags, ws=one, nbytes=ok_ws: lib.fsg_deflate_batch_flags(
        one, one, one, 1, one, one, one, one, fmt, level, flags, ws, nbytes, None)
    assert deflate(0, 1, 1) == deflate(1, 1, 1) == deflate(2, 1, 2) == deflate(2, 3, 1) == deflate(3, 1, 0) == inval
    assert deflate(2, 1, 1, None) == deflate(2, 1, 1, 8) == deflate(2, 1, 1, one, 16) == inval
    assert lib.fsg_deflate_batch_flags(None, None, None, 0, None, None, None, None, 2, 1, 1, None, 0, None) == 0
    need = lib.fsg_inflate_units_workspace_bytes(1, 0)
    assert lib.fsg_inflate_units_workspace_bytes(1, 10) == need + 320 and need >= 256
    units = lambda fmt, ws, nbytes: lib.fsg_inflate_units_batch(one, one, one, 1, one, one, one, one, one, fmt, ws,
                                                                nbytes, None)
    lengths = lambda fmt, ws, nbytes: lib.fsg_inflate_units_lengths_batch(one, one, one, 1, one, one, fmt, ws, nbytes,
                                                                          None)
    for call in (units, lengths):
        assert call(3, one, big) == call(2, None, big) == call(2, 8, big) == call(2, one, need - 1) == inval
    assert lib.fsg_inflate_units_batch(None, None, None, 0, None, None, None, None, None, 2, None, 0, None) == 0
    assert lib.fsg_inflate_units_lengths_batch(None, None, None, 0, None, None, 2, None, 0, None) == 0
    assert lib.fsg_inflate_units_batch(None, one, one, 1, one, one, one, one, one, 2, one, big, None) == inval
