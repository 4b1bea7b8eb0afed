"""Bodies for the unit-index tests (tests/test_gzip_index.py on the host model,
tests/test_inflate_units_gpu.py and tests/test_deflate_index_gpu.py on the
device): gzip bodies that carry dictzip's `RA` subfield (csrc/gzip_index.h).

Own bodies come from the host writer (fsh_cpu_deflate_flags).  FOREIGN bodies
are written by Python's zlib: compressobj(level, DEFLATED, -15), per chunk of
CHLEN bytes compress(chunk) + flush(Z_FULL_FLUSH), flush(Z_FINISH) last, and a
hand-built head.  A full flush ends on a byte boundary and forgets the window,
so every unit slice inflates alone; a unit boundary can sit anywhere, which
keeps every case small.  With Z_SYNC_FLUSH the window is kept and units depend
on their predecessors: the mismatch fixture.

Python's zlib is the judge everywhere: D.zlib_verdict for the whole body, and
slices() inflates the indexed slices one by one."""
from __future__ import annotations

import ctypes
import functools
import struct
import zlib

import deflate_cases as C
import deflate_streams as D

U = C.U
GZIP = D.GZIP
FLAG = 1  # FSG_DEFLATE_FLAG_UNIT_INDEX
PARALLEL, NO_INDEX, UNUSABLE, MISMATCH = 0, 1, 2, 3  # FSH_UNITS_ROUTE_*
INDEX_NONE, INDEX_UNUSABLE, INDEX_USABLE = 0, 1, 2
OK, CORRUPT, BAD_HEADER, SLOT_TOO_SMALL = 0, 1, 2, 3


@functools.lru_cache(maxsize=None)
def host():
    L = C.host()
    c = ctypes
    L.fsh_cpu_deflate_flags.argtypes = [c.c_uint32, c.c_uint32, c.c_uint32, c.c_char_p, c.c_size_t, c.c_void_p,
                                        c.c_size_t, c.POINTER(c.c_uint64)]
    L.fsh_cpu_deflate_bound_flags.argtypes = [c.c_size_t, c.c_uint32, c.c_uint32]
    L.fsh_cpu_deflate_bound_flags.restype = c.c_size_t
    L.fsh_cpu_deflate_level.argtypes = [c.c_uint32, c.c_uint32, c.c_char_p, c.c_size_t, c.c_void_p, c.c_size_t,
                                        c.POINTER(c.c_uint64)]
    L.fsh_cpu_gzip_index.argtypes = [c.c_char_p, c.c_size_t, c.POINTER(c.c_uint32), c.POINTER(c.c_uint32),
                                     c.POINTER(c.c_uint64), c.c_size_t]
    L.fsh_cpu_inflate_units_route.argtypes = [c.c_uint32, c.c_char_p, c.c_size_t, c.c_size_t, c.c_int,
                                              c.POINTER(c.c_uint32)]
    L.fsh_cpu_inflate.argtypes = [c.c_uint32, c.c_char_p, c.c_size_t, c.c_void_p, c.c_size_t, c.POINTER(c.c_uint64)]
    return L


def bound(n: int, fmt: int = GZIP, flags: int = FLAG) -> int:
    """The issue's formula for fsg_deflate_max_length_flags."""
    units = max(1, -(-n // U))
    return C.bound(n, fmt) + (12 + 2 * units if flags and fmt == GZIP and units <= 32762 else 0)


@functools.lru_cache(maxsize=None)
def own(data: bytes, level: int = 1, flags: int = FLAG, fmt: int = GZIP) -> bytes:
    """The host writer's flagged body: the definition of the device's bytes."""
    cap = host().fsh_cpu_deflate_bound_flags(len(data), fmt, flags)
    out = ctypes.create_string_buffer(cap + 32)
    out[cap:cap + 32] = C.GUARD
    ln = ctypes.c_uint64(99)
    st = host().fsh_cpu_deflate_flags(fmt, level, flags, data, len(data), out, cap, ctypes.byref(ln))
    assert st == 0 and ln.value <= cap and out.raw[cap:] == C.GUARD
    return out.raw[:ln.value]


def index(body: bytes):
    """fsh_cpu_gzip_index: (state, chlen, chcnt, unit starts)."""
    chlen, chcnt = ctypes.c_uint32(0), ctypes.c_uint32(0)
    starts = (ctypes.c_uint64 * 32768)()
    st = host().fsh_cpu_gzip_index(body, len(body), ctypes.byref(chlen), ctypes.byref(chcnt), starts, 32768)
    return st, chlen.value, chcnt.value, [int(v) for v in starts[:chcnt.value]]


def route(body: bytes, cap=None, fmt: int = GZIP, store: bool = True):
    """fsh_cpu_inflate_units_route: (route, unit entries)."""
    units = ctypes.c_uint32(77)
    r = host().fsh_cpu_inflate_units_route(fmt, body, len(body), len(body) * 1100 + 64 if cap is None else cap,
                                           1 if store else 0, ctypes.byref(units))
    return r, units.value


def host_inflate(body: bytes, cap: int, fmt: int = GZIP):
    out = ctypes.create_string_buffer(cap + 1)
    ln = ctypes.c_uint64(0)
    st = host().fsh_cpu_inflate(fmt, body, len(body), out, cap, ctypes.byref(ln))
    return st, ln.value, out.raw[:min(ln.value, cap)]


def slices(body: bytes):
    """The independent judge: the indexed slices inflated one by one by zlib,
    joined -- or None when a slice does not inflate alone, a slice in front of
    the last is not exactly CHLEN bytes or ends its stream, or bytes are left."""
    st, chlen, chcnt, starts = index(body)
    assert st == INDEX_USABLE
    ends = starts[1:] + [len(body) - 8]
    out = []
    for k, (a, b) in enumerate(zip(starts, ends)):
        d = zlib.decompressobj(-15)
        try:
            o = d.decompress(body[a:b])
        except zlib.error:
            return None
        last = k + 1 == chcnt
        if d.unused_data or d.eof != last or (not last and len(o) != chlen):
            return None
        out.append(o)
    return b"".join(out)


# ---- foreign bodies

def parts_of(data: bytes, chlen: int, level: int = 6, flush=zlib.Z_FULL_FLUSH):
    co = zlib.compressobj(level, zlib.DEFLATED, -15)
    chunks = [data[i:i + chlen] for i in range(0, len(data), chlen)] or [b""]
    return [co.compress(c) + co.flush(flush if k + 1 < len(chunks) else zlib.Z_FINISH) for k, c in enumerate(chunks)]


def subfield(si: bytes, data: bytes) -> bytes:
    return si + struct.pack("<H", len(data)) + data


def ra(chlen: int, sizes, *, ver=1, chcnt=None, len_adj=0) -> bytes:
    body = struct.pack("<HHH", ver, chlen, len(sizes) if chcnt is None else chcnt)
    body += b"".join(struct.pack("<H", s) for s in sizes)
    return b"RA" + struct.pack("<H", len(body) + len_adj) + body


def assemble(parts, data: bytes, extra: bytes, *, fhcrc=False) -> bytes:
    h = b"\x1f\x8b\x08" + bytes([4 | (2 if fhcrc else 0)]) + b"\x00\x00\x00\x00\x00\x03"
    h += struct.pack("<H", len(extra)) + extra
    if fhcrc:
        h += struct.pack("<H", zlib.crc32(h) & 0xffff)
    return h + b"".join(parts) + struct.pack("<II", zlib.crc32(data), len(data) & 0xffffffff)


def foreign(data: bytes, chlen: int, level: int = 6, flush=zlib.Z_FULL_FLUSH, **kw) -> bytes:
    parts = parts_of(data, chlen, level, flush)
    return assemble(parts, data, ra(chlen, [len(p) for p in parts]), **kw)


TEXT5K = D.text(5000, 41)
CHCNTS = (1, 2, 63, 64, 65, 200)
OWN_SIZES = (0, 1, U - 1, U, U + 1, 2 * U, 3 * U + 5)


@functools.lru_cache(maxsize=None)
def parallel_bodies():
    """(name, body, data): bodies the route model must call parallel."""
    out = []
    for n in OWN_SIZES:
        data = D.text(n, 3)
        for level in (0, 1, 2):
            out.append((f"own_{n}_l{level}", own(data, level), data))
    out.append(("own_noise", own(D.noise(U + 100, 4)), D.noise(U + 100, 4)))
    for cnt in CHCNTS:
        chlen = 64 if cnt < 200 else 7
        data = D.text(cnt * chlen - 3, cnt)
        out.append((f"foreign_{cnt}x{chlen}", foreign(data, chlen), data))
    for chlen in (1, 1000, 65535):
        data = D.text(5 if chlen == 1 else 2 * chlen + 17, chlen)
        out.append((f"foreign_chlen{chlen}", foreign(data, chlen), data))
    data = D.noise(3000, 8)
    out.append(("foreign_stored", foreign(data, 1000, 0), data))
    out.append(("foreign_fixed", foreign(D.text(300, 9), 100, 1), D.text(300, 9)))
    parts = parts_of(TEXT5K, 1000)
    sizes = [len(p) for p in parts]
    out.append(("ra_behind_another", assemble(parts, TEXT5K, subfield(b"XY", b"abc") + ra(1000, sizes)), TEXT5K))
    out.append(("ra_before_another", assemble(parts, TEXT5K, ra(1000, sizes) + subfield(b"XY", b"abc")), TEXT5K))
    out.append(("fhcrc", foreign(TEXT5K, 1000, fhcrc=True), TEXT5K))
    out.append(("exact_multiple", foreign(TEXT5K, 1250), TEXT5K))
    return out


def _bfinal_mid():
    """Chunk 1 is a stream of its own, ended with Z_FINISH: BFINAL inside the body."""
    chunks = [TEXT5K[i:i + 1000] for i in range(0, 5000, 1000)]
    parts = []
    for k, c in enumerate(chunks):
        co = zlib.compressobj(6, zlib.DEFLATED, -15)
        parts.append(co.compress(c) + co.flush(zlib.Z_FINISH if k in (1, 4) else zlib.Z_FULL_FLUSH))
    return assemble(parts, TEXT5K, ra(1000, [len(p) for p in parts]))


@functools.lru_cache(maxsize=None)
def mismatch_bodies():
    """(name, body): a usable index whose units are not clean."""
    parts = parts_of(TEXT5K, 1000)
    sizes = [len(p) for p in parts]
    out = [("sync_flush", foreign(D.text(20000, 42), 1000, 6, zlib.Z_SYNC_FLUSH))]
    for d in (1, -1):
        bent = list(sizes)
        bent[1] += d
        out.append((f"size{d:+d}", assemble(parts, TEXT5K, ra(1000, bent))))
        out.append((f"chlen{d:+d}", assemble(parts, TEXT5K, ra(1000 + d, sizes))))
    out.append(("bfinal_mid", _bfinal_mid()))
    return out


@functools.lru_cache(maxsize=None)
def unusable_bodies():
    """(name, body): an RA subfield, or a chain, that misses a rule."""
    parts = parts_of(TEXT5K, 1000)
    sizes = [len(p) for p in parts]
    good = ra(1000, sizes)
    return [
        ("ver2", assemble(parts, TEXT5K, ra(1000, sizes, ver=2))),
        ("chlen0", assemble(parts, TEXT5K, ra(0, sizes))),
        ("chcnt0", assemble(parts, TEXT5K, ra(1000, sizes, chcnt=0))),
        ("len+2", assemble(parts, TEXT5K, ra(1000, sizes, len_adj=2) + b"\x00\x00")),
        ("len-2", assemble(parts, TEXT5K, ra(1000, sizes[:-1], chcnt=5) + struct.pack("<H", sizes[-1]))),
        ("sizes_past_stream", assemble(parts, TEXT5K, ra(1000, [60000] + sizes[1:]))),
        ("chain_past_xlen", assemble(parts, TEXT5K, b"XY" + struct.pack("<H", 60000) + good)),
        ("chain_cut", assemble(parts, TEXT5K, good + b"Z")),  # behind the index: the index is still the first RA
    ]


def plain_bodies():
    """(name, body): gzip bodies without an index."""
    parts = parts_of(TEXT5K, 1000)
    return [("no_fextra", D.compress(GZIP, TEXT5K)),
            ("other_subfield", assemble(parts, TEXT5K, subfield(b"XY", b"abc"))),
            ("empty_extra", assemble(parts, TEXT5K, b""))]


@functools.lru_cache(maxsize=None)
def fixtures():
    """(name, body, route with a roomy slot): everything above."""
    out = [(n, b, PARALLEL) for n, b, _ in parallel_bodies()]
    out += [(n, b, MISMATCH) for n, b in mismatch_bodies()]
    out += [(n, b, UNUSABLE if n != "chain_cut" else PARALLEL) for n, b in unusable_bodies()]
    out += [(n, b, NO_INDEX) for n, b in plain_bodies()]
    return out


@functools.lru_cache(maxsize=None)
def flip_set(count=2000):
    """`count` single-bit flips over one indexed body of about 5 KB, CHLEN 1000:
    (body, zlib's bytes or None)."""
    import random
    base = foreign(TEXT5K, 1000)
    r = random.Random(4141)
    out = []
    for _ in range(count):
        bit = r.randrange(8 * len(base))
        b = bytearray(base)
        b[bit >> 3] ^= 1 << (bit & 7)
        b = bytes(b)
        out.append((b, D.zlib_verdict(GZIP, b)))
    return tuple(out)
