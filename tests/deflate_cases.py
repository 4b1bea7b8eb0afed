"""The input family of the deflate compress tests (tests/test_deflate.py on the
host model, tests/test_deflate_gpu.py on the device): the smallest shapes at
which each piece of csrc/deflate_format.h can go wrong.  cases() is a list of
(name, bytes); everything is seeded, so the host model's bytes are computed
once per process and shared."""
from __future__ import annotations

import functools

import numpy as np

import deflate_streams as D

U = 65472  # defl::kUnit
RAW, ZLIB, GZIP = D.RAW, D.ZLIB, D.GZIP
WBITS = {RAW: -15, ZLIB: 15, GZIP: 31}
WRAPPER = {RAW: 0, ZLIB: 6, GZIP: 18}


def bound(n: int, fmt: int) -> int:
    """The issue's formula for fsg_deflate_max_length."""
    return n + 5 * max(1, -(-n // U)) + WRAPPER[fmt]


def alphabet(n: int, values: int, seed: int = 0) -> bytes:
    rng = np.random.default_rng(1000 + 7 * values + seed)
    return rng.integers(0, values, n, dtype=np.uint8).tobytes() if values > 1 else b"q" * n


def repeat_at(dist: int) -> bytes:
    """50 bytes of noise, then a 100-byte string without a zero and the same
    string `dist` bytes further on, zeros between them (one hash slot: the
    single-candidate table still holds the first copy when the second comes).
    For dist < 100: a string of period dist, 100 + dist long."""
    s = bytes(b % 255 + 1 for b in D.noise(100, 77))
    if dist >= 100:
        return D.noise(50, 5) + s + bytes(dist - 100) + s
    return D.noise(50, 5) + (s[:dist] * (200 // dist + 2))[:100 + dist]


def fibonacci_body() -> bytes:
    """24 byte values, 21 of them with Fibonacci counts 1, 1, 2, ... 10,946 and
    three more seen once, shuffled: 28,659 bytes whose Huffman code is deeper
    than 15 bits."""
    rng = np.random.default_rng(24)
    values = rng.permutation(256)[:24]
    fib = [1, 1]
    while len(fib) < 21:
        fib.append(fib[-1] + fib[-2])
    counts = fib + [1, 1, 1]
    body = np.repeat(values.astype(np.uint8), counts)
    rng.shuffle(body)
    assert len(body) < 40000
    return body.tobytes()


def deep_body() -> bytes:
    """A body whose literal code IS deeper than 15 bits after the parse, which
    fibonacci_body() is not.  Its 28,659 bytes have an entropy of 2.4 bits a
    byte, so their 4-byte strings must repeat, the parse turns most of them
    into matches and the Huffman code of what is left is 14 deep; besides, the
    end-of-block symbol's count of 1 next to exact Fibonacci counts makes the
    merge pair up and halves the depth.  Here 12 byte values with counts 1, 2,
    4, 7, 12, ... 375 (each the sum of the two before plus 1, so the chain
    holds with the end-of-block symbol in it) are scattered over noise on 200
    other values, 39,000 bytes in all: almost nothing matches, the rare
    values' subtree is 12 deep and hangs several levels below the root."""
    rng = np.random.default_rng(16)
    values = rng.permutation(256)
    w = [1, 2]
    while len(w) < 12:
        w.append(w[-1] + w[-2] + 1)
    rare = np.repeat(values[:12].astype(np.uint8), w)
    body = np.concatenate([rare, values[12:212][rng.integers(0, 200, 39000 - len(rare))].astype(np.uint8)])
    rng.shuffle(body)
    return body.tobytes()


def straddle() -> bytes:
    """A 200-byte string that ends a unit's worth of noise 100 bytes past the
    unit boundary, and again right behind: the second copy lies in unit 2 and
    may match only the 100 bytes of the first that unit 2 holds."""
    s = D.noise(200, 9)
    return D.noise(U - 100, 10) + s + s + D.text(500, 3)


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    for n in (0, 1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129):
        out.append((f"text_{n}", D.text(n, n)))
        out.append((f"noise_{n}", D.noise(n, n)))
    for n in (U - 1, U, U + 1, 2 * U, 2 * U + 1, 300000):
        out.append((f"text_{n}", D.text(n, 1)))
    out.append((f"noise_{U + 1}", D.noise(U + 1, 2)))
    for values in (1, 2, 4, 256):
        out.append((f"alphabet{values}_1000", alphabet(1000, values)))
        out.append((f"alphabet{values}_70000", alphabet(70000, values, 1)))
    for r in (257, 258, 259, 260, 516, 517):
        out.append((f"run_{r}", b"z" * r))
        out.append((f"xyz_run_{r}", b"xyz" + b"z" * r))
    for d in (1, 3, 4, 63, 64, 65, 32767, 32768, 32769):
        out.append((f"repeat_at_{d}", repeat_at(d)))
    out.append(("straddle", straddle()))
    out.append(("all_256_once", bytes(range(256))))
    rng = np.random.default_rng(3)
    out.append(("all_256_equally", b"".join(rng.permutation(256).astype(np.uint8).tobytes() for _ in range(40))))
    out.append(("fibonacci", fibonacci_body()))
    out.append(("fibonacci_deep", deep_body()))
    out.append(("literals_only", b"abcdefgh"))
    out.append(("one_distance", bytes(range(64)) + bytes(range(10))))
    out.append(("one_byte", b"\x00"))
    out.append(("block_choice", block_choice()))
    return out


def block_choice() -> bytes:
    """Three units: text (dynamic), noise (stored), text (dynamic)."""
    return D.text(U, 11) + D.noise(U, 12) + D.text(30000, 13)


def by_name(name: str) -> bytes:
    return dict(cases())[name]


# ---- the host model (host/deflate_cpu.cc through libflare_rpc_snappy.so)

@functools.lru_cache(maxsize=None)
def host():
    import ctypes
    import subprocess
    from pathlib import Path
    repo = Path(__file__).resolve().parents[1]
    lib = repo / "flare-cpp_amd" / "lib" / "libflare_rpc_snappy.so"
    if not lib.exists():
        subprocess.run(["make", "-C", str(repo), "host"], check=True, capture_output=True)
    L = ctypes.CDLL(str(lib))
    c = ctypes
    L.fsh_cpu_deflate.argtypes = [c.c_uint32, c.c_char_p, c.c_size_t, c.c_void_p, c.c_size_t, c.POINTER(c.c_uint64)]
    L.fsh_cpu_deflate_bound.argtypes = [c.c_size_t, c.c_uint32]
    L.fsh_cpu_deflate_bound.restype = c.c_size_t
    L.fsh_cpu_deflate_unit_types.argtypes = [c.c_char_p, c.c_size_t, c.POINTER(c.c_uint64)]
    L.fsh_cpu_deflate_unit_types.restype = None
    L.fsh_cpu_deflate_tokens.argtypes = [c.c_char_p, c.c_size_t, c.c_void_p, c.c_size_t]
    L.fsh_cpu_deflate_tokens.restype = c.c_size_t
    L.fsh_cpu_deflate_limited.argtypes = [c.c_char_p, c.c_size_t]
    L.fsh_cpu_deflate_limited.restype = c.c_uint64
    L.fsh_cpu_inflate.argtypes = [c.c_uint32, c.c_char_p, c.c_size_t, c.c_void_p, c.c_size_t, c.POINTER(c.c_uint64)]
    return L


GUARD = b"\xa5" * 32


def deflate_into(fmt: int, data: bytes, cap: int):
    """(status, length, the cap bytes of the buffer): fsh_cpu_deflate into a
    buffer of cap bytes filled with GUARD and followed by GUARD, which must
    stay as it was."""
    import ctypes
    out = ctypes.create_string_buffer((GUARD * (cap // 32 + 2))[:cap + 32], cap + 32)
    ln = ctypes.c_uint64(99)
    st = host().fsh_cpu_deflate(fmt, data, len(data), out, cap, ctypes.byref(ln))
    assert out.raw[cap:] == GUARD, "the host model wrote past the capacity"
    return st, ln.value, out.raw[:cap]


@functools.lru_cache(maxsize=None)
def model(fmt: int, data: bytes) -> bytes:
    """The host model's body for `data`: the definition of the device's bytes."""
    cap = host().fsh_cpu_deflate_bound(len(data), fmt)
    st, ln, buf = deflate_into(fmt, data, cap)
    assert st == 0 and ln <= cap
    return buf[:ln]


def unit_types(data: bytes):
    """(stored, fixed, dynamic) units the model chooses for `data`."""
    import ctypes
    counts = (ctypes.c_uint64 * 3)()
    host().fsh_cpu_deflate_unit_types(data, len(data), counts)
    return tuple(int(v) for v in counts)


def tokens(data: bytes):
    """The model's parse of one unit: a list of ("lit", byte) / ("match", length, distance)."""
    import ctypes
    buf = (ctypes.c_uint32 * (len(data) + 1))()
    k = host().fsh_cpu_deflate_tokens(data, len(data), buf, len(data) + 1)
    assert k or not data
    return [("lit", t & 0xff) if t >> 31 else ("match", t & 511, (t >> 9) & 0x1ffff) for t in buf[:k]]
