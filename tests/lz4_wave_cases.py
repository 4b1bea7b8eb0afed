"""Inputs for the LZ4 wave encoder's tests (test_lz4_wave_model.py on the CPU
model, test_lz4_wave_gpu.py on the kernel): the boundary family -- the
lengths around the parse's limits and the two table forms, over data kinds
that take every path of the window search -- and the shaped bodies that aim
at one rule each."""
from __future__ import annotations

import numpy as np

import fsg

LENGTHS = (0, 1, 12, 13, 14, 63, 64, 65, 65546, 65547, 65548, 131073)
PERIODS = (1, 2, 3, 15, 16, 17, 1536, 65535, 65536, 70000)


def _rand(rng, n: int) -> bytes:
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


def _periodic(rng, p: int, n: int) -> bytes:
    base = rng.integers(1, 256, p, dtype=np.uint8)
    return np.resize(base, n).tobytes() if n else b""


def length_family() -> list[tuple[str, bytes]]:
    """Every length of LENGTHS over zeros, the periods, random bytes, Zipf text."""
    rng = np.random.default_rng(4101)
    out = []
    for n in LENGTHS:
        out.append((f"zeros-{n}", bytes(n)))
        for p in PERIODS:
            out.append((f"period{p}-{n}", _periodic(rng, p, n)))
        out.append((f"random-{n}", _rand(rng, n)))
        out.append((f"text-{n}", fsg.make_batch(fsg.KIND_TEXT, [n], first_index=n % 977).item(0) if n else b""))
    return out


def shaped() -> list[tuple[str, bytes]]:
    rng = np.random.default_rng(4102)
    out = []
    # an incompressible prefix, then a repeat of it: the literal-length extension bytes
    for p in (14, 15, 16, 269, 270, 271):
        a = _rand(rng, p)
        out.append((f"prefix-{p}", a + a + _rand(rng, 13)))
    # matches of length 4 + k: the match-length extension bytes
    for k in (14, 15, 16, 269, 270, 271, 525):
        a = _rand(rng, 600)
        stop = bytes([a[4 + k] ^ 0x55])
        out.append((f"matchlen-{k}", a + _rand(rng, 7) + a[:4 + k] + stop + _rand(rng, 20)))
    # a match that runs to the end of the body (last-5-literals, ip >= mflimit + 1)
    for n in (20, 100, 1000):
        a = _rand(rng, n)
        out.append((f"match-to-end-{n}", a + a))
        out.append((f"match-to-end-{n}+zeros", a + bytes(64)))
    # backward extension down to the anchor: past 64 misses the search probes
    # every second position, so of two neighbours one is in the table; a match
    # ends at the anchor (its next byte differs) and the bytes there repeat
    # from r[260] or r[261] -- for one of the two the anchor's own position
    # misses and the next probe hits, one byte late
    r = _rand(rng, 400)
    for s in (260, 261, 262):
        out.append((f"back-to-anchor-{s}", r + r[200:230] + r[s:s + 40] + _rand(rng, 16)))
    # backward extension down to position 0
    out.append(("back-to-zero-zeros", bytes(100)))
    out.append(("back-to-zero-rep", r[:3] * 40))
    r2 = _rand(rng, 200)
    out.append(("back-to-zero-late", r2 + _rand(rng, 300) + r2 + _rand(rng, 16)))
    # 4,000 random bytes and a copy of them: the step passes 1, several windows per search
    r4 = _rand(rng, 4000)
    out.append(("random4000-twice", r4 + r4))
    out.append(("random4000-twice-tail", r4 + r4 + _rand(rng, 50)))
    # chains of immediate re-matches: period 5, a byte flipped every 40
    for n in (400, 4000, 70000):
        x = bytearray(_periodic(rng, 5, n))
        for i in range(17, n, 40):
            x[i] ^= 0x21
        out.append((f"rematch-chain-{n}", bytes(x)))
    return out


def boundary_family() -> list[tuple[str, bytes]]:
    return length_family() + shaped()


def random_bodies(seed: int, count: int, sizes) -> list[bytes]:
    """`count` bodies over alphabets of 1, 2, 4 or 256 symbols; sizes(rng) -> n."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        n = int(sizes(rng))
        out.append(rng.integers(0, int(rng.choice([1, 2, 4, 256])), n, dtype=np.uint8).tobytes())
    return out
