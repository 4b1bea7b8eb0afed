"""Hand-built Snappy tag streams shared by the GPU tests: valid by
construction, made of what the encoder rarely emits."""
import numpy as np


def lit_tag(b: bytes) -> bytes:
    n = len(b) - 1
    if n < 60:
        return bytes([n << 2]) + b
    k = (n.bit_length() + 7) // 8
    return bytes([(59 + k) << 2]) + n.to_bytes(k, "little") + b


def copy_tag(off: int, ln: int, wide: bool = False) -> bytes:
    if wide or off > 0xFFFF:                             # COPY_4
        return bytes([((ln - 1) << 2) | 3]) + off.to_bytes(4, "little")
    if 4 <= ln <= 11 and off < 2048:                     # COPY_1
        return bytes([((off >> 8) << 5) | ((ln - 4) << 2) | 1, off & 0xFF])
    return bytes([((ln - 1) << 2) | 2]) + off.to_bytes(2, "little")  # COPY_2


def synthetic_stream(rng, target):
    """A valid-by-construction tag stream stressing what the encoder rarely
    emits: offsets 1..15 (pattern copies) at every length 1..64, COPY_4,
    long literals (which jump the decoder's input ring), back-to-back short
    copies, and output ends at every alignment."""
    body, out = [], bytearray()
    first = bytes(rng.integers(0, 256, int(rng.integers(1, 40)), dtype=np.uint8))
    body.append(lit_tag(first)); out += first
    while len(out) < target:
        r = rng.random()
        if r < 0.45:
            off = int(rng.integers(1, min(16, len(out)) + 1))
        elif r < 0.75:
            off = int(rng.integers(1, min(300, len(out)) + 1))
        elif r < 0.85:
            off = int(rng.integers(1, len(out) + 1))
        else:
            n = int(rng.integers(1, 3000 if rng.random() < 0.1 else 30))
            lit = bytes(rng.integers(0, 256, n, dtype=np.uint8))
            body.append(lit_tag(lit)); out += lit
            continue
        ln = int(rng.integers(1, 65))
        body.append(copy_tag(off, ln, wide=rng.random() < 0.05))
        for _ in range(ln):
            out.append(out[-off])
    hdr = bytearray()
    n = len(out)
    while n >= 0x80:
        hdr.append((n & 0x7F) | 0x80); n >>= 7
    hdr.append(n)
    return bytes(hdr) + b"".join(body), bytes(out)
