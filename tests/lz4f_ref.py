"""TEST INFRASTRUCTURE ONLY: the LZ4 frame oracle (LZ4 Frame Format 1.6.x;
include/flare_lz4_gpu.h, "LZ4 frames", states the rules).

* `compress_frame`: a frame writer composed from bind.Lz4Oracle's block
  compressor -- the bytes LZ4F_compressFrame writes with independent blocks, a
  content size, level 0 and no block checksums.
* `decode_frame`: a strict frame reader, one frame per body.  Blocks of
  independent frames go through bind.Lz4Oracle.decompress_block once their
  decoded length is known (`block_length`); linked blocks through the
  pure-Python `decode_block`, the same rules with a history.
* `xxh32`: pure Python.

Status words are the library's: 0 ok, 1 corrupt, 2 bad header, 3 slot too
small."""
from __future__ import annotations

import struct

OK, CORRUPT, BAD_HEADER, SLOT_TOO_SMALL = 0, 1, 2, 3
MAGIC = 0x184D2204
RAW = 0x80000000
NO_SIZE = None
F_INDEP, F_BSUM, F_SIZE, F_CSUM, F_RESERVED, F_DICT = 0x20, 0x10, 0x08, 0x04, 0x02, 0x01
M32 = 0xFFFFFFFF
P1, P2, P3, P4, P5 = 2654435761, 2246822519, 3266489917, 668265263, 374761393


def block_bytes(bid: int) -> int:
    return 1 << (8 + 2 * bid)


def _rotl(x, r):
    return ((x << r) | (x >> (32 - r))) & M32


def xxh32(data: bytes, seed: int = 0) -> int:
    n, i = len(data), 0
    if n >= 16:
        v = [(seed + P1 + P2) & M32, (seed + P2) & M32, seed, (seed - P1) & M32]
        words = struct.unpack_from("<%dI" % (n // 16 * 4), data)
        for j in range(0, len(words), 4):
            for k in range(4):
                v[k] = (_rotl((v[k] + words[j + k] * P2) & M32, 13) * P1) & M32
        i = n // 16 * 16
        h = (_rotl(v[0], 1) + _rotl(v[1], 7) + _rotl(v[2], 12) + _rotl(v[3], 18)) & M32
    else:
        h = (seed + P5) & M32
    h = (h + n) & M32
    while i + 4 <= n:
        h = (_rotl((h + struct.unpack_from("<I", data, i)[0] * P3) & M32, 17) * P4) & M32
        i += 4
    while i < n:
        h = (_rotl((h + data[i] * P5) & M32, 11) * P1) & M32
        i += 1
    h ^= h >> 15
    h = (h * P2) & M32
    h ^= h >> 13
    h = (h * P3) & M32
    h ^= h >> 16
    return h


def max_frame_length(n: int, bid: int) -> int:
    bs = block_bytes(bid)
    return n + 4 * ((n + bs - 1) // bs) + 23


def frame_block_id(n: int, bid: int) -> int:
    """The id LZ4F_compressFrame writes: the smallest one, up to `bid`, whose
    block holds all n bytes (LZ4F_optimalBSID)."""
    p = 4
    while p < bid and n > block_bytes(p):
        p += 1
    return p


def header(n: int | None, bid: int, checksum: bool, indep: bool = True, bsum: bool = False) -> bytes:
    flg = 0x40 | (F_INDEP if indep else 0) | (F_BSUM if bsum else 0) | (F_SIZE if n else 0) | (F_CSUM if checksum else 0)
    d = bytes([flg, bid << 4]) + (struct.pack("<Q", n) if n else b"")
    return struct.pack("<I", MAGIC) + d + bytes([(xxh32(d) >> 8) & 0xFF])


def blocks_of(o, x: bytes, bid: int):
    """[(stored bytes, raw)] of the compressor's frame for x."""
    bs = block_bytes(bid)
    out = []
    for i in range(0, len(x), bs):
        part = x[i:i + bs]
        c = o.compress_block(part)
        out.append((part, True) if len(c) >= len(part) else (c, False))
    return out


def compress_frame(o, x: bytes, bid: int = 4, checksum: bool = False, bsum: bool = False) -> bytes:
    """bsum: block checksums too (the product's compressor writes none; the
    mutated-frame fixtures start from such frames)."""
    out = [header(len(x), frame_block_id(len(x), bid), checksum, bsum=bsum)]
    for b, raw in blocks_of(o, x, bid):
        out.append(struct.pack("<I", len(b) | (RAW if raw else 0)) + b)
        if bsum:
            out.append(struct.pack("<I", xxh32(b)))
    out.append(b"\0\0\0\0")
    if checksum:
        out.append(struct.pack("<I", xxh32(x)))
    return b"".join(out)


def parse_header(f: bytes):
    """(status, header length, block maximum, flg, content size or None)."""
    bad = (BAD_HEADER, 0, 0, 0, NO_SIZE)
    if len(f) < 7 or struct.unpack_from("<I", f)[0] != MAGIC:
        return bad
    flg, bd = f[4], f[5]
    if flg >> 6 != 1 or flg & (F_RESERVED | F_DICT):
        return bad
    bid = (bd >> 4) & 7
    if bd & 0x8F or bid < 4:
        return bad
    hl = 7 + (8 if flg & F_SIZE else 0)
    if len(f) < hl or (xxh32(f[4:hl - 1]) >> 8) & 0xFF != f[hl - 1]:
        return bad
    size = struct.unpack_from("<Q", f, 6)[0] if flg & F_SIZE else NO_SIZE
    return OK, hl, block_bytes(bid), flg, size


def block_length(b: bytes, limit: int):
    """Decoded length of a block from its sequences' lengths alone: the
    sequence whose literals end at the block's last byte is the last one.
    None: no such sequence, or more than `limit` bytes."""
    n, ip, op = len(b), 0, 0
    while True:
        if ip >= n:
            return None
        token = b[ip]
        ip += 1
        lit = token >> 4
        if lit == 15:
            while True:
                if ip >= n:
                    return None
                c = b[ip]
                ip += 1
                lit += c
                if c != 255:
                    break
        if lit > n - ip or op + lit > limit:
            return None
        if ip + lit == n:
            return op + lit
        ip += lit + 2
        if ip > n:
            return None
        ml = (token & 15) + 4
        if token & 15 == 15:
            while True:
                if ip >= n:
                    return None
                c = b[ip]
                ip += 1
                ml += c
                if c != 255:
                    break
        op += lit + ml
        if op > limit:
            return None


def decode_block(b: bytes, ulen: int, history: bytes = b""):
    """One block to exactly ulen bytes by the rules of lz4o_decompress_block
    (end rules against ulen, offset 0 rejected); a match may reach back into
    `history`.  Returns the bytes or None."""
    n, ip = len(b), 0
    out = bytearray(history)
    base = len(out)
    while True:
        op = len(out) - base
        if ip >= n:
            return None
        token = b[ip]
        ip += 1
        lit = token >> 4
        if lit == 15:
            while True:
                if ip >= n:
                    return None
                c = b[ip]
                ip += 1
                lit += c
                if c != 255:
                    break
        if lit > n - ip or lit > ulen - op:
            return None
        if op + lit + 12 > ulen or ip + lit + 8 > n:
            if ip + lit != n or op + lit != ulen:
                return None
            out += b[ip:ip + lit]
            return bytes(out[base:])
        out += b[ip:ip + lit]
        ip += lit
        op += lit
        off = b[ip] | (b[ip + 1] << 8)
        ip += 2
        if off == 0 or off > op + base:
            return None
        ml = (token & 15) + 4
        if token & 15 == 15:
            while True:
                if ip >= n:
                    return None
                c = b[ip]
                ip += 1
                ml += c
                if c != 255:
                    break
        if ml + 5 > ulen - op:
            return None
        start = len(out) - off
        if off >= ml:
            out += out[start:start + ml]
        else:
            piece = bytes(out[start:])
            out += (piece * (ml // off + 1))[:ml]


def decode_frame(o, f: bytes, cap: int):
    """(status, d_out_len, bytes or None) of the strict frame reader.  `o`: a
    bind.Lz4Oracle for the blocks of independent frames, or None (pure
    Python throughout)."""
    st, hl, bmax, flg, size = parse_header(f)
    if st != OK:
        return BAD_HEADER, 0, None
    if size is not NO_SIZE and size > cap:
        return SLOT_TOO_SMALL, min(size, M32), None
    limit = size if size is not NO_SIZE else cap
    bsum = 4 if flg & F_BSUM else 0
    n, ip = len(f), hl
    out = bytearray()
    bad = (CORRUPT, 0, None)
    while True:
        if n - ip < 4:
            return bad
        word = struct.unpack_from("<I", f, ip)[0]
        ip += 4
        if word == 0:
            break
        sz = word & ~RAW
        if sz > bmax or n - ip < sz + bsum:
            return bad
        blk = f[ip:ip + sz]
        ip += sz + bsum
        if bsum and xxh32(blk) != struct.unpack_from("<I", f, ip - 4)[0]:
            return bad
        if word & RAW:
            if sz > limit - len(out):
                return bad
            out += blk
            continue
        ln = block_length(blk, min(bmax, limit - len(out)))
        if ln is None:
            return bad
        if flg & F_INDEP and o is not None:
            ok, y = o.decompress_block(blk, ln)
            y = y if ok else None
        else:
            y = decode_block(blk, ln, b"" if flg & F_INDEP else bytes(out[-65535:]))
        if y is None:
            return bad
        out += y
    if flg & F_CSUM:
        if n - ip < 4 or xxh32(bytes(out)) != struct.unpack_from("<I", f, ip)[0]:
            return bad
        ip += 4
    if ip != n or (size is not NO_SIZE and len(out) != size):
        return bad
    return OK, len(out), bytes(out)
