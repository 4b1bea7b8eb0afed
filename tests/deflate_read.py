"""A small raw-deflate stream READER for the deflate compress tests: plain
Python over RFC 1951, nothing of the project's C++ in it.  It does what a
decoder does and keeps what a decoder throws away: per block the type, the
header's length in bits and, per token, the bit position at which it starts
and the bits it takes.  tests/deflate_parse_cases.py uses it to say where the
writer's long tokens lie in its bit window; tests/test_deflate_parse.py checks
it against deflate_streams.Deflate, the writer of the inflate tests.

Tokens are deflate_streams' own: an int 0..255 is a literal, (length,
distance) a copy.  The end-of-block code is a block's `eob` pair, not a token."""
from __future__ import annotations

from dataclasses import dataclass, field

from deflate_streams import CL_ORDER, DIST_BASE, DIST_EXTRA, FIXED_D, FIXED_LL, LEN_BASE, LEN_EXTRA, canonical


@dataclass
class Block:
    btype: int
    final: bool
    start: int           # bit position of BFINAL
    header_bits: int     # BFINAL to the last bit before the first token (stored: to the last bit of NLEN)
    tokens: list = field(default_factory=list)   # literal int or (length, distance)
    pos: list = field(default_factory=list)      # bit position of each token's first bit
    nbits: list = field(default_factory=list)    # bits of each token, extra bits included
    eob: tuple = (0, 0)  # (position, bits) of the end-of-block code; stored: (end of the data, 0)
    end: int = 0         # bit position behind the block


class _Bits:
    def __init__(self, raw: bytes):
        self.v = int.from_bytes(raw, "little")
        self.n = 8 * len(raw)
        self.at = 0

    def take(self, k: int) -> int:
        if self.at + k > self.n:
            raise ValueError("the stream ends inside a field")
        r = (self.v >> self.at) & ((1 << k) - 1)
        self.at += k
        return r

    def symbol(self, table) -> int:
        """One Huffman symbol: table maps (length, code as sent, first bit highest) to the symbol."""
        code = 0
        for n in range(1, 16):
            code = code << 1 | self.take(1)
            s = table.get((n, code))
            if s is not None:
                return s
        raise ValueError("no code matches")


def _table(lengths):
    return {(n, code): s for s, (code, n) in canonical(list(lengths)).items()}


def read(raw: bytes):
    """(blocks, the decoded bytes, bits used).  Raises ValueError on a stream
    the RFC does not allow in a way this reader meets (it is no validator:
    Python's zlib is the judge of legality everywhere in the suite)."""
    b = _Bits(raw)
    out = bytearray()
    blocks = []
    while True:
        start = b.at
        final, btype = b.take(1), b.take(2)
        blk = Block(btype, bool(final), start, 0)
        if btype == 0:
            b.at = (b.at + 7) & ~7
            ln, nln = b.take(16), b.take(16)
            if ln ^ nln != 0xffff:
                raise ValueError("LEN / NLEN")
            blk.header_bits = b.at - start
            if b.at + 8 * ln > b.n:
                raise ValueError("stored data past the stream")
            out += raw[b.at // 8:b.at // 8 + ln]
            b.at += 8 * ln
            blk.eob = (b.at, 0)
        elif btype == 3:
            raise ValueError("BTYPE 3")
        else:
            if btype == 1:
                ll, dd = _table(FIXED_LL), _table(FIXED_D)
            else:
                hlit, hdist, hclen = b.take(5) + 257, b.take(5) + 1, b.take(4) + 4
                cl = [0] * 19
                for s in CL_ORDER[:hclen]:
                    cl[s] = b.take(3)
                clt = _table(cl)
                lens = []
                while len(lens) < hlit + hdist:
                    s = b.symbol(clt)
                    if s < 16:
                        lens.append(s)
                    elif s == 16:
                        if not lens:
                            raise ValueError("repeat with nothing before")
                        lens += [lens[-1]] * (3 + b.take(2))
                    else:
                        lens += [0] * (3 + b.take(3) if s == 17 else 11 + b.take(7))
                if len(lens) != hlit + hdist:
                    raise ValueError("repeat past the list")
                ll, dd = _table(lens[:hlit]), _table(lens[hlit:])
            blk.header_bits = b.at - start
            while True:
                at = b.at
                s = b.symbol(ll)
                if s < 256:
                    out.append(s)
                    blk.tokens.append(s)
                elif s == 256:
                    blk.eob = (at, b.at - at)
                    break
                else:
                    if s > 285:
                        raise ValueError("length symbol 286 / 287")
                    length = LEN_BASE[s - 257] + b.take(LEN_EXTRA[s - 257])
                    d = b.symbol(dd)
                    if d > 29:
                        raise ValueError("distance symbol 30 / 31")
                    dist = DIST_BASE[d] + b.take(DIST_EXTRA[d])
                    if dist > len(out):
                        raise ValueError("distance before the first byte")
                    for _ in range(length):
                        out.append(out[-dist])
                    blk.tokens.append((length, dist))
                blk.pos.append(at)
                blk.nbits.append(b.at - at)
        blk.end = b.at
        blocks.append(blk)
        if final:
            return blocks, bytes(out), b.at
