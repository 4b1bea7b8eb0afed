"""A small deflate *writer* for the inflate tests, and the vector sets built
with it.  The writer takes chosen code lengths and a token list and returns the
bits, so a test can place what zlib's compressor never emits: 15-bit codes, a
single distance code, symbols without a code, broken headers.  Nothing here
decodes; Python's zlib (the library the reference calls) is the judge
(`zlib_verdict`).  zlib.ZLIB_RUNTIME_VERSION read 1.2.11 both on the host where
the CPU tests were written and on the MI355X host where the GPU tests ran, so
no stream was judged by two releases; the acceptance rules for deflate streams
have not changed between zlib releases, only the compressor's bytes may (the
digests of test_writer_changes_keep_the_old_vectors hold for 1.2.11's).
tests/deflate_random.py builds the seeded random family with this writer.

Tokens of a block: an int 0..255 is a literal; (length, distance) is a copy;
("ll", sym) is a raw literal/length symbol with no extra bits (286, 287);
("ld", length, dsym) is a length and then a raw distance symbol with no extra
bits (30, 31).  The end-of-block code is added unless eob=False."""
from __future__ import annotations

import functools
import random
import struct
import zlib

RAW, ZLIB, GZIP = 0, 1, 2
WBITS = {RAW: -15, ZLIB: 15, GZIP: 31}
OK, CORRUPT, BAD_HEADER, SLOT_TOO_SMALL = 0, 1, 2, 3

CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195,
            227, 258)
LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073,
             4097, 6145, 8193, 12289, 16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_D = [5] * 32


def length_symbol(length: int):
    for s in range(28, -1, -1):
        if LEN_BASE[s] <= length and (s != 28 or length == 258):
            return 257 + s, length - LEN_BASE[s], LEN_EXTRA[s]
    raise ValueError(length)


def dist_symbol(dist: int):
    for s in range(29, -1, -1):
        if DIST_BASE[s] <= dist:
            return s, dist - DIST_BASE[s], DIST_EXTRA[s]
    raise ValueError(dist)


def canonical(lengths):
    """symbol -> (code, length) by RFC 1951 3.2.2, whether the set is complete or not."""
    count = [0] * 16
    for n in lengths:
        count[n] += 1
    count[0] = 0
    code, nxt = 0, [0] * 16
    for b in range(1, 16):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    out = {}
    for s, n in enumerate(lengths):
        if n:
            out[s] = (nxt[n], n)
            nxt[n] += 1
    return out


def flat_lengths(used, nsyms):
    """A complete code over the symbols `used` (two or more): lengths b and b + 1."""
    used = sorted(used)
    k = len(used)
    assert k >= 2
    b = k.bit_length() - 1
    short = (1 << (b + 1)) - k
    lens = [0] * nsyms
    for i, s in enumerate(used):
        lens[s] = b if i < short else b + 1
    return lens


class Bits:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, v, nbits):
        """nbits of v, least significant first (header fields, extra bits)."""
        self.acc |= (v & ((1 << nbits) - 1)) << self.n
        self.n += nbits
        while self.n >= 8:
            self.out.append(self.acc & 0xff)
            self.acc >>= 8
            self.n -= 8

    def code(self, code, nbits):
        """A Huffman code: most significant bit first."""
        if nbits:  # the low nbits of the code (an over-subscribed set's codes can be wider), reversed
            self.put(int(format(code & ((1 << nbits) - 1), f"0{nbits}b")[::-1], 2), nbits)

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)

    @property
    def bitpos(self):
        return 8 * len(self.out) + self.n

    def bytes(self):
        self.align()
        return bytes(self.out)


class Deflate:
    def __init__(self):
        self.b = Bits()
        self.headers = []  # (first bit, end bit) of every dynamic block header written, BFINAL to the last length

    def header(self, final, btype):
        self.b.put(1 if final else 0, 1)
        self.b.put(btype, 2)

    def stored(self, data: bytes, final=False, nlen=None):
        self.header(final, 0)
        self.b.align()
        self.b.put(len(data), 16)
        self.b.put((len(data) ^ 0xffff) if nlen is None else nlen, 16)
        self.b.out += data
        return self

    def tokens(self, toks, ll, dd, eob=True, marks=None):
        """marks: a list that receives the bit position at which each token starts."""
        for t in toks:
            if marks is not None:
                marks.append(self.b.bitpos)
            if isinstance(t, int):
                self.b.code(*ll[t])
            elif t[0] == "ll":
                self.b.code(*ll[t[1]])
            else:
                raw_d = t[0] == "ld"
                length = t[1] if raw_d else t[0]
                s, ev, eb = length_symbol(length)
                self.b.code(*ll[s])
                self.b.put(ev, eb)
                if raw_d:
                    self.b.code(*dd[t[2]])
                else:
                    s, ev, eb = dist_symbol(t[1])
                    self.b.code(*dd[s])
                    self.b.put(ev, eb)
        if eob:
            self.b.code(*ll[256])

    def fixed(self, toks, final=False, eob=True):
        self.header(final, 1)
        self.tokens(toks, canonical(FIXED_LL), canonical(FIXED_D), eob)
        return self

    def dynamic(self, ll_lens, d_lens, toks, final=False, eob=True, cl_lens=None, cl_syms=None, hlit=None,
                hdist=None, body=True, hclen=19, marks=None):
        """ll_lens / d_lens: the code lengths the header declares.  cl_lens:
        the 19 code-length code lengths (default: a complete code over all 19);
        cl_syms: the code-length symbols to send as (sym, extra value) pairs
        (default: one plain length per symbol, no repeats).  hlit / hdist
        override the header's counts.  body=False: the header alone.  hclen: how
        many code-length code lengths are sent (4..19, in CL_ORDER); the rest are
        implied zero.  marks: see tokens()."""
        start = self.b.bitpos
        self.header(final, 2)
        ll_lens, d_lens = list(ll_lens), list(d_lens)
        if cl_lens is None:
            cl_lens = [4] * 13 + [5] * 6
        self.b.put((len(ll_lens) - 257) if hlit is None else hlit, 5)
        self.b.put((len(d_lens) - 1) if hdist is None else hdist, 5)
        self.b.put(hclen - 4, 4)
        for s in CL_ORDER[:hclen]:
            self.b.put(cl_lens[s], 3)
        cl = canonical(cl_lens)
        if cl_syms is None:
            cl_syms = [(n, 0) for n in ll_lens + d_lens]
        for sym, extra in cl_syms:
            self.b.code(*cl[sym])
            if sym >= 16:
                self.b.put(extra, {16: 2, 17: 3, 18: 7}[sym])
        self.headers.append((start, self.b.bitpos))
        if body:
            self.tokens(toks, canonical(ll_lens), canonical(d_lens), eob, marks)
        return self

    def raw(self) -> bytes:
        return self.b.bytes()


def wrap(fmt, raw: bytes, data: bytes, *, adler=None, crc=None, isize=None, flg=0, extra=b"", name=b"",
         comment=b"", hcrc=None, zhead=b"\x78\x9c") -> bytes:
    """The raw stream in the format's wrapper, with the checksums of `data`
    unless given.  gzip: FLG bits 2 / 3 / 4 / 1 add XLEN + extra, name + NUL,
    comment + NUL and the header CRC."""
    if fmt == RAW:
        return raw
    if fmt == ZLIB:
        return zhead + raw + struct.pack(">I", zlib.adler32(data) if adler is None else adler)
    h = bytearray(b"\x1f\x8b\x08" + bytes([flg]) + b"\x00\x00\x00\x00\x00\x03")
    if flg & 4:
        h += struct.pack("<H", len(extra)) + extra
    if flg & 8:
        h += name + b"\x00"
    if flg & 16:
        h += comment + b"\x00"
    if flg & 2:
        h += struct.pack("<H", (zlib.crc32(bytes(h)) & 0xffff) if hcrc is None else hcrc)
    return bytes(h) + raw + struct.pack("<II", zlib.crc32(data) if crc is None else crc,
                                        (len(data) & 0xffffffff) if isize is None else isize)


def zlib_verdict(fmt, body: bytes):
    """zlib's output when the acceptance rule holds for the body (capacity
    aside), else None."""
    d = zlib.decompressobj(WBITS[fmt])
    try:
        o = d.decompress(body)
    except zlib.error:
        return None
    return o if d.eof and not d.unused_data else None


def compress(fmt, data: bytes, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_every=0) -> bytes:
    c = zlib.compressobj(level, zlib.DEFLATED, WBITS[fmt], 8, strategy)
    if not flush_every:
        return c.compress(data) + c.flush()
    parts = []
    for i in range(0, len(data), flush_every):
        parts.append(c.compress(data[i:i + flush_every]) + c.flush(zlib.Z_SYNC_FLUSH))
    return b"".join(parts) + c.flush()


_WORDS = None


def text(n: int, seed: int = 0) -> bytes:
    global _WORDS
    if _WORDS is None:
        r = random.Random(12345)
        _WORDS = [bytes(r.choices(b"abcdefghijklmnopqrstuvwxyzETAOIN", k=r.randint(2, 9))) for _ in range(600)]
    r = random.Random(seed * 7919 + n)
    out = bytearray()
    while len(out) < n:
        out += r.choice(_WORDS)
        out += b" " if r.random() < 0.9 else b".\n"
    return bytes(out[:n])


def noise(n: int, seed: int = 0) -> bytes:
    return random.Random(seed * 104729 + n + 1).randbytes(n)


SIZES = (0, 1, 10, 100, 1000, 5000, 70000, 300000)


# ---- hand-built raw streams that zlib accepts: (name, raw stream)

def _fifteen_bit_block():
    # literals 0..14 and the end-of-block code with lengths 1, 2, ..., 14, 15, 15: sub-tables below the 9-bit root
    ll = [0] * 257
    for i in range(14):
        ll[i] = i + 1
    ll[14], ll[256] = 15, 15
    toks = [i % 15 for i in range(200)]
    return Deflate().dynamic(ll, [0], toks, final=True).raw()


def _fifteen_bit_distances():
    # distance symbols 0..15 with lengths 1..15, 15; literal/length: a flat code over what is used
    dl = [i + 1 for i in range(15)] + [15]
    toks = list(b"0123456789abcdefghijklmnopqrstuvwxyz" * 8)
    r = random.Random(5)
    for _ in range(300):
        toks.append((r.randint(3, 40), r.randint(1, 192)))
        toks.append(r.randrange(48, 58))
    used = {t for t in toks if isinstance(t, int)} | {length_symbol(t[0])[0] for t in toks if not isinstance(t, int)}
    return Deflate().dynamic(flat_lengths(used | {256}, 286), dl, toks, final=True).raw()


def accept_streams():
    out = []
    lit = list(text(400, 3))
    # every length 3..258 at distance 1 and at a far distance; every distance 1..300 and three far ones
    toks = list(lit)
    for n in range(3, 259):
        toks += [(n, 1), 65 + n % 26, (n, 37 + n)]
    out.append(("fixed_every_length", Deflate().fixed(toks, final=True).raw()))
    toks = list(lit)
    for d in range(1, 301):
        toks += [(3 + d % 9, d), 97 + d % 26]
    out.append(("fixed_every_distance_to_300", Deflate().fixed(toks, final=True).raw()))
    big = list(noise(33000, 9))
    d = Deflate()
    d.stored(bytes(big), final=False)
    d.fixed([(100, 4096), 1, (258, 32767), 2, (258, 32768), 3, (3, 32768)], final=True)
    out.append(("fixed_far_distances", d.raw()))
    # copies whose source ends 0..24 bytes below their destination, at every place in a 64-symbol group
    for gap in range(0, 25):
        toks = list(text(300, gap))
        for k in range(130):
            n = 3 + (k * 7) % 40
            toks += [(n, n + gap), 48 + k % 10] if k % 3 else [(n, n + gap)]
        out.append((f"fixed_source_gap_{gap}", Deflate().fixed(toks, final=True).raw()))
    # overlapping copies (distance below the length) chained inside one group
    toks = [65, 66, 67]
    for k in range(200):
        toks += [(3 + k % 250, 1 + k % 7), (4 + k % 30, 2 + k % 3)]
    out.append(("fixed_overlap_chains", Deflate().fixed(toks, final=True).raw()))
    out.append(("dynamic_15_bit_codes", _fifteen_bit_block()))
    out.append(("dynamic_15_bit_distance_codes", _fifteen_bit_distances()))
    # a single distance code of length 1: incomplete and legal
    ll = flat_lengths({97, 98, 256, 257, 260}, 261)
    out.append(("dynamic_single_distance_code",
                Deflate().dynamic(ll, [1], [97, 98, 97, (3, 1), (6, 1), 98], final=True).raw()))
    # no distance code at all, only literals
    ll = flat_lengths({97, 98, 99, 256}, 257)
    out.append(("dynamic_no_distance_code", Deflate().dynamic(ll, [0], [97, 98, 99] * 30, final=True).raw()))
    # a block that ends on the input's last bit
    for pad in range(0, 9):  # literal 200 has a 9-bit code: each one moves the end by one bit mod 8
        d = Deflate().fixed([97] + [200] * pad + [(5, 1)], final=True)
        if d.b.bitpos % 8 == 0:
            out.append(("fixed_ends_on_last_bit", d.raw()))
            break
    else:
        raise AssertionError("no byte-aligned end found")
    # empty stored blocks between fixed and dynamic ones; a non-final empty fixed block
    d = Deflate().fixed([104, 105], final=False).stored(b"", final=False).fixed([], final=False)
    d.dynamic(flat_lengths({33, 256, 258}, 259), [2, 2, 2, 2], [33, 33, (4, 2), (4, 4), (4, 3)], final=False)
    d.stored(b"tail", final=True)
    out.append(("mixed_block_types", d.raw()))
    # repeat codes 16, 17, 18 in the length list: 255 eights (one, then 42 times "repeat 6", then two),
    # two nines, 29 zeros (10 by a code 17, 19 by a code 18), and distance symbol 29 with length 1
    ll = [8] * 255 + [9, 9]
    syms = [(8, 0)] + [(16, 3)] * 42 + [(8, 0), (8, 0)] + [(9, 0), (9, 0)]
    dl = [0] * 29 + [1]
    syms += [(17, 10 - 3), (18, 19 - 11), (1, 0)]
    out.append(("dynamic_repeat_codes",
                Deflate().dynamic(ll, dl, list(range(0, 255)) * 2, final=True, cl_syms=syms).raw()))
    return out


# ---- streams zlib refuses, one per cause: (name, format, body, status)

def reject_streams():
    out = []
    ok_ll = flat_lengths({97, 98, 256, 257}, 258)
    add = lambda name, raw, fmt=RAW, st=CORRUPT: out.append((name, fmt, raw, st))
    add("btype_3", bytes([0b111]) + b"\x00" * 8)
    add("stored_len_nlen", Deflate().stored(b"abcd", final=True, nlen=0x1234).raw())
    add("hlit_287", Deflate().dynamic(ok_ll, [1], [97], final=True, hlit=30).raw() + b"\x00" * 64)
    add("hdist_31", Deflate().dynamic(ok_ll, [1], [97], final=True, hdist=30).raw() + b"\x00" * 64)
    add("repeat_with_nothing_before", Deflate().dynamic(ok_ll, [1], [97], final=True,
                                                        cl_syms=[(16, 0)] + [(1, 0)] * 200).raw())
    add("repeat_past_the_list", Deflate().dynamic(ok_ll, [1], [97], final=True,
                                                  cl_syms=[(n, 0) for n in ok_ll] + [(18, 127)]).raw())
    no_eob = flat_lengths({97, 98, 99, 100}, 257)
    add("no_end_of_block_code", Deflate().dynamic(no_eob, [1], [], final=True, body=False).raw() + b"\x00" * 8)
    over = list(ok_ll)
    over[99] = 1
    add("oversubscribed_literal_set", Deflate().dynamic(over, [1], [], final=True, body=False).raw() + b"\x00" * 8)
    add("oversubscribed_distance_set", Deflate().dynamic(ok_ll, [1, 1, 1], [], final=True, body=False).raw() + b"\x00" * 8)
    add("oversubscribed_code_length_code",
        Deflate().dynamic(ok_ll, [1], [], final=True, body=False, cl_lens=[1, 1, 1] + [0] * 16,
                          cl_syms=[]).raw() + b"\x00" * 8)
    inc = [0] * 257
    inc[97], inc[256] = 2, 2
    add("incomplete_literal_set", Deflate().dynamic(inc, [1], [97], final=True).raw())
    add("incomplete_distance_set", Deflate().dynamic(ok_ll, [2, 2], [97, (3, 1)], final=True).raw())
    add("incomplete_code_length_code",
        Deflate().dynamic(ok_ll, [1], [], final=True, body=False, cl_lens=[1] + [0] * 18, cl_syms=[]).raw() + b"\x00" * 64)
    add("empty_code_length_code",
        Deflate().dynamic(ok_ll, [1], [], final=True, body=False, cl_lens=[0] * 19, cl_syms=[]).raw() + b"\x00" * 64)
    add("symbol_286", Deflate().fixed([97, ("ll", 286)], final=True).raw())
    add("symbol_287", Deflate().fixed([97, ("ll", 287)], final=True).raw())
    add("distance_symbol_30", Deflate().fixed([97, 98, 99, ("ld", 3, 30)], final=True).raw())
    add("distance_symbol_31", Deflate().fixed([97, 98, 99, ("ld", 3, 31)], final=True).raw())
    # the unused half of a single-code distance set: code "1" of a set whose only code is "0"
    d2 = Deflate().dynamic(flat_lengths({97, 256, 257, 258}, 259), [1], [97], final=True, eob=False)
    ll = canonical(flat_lengths({97, 256, 257, 258}, 259))
    d2.b.code(*ll[257])
    d2.b.put(1, 1)
    d2.b.code(*ll[256])
    add("unused_half_of_single_distance_code", d2.raw())
    # the same with a literal/length set of one code: sending its other half
    one = [0] * 257
    one[256] = 1
    d3 = Deflate().dynamic(one, [0], [], final=True, eob=False)
    d3.b.put(1, 1)
    add("unused_half_of_single_literal_code", d3.raw() + b"\x00" * 4)
    d4 = Deflate().dynamic(flat_lengths({97, 256, 257}, 258), [0], [97], final=True, eob=False)
    d4.b.code(*canonical(flat_lengths({97, 256, 257}, 258))[257])
    d4.b.put(0, 1)
    add("use_of_empty_distance_set", d4.raw() + b"\x00" * 4)
    add("distance_before_first_byte", Deflate().fixed([97, 98, (3, 3)], final=True).raw())
    add("distance_before_first_byte_far", Deflate().fixed(list(text(100)) + [(3, 101)], final=True).raw())
    good = compress(RAW, text(2000, 1))
    add("input_ends_early", good[:-3])
    add("input_ends_in_dynamic_header", good[:20])
    add("no_final_block", Deflate().fixed([97, 98], final=False).raw())
    add("empty_input", b"")
    add("bytes_after_stream", good + b"\x00")
    add("stored_runs_past_input", Deflate().stored(b"abcdefgh", final=True).raw()[:-2])
    # wrappers
    data = text(2000, 1)
    z, g = compress(ZLIB, data), compress(GZIP, data)
    assert z[:2] == b"\x78\x9c"
    add("zlib_header_check", b"\x78\x9d" + z[2:], ZLIB, BAD_HEADER)
    add("zlib_cm_7", bytes([0x77, 31 - (0x7700 % 31)]) + z[2:], ZLIB, BAD_HEADER)
    add("zlib_cinfo_8", bytes([0x88, 31 - (0x8800 % 31)]) + z[2:], ZLIB, BAD_HEADER)
    add("zlib_fdict", bytes([0x78, 0x20 + 31 - (0x7820 % 31)]) + z[2:], ZLIB, BAD_HEADER)
    add("zlib_one_byte", z[:1], ZLIB, BAD_HEADER)
    add("zlib_empty", b"", ZLIB, BAD_HEADER)
    add("zlib_adler", z[:-1] + bytes([z[-1] ^ 1]), ZLIB, CORRUPT)
    add("zlib_trailer_cut", z[:-2], ZLIB, CORRUPT)
    add("zlib_header_only", z[:2], ZLIB, CORRUPT)
    add("zlib_bytes_after", z + b"\x00", ZLIB, CORRUPT)
    add("gzip_magic", b"\x1f\x8c" + g[2:], GZIP, BAD_HEADER)
    add("gzip_cm", g[:2] + b"\x07" + g[3:], GZIP, BAD_HEADER)
    add("gzip_reserved_flag", g[:3] + b"\x20" + g[4:], GZIP, BAD_HEADER)
    add("gzip_header_cut", g[:7], GZIP, BAD_HEADER)
    add("gzip_empty", b"", GZIP, BAD_HEADER)
    raw = compress(RAW, data)
    add("gzip_fextra_past_input", wrap(GZIP, b"", b"", flg=4, extra=b"xy")[:10] + b"\xff\x7f" + raw, GZIP, BAD_HEADER)
    add("gzip_fextra_length_cut", wrap(GZIP, b"", b"")[:3] + b"\x04" + b"\x00" * 6 + b"\x05", GZIP, BAD_HEADER)
    add("gzip_fname_unterminated", b"\x1f\x8b\x08\x08\x01\x01\x01\x01\x01\x03" + b"name without end", GZIP,
        BAD_HEADER)
    add("gzip_fcomment_unterminated", b"\x1f\x8b\x08\x10\x01\x01\x01\x01\x01\x03" + b"comment without end", GZIP,
        BAD_HEADER)
    add("gzip_fhcrc", wrap(GZIP, raw, data, flg=2, hcrc=0x1234), GZIP, BAD_HEADER)
    add("gzip_fhcrc_cut", wrap(GZIP, b"", b"", flg=2)[:11], GZIP, BAD_HEADER)
    add("gzip_crc", wrap(GZIP, raw, data, crc=zlib.crc32(data) ^ 0x80), GZIP, CORRUPT)
    add("gzip_isize", wrap(GZIP, raw, data, isize=len(data) + 1), GZIP, CORRUPT)
    add("gzip_trailer_cut", g[:-5], GZIP, CORRUPT)
    add("gzip_bytes_after", g + b"\x00", GZIP, CORRUPT)
    add("gzip_second_member", g + g, GZIP, CORRUPT)
    return out


def gzip_flag_bodies():
    """gzip members with every combination of FEXTRA, FNAME, FCOMMENT, FHCRC (and FTEXT)."""
    data = text(1500, 2)
    raw = compress(RAW, data)
    out = []
    for flg in range(32):
        out.append((f"gzip_flg_{flg:02x}", wrap(GZIP, raw, data, flg=flg, extra=b"\x01\x02extra field",
                                                name=b"file.txt", comment=b"a comment")))
    out.append(("gzip_empty_fields", wrap(GZIP, raw, data, flg=0x1e)))
    return out


@functools.lru_cache(maxsize=None)
def accept_vectors():
    """(name, format, body) of everything zlib must accept; the expected bytes are zlib's."""
    out = []
    for n in SIZES:
        for kind, gen in (("text", text), ("random", noise)):
            data = gen(n)
            for level in (1, 6, 9):
                for fmt in (RAW, ZLIB, GZIP):
                    out.append((f"{kind}_{n}_l{level}_f{fmt}", fmt, compress(fmt, data, level)))
    for fmt in (RAW, ZLIB, GZIP):
        for n in (10, 1000, 70000):
            out.append((f"zfixed_{n}_f{fmt}", fmt, compress(fmt, text(n, 4), 6, zlib.Z_FIXED)))
            out.append((f"level0_{n}_f{fmt}", fmt, compress(fmt, text(n, 5), 0)))
        out.append((f"sync_flush_f{fmt}", fmt, compress(fmt, text(20000, 6), 6, flush_every=700)))
        out.append((f"huffman_only_f{fmt}", fmt, compress(fmt, text(5000, 7), 6, zlib.Z_HUFFMAN_ONLY)))
        out.append((f"rle_f{fmt}", fmt, compress(fmt, b"ab" * 3000 + b"\x00" * 70000, 6, zlib.Z_RLE)))
    c = zlib.compressobj(6, zlib.DEFLATED, 9)  # a header that declares a 512-byte window
    out.append(("zlib_window_512", ZLIB, c.compress(text(5000, 8)) + c.flush()))
    for name, body in gzip_flag_bodies():
        out.append((name, GZIP, body))
    for name, raw in accept_streams():
        data = zlib_verdict(RAW, raw)
        assert data is not None, f"zlib refuses the hand-built stream {name}"
        for fmt in (RAW, ZLIB, GZIP):
            out.append((f"{name}_f{fmt}", fmt, wrap(fmt, raw, data)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def expected():
    """name -> zlib's bytes for accept_vectors()."""
    return {name: zlib_verdict(fmt, body) for name, fmt, body in accept_vectors()}


@functools.lru_cache(maxsize=None)
def mutation_set(fmt, count=2000):
    """`count` single-bit flips of a 3,000-byte level-6 body: (body, zlib's bytes or None)."""
    base = compress(fmt, text(3000, 11), 6)
    r = random.Random(77 + fmt)
    out = []
    for _ in range(count):
        bit = r.randrange(8 * len(base))
        b = bytearray(base)
        b[bit >> 3] ^= 1 << (bit & 7)
        b = bytes(b)
        out.append((b, zlib_verdict(fmt, b)))
    return tuple(out)
