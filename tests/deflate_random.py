"""A seeded generator of valid deflate streams for the inflate tests, beside the
hand-picked vectors of tests/deflate_streams.py and written with its `Deflate`
writer: random blocks of all three types, random Kraft-complete code sets up to
the deepest codes, random run-length encodings of the code lengths (runs cross
the HLIT/HDIST boundary), every HCLEN, and copies whose distances are chosen by
replaying the decoder's grouping rule (a group is up to 64 symbols; a new one
starts at each block start and after every 64th symbol), plus the worst-case
code sets that fill the decode tables to their bounds (852 and 592 entries).

The generator assembles the expected bytes itself; nothing here decodes.
Python's zlib stays the judge (the CPU tests compare `expected` with
`zlib_verdict` first, so a generator bug fails there and not on the GPU).
`table_entries` restates the decoder's table-size rule and is used only to
assert what the family covers, never to judge the decoder.

random_family() builds in under a second (measured: 0.75 s for 308 streams,
0.84 MB of compressed stream, 4.0 MB decoded)."""
from __future__ import annotations

import bisect
import functools
import random
from collections import Counter

import deflate_streams as D
from deflate_streams import CL_ORDER, DIST_BASE, DIST_EXTRA, LEN_BASE, LEN_EXTRA, Deflate, dist_symbol, length_symbol

BOUNDARY_LENGTHS = (3, 4, 10, 11, 18, 19, 34, 35, 66, 67, 130, 131, 227, 257, 258)
DIST_CLASSES = ("small", "overlap", "equal", "straddle", "gap", "total", "far", "stored")
FAR = 1024  # a distance from here on counts as far
TARGETS = (50, 700, 5000, 40000)

# symbols per code length that fill the decode tables to zlib's bounds (root 9: 852 entries, root 6: 592)
WORST_LL_COUNTS = {1: 1, 2: 1, 3: 1, 10: 37, 11: 161, 12: 17, 13: 33, 14: 33, 15: 2}
WORST_D_COUNTS = {1: 1, 2: 1, 3: 1, 4: 1, 7: 1, 8: 9, 9: 9, 10: 1, 11: 1, 12: 1, 13: 1, 14: 1, 15: 2}


def table_entries(lens, root):
    """The entries build_table (csrc/inflate_format.h) uses for the code with
    these lengths: the root is clamped to the shortest and longest code, and
    every root prefix of the longer codes gets a sub-table that grows while the
    codes still to come do not fill it."""
    count = [0] * 16
    for n in lens:
        count[n] += 1
    count[0] = 0
    if not any(count):
        return 2
    longest = max(n for n in range(16) if count[n])
    shortest = min(n for n in range(1, 16) if count[n])
    root = max(min(root, longest), shortest)
    used, code, prev = 1 << root, 0, None
    for ln in range(1, 16):
        for rank in range(count[ln]):
            if ln > root and code >> (ln - root) != prev:
                prev = code >> (ln - root)
                curr, left = ln - root, 1 << (ln - root)
                for cl in range(ln, longest):
                    left -= count[ln] - rank if cl == ln else count[cl]
                    if left <= 0:
                        break
                    curr += 1
                    left <<= 1
                used += 1 << curr
            code += 1
        code <<= 1
    return used


def random_complete_lengths(rng, symbols, max_len, depth_bias):
    """symbol -> code length of a Kraft-complete code over `symbols`, no code
    longer than max_len: leaves are split at random, with probability
    depth_bias the deepest one that can still be split.  No symbol gives {}
    (no code at all) and one symbol a single 1-bit code: the two incomplete
    sets deflate allows."""
    symbols = list(symbols)
    if len(symbols) < 2:
        return {s: 1 for s in symbols}
    assert len(symbols) <= 1 << max_len
    count = [0] * (max_len + 1)  # leaves per depth
    count[1] = 2
    for _ in range(len(symbols) - 2):
        open_depths = [d for d in range(1, max_len) if count[d]]
        if rng.random() < depth_bias:
            d = open_depths[-1]
        else:  # a leaf drawn uniformly among those that can be split
            d = rng.choices(open_depths, [count[x] for x in open_depths])[0]
        count[d] -= 1
        count[d + 1] += 2
    depths = [d for d in range(1, max_len + 1) for _ in range(count[d])]
    rng.shuffle(depths)
    return dict(zip(symbols, depths))


def rle_lengths(lens, rng, repeat=0.7):
    """The code lengths `lens` (literal/length then distance lengths, as one
    list) as code-length symbols (sym, extra value), choosing at random among
    the legal encodings: plain lengths, code 16 after equal non-zero lengths,
    codes 17 and 18 for zero runs."""
    out, i, n = [], 0, len(lens)
    while i < n:
        v = lens[i]
        run = 1
        while i + run < n and lens[i + run] == v:
            run += 1
        if rng.random() < repeat:
            top = rng.random() < 0.5  # the longest repeat that fits, else any
            if v == 0 and run >= 3:
                if run >= 11 and rng.random() < 0.7:
                    rep = min(run, 138) if top else rng.randint(11, min(run, 138))
                    out.append((18, rep - 11))
                else:
                    rep = min(run, 10) if top else rng.randint(3, min(run, 10))
                    out.append((17, rep - 3))
                i += rep
                continue
            if i > 0 and lens[i - 1] == v and run >= 3:  # v != 0, or a zero run continued by code 16
                rep = min(run, 6) if top else rng.randint(3, min(run, 6))
                out.append((16, rep - 3))
                i += rep
                continue
        out.append((v, 0))
        i += 1
    return out


def boundary_repeats(cl_syms, nlen):
    """How many repeat codes cover lengths on both sides of position nlen."""
    at = hits = 0
    for sym, extra in cl_syms:
        rep = 1 if sym < 16 else extra + {16: 3, 17: 3, 18: 11}[sym]
        hits += sym >= 16 and at < nlen < at + rep
        at += rep
    return hits


class _Builder:
    """Random blocks appended to one Deflate writer and one expected output.
    base: the first output byte a distance may reach (a unit's first byte)."""

    def __init__(self, rng, big=False):
        self.rng, self.big = rng, big
        self.d = Deflate()
        self.out = bytearray()
        self.base = 0
        self.stats = Counter()
        self.hclens = set()
        self.spans = []        # (kind, first output byte, end) of every literal, copy and stored block
        self.stored_at = None  # output range of the last stored block with bytes
        self.exact = False

    # ---- tokens
    def _distance(self, cls, length, g):
        rng, pos = self.rng, len(self.out)
        if cls == "small":
            return rng.randint(1, 15)
        if cls == "overlap":
            return rng.randint(1, length - 1)
        if cls == "equal":
            return length
        if cls == "straddle":  # the source begins 1 .. length - 1 bytes below the group's first byte
            return pos - g + rng.randint(1, length - 1) if pos > g else 0
        if cls == "gap":
            return length + rng.randint(0, 24)
        if cls == "total":
            return pos - self.base - rng.choice((0, 0, 1, 2, 3))
        if cls == "far":
            top = min(pos - self.base, 32768)
            return 0 if top < FAR else rng.choice((top, top - 1, rng.randint(FAR, top), rng.randint(FAR, top)))
        if self.stored_at is None:
            return 0
        a, b = self.stored_at
        return pos - rng.randint(max(a, b - 64), b - 1) if rng.random() < 0.5 else pos - rng.randint(a, b - 1)

    def _token(self, mode, g, room):
        """One symbol: appended to the expected output, returned as the writer's token."""
        rng, out = self.rng, self.out
        pos = len(out)
        p_lit = {"mixed": 0.35, "chain": 0.03, "long": 0.0, "max": 0.0, "lits": 1.0}[mode]
        if pos == self.base or room < 3 or rng.random() < p_lit:
            byte = rng.choice(b"abcdefgh") if rng.random() < 0.5 else rng.randrange(256)
            out.append(byte)
            self.spans.append(("lit", pos, pos + 1))
            return byte
        if mode == "max":
            length = 258
        elif mode == "long":
            length = rng.choice((258, 258, 257, 227, rng.randint(200, 258)))
        else:
            length = rng.choice(BOUNDARY_LENGTHS) if rng.random() < 0.5 else rng.randint(3, 258)
        length = min(length, room)
        classes = ("small", "overlap", "equal", "gap") if mode == "chain" else DIST_CLASSES
        for cls in rng.sample(classes, len(classes)) + ["small", "small", "small", "small"]:
            dist = self._distance(cls, length, g)
            if 1 <= dist <= min(pos - self.base, 32768):
                break
        else:
            dist, cls = 1, "small"
        self.stats["d_" + cls] += 1
        if dist >= length:
            out += out[pos - dist:pos - dist + length]
        else:
            for _ in range(length):
                out.append(out[-dist])
        self.spans.append(("copy", pos, pos + length))
        return (length, dist)

    def _tokens(self, room):
        """The tokens of one Huffman block, with the decoder's groups replayed."""
        rng = self.rng
        if self.big:
            mode = rng.choices(("mixed", "chain", "long", "max", "lits"), (50, 15, 15, 10, 10))[0]
        else:
            mode = rng.choices(("mixed", "chain", "lits"), (70, 15, 15))[0]
        nsym = rng.choice((0, 1, 2, 63, 64, 65, 128, 129)) if rng.random() < 0.25 else rng.randint(1, 300)
        if mode in ("long", "max"):
            nsym = max(nsym, rng.randint(64, 140))
        toks, g, gcount, g258 = [], len(self.out), 0, True
        first = g
        starts, hops = [], []  # per record of the group: first byte, records its first byte resolves through
        for _ in range(nsym):
            left = room - (len(self.out) - first)
            if left <= 0:
                break
            pos = len(self.out)
            t = self._token(mode, g, left)
            toks.append(t)
            gcount += 1
            g258 &= not isinstance(t, int) and t[0] == 258
            src = pos if isinstance(t, int) else pos - t[1]
            hops.append(0 if src == pos else 1 if src < g else 1 + hops[bisect.bisect_right(starts, src) - 1])
            starts.append(pos)
            self.stats["max_chain"] = max(self.stats["max_chain"], hops[-1])
            self.stats["chains_over_24"] += hops[-1] == 25
            if gcount == 64:
                self.stats["groups64"] += 1
                self.stats["groups64_over_12000"] += len(self.out) - g > 12000
                self.stats["groups64_all_258"] += g258
                g, gcount, g258 = len(self.out), 0, True
                starts, hops = [], []
        return toks

    # ---- blocks
    def stored(self, final, room):
        rng = self.rng
        n = rng.choice((0, 0, 1, 15, 16, 17, 31, 32, 33, rng.randint(1, 300), rng.randint(1, 300),
                        rng.randint(1, 2000)))
        n = min(n, room)
        if self.big and not self.exact and rng.random() < 0.05:
            n = 65535  # the longest stored block, whatever the target
        data = rng.randbytes(n)
        self.stats["stored_misaligned"] += (self.d.b.bitpos + 3) % 8 != 0
        if n in (0, 65535):
            self.stats["stored_len_%d" % n] += 1
        self.d.stored(data, final=final)
        pos = len(self.out)
        self.out += data
        if n:
            self.spans.append(("stored", pos, pos + n))
            self.stored_at = (pos, pos + n)
        self.stats["stored"] += 1

    def fixed(self, final, room):
        self.d.fixed(self._tokens(room), final=final)
        self.stats["fixed"] += 1

    def dynamic(self, final, room):
        rng = self.rng
        toks = self._tokens(room)
        lits = {t for t in toks if isinstance(t, int)}
        used_ll = lits | {length_symbol(t[0])[0] for t in toks if not isinstance(t, int)} | {256}
        used_d = {dist_symbol(t[1])[0] for t in toks if not isinstance(t, int)}
        # coded symbols nothing uses, and zero lengths at the end of the literal/length list
        spare_ll = sorted(set(range(286)) - used_ll)
        coded_ll = used_ll | set(rng.sample(spare_ll, min(len(spare_ll), rng.choice((0, 1, 5, 30, 286)))))
        if len(coded_ll) < 2 and rng.random() < 0.8:
            coded_ll.add(rng.randrange(256))
        nlen = rng.randint(max(257, max(coded_ll) + 1), 286)
        spare_d = sorted(set(range(30)) - used_d)
        how = rng.random()
        if not used_d and how < 0.7:  # no distance code at all, or a single one nothing uses
            coded_d = set() if how < 0.4 else {rng.randrange(30)}
        else:
            coded_d = used_d | set(rng.sample(spare_d, min(len(spare_d), rng.choice((0, 0, 1, 3, 12, 30)))))
        ndist = rng.randint(max(coded_d, default=0) + 1, 30)
        bias = rng.choice((0.0, 0.3, 0.8, 0.97))
        ll = random_complete_lengths(rng, sorted(coded_ll), 15, bias)
        dd = random_complete_lengths(rng, sorted(coded_d), 15, rng.choice((0.0, 0.5, 0.97, 1.0)))
        ll_lens = [ll.get(s, 0) for s in range(nlen)]
        d_lens = [dd.get(s, 0) for s in range(ndist)]
        narrow = rng.random() < 0.25  # flat sets: few distinct lengths, so a short code-length code and a small HCLEN
        if narrow:
            want = rng.choice((32, 64, 128, 256, rng.randint(2, 286)))
            coded_ll = used_ll | set(rng.sample(spare_ll, max(0, min(len(spare_ll), want - len(used_ll)))))
            if len(coded_ll) < 2:
                coded_ll.add(rng.randrange(256))
            nlen = rng.randint(max(257, max(coded_ll) + 1), 286)
            ll_lens = D.flat_lengths(coded_ll, nlen)
            if len(coded_d) == 1:
                coded_d.add(rng.choice(sorted(set(range(30)) - coded_d)))
            if coded_d:
                ndist = rng.randint(max(coded_d) + 1, 30)
                d_lens = D.flat_lengths(coded_d, ndist)
        cl_syms = rle_lengths(ll_lens + d_lens, rng, rng.choice((0.0, 0.5, 0.9, 1.0)))
        used_cl = {s for s, _ in cl_syms}
        spare_cl = sorted(set(range(19)) - used_cl)
        coded_cl = used_cl | set(rng.sample(spare_cl, 0 if narrow else rng.randint(0, len(spare_cl))))
        if len(coded_cl) < 2:
            coded_cl.add(rng.choice((0, 16, 17, 18) if narrow else spare_cl))
        cl = random_complete_lengths(rng, sorted(coded_cl), 7, rng.choice((0.0, 0.5, 0.9, 1.0)))
        cl_lens = [cl.get(s, 0) for s in range(19)]
        least = max(4, 1 + max(i for i, s in enumerate(CL_ORDER) if cl_lens[s]))
        hclen = least if rng.random() < 0.6 else rng.randint(least, 19)
        self.d.dynamic(ll_lens, d_lens, toks, final=final, cl_lens=cl_lens, cl_syms=cl_syms, hclen=hclen)
        st = self.stats
        st["dynamic"] += 1
        st["ll_15_bit"] += 15 in ll_lens
        st["d_15_bit"] += 15 in d_lens
        st["cl_7_bit"] += 7 in cl_lens
        st["boundary_repeat_headers"] += boundary_repeats(cl_syms, nlen) > 0
        st["no_distance_code"] += not coded_d
        st["single_distance_code"] += len(coded_d) == 1
        st["max_ll_entries"] = max(st["max_ll_entries"], table_entries(ll_lens, 9))
        st["max_d_entries"] = max(st["max_d_entries"], table_entries(d_lens, 6))
        self.hclens.add(hclen)

    def blocks(self, nbytes, exact, final):
        """Random blocks until nbytes are declared: exactly nbytes if `exact`,
        else the last block may pass it.  final: the last block carries BFINAL."""
        rng = self.rng
        self.exact = exact
        start = len(self.out)
        while True:
            have = len(self.out) - start
            if not final and have >= nbytes:
                return
            room = nbytes - have if exact else max(nbytes - have, 0) + 258  # not exact: up to a symbol past it
            last = have >= nbytes or (not exact and rng.random() < 0.02)
            if exact and not last and rng.random() < 0.1:
                room = 0  # an empty block in the middle
            kind = rng.choice((self.stored, self.fixed, self.dynamic))
            kind(final and last, room)
            if final and last:
                return

    def finish(self):
        stats = dict(self.stats)
        stats["hclen_values"] = sorted(self.hclens)
        stats["spans"] = self.spans
        stats["headers"] = list(self.d.headers)
        return self.d.raw(), bytes(self.out), stats


def random_stream(rng, target):
    """(raw stream, expected bytes, stats): random blocks declaring about
    `target` bytes.  stats counts what was placed -- blocks per type, copies
    per distance class ("d_" + DIST_CLASSES), groups, "max_chain" (the most
    records of one group that a copy's first byte resolves through) -- and
    holds "spans" (kind, first, end in the output, of every literal, copy and
    stored block), "headers" (bit range of every dynamic header) and
    "hclen_values"."""
    b = _Builder(rng, big=target >= 40000)
    b.blocks(target, exact=False, final=True)
    return b.finish()


def unit_parts(rng, chlen, units, reach_below=None):
    """The deflate stream of a gzip body as `units` byte strings (the unit
    slices of an RA index with this CHLEN) and its expected bytes.  Every unit
    in front of the last is a run of non-final random blocks that declares
    exactly chlen bytes, uses no distance below its own first byte and is
    closed on a byte boundary by an empty stored block; the last unit ends
    with BFINAL.  reach_below: the index (1 or more) of one unit whose first
    symbol is a copy from below its first byte instead."""
    out, parts = bytearray(), []
    for k in range(units):
        b = _Builder(rng)
        b.out = out
        b.base = len(out)
        last = k + 1 == units
        if k == reach_below:
            length, dist = rng.randint(3, min(40, chlen)), rng.randint(1, min(len(out), 300))
            for _ in range(length):
                out.append(out[-dist])
            b.d.fixed([(length, dist)])
            room = chlen - length
        else:
            room = chlen
        if last:
            b.blocks(rng.randint(min(1, room), room), exact=True, final=True)
        else:
            if room:
                b.blocks(room, exact=True, final=False)
            b.d.stored(b"")
            assert len(out) - b.base == chlen and b.d.b.bitpos % 8 == 0
        parts.append(b.d.raw())
    return parts, bytes(out)


def _spread(counts, rng, forced=()):
    """Code lengths by symbol for symbols-per-length `counts`, shuffled;
    forced: (symbol, length) pairs placed first."""
    pool = [n for n, c in sorted(counts.items()) for _ in range(c)]
    lens = [0] * len(pool)
    for sym, n in forced:
        pool.remove(n)
        lens[sym] = n
    rng.shuffle(pool)
    for sym in range(len(lens)):
        if not lens[sym]:
            lens[sym] = pool.pop()
    return lens


def _copy(out, toks, length, dist):
    toks.append((length, dist))
    for _ in range(length):
        out.append(out[-dist])


def worst_case_streams():
    """8 x (name, raw, expected, info): a 33,000-byte stored block of noise,
    then one dynamic block whose two code sets have the worst-case counts,
    assigned to symbols by a seeded shuffle, with every coded symbol used.  In
    streams 0 and 1 the 15-bit codes sit on two length symbols with 5 extra
    bits and on distance symbols 28 and 29, and that 48-bit pair of symbols is
    sent 48 times in a row and then in 40 short runs, each moved by a
    literal with an odd code length; info["long_marks"] lists the bit
    positions at which those symbols start."""
    res = []
    for k in range(8):
        rng = random.Random(8520 + k)
        special = k < 2
        forced_ll = [(s, 15) for s in rng.sample(range(281, 285), 2)] if special else []
        ll_lens = _spread(WORST_LL_COUNTS, rng, forced_ll)
        d_lens = _spread(WORST_D_COUNTS, rng, [(28, 15), (29, 15)] if special else [])
        out = bytearray(D.noise(33000, 40 + k))
        toks, marks = [], []
        d = Deflate().stored(bytes(out))
        lits = list(range(256))
        rng.shuffle(lits)
        for dsym in rng.sample(range(30), 30):  # every distance symbol and every length symbol; the literals between
            lsym = dsym if dsym < 29 else rng.randrange(29)
            length = 258 if lsym == 28 else LEN_BASE[lsym] + rng.randrange(1 << LEN_EXTRA[lsym])
            dist = DIST_BASE[dsym] + rng.randrange(1 << DIST_EXTRA[dsym])
            _copy(out, toks, length, dist)
            for _ in range(9):
                if lits:
                    toks.append(lits.pop())
                    out.append(toks[-1])
        assert not lits
        long_at = []
        if special:
            lsyms = [s for s, _ in forced_ll]
            shifter = next(b for b in range(256) if ll_lens[b] % 2 == 1 and ll_lens[b] > 3)

            def long_pair():
                s = rng.choice(lsyms) - 257
                long_at.append(len(toks))
                length = LEN_BASE[s] + rng.randrange(31 if s == 27 else 32)  # 258 has a symbol of its own
                _copy(out, toks, length, DIST_BASE[rng.choice((28, 29))] + rng.randrange(8192))
            for _ in range(48):
                long_pair()
            for _ in range(40):
                toks.append(shifter)
                out.append(shifter)
                long_pair()
                long_pair()
        b = _Builder(rng)  # random symbols behind them, under the same code sets
        b.out = out
        for _ in range(300):
            toks.append(b._token("mixed", len(out), 1 << 30))
        d.dynamic(ll_lens, d_lens, toks, final=True, cl_syms=rle_lengths(ll_lens + d_lens, rng), marks=marks)
        run = longest = 0
        for i in long_at:  # the longest row of 48-bit symbols with nothing between them
            run = run + 1 if i - 1 in long_at else 1
            longest = max(longest, run)
        copies = [t for t in toks if not isinstance(t, int)]
        info = {"ll_lens": ll_lens, "d_lens": d_lens, "long_marks": [marks[i] for i in long_at],
                "longest_run": longest,
                "used_ll": {t for t in toks if isinstance(t, int)} | {length_symbol(t[0])[0] for t in copies} | {256},
                "used_d": {dist_symbol(t[1])[0] for t in copies},
                "headers": list(d.headers),
                "spans": [("stored", 0, 33000)] + [s for s in b.spans]}
        res.append((f"worst_{k}", d.raw(), bytes(out), info))
    return res


class Stream:
    """One stream of the family: raw deflate bytes, the expected output, stats."""

    def __init__(self, name, raw, expected, stats):
        self.name, self.raw, self.expected, self.stats = name, raw, expected, stats

    def body(self, fmt):
        return D.wrap(fmt, self.raw, self.expected)


@functools.lru_cache(maxsize=None)
def random_family():
    """The 8 worst-case streams, then 300 random ones (seeded)."""
    fam = [Stream(*w) for w in worst_case_streams()]
    for k in range(300):
        rng = random.Random(31000 + k)
        fam.append(Stream(f"random_{k}", *random_stream(rng, TARGETS[k % 4])))
    return tuple(fam)


def family_totals():
    """The random streams' counters summed, and the set of HCLEN values."""
    total, hclens = Counter(), set()
    for s in random_family()[8:]:
        for key, v in s.stats.items():
            if isinstance(v, int):
                if key.startswith("max_"):
                    total[key] = max(total[key], v)
                else:
                    total[key] += v
        hclens |= set(s.stats["hclen_values"])
    return total, hclens


def inner_capacity(s, fmt):
    """A seeded capacity strictly inside the stream's output (None when it has
    under 3 bytes), and the kind of the token it falls inside ("lit" when it
    falls on a token's first byte: nothing is cut)."""
    n = len(s.expected)
    if n < 3:
        return None, None
    cap = random.Random(f"{s.name}/{fmt}").randint(1, n - 2)
    for kind, a, b in s.stats["spans"]:
        if a < cap < b:
            return cap, kind
    return cap, "lit"


@functools.lru_cache(maxsize=None)
def hand_flip_set(fmt, count=2000):
    """`count` single-bit flips spread over 100 streams of the family (seeded:
    random streams with a dynamic block and up to 6,000 bytes of stream),
    half of them inside the stream's first dynamic header:
    (body, zlib's bytes or None)."""
    rng = random.Random(2024 + fmt)
    pool = [s for s in random_family()[8:]
            if s.stats["headers"] and len(s.raw) <= 6000]
    picks = rng.sample(pool, 100)
    out = []
    for i in range(count):
        s = picks[i % 100]
        body = bytearray(s.body(fmt))
        lead = 8 * {D.RAW: 0, D.ZLIB: 2, D.GZIP: 10}[fmt]
        if i % 200 < 100:
            a, b = s.stats["headers"][0]
            bit = lead + rng.randrange(a, b)
        else:
            bit = rng.randrange(8 * len(body))
        body[bit >> 3] ^= 1 << (bit & 7)
        body = bytes(body)
        out.append((body, D.zlib_verdict(fmt, body)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def unit_bodies():
    """(body, expected, parallel) of 40 gzip bodies with an RA unit index over
    2 to 6 hand-built units (tests/gzip_index_cases.py: ra, assemble); in 5 of
    them one unit reaches below its first byte, so the index cannot be used."""
    import gzip_index_cases as G
    res = []
    for k in range(40):
        rng = random.Random(77000 + k)
        units = rng.randint(2, 6)
        reach = rng.randint(1, units - 1) if k % 8 == 3 else None
        sizes = (1, 7, 64, 100, 257, 258, 1000, 3000, rng.randint(1, 5000)) if reach is None else (64, 700, 3000)
        chlen = rng.choice(sizes)
        parts, data = unit_parts(rng, chlen, units, reach)
        res.append((G.assemble(parts, data, G.ra(chlen, [len(p) for p in parts])), data, reach is None))
    return tuple(res)
