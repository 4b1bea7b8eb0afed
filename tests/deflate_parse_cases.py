"""A seeded family of constructed bodies for the device-only code of the
deflate writer (csrc/deflate_unit.h): the things the text bodies of
tests/deflate_cases.py reach only where English happens to.  Used by
tests/test_deflate_parse.py (host model: every case's precondition, the
coverage floors) and tests/test_deflate_parse_gpu.py (device).

cases() is a list of (name, level, bytes).  Every case has a TARGET and a
precondition hit(level) -> bool that is read from the host model's tokens
(host/deflate_cpu.cc), so a case that stops hitting its target fails on the
CPU instead of passing quietly on the GPU.  TARGETS says at which levels a
target has to be met at least once.

As in tests/deflate_level_cases.py the strings under test are letters and the
filler between them is bytes of 128 and up, so nothing but the strings
repeats.  Two groups differ and say so: the two-unit body needs a coded first
unit and is text with capital-letter strings, and the long-token bodies are
noise in the manner of deflate_cases.deep_body().  Every case's unit must be
a coded block at both levels (a stored unit is a copy, on the device as in
the model, and its tokens never reach the bytes): hit() includes that, and the
short bodies (lazy step, chain, token counts) keep their filler to 16 values
for it (_narrow).

What a case aims at (W = the 64-position window, lanes = positions mod 64):
  same_slot         two or three lanes of one window hash alike ("ABCD" + X at
                    lane i, "ABCD" + Y at lane j > i; adjacent lanes share the
                    run "AAAAA"): one LDS store a lane, the highest lane must
                    be what the table holds.  "ABCD" + X again, at a window's
                    last lane (no lazy step there), finds 4 bytes at j, not
                    the long match at i.
  same_slot_older   level 2: the slot held z before.  After the window the word
                    is (z, j): a query for z's string finds z (the older half),
                    the query for X behind it finds 4 bytes at the first query
                    (the halves are (j, q1) then; i would give the long match).
  neighbour_slots   two strings whose slots are h and h ^ 1 (one dword of the
                    level-1 table) in one window: both are found again.
  same_window_repeat  see same_window_repeat(): the probe for a position table
                    that a wave's second unit did not start from empty.
  lazy_row_edge     deflate_level_cases.lazy_pair with the deferring lane at
                    15, 31, 47 (its neighbour is the next DPP row's first lane)
                    and at 16.
  chain_carry       a match of m bytes from lane L that crosses zero to five
                    window ends, s bytes behind it, then the unit ends.
  unit_end          a match that must stop at its unit's end although the
                    bytes behind the unit go on matching (two units), or with
                    the source going on (one unit): the reader returns zeros
                    past the unit at every source alignment.
  tokens_N          N tokens with the end token: 63, 64, 65, 127, 128, 129.
  long_token_*      see long_body()."""
from __future__ import annotations

import functools
import random
from collections import namedtuple

import numpy as np

import deflate_cases as C
import deflate_level_cases as V
import deflate_read as R
import deflate_streams as D

FAST, BEST = V.FAST, V.BEST
U = C.U
W = 64

Case = namedtuple("Case", "name level data target hit")

# target -> the levels at which the family must meet it at least once
TARGETS = {
    "same_slot": (FAST, BEST),
    "same_slot_older": (BEST,),
    "neighbour_slots": (FAST, BEST),
    "same_window_repeat": (FAST, BEST),
    "lazy_row_edge": (BEST,),
    "chain_carry": (FAST, BEST),
    "unit_end": (FAST, BEST),
    **{f"tokens_{k}": (FAST, BEST) for k in (63, 64, 65, 127, 128, 129)},
    "long_token_bits": (FAST, BEST),
    "long_token_three_words": (FAST, BEST),
    "long_token_flush_edge": (FAST, BEST),
}


def hash4(four: bytes) -> int:
    """defl::hash4 (csrc/deflate_format.h), restated."""
    return ((int.from_bytes(four[:4], "little") * 2654435761) & 0xffffffff) >> (32 - 13)


def _tok(level, x, pos):
    return V.token_starting_at(V.tokens(level, x), pos)


def first_match(level, x):
    """(position, length) of the first match among the model's tokens, or None."""
    pos = 0
    for t in V.tokens(level, x):
        if t[0] == "match":
            return pos, t[1]
        pos += 1
    return None


def coded(level, x):
    """No unit of x is a stored block: the parse shows in the bytes."""
    return V.unit_types(level, x)[0] == 0


def _narrow(x, k):
    """The filler on 16 values (128 to 143, from bits k to k + 3 of each byte).
    A short body of filler on 128 values is cheapest as a stored block, on the
    device as in the model, and then its tokens are never seen; on 16 values
    the fixed or the dynamic code wins."""
    return bytes(b if b < 128 else 128 | (b >> k) & 15 for b in x)


def _coded_variant(make, levels):
    """make(k) -> (body, hit) for the filler variants k = 0 .. 3 (and the seeds
    make derives from k above that): the first whose target is hit in a coded
    block at `levels`.  Filler on 16 values repeats four bytes now and then."""
    for k in range(16):
        x, hit = make(k)
        if all(hit(lv) and coded(lv, x) for lv in levels):
            return x, hit
    raise AssertionError("no coded variant")


# ---- same-slot stores

PAIRS = ((0, 1), (0, 63), (15, 16), (14, 15), (31, 32), (47, 48), (62, 63))
TRIPLE = (3, 35, 60)


def _slot_strings(lanes, seed):
    """(position in the window, string) per lane and the first lane's string:
    adjacent lanes overlap in a run of A, the others carry "ABCD" + 8 letters."""
    if len(lanes) == 2 and lanes[1] == lanes[0] + 1:
        y = V._letters(8, seed)
        return [(lanes[0], b"AAAAA" + y)], b"AAAAA" + y, b"AAAA"
    tails = []
    for k in range(len(lanes)):  # tails that differ in their first letter
        tails.append(next(t for t in (V._letters(8, seed + k + 50 * i) for i in range(99))
                          if t[0] not in {u[0] for u in tails}))
    assert all(b - a >= 12 for a, b in zip(lanes, lanes[1:]))
    return [(l, b"ABCD" + t) for l, t in zip(lanes, tails)], b"ABCD" + tails[0], b"ABCD"


def same_slot(lanes, seed):
    """Level 1's body: the lanes in window 1, the first lane's string again at 383."""
    placed, first, _ = _slot_strings(lanes, 40 + seed)
    q = 5 * W + 63
    x = V._place([(W + l, s) for l, s in placed] + [(q, first)], q + 40, 100 + seed)
    j = W + lanes[-1]
    assert x[q:q + len(first)] == x[W + lanes[0]:W + lanes[0] + len(first)] and x[j:j + 4] == x[q:q + 4]
    assert x[j + 4] != x[q + 4] and all(hash4(x[W + l:]) == hash4(x[q:]) for l in lanes)
    return x, lambda level: _tok(level, x, q) == ("match", 4, q - j)


def same_slot_older(lanes, seed):
    """Level 2's body: z's string at 5, the lanes in window 2, z's string again
    at 319 and the first lane's at 447."""
    placed, first, stem = _slot_strings(lanes, 60 + seed)
    taken = {c for _, s in placed for c in s[4:6]}  # what follows the stem at any lane
    zs = next(stem + t for t in (V._letters(8, 90 + seed + 50 * k) for k in range(99)) if t[0] not in taken)
    z, q1, q2 = 5, 4 * W + 63, 6 * W + 63
    x = V._place([(z, zs)] + [(2 * W + l, s) for l, s in placed] + [(q1, zs), (q2, first)], q2 + 40, 200 + seed)
    assert all(hash4(x[2 * W + l:]) == hash4(x[z:]) == hash4(x[q1:]) == hash4(x[q2:]) for l in lanes)
    return x, lambda level: (_tok(level, x, q1) == ("match", len(zs), q1 - z)
                             and _tok(level, x, q2) == ("match", 4, q2 - q1))


@functools.lru_cache(maxsize=None)
def neighbour_strings():
    """Two 4-letter strings whose slots are h and h ^ 1: a seeded search."""
    r = random.Random(4242)
    seen = {}
    while True:
        s = bytes(r.choice(b"ABCDEFGHIJKLMNOPQRSTUVWXYZ") for _ in range(4))
        h = hash4(s)
        if h ^ 1 in seen and len(set(s) & set(seen[h ^ 1])) == 0:
            return seen[h ^ 1], s
        seen[h] = s


def neighbour_slots():
    s1, s2 = neighbour_strings()
    assert hash4(s1) ^ hash4(s2) == 1
    a, b = s1 + V._letters(8, 31), s2 + V._letters(8, 32)
    p1, p2, q1, q2 = W + 10, W + 40, 3 * W + 63, 5 * W + 63
    x = V._place([(p1, a), (p2, b), (q1, a), (q2, b)], q2 + 40, 33)
    return x, lambda level: (_tok(level, x, q1) == ("match", 12, q1 - p1)
                             and _tok(level, x, q2) == ("match", 12, q2 - p2))


def same_window_repeat(first=False):
    """"ABCD" + X at 70 and "ABCD" + Y at 100, one window, nothing before: both
    are literals, a window has no candidates of its own; "ABCD" + Y again at
    300 finds the one at 100.  first=True: the same bytes with filler in place
    of the strings at 100 and 300.  A wave that takes the second body behind
    the first and does not empty its position table finds 70 in the slot when
    it stands at 100, and writes a match where the model has a literal."""
    strings = [(70, b"ABCD" + V._letters(8, 21)), (100, b"ABCD" + V._letters(8, 22)),
               (300, b"ABCD" + V._letters(8, 22))]
    x = V._place(strings, 340, 23)
    if first:
        keep = bytearray(V.filler(340, 24))
        keep[70:82] = x[70:82]
        return bytes(keep)
    return x, lambda level: (_tok(level, x, 70) == ("lit", ord("A")) and _tok(level, x, 100) == ("lit", ord("A"))
                             and _tok(level, x, 300) == ("match", 12, 200))


# ---- the lazy step at the DPP rows' edges

LAZY_AT = (128 + 15, 128 + 31, 128 + 47, 128 + 16)


def lazy_row_edge(at):
    def make(k):
        x = _narrow(V.lazy_pair(at), k % 4)
        return x, lambda level: (level == BEST and _tok(level, x, at) == ("lit", ord("a"))
                                 and _tok(level, x, at + 1) == ("match", 9, at + 1 - V.Q_AT))
    return _coded_variant(make, (BEST,))


# ---- the chain's carry

CHAIN_LANES = (0, 1, 31, 62, 63)
CHAIN_SUFFIX = (0, 1, 2, 3, 4)


def chain_lengths(lane):
    """4, to the window's end, one past it, 130, 258, 259 (split); the two
    lengths below 4 that lanes 62 and 63 would have are no matches."""
    return sorted({m for m in (4, 64 - lane, 65 - lane, 130, 258, 259) if m >= 4})


@functools.lru_cache(maxsize=None)
def _chain_string():
    return V._letters(259, 7)


def chain_carry(lane, m, s, seed):
    """The string's first m letters at 0 and again at lane `lane` of the first
    window behind them, s filler bytes, the unit's end.  The match is the
    body's first, at both levels, and the block is a coded one."""
    src = _chain_string()[:m]
    p = W * (-(-(m + 1) // W)) + lane

    def make(k):
        x = _narrow(V._place([(0, src), (p, src)], p + m + s, seed + 1000 * (k // 4)), k % 4)
        assert len(x) == p + m + s and x[p:p + m] == src
        return x, lambda level: ((s == 0 or x[m] != x[p + m]) and first_match(level, x) == (p, min(m, 258))
                                 and _tok(level, x, p) == ("match", min(m, 258), p))
    return _coded_variant(make, (FAST, BEST))


# ---- the unit's end

UNIT_END_LENGTHS = (61, 62, 63, 64, 65, 66, 67)


def _capitals(n, seed):
    r = random.Random(700 + seed)
    while True:
        s = bytes(r.choice(b"BCDFGHJKLMPQRSUVWXYZ") for _ in range(n))
        if len({s[i:i + 3] for i in range(n - 2)}) == n - 2:
            return s


@functools.lru_cache(maxsize=None)
def two_units():
    """Text (the first unit has to be a coded block for its tokens to show) with
    a 60-capital string 300 bytes below the unit's end; its first 40 again as
    the unit's last 40 bytes, and the other 20 as the next unit's first."""
    s = _capitals(60, 1)
    x = D.text(U - 300, 21) + s + D.text(200, 22) + s + D.text(180, 23)
    assert len(x) == U + 200 and x[U - 40:U + 20] == s == x[U - 300:U - 240]

    def hit(level):
        toks = V.tokens(level, x[:U])
        return toks[-1] == ("match", 40, 260) and V.token_starting_at(toks, U - 40) == toks[-1] \
            and V.unit_types(level, x)[0] == 0
    return x, hit


def one_long_match(k):
    """67 letters at 0, the first k of them from 128 to the unit's end: one match
    of k bytes that ends with the unit while its source goes on (k < 67).  The
    first window of a unit has no candidates, so a body of k bytes in all
    cannot be one match; this is the nearest thing."""
    s = V._letters(67, 11)
    x = V._place([(0, s), (2 * W, s[:k])], 2 * W + k, 300 + k)

    def hit(level):
        toks = V.tokens(level, x)
        return toks[-1] == ("match", k, 2 * W) and V.token_starting_at(toks, 2 * W) == toks[-1]
    return x, hit


# ---- token counts

TOKEN_COUNTS = (63, 64, 65, 127, 128, 129)


@functools.lru_cache(maxsize=None)
def _token_stock(k):
    out = bytearray(b"ABCD" + V.filler(60, 50))
    for g in range(60):
        out += b"ABCD" + V.filler(1 + g % 3, 51 + g)
    return bytes(out) if k is None else _narrow(bytes(out), k)


@functools.lru_cache(maxsize=None)
def token_count(level, want):
    """The shortest cut of "ABCD", 60 filler bytes and "ABCD" + 1 to 3 filler
    bytes over and over that has `want` tokens with the end token -- and a
    match among them where that can be (a unit's first window is literals, so
    up to 65 tokens there is none).  The block is a coded one."""
    def make(k):
        # narrow filler up to 65 tokens (all literals: the fixed code must beat a copy); above, the
        # matches pay for the block, and "ABCD" + one of 16 values would repeat as 5 bytes
        stock = _token_stock(k % 4 if want <= 65 else None)
        for n in range(want - 1, len(stock)):
            x = stock[:n]
            toks = V.tokens(level, x)
            if len(toks) + 1 == want and (want <= 65 or any(t[0] == "match" for t in toks)):
                break
        else:
            raise AssertionError(want)

        def hit(lv):
            toks = V.tokens(lv, x)
            return len(toks) + 1 == want and all(t[0] == "lit" or t[1] == 4 for t in toks) \
                and (want <= 65 or any(t[0] == "match" for t in toks))
        return x, hit
    return _coded_variant(make, (level,))


# ---- long tokens

@functools.lru_cache(maxsize=None)
def token_layout(level, x):
    """(bit position, bits) of every token of a one-unit body's coded block, read
    back from the model's raw stream by tests/deflate_read.py; positions count
    from the block's first bit, which is bit 0 of the device's bit window."""
    blocks, out, _ = R.read(V.model(C.RAW, level, x))
    assert out == x and len(blocks) == 1 and blocks[0].btype in (1, 2)
    return tuple(zip(blocks[0].pos, blocks[0].nbits))


def longest_token(level, x):
    return max(nb for _, nb in token_layout(level, x))


def three_words(layout):
    """A token that put_bits spreads over three window words."""
    return any(pos % 32 + nb > 64 for pos, nb in layout)


def flush_edge(layout):
    """A token that lies across a multiple of 128 bits: a 16-byte block of the flush."""
    return any(pos // 128 != (pos + nb - 1) // 128 for pos, nb in layout)


LONG_FAR_LENGTH = 200
LONG_NEAR = ((1, 1029), (2, 773), (3, 517), (5, 389), (8, 261), (13, 197), (21, 133), (34, 101), (55, 69))


@functools.lru_cache(maxsize=None)
def long_body(pad: int, far: int = 1) -> bytes:
    """In the manner of deflate_cases.deep_body(): noise on 200 byte values with
    12 rare values whose counts chain (1, 2, 4, 7, 12, ...), which makes the
    literal/length code 15 bits deep.  Into it go
      - `far` matches of 200 bytes (length symbol 283, 5 extra bits) at a
        distance above 16,384 (distance symbol 28 or 29, 13 extra bits), and
      - 4-byte matches at nine other distance symbols with counts 1, 2, 3, 5,
        ... 55, the rarest the farthest, so that the distance code is deep too
        and the far match's symbol, seen `far` times, is its longest code.
    A near match is a 4-byte string, d - 4 filler bytes and the string again
    (d >= 64: another window).  `pad` filler bytes in front of the far matches
    move them through the bit window."""
    rng = np.random.default_rng(16)
    values = rng.permutation(256)
    common = values[12:212].astype(np.uint8)
    w = [1, 2]
    while len(w) < 12:
        w.append(w[-1] + w[-2] + 1)
    near = sum(c * (d + 4) for c, d in LONG_NEAR)
    n_fill = near - 8 * sum(c for c, _ in LONG_NEAR) + pad + 60 * far + 60
    pool = np.concatenate([np.repeat(values[:12].astype(np.uint8), w), common[rng.integers(0, 200, n_fill - sum(w))]])
    rng.shuffle(pool)
    pool = pool.tobytes()
    take = [0]

    def fill(n):
        take[0] += n
        return pool[take[0] - n:take[0]]
    pick = lambda n: common[rng.integers(0, 200, n)].tobytes()
    out = bytearray()
    for c, d in reversed(LONG_NEAR):
        for _ in range(c):
            s = pick(4)
            out += s + fill(d - 4) + s
    out += fill(pad)
    # the far string goes in front and behind: one whose first four bytes hash to a slot that no
    # position between the two copies takes, or the single-candidate table would not hold it so long
    lead, trail = fill(60), [fill(60) for _ in range(far)]
    while True:
        string = pick(LONG_FAR_LENGTH)
        body = string + lead + bytes(out) + string
        if hash4(string) not in {hash4(body[i:i + 4]) for i in range(1, len(body) - LONG_FAR_LENGTH)}:
            break
    out = bytearray(body) + trail[0]
    for t in trail[1:]:
        out += string + t
    assert take[0] == len(pool) and len(out) <= U
    return bytes(out)


def far_matches(level, x):
    return [t for t in V.tokens(level, x) if t[0] == "match" and t[1] == LONG_FAR_LENGTH and t[2] > 16384]


# The longest token the host model writes for long_body(PAD_LONGEST), the body
# of the cases "long_token_bits_l1" and "long_token_bits_l2": the floor of
# "long_token_bits" at both levels.  48 is the format's maximum; here the
# length code takes 5 extra bits and the distance code 13, and the two codes
# of the far match are as deep as the writer's code build makes them.  Pads 0
# to 8 were tried; they give 39 to 42 bits.
LONGEST_TOKEN_BITS = 42
LONGEST_TOKEN_BODY = "long_token_bits"  # the cases of this name, _l1 and _l2
PAD_LONGEST = 4
# the first pads (tried 0, 1, 2, ...) at which the far match lies over three
# window words, and over a 128-bit edge, per level
PAD_THREE_WORDS = {FAST: 5, BEST: 7}
PAD_FLUSH_EDGE = {FAST: 5, BEST: 8}


def long_token(kind, level):
    """The far match is the token in question: the tests are made on the tokens of 38 bits and up."""
    if kind == "long_token_bits":
        x = long_body(PAD_LONGEST)
        return x, lambda lv: bool(far_matches(lv, x)) and longest_token(lv, x) >= LONGEST_TOKEN_BITS
    pad = (PAD_THREE_WORDS if kind == "long_token_three_words" else PAD_FLUSH_EDGE)[level]
    test = three_words if kind == "long_token_three_words" else flush_edge
    x = long_body(pad)
    return x, lambda lv: bool(far_matches(lv, x)) and test([t for t in token_layout(lv, x) if t[1] >= 38])


# ---- the family

@functools.lru_cache(maxsize=None)
def family():
    out = []
    # a target is hit only in a coded block: a stored unit's tokens never reach the bytes
    add = lambda name, level, target, built: out.append(
        Case(name, level, built[0], target, lambda lv, x=built[0], hit=built[1]: hit(lv) and coded(lv, x)))
    for k, lanes in enumerate(PAIRS + (TRIPLE,)):
        tag = "_".join(map(str, lanes))
        add(f"same_slot_{tag}", FAST, "same_slot", same_slot(lanes, k))
        add(f"same_slot_older_{tag}", BEST, "same_slot_older", same_slot_older(lanes, k))
    add("neighbour_slots", FAST, "neighbour_slots", neighbour_slots())
    add("neighbour_slots_l2", BEST, "neighbour_slots", neighbour_slots())
    add("same_window_repeat", FAST, "same_window_repeat", same_window_repeat())
    for at in LAZY_AT:
        add(f"lazy_lane_{at % W}", BEST, "lazy_row_edge", lazy_row_edge(at))
    k = 0
    for lane in CHAIN_LANES:
        for m in chain_lengths(lane):
            for s in CHAIN_SUFFIX:
                add(f"chain_{lane}_{m}_{s}", FAST, "chain_carry", chain_carry(lane, m, s, 400 + k))
                k += 1
    add("two_units", FAST, "unit_end", two_units())
    for n in UNIT_END_LENGTHS:
        add(f"one_match_{n}", FAST, "unit_end", one_long_match(n))
    for level in (FAST, BEST):
        for want in TOKEN_COUNTS:
            add(f"tokens_{want}_l{level}", level, f"tokens_{want}", token_count(level, want))
        for kind in ("long_token_bits", "long_token_three_words", "long_token_flush_edge"):
            add(f"{kind}_l{level}", level, kind, long_token(kind, level))
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


def cases():
    return [(c.name, c.level, c.data) for c in family()]


def by_name(name):
    return {c.name: c for c in family()}[name]


def alignment_bodies():
    """The bodies that are submitted sixteen times in one batch, so that
    inflate_harness.skewed_batch places each at every source address mod 16."""
    return [by_name("two_units").data] + [by_name(f"one_match_{n}").data for n in UNIT_END_LENGTHS]
