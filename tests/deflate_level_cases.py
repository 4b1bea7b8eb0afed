"""Compression levels of the deflate writer (include/flare_deflate_level_gpu.h;
csrc/deflate_format.h, "levels"): the host model at a level, and the
constructed bodies that tell level 2's parse from level 1's -- two candidates
per hash slot, the insert rule, the lazy step.  Used by
tests/test_deflate_level.py (host model) and tests/test_deflate_level_gpu.py
(device); the family itself is tests/deflate_cases.py's.

The constructed bodies use letters for the strings under test and filler
bytes of 128 and up between them, so that nothing but the strings repeats;
everything is seeded, and the token tests assert what they rely on."""
from __future__ import annotations

import ctypes
import functools
import random

import deflate_cases as C

STORED, FAST, BEST = 0, 1, 2
LEVELS = (STORED, FAST, BEST)


@functools.lru_cache(maxsize=None)
def host():
    L = C.host()
    c = ctypes
    L.fsh_cpu_deflate_level.argtypes = [c.c_uint32, c.c_uint32, c.c_char_p, c.c_size_t, c.c_void_p, c.c_size_t,
                                        c.POINTER(c.c_uint64)]
    L.fsh_cpu_deflate_unit_types_level.argtypes = [c.c_uint32, c.c_char_p, c.c_size_t, c.POINTER(c.c_uint64)]
    L.fsh_cpu_deflate_unit_types_level.restype = None
    L.fsh_cpu_deflate_tokens_level.argtypes = [c.c_uint32, c.c_char_p, c.c_size_t, c.c_void_p, c.c_size_t]
    L.fsh_cpu_deflate_tokens_level.restype = c.c_size_t
    return L


def deflate_into(fmt: int, level: int, data: bytes, cap: int):
    """(status, length, the cap bytes of the buffer): fsh_cpu_deflate_level
    into a buffer of cap bytes of GUARD, followed by GUARD, which must stay."""
    out = ctypes.create_string_buffer((C.GUARD * (cap // 32 + 2))[:cap + 32], cap + 32)
    ln = ctypes.c_uint64(99)
    st = host().fsh_cpu_deflate_level(fmt, level, data, len(data), out, cap, ctypes.byref(ln))
    assert out.raw[cap:] == C.GUARD, "the host model wrote past the capacity"
    return st, ln.value, out.raw[:cap]


@functools.lru_cache(maxsize=None)
def model(fmt: int, level: int, data: bytes) -> bytes:
    """The host model's body for `data` at `level`: the definition of the device's bytes."""
    cap = host().fsh_cpu_deflate_bound(len(data), fmt)
    st, ln, buf = deflate_into(fmt, level, data, cap)
    assert st == 0 and ln <= cap
    return buf[:ln]


def unit_types(level: int, data: bytes):
    counts = (ctypes.c_uint64 * 3)()
    host().fsh_cpu_deflate_unit_types_level(level, data, len(data), counts)
    return tuple(int(v) for v in counts)


def tokens(level: int, data: bytes):
    """The model's parse of one unit at level 1 or 2, as deflate_cases.tokens gives it."""
    buf = (ctypes.c_uint32 * (len(data) + 1))()
    k = host().fsh_cpu_deflate_tokens_level(level, data, len(data), buf, len(data) + 1)
    assert k or not data
    return [("lit", t & 0xff) if t >> 31 else ("match", t & 511, (t >> 9) & 0x1ffff) for t in buf[:k]]


def token_starting_at(toks, pos: int):
    """The token whose first byte is input position pos, or None when a match covers it."""
    at = 0
    for t in toks:
        if at == pos:
            return t
        if at > pos:
            return None
        at += 1 if t[0] == "lit" else t[1]
    return None


# ---- the constructed bodies

def filler(n: int, seed: int) -> bytes:
    r = random.Random(9000 + seed)
    return bytes(r.randrange(128, 256) for _ in range(n))


def _letters(n: int, seed: int) -> bytes:
    """n letters with no 4 of them in a row seen twice (a shuffled walk over pairs would do; here: checked)."""
    r = random.Random(500 + seed)
    while True:
        s = bytes(r.choice(b"efghijklmnopqrstuvwxyz") for _ in range(n))
        if len({s[i:i + 3] for i in range(n - 2)}) == n - 2:
            return s


def _place(parts, total: int, seed: int) -> bytes:
    """parts: (position, bytes) ascending; filler everywhere else, `total` bytes in all."""
    out = bytearray()
    for k, (pos, s) in enumerate(parts):
        assert pos >= len(out), (pos, len(out))
        out += filler(pos - len(out), seed * 16 + k)
        out += s
    out += filler(total - len(out), seed * 16 + 15)
    return bytes(out)


S_AT, T_AT, S_AGAIN = 0, 192, 320


def two_candidates() -> bytes:
    """A 100-byte string S at 0, T = S's first 4 bytes and nothing more at 192
    (three windows on), S again at 320: the slot's newer candidate is T, the
    older S.  Level 1 finds 4 bytes at distance 128, level 2 the 100 at 320."""
    s = b"ABCD" + _letters(96, 1)
    t = b"ABCD" + filler(16, 2)
    return _place([(S_AT, s), (T_AT, t), (S_AGAIN, s)], 480, 1)


SAME_WINDOW_AT = 191


def insert_same_window() -> bytes:
    """"ABCD" + X at 0 and "ABCD" + Y at 20, one window, one slot; "ABCD" + X
    again at 191, a window's last position (no lazy step there).  Only
    position 20 was kept: the match is the 4 bytes at distance 171, not X's 12
    at 191."""
    return _place([(0, b"ABCD" + _letters(8, 2)), (20, b"ABCD" + _letters(8, 3)),
                   (SAME_WINDOW_AT, b"ABCD" + _letters(8, 2))], 260, 2)


THREE_WINDOWS_AT = 255


def insert_three_windows() -> bytes:
    """"ABCD" + A at 0, + B at 64, + C at 128: three windows, one slot.  At 255
    "ABCD" + A again: the slot holds 128 and 64, the first is gone, so the
    match is 4 bytes at distance 127 (equal lengths: the nearer), not A's 24."""
    a, b, c = (_letters(20, k) for k in (4, 5, 6))
    return _place([(0, b"ABCD" + a), (64, b"ABCD" + b), (128, b"ABCD" + c), (THREE_WINDOWS_AT, b"ABCD" + a)], 330, 3)


Q_AT = 31  # where "bcdefghij" starts in the lazy bodies


def lazy_pair(at: int, successor: int = 9) -> bytes:
    """"abcd" at 0 and "bcdefghij" (or "bcde": successor = 4) at 31, then
    "abcdefghij" at `at`: position `at` has a 4-byte match, `at + 1` one of
    `successor` bytes."""
    q = b"bcdefghij"[:successor]
    return _place([(0, b"abcd"), (Q_AT, q), (at, b"abcdefghij")], at + 80, 4 + at)


LAZY = {"lazy_lanes_0_1": (128, 9), "lazy_lanes_62_63": (190, 9), "lazy_lanes_63_64": (191, 9),
        "lazy_equal_lengths": (140, 4)}


@functools.lru_cache(maxsize=None)
def constructed():
    out = [("two_candidates", two_candidates()), ("insert_same_window", insert_same_window()),
           ("insert_three_windows", insert_three_windows())]
    out += [(name, lazy_pair(at, succ)) for name, (at, succ) in LAZY.items()]
    return out


def constructed_by_name(name: str) -> bytes:
    return dict(constructed())[name]
