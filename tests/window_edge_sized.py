"""window_edge.py's model and generator for any window size and kept history.

exec_kernel<5> runs two instances of exec5_message
(flare-cpp_amd/csrc/decode_v4_exec5.h): the general one assembles a message's
output in a 3,072-byte LDS window, which tests/window_edge.py models; the
folded one (whole bodies of at most big_threshold compressed bytes, one wave
each) in a 4,096-byte window whose kept history at a slide is 512..3,024
bytes.  Group, restart and slide rules are the same:

  * a group is the next <= 64 tags, cut before a literal longer than 64 bytes
    and where the group's output would pass 1,024 bytes;
  * a literal longer than 64 bytes runs alone, and the window restarts at
    sbase = (op & ~15) - 16;
  * before a group whose output would overrun the window, the window slides to
    sbase = (op - keep) & ~15.

`edge_stream` lays down tag lengths, runs the model and gives each copy an
offset that puts its source within `spread` bytes of its group's sbase.
(Slots 16-byte aligned; at another alignment the base moves by less than 16
bytes and the sources stay within spread + 16 of it.)
"""
from __future__ import annotations

import numpy as np

from window_edge import _emit_copy, _emit_literal

GROUP_BYTES, GROUP_TAGS = 1024, 64
WINDOW_FOLDED = 4096
MAX_KEEP_FOLDED = (WINDOW_FOLDED - 1024 - 48) & ~15  # kMaxKeepWhole, decode_v4_plan.h


def window_model(tags, window: int, keep: int):
    """tags: list of (is_literal, length, offset).  Per tag: the window base
    in force when its group runs, and its output position."""
    sb = [0] * len(tags)
    pos = [0] * len(tags)
    op, sbase, i = 0, 0, 0
    while i < len(tags):
        lit, ln, _ = tags[i]
        if lit and ln > 64:
            sb[i], pos[i] = sbase, op
            op += ln
            sbase = (op & ~15) - 16
            i += 1
            continue
        j, tot = i, 0
        while j < len(tags) and j - i < GROUP_TAGS:
            l2, n2, _ = tags[j]
            if (l2 and n2 > 64) or tot + n2 > GROUP_BYTES:
                break
            tot += n2
            j += 1
        if op + tot - sbase > window:
            sbase = (op - keep) & ~15
        t = op
        for k in range(i, j):
            sb[k], pos[k] = sbase, t
            t += tags[k][1]
        op, i = t, j
    return sb, pos


def edge_stream(rng, target: int, window: int, keep: int, spread: int = 24):
    """(compressed, raw, n_edge): a valid stream of ~target output bytes whose
    copies read from sbase - spread .. sbase + spread of their group (when the
    output so far allows); n_edge counts the copies whose first 16-byte source
    load straddles sbase."""
    tags = []
    n = 0
    while n < target:
        r = rng.random()
        if r < 0.08 and n > 0:
            ln = int(rng.integers(65, 400))       # long literal: window restart
            tags.append((True, ln, 0))
        elif r < 0.35 or n < 32:
            ln = int(rng.integers(1, 17))
            tags.append((True, ln, 0))
        else:
            ln = int(rng.integers(4, 65))
            tags.append((False, ln, 16))          # offset fixed below (>= 16)
        n += ln
    sb, pos = window_model(tags, window, keep)
    out = bytearray()
    body = []
    n_edge = 0
    for (lit, ln, _), s, p in zip(tags, sb, pos):
        assert p == len(out)
        if lit:
            data = bytes(rng.integers(0, 256, ln, dtype=np.uint8))
            body.append(_emit_literal(data))
            out += data
            continue
        src = s + int(rng.integers(-spread, spread + 1))
        off = p - src
        if off < 16 or off > p or off > 0xFFFF:
            off = int(rng.integers(16, p + 1)) if p >= 16 else p
        if off < 16:  # too little output yet for a non-pattern copy: a literal instead
            data = bytes(rng.integers(0, 256, ln, dtype=np.uint8))
            body.append(_emit_literal(data))
            out += data
            continue
        src = p - off
        n_edge += src < s < src + 16
        body.append(_emit_copy(off, ln))
        for _ in range(ln):
            out.append(out[-off])
    hdr = bytearray()
    v = len(out)
    while v >= 0x80:
        hdr.append((v & 0x7F) | 0x80)
        v >>= 7
    hdr.append(v)
    return bytes(hdr) + b"".join(body), bytes(out), n_edge
