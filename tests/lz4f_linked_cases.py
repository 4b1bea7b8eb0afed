"""TEST INFRASTRUCTURE ONLY: LZ4 frames with linked blocks (B.Indep = 0), built
without liblz4, and the case sets shared by tests/test_lz4f_linked.py (CPU) and
tests/test_lz4f_linked_gpu.py.

* `compress_linked`: a small greedy block writer whose matches may reach up to
  65,535 bytes back over the whole frame.  Valid, not liblz4's bytes.
* `hand_blocks`, `far_blocks`: blocks put together sequence by sequence (lz4_blocks.
  encode_block) with offsets larger than the position in the block.
* `matches`: a walker over a frame's sequences that says where each match's
  source lies; `kinds` names what the kernels can get wrong.
* `fixture`: tests/golden/lz4f_linked_vectors.json, liblz4's own linked frames.

Expected values come from lz4f_ref.decode_frame alone."""
from __future__ import annotations

import json
import struct
from pathlib import Path

import numpy as np

import lz4f_ref as R
from gen_inputs import build_input
from lz4_blocks import encode_block
from lz4f_nosize_cases import END, blocks_in, text, xxh

GOLDEN = Path(__file__).resolve().parent / "golden" / "lz4f_linked_vectors.json"
MAX_OFF = 65535


def prefix(produced: int) -> int:
    """The history a block can reach when its frame has produced `produced`
    bytes before it (lz4f::linked_prefix)."""
    return min(produced, MAX_OFF)


# ---- the greedy writer

def _block_seqs(x: bytes, a: int, b: int, table: dict):
    """(sequences, final literals) of x[a:b] with matches into x[:b]: a match
    starts at least 12 bytes and ends at least 5 bytes before the block's end
    (the decoder's end rules)."""
    seqs, anchor, i = [], a, a
    last_start, last_end = b - 12, b - 5
    while i <= last_start:
        key = x[i:i + 4]
        cand = table.get(key)
        table[key] = i
        if cand is None or i - cand > MAX_OFF:
            i += 1
            continue
        ml = 4
        while i + ml < last_end and x[cand + ml] == x[i + ml]:
            ml += 1
        seqs.append((x[anchor:i], i - cand, ml))
        for j in range(i + 1, min(i + ml, last_start + 1), 7):  # a few positions inside the match
            table[x[j:j + 4]] = j
        i += ml
        anchor = i
    return seqs, x[anchor:b]


def compress_linked(x: bytes, cuts, raw_pieces=()):
    """[(stored bytes, raw)] of x cut at `cuts` (piece lengths); a piece that
    does not shrink, or whose index is in raw_pieces, is stored raw."""
    table, out, at = {}, [], 0
    for k, n in enumerate(cuts):
        seqs, final = _block_seqs(x, at, at + n, table)
        blk = encode_block(seqs, final)
        raw = k in raw_pieces or len(blk) >= n
        out.append((x[at:at + n], True) if raw else (blk, False))
        at += n
    assert at == len(x)
    return out


def frame(blocks, content: bytes, bid: int = 4, sized=False, checksum=False, bsum=False) -> bytes:
    """A linked frame from [(stored bytes, raw)]."""
    out = [R.header(len(content) if sized else None, bid, checksum, False, bsum)]
    for b, raw in blocks:
        out.append(struct.pack("<I", len(b) | (R.RAW if raw else 0)) + b)
        if bsum:
            out.append(struct.pack("<I", xxh(b)))
    out.append(END)
    if checksum:
        out.append(struct.pack("<I", xxh(content)))
    return b"".join(out)


def full_cuts(n: int, bs: int = 65536):
    return [bs] * (n // bs) + ([n % bs] if n % bs else [])


def _rnd(seed: int, n: int) -> bytes:
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


# ---- hand-built blocks

def _apply(out: bytearray, seqs, final: bytes):
    for lit, off, ml in seqs:
        out += lit
        assert 0 < off <= len(out)
        for _ in range(ml):
            out.append(out[-off])
    out += final


def hand_blocks():
    """([(stored bytes, raw)], content) of a frame of short blocks whose
    matches sit at every edge of the history; the comments give the source of
    each match relative to its block's first byte."""
    out, blocks = bytearray(), []

    def add(seqs, final):
        _apply(out, seqs, final)
        blocks.append((encode_block(seqs, final), False))

    add([], _rnd(1, 40))                                   # 40 bytes produced
    add([(b"", 40, 20),                                    # no literals; offset = all that was produced; [-40, -20)
         (b"ab", 5, 30)], _rnd(2, 12))                     # 104
    add([(b"", 3, 40),                                     # pattern from the previous block's last 3 bytes
         (_rnd(3, 5), 55, 30)], _rnd(4, 12))               # [-10, 20): history into the block; 191
    add([(_rnd(5, 10), 20, 50),                            # [-10, 40): the same, overlapping its output
         (b"", 210, 100),                                  # [-150, -50): a whole-wave match from history
         (_rnd(6, 3), 193, 20)], _rnd(7, 12))              # [-30, -10): ends 10 below the block; 386
    raw = _rnd(8, 50)
    out += raw
    blocks.append((raw, True))                             # 436
    add([(b"xy", 32, 8)], _rnd(9, 12))                     # [-30, -22): inside the raw block; 458
    for s in (10, 11, 12):
        add([], _rnd(s, 30))                               # three short blocks; 548
    add([(b"q", 101, 16),                                  # [-100, -84): three blocks back
         (b"", 17 + 548, 70)], _rnd(13, 12))               # offset = all that was produced, a long match
    return blocks, bytes(out)


def far_blocks():
    """([(stored bytes, raw)], content): a full raw block of 65,536 bytes, then
    a block whose matches reach 65,535 bytes back."""
    first = text(65536, seed=77)
    out = bytearray(first)
    seqs = [(b"x", MAX_OFF, 5000),    # [-65534, -60534): longer than 4,096 bytes, 65,537 produced
            (b"", MAX_OFF, 10),
            (_rnd(14, 20), 16, 64)]
    final = _rnd(15, 13)
    _apply(out, seqs, final)
    return [(first, True), (encode_block(seqs, final), False)], bytes(out)


_FRAMES = {}


def frames():
    """[(name, content, frame, block count)]: every frame of the case set but
    the fixture's."""
    if "v" in _FRAMES:
        return _FRAMES["v"]
    out = []

    def add(name, blocks, x, **kw):
        out.append((name, x, frame(blocks, x, **kw), len(blocks)))
    hb, hx = hand_blocks()
    add("hand", hb, hx)
    add("hand_sums", hb, hx, checksum=True, bsum=True)
    fb, fx = far_blocks()
    add("far_sized", fb, fx, sized=True, checksum=True)
    add("far", fb, fx)
    for n in (65537, 68536, 131073):
        x = text(n, seed=n % 89)
        add(f"greedy_sized_{n}", compress_linked(x, full_cuts(n)), x, sized=True, checksum=n == 131073)
    x = text(200000, seed=12)
    add("greedy_id5_sized", compress_linked(x, [200000]), x, bid=5, sized=True)
    x = text(30000, seed=13)
    add("greedy_pieces", compress_linked(x, [1000] * 30), x, bsum=True)
    x = text(9000, seed=14) + _rnd(16, 3000) + text(9000, seed=14)
    add("greedy_raw_middle", compress_linked(x, [3000] * 7), x, checksum=True)
    x = text(5000, seed=15)
    add("greedy_forced_raw", compress_linked(x, [1, 70, 2000, 900, 2029], raw_pieces=(2,)), x)
    _FRAMES["v"] = out
    return out


def fixture():
    """[(name, content, frame, block count)] of liblz4's linked frames."""
    if "fix" not in _FRAMES:
        v = json.loads(GOLDEN.read_text())
        out = []
        for e in v["frames"]:
            x = fixture_input(e["input"])
            assert len(x) == e["out_len"]
            f = bytes.fromhex(e["hex"])
            out.append((e["name"], x, f, len(blocks_in(f)[2])))
        _FRAMES["fix"] = out
    return _FRAMES["fix"]


def fixture_input(spec: dict) -> bytes:
    """gen_inputs recipes and two more: "text_random_middle", text with one
    random piece, and "text_repeated", the first `period` bytes of a text over
    and over (most of such a frame is long matches that far back, many of them
    into an earlier block, which keeps the fixture file small)."""
    if spec["gen"] == "text_repeated":
        t = build_input({"gen": "text", "seed": spec["seed"], "size": spec["period"]})
        return (t * (spec["size"] // spec["period"] + 1))[:spec["size"]]
    if spec["gen"] == "text_random_middle":
        t = fixture_input({"gen": "text_repeated", "seed": spec["seed"], "size": spec["size"], "period": spec["period"]})
        k, n = spec["at"], spec["piece"]
        return t[:k] + _rnd(spec["seed"], n) + t[k + n:]
    return build_input(spec)


def all_frames():
    return frames() + fixture()


# ---- the walker

def matches(f: bytes):
    """Every match of a frame's compressed blocks: dicts of k (block), first
    (first sequence of its block), lit, p (bytes its block produced before the
    match), off, ml, before (bytes the frame produced before the block), src
    (block holding the source's first byte) and src_raw."""
    ok, bmax, blocks = blocks_in(f)
    assert ok
    starts, produced, out = [], 0, []
    for k, (b, raw) in enumerate(blocks):
        starts.append((produced, raw))
        if raw:
            produced += len(b)
            continue
        n, ip, p, first = len(b), 0, 0, True
        while True:
            token = b[ip]
            ip += 1
            lit = token >> 4
            if lit == 15:
                while True:
                    c = b[ip]
                    ip += 1
                    lit += c
                    if c != 255:
                        break
            ip += lit
            p += lit
            if ip == n:
                break
            off = b[ip] | (b[ip + 1] << 8)
            ip += 2
            ml = (token & 15) + 4
            if token & 15 == 15:
                while True:
                    c = b[ip]
                    ip += 1
                    ml += c
                    if c != 255:
                        break
            at = produced + p - off
            src = max(j for j, (s, _) in enumerate(starts) if s <= at) if at >= 0 else -1
            out.append({"k": k, "first": first, "lit": lit, "p": p, "off": off, "ml": ml, "before": produced,
                        "src": src, "src_raw": src >= 0 and starts[src][1]})
            p += ml
            first = False
        produced += p
    return out


KINDS = ("history_only", "history_into_block", "history_into_block_overlapping", "offset_65535", "offset_all_produced",
         "three_blocks_back", "raw_history", "first_without_literals", "pattern_from_previous_block",
         "long_from_history", "over_4096_from_history", "far_ends_just_below_block")


def kinds(m: dict) -> set:
    """The kinds (KINDS) one match belongs to; s, e: its source relative to the
    block's first byte."""
    s = m["p"] - m["off"]
    e = s + m["ml"]
    out = set()
    if e <= 0:
        out.add("history_only")
    if s < 0 < e:
        out.add("history_into_block")
        if m["off"] < m["ml"]:
            out.add("history_into_block_overlapping")
    if m["off"] == MAX_OFF and m["before"] + m["p"] >= MAX_OFF:
        out.add("offset_65535")
    if m["off"] == m["before"] + m["p"] < MAX_OFF:
        out.add("offset_all_produced")
    if s < 0 and m["k"] - m["src"] >= 3:
        out.add("three_blocks_back")
    if s < 0 and m["src_raw"]:
        out.add("raw_history")
    if m["first"] and m["lit"] == 0:
        out.add("first_without_literals")
    if m["off"] < 16 and m["ml"] > m["off"] and s < 0:
        out.add("pattern_from_previous_block")
    if m["ml"] > 64 and s < 0:
        out.add("long_from_history")
    if m["ml"] > 4096 and s < 0:
        out.add("over_4096_from_history")
    if m["off"] >= 16 and m["ml"] <= 64 and -24 <= e <= 0:
        out.add("far_ends_just_below_block")
    return out


def block_prefixes(f: bytes):
    """[bytes the frame produced before each block] by the frame's own lengths."""
    ok, bmax, blocks = blocks_in(f)
    out, produced = [], 0
    for b, raw in blocks:
        out.append(produced)
        produced += len(b) if raw else R.block_length(b, bmax)
    return out


# ---- negative cases

def negatives():
    """[(name, frame, capacity)], all CORRUPT by the oracle: an offset one byte
    beyond what the frame has produced, at block 1 and at a later block, and a
    linked frame cut to its second block alone."""
    out = []
    a = _rnd(20, 40)
    ok1 = encode_block([(b"", 40, 20)], _rnd(21, 12))
    bad1 = encode_block([(b"", 41, 20)], _rnd(21, 12))
    out.append(("beyond_at_block_1", frame([(encode_block([], a), False), (bad1, False)], b""), 72))
    mid = encode_block([(b"ab", 3, 10)], _rnd(22, 12))  # 24 bytes: 96 produced after blocks 0..2
    bad3 = encode_block([(b"zz", 99, 8)], _rnd(23, 12))  # 98 produced at the match: 99 is one beyond
    ok3 = encode_block([(b"zz", 98, 8)], _rnd(23, 12))
    out.append(("beyond_at_block_3",
                 frame([(encode_block([], a), False), (ok1, False), (mid, False), (bad3, False)], b""), 118))
    good = frame([(encode_block([], a), False), (ok1, False), (mid, False), (ok3, False)], b"")
    assert R.decode_frame(None, good, 118)[0] == R.OK
    name, x, f, nb = next(t for t in frames() if t[0] == "greedy_sized_68536")
    ok, bmax, blocks = blocks_in(f)
    assert any(k["k"] == 1 and k["p"] < k["off"] for k in matches(f))
    out.append(("second_block_alone", frame(blocks[1:], b""), len(x)))
    return out


# ---- mutated frames
MUT_SEED = 7
MUT_COUNT = 200


def mutation_bases():
    """One sized 65,536 + 3,000 B frame and three no-size frames of short pieces."""
    by = {n: (x, f) for n, x, f, _ in frames()}
    return [by["greedy_sized_68536"], by["greedy_pieces"], by["greedy_raw_middle"], by["hand_sums"]]


def mutated():
    """(frames, capacities): MUT_COUNT mutations (flip, truncate, insert, as
    lz4f_nosize_cases.mutated) at the exact capacity of the base's content."""
    rng = np.random.default_rng(MUT_SEED)
    bases = mutation_bases()
    out, caps = [], []
    for t in range(MUT_COUNT):
        x, f = bases[t % len(bases)]
        b = bytearray(f)
        kind = rng.random()
        if kind < 0.6:
            for _ in range(int(rng.integers(1, 3))):
                p = int(rng.integers(7, len(b)))
                b[p] ^= 1 << int(rng.integers(0, 8))
        elif kind < 0.8:
            b = b[:int(rng.integers(7, len(b)))]
        else:
            p = int(rng.integers(7, len(b) + 1))
            b[p:p] = rng.integers(0, 256, int(rng.integers(1, 5)), dtype=np.uint8).tobytes()
        out.append(bytes(b))
        caps.append(len(x))
    return out, caps
