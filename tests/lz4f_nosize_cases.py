"""TEST INFRASTRUCTURE ONLY: LZ4 frames without a content size, built from the
frame oracle's pieces (tests/lz4f_ref.py: header, xxh32; bind.Lz4Oracle's block
compressor), and the case sets shared by tests/test_lz4f_nosize.py (CPU) and
tests/test_lz4f_nosize_gpu.py.  Expected values come from lz4f_ref alone:
`decode_frame`, `block_length`, and `decoded_length` here, which is the
definition of fsg_lz4f_decoded_lengths_batch (include/flare_lz4_gpu.h) written
with lz4f_ref's functions."""
from __future__ import annotations

import struct

import numpy as np

import fsg
import lz4f_ref as R
from lz4_blocks import encode_block, header as varint, random_block

END = b"\0\0\0\0"
EDGE_LENGTHS = (1, 13, 65535, 65536, 65537, 131073, 200000)
BIG = (4 << 20) + 17  # the fixture's 4 MiB + 17 random bytes ({"gen": "random", "seed": 6})
_XXH = {}


def xxh(x: bytes) -> int:
    """R.xxh32, once per input (pure Python: seconds for 4 MiB)."""
    key = (len(x), fsg.fnv1a64(x))
    if key not in _XXH:
        _XXH[key] = R.xxh32(x)
    return _XXH[key]


def bid_for(n: int) -> int:
    """The smallest block size id whose block holds n bytes."""
    return R.frame_block_id(n, 7)


def stored(o, piece: bytes, raw=None):
    """(stored bytes, raw) of one piece: the oracle's block, or the piece
    itself when that is not shorter (the compressor's rule) or raw is True."""
    if raw is None or raw is False:
        c = o.compress_block(piece)
        if raw is False or len(c) < len(piece):
            return c, False
    return piece, True


def frame_of_blocks(blocks, content: bytes | None, bid: int, checksum=False, bsum=False, indep=True) -> bytes:
    """A frame without a content size from [(stored bytes, raw)]; the content
    checksum is over `content`."""
    out = [R.header(None, bid, checksum, indep, bsum)]
    for b, raw in blocks:
        out.append(struct.pack("<I", len(b) | (R.RAW if raw else 0)) + b)
        if bsum:
            out.append(struct.pack("<I", xxh(b)))
    out.append(END)
    if checksum:
        out.append(struct.pack("<I", xxh(content)))
    return b"".join(out)


def frame_of_pieces(o, pieces, bid: int, checksum=False, bsum=False, raw=None) -> bytes:
    """raw: {piece index: True / False} to force a piece raw or compressed."""
    raw = raw or {}
    return frame_of_blocks([stored(o, p, raw.get(i)) for i, p in enumerate(pieces)], b"".join(pieces), bid, checksum,
                           bsum)


def nosize_frame(o, x: bytes, bid: int = 4, checksum=False, bsum=False) -> bytes:
    """What LZ4F_compressFrame writes for x with contentSize left 0."""
    bs = R.block_bytes(bid)
    return frame_of_pieces(o, [x[i:i + bs] for i in range(0, len(x), bs)], R.frame_block_id(len(x), bid), checksum,
                           bsum)


def block_frame(blk: bytes, bid: int) -> bytes:
    """One compressed block, as it is, in a frame of its own."""
    return frame_of_blocks([(blk, False)], None, bid)


def blocks_in(f: bytes):
    """(ok, block maximum, [(stored bytes, raw)]) by the frame's size words: the
    structure rules of the serial reader, no checksum looked at."""
    st, hl, bmax, flg, size = R.parse_header(f)
    bsum = 4 if flg & R.F_BSUM else 0
    n, ip, out = len(f), hl, []
    while True:
        if n - ip < 4:
            return False, bmax, out
        word = struct.unpack_from("<I", f, ip)[0]
        ip += 4
        if word == 0:
            break
        sz = word & ~R.RAW
        if sz > bmax or n - ip < sz + bsum:
            return False, bmax, out
        out.append((f[ip:ip + sz], bool(word & R.RAW)))
        ip += sz + bsum
    if flg & R.F_CSUM:
        ip += 4
    return ip == n, bmax, out


def decoded_length(f: bytes):
    """(status, length) as fsg_lz4f_decoded_lengths_batch defines them."""
    st, hl, bmax, flg, size = R.parse_header(f)
    if st != R.OK:
        return R.BAD_HEADER, 0
    if size is not R.NO_SIZE:
        return R.OK, size
    ok, bmax, blocks = blocks_in(f)
    lens = [len(b) if raw else R.block_length(b, bmax) for b, raw in blocks]
    if not ok or None in lens:
        return R.CORRUPT, 0
    return R.OK, sum(lens)


def text(n: int, seed: int | None = None) -> bytes:
    return fsg.make_batch(fsg.KIND_TEXT, [n], first_index=n if seed is None else seed).item(0)


def big_input() -> bytes:
    from gen_inputs import build_input
    return build_input({"gen": "random", "seed": 6, "size": BIG})


# ---- GPU test 1: the routing edges
_EDGES = {}


def routing_edges(o):
    """[(input, frame, block count)]: the edge lengths and the 4 MiB + 17 input
    at ids 4..7, without and with a content checksum."""
    if not _EDGES:
        xs = [text(n) for n in EDGE_LENGTHS] + [big_input()]
        out = []
        for bid in (4, 5, 6, 7):
            for cs in (False, True):
                for x in xs:
                    out.append((x, nosize_frame(o, x, bid, cs), -(-len(x) // R.block_bytes(bid))))
        _EDGES["v"] = out
    return _EDGES["v"]


# ---- GPU test 2: free-form blocks
def free_form(o):
    """[(content, frame, block count)]: pieces of any length, as
    LZ4F_compressUpdate with a flush after each writes them."""
    out = []

    def add(lens, bid, raw=None, cs=True):
        src = text(sum(lens), seed=7 + len(out))
        pieces, at = [], 0
        for n in lens:
            pieces.append(src[at:at + n])
            at += n
        out.append((src, frame_of_pieces(o, pieces, bid, cs, raw=raw), len(lens)))
    add([1, 70, 65536, 5, 30000], 4)
    add([262144, 3, 262143], 5)
    add([5000, 3000, 7000], 4, raw={0: False, 1: True, 2: False})
    add([1000] * 130, 4, cs=False)
    return out


def one_block_frames(o, count=300):
    """`count` frames of one small block each."""
    return [(x, nosize_frame(o, x, 4, i % 3 == 0), 1) for i, x in
            enumerate(text(20 + (i * 37) % 900, seed=1000 + i) for i in range(count))]


# ---- GPU test 3: hard blocks for both walkers
def _rnd(rng, n):
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


def _ext(lit: int) -> int:
    """Extension bytes of a literal length."""
    return 0 if lit < 15 else 1 + (lit - 15) // 255


def _seq_bytes(pad: int) -> int:
    """Stored bytes of a sequence of `pad` literals and a match below 19."""
    return 1 + _ext(pad) + pad + 2


def window_blocks():
    """Blocks built for the 64-byte window walk: [(name, block)]."""
    rng = np.random.default_rng(77)
    out = []
    tail = _rnd(rng, 12)
    # a literal of L bytes that ends exactly at a 64-byte edge of the block
    # (the offset field starts there), or one byte past it, after a first
    # sequence of `pad` literals
    for L in (64, 65, 4097):
        for past in (0, 1):
            for edge in (64 * (L // 64 + 2), 4096 + 64 * (L // 64 + 2), 8192 + 64 * (L // 64 + 2)):
                pad = next(p for p in range(1, edge) if _seq_bytes(p) + 1 + _ext(L) + L == edge + past)
                out.append((f"lit{L}_edge{edge}+{past}",
                            encode_block([(_rnd(rng, pad), 1, 4), (_rnd(rng, L), 3, 5)], tail)))
    # the last sequence's literals end the block at a window edge
    for n in (64, 128, 4096, 8192):
        pad = next(p for p in range(1, n) if _seq_bytes(p) + 1 + _ext(20) + 20 == n)
        blk = encode_block([(_rnd(rng, pad), 2, 6)], _rnd(rng, 20))
        assert len(blk) == n
        out.append((f"last_at_{n}", blk))
    # a run of 255s in each length field across the staging boundaries (4 KiB
    # halves of the ring): the run starts a little below byte 4096 / 8192
    for at in (4096, 8192):
        for shift in (0, 7, 16, 40):
            pad = at - 60 - shift
            run = 255 * 120 + 15 + 33
            out.append((f"lit_run_{at}_{shift}", encode_block([(_rnd(rng, pad), 9, 8), (_rnd(rng, run), 5, 9)], tail)))
            out.append((f"match_run_{at}_{shift}",
                        encode_block([(_rnd(rng, pad), 9, 8), (_rnd(rng, 3), 5, 255 * 120 + 19 + 60)], tail)))
    # blocks of one token
    out.append(("one_token_empty", b"\x00"))
    out.append(("one_token_5", b"\x50hello"))
    out.append(("one_token_ext", encode_block([], _rnd(rng, 300))))
    return out


def hard_blocks():
    """[(block, id)]: the 120 blocks of tests/lz4_blocks.py (the recipe of
    test_lz4_gpu's two-pass test), then window_blocks; the id by decoded size."""
    rng = np.random.default_rng(41)
    out = []
    for t in range(120):
        body, want = random_block(rng, int(rng.choice([50, 3000, 40000, 200000])))
        out.append((body[len(varint(len(want))):], bid_for(len(want))))
    for name, blk in window_blocks():
        ln = R.block_length(blk, 4 << 20)
        assert ln is not None, name
        out.append((blk, bid_for(ln)))
    return out


# ---- GPU test 4: mutated frames
MUT_SEED = 2024
MUT_COUNT = 400


def mutated(o):
    """(frames, capacities, base index): MUT_COUNT mutations of a few base
    frames of 1 to 5 blocks, each at the capacities exact, 0 and exact - 1 of
    its base's content."""
    rng = np.random.default_rng(MUT_SEED)
    bases = []
    for lens, cs, bsum in (([300], True, False), ([3000, 40], False, False), ([20000, 500, 70], True, True),
                           ([70000, 3, 9000, 1200], False, True), ([900, 5000, 65536, 20, 700], True, False)):
        src = text(sum(lens), seed=300 + len(bases))
        pieces, at = [], 0
        for n in lens:
            pieces.append(src[at:at + n])
            at += n
        bases.append((src, frame_of_pieces(o, pieces, 4, cs, bsum)))
    frames, caps, which = [], [], []
    for t in range(MUT_COUNT):
        k = t % len(bases)
        x, f = bases[k]
        b = bytearray(f)
        kind = rng.random()
        if kind < 0.6:  # byte flips after the descriptor
            for _ in range(int(rng.integers(1, 3))):
                p = int(rng.integers(7, len(b)))
                b[p] ^= 1 << int(rng.integers(0, 8))
        elif kind < 0.8:  # truncation
            b = b[:int(rng.integers(7, len(b)))]
        else:  # insertion
            p = int(rng.integers(7, len(b) + 1))
            b[p:p] = _rnd(rng, int(rng.integers(1, 5)))
        for cap in (len(x), 0, max(len(x) - 1, 0)):
            frames.append(bytes(b))
            caps.append(cap)
            which.append(k)
    return frames, caps, which


def mutated_classes(o, frames, caps):
    """By the reference alone, over the frames at their exact capacity (every
    third case): (accepted, every block has a length yet the frame does not
    decode, some block has no length)."""
    acc = nolen = undec = 0
    for f, cap in list(zip(frames, caps))[::3]:
        if R.parse_header(f)[0] != R.OK:
            continue
        if R.decode_frame(o, f, cap)[0] == R.OK:
            acc += 1
            continue
        ok, bmax, blocks = blocks_in(f)
        if not ok or not blocks:
            continue
        lens = [len(b) if raw else R.block_length(b, bmax) for b, raw in blocks]
        if None in lens:
            nolen += 1
        elif sum(lens) <= cap:
            undec += 1
    return acc, undec, nolen


# ---- GPU test 5: a mixed batch
def mixed(o):
    """[(frame, capacity, kind)] with kind in fast / nosize / linked / empty /
    bad_header: sized, no-size, linked and empty frames and a bad header."""
    from lz4f_cases import load
    vec = load()
    out = []
    for i, n in enumerate((500, 70000, 200000, 300000)):
        x = text(n, seed=50 + i)
        out.append((R.compress_frame(o, x, 4, bool(i % 2)), n, "fast"))
        out.append((nosize_frame(o, x, 4, bool(i % 2)), n + (i % 2) * 100, "nosize"))
    for d in vec["decode_ok"]:
        if d["route"] == "serial_linked":
            out.append((bytes.fromhex(d["hex"]), d["out_len"], "linked"))
    out.append((R.header(None, 4, False) + END, 0, "empty"))
    out.append((R.header(None, 4, True) + END + struct.pack("<I", R.xxh32(b"")), 10, "empty"))
    bad = bytearray(nosize_frame(o, text(100), 4))
    bad[5] ^= 0x10
    out.append((bytes(bad), 100, "bad_header"))
    return out
