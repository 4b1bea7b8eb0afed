"""Compressed Snappy batches shared by the GPU tests (built with the oracle's
encoder and tests/snappy_streams.py; the expected statuses and bytes come from
the oracle's decoder, see check_against_oracle)."""
import json
from pathlib import Path

import numpy as np

import fsg
from snappy_streams import copy_tag as _copy, lit_tag as _lit, synthetic_stream as _synthetic_stream

GOLDEN = Path(__file__).resolve().parent / "golden"


def text(n: int, first_index: int | None = None) -> bytes:
    return fsg.make_batch(fsg.KIND_TEXT, [n], first_index=n if first_index is None else first_index).item(0)


def rand(n: int, first_index: int = 0) -> bytes:
    return fsg.make_batch(fsg.KIND_RANDOM, [n], first_index=first_index).item(0)


def small_bodies_forked_batch(oracle) -> list[bytes]:
    """Bodies under 512 compressed bytes for the forked path's lane walk and
    small-body execution: text of every small size, hand-built streams
    (patterns of every offset, COPY_4, 4-byte literal lengths, literals over
    64 bytes from global memory), random single literals, runs with a large
    output, mutated bodies, trailing zero-length literals and the reference's
    negative vectors; padded with three larger text bodies so the batch has
    every path of the fork.  Outputs fit 1 << 17 bytes."""
    rng = np.random.default_rng(77)
    comps = []
    for n in list(range(1, 200, 7)) + list(range(200, 800, 23)):
        comps.append(oracle.compress(text(n)))
    for i in range(400):
        c, _ = _synthetic_stream(rng, int(rng.integers(1, 760)))
        comps.append(c)
    for n in (1, 15, 16, 17, 63, 64, 65, 100, 300, 490):
        comps.append(oracle.compress(rng.integers(0, 256, n, dtype=np.uint8).tobytes()))
    for n in (700, 768, 769, 2000, 5000, 20000):  # runs: small compressed, large output
        comps.append(oracle.compress(bytes([n % 251]) * n))
    comps.append(b"\x05" + _lit(b"abcde"))                          # 1-byte literal length field
    comps.append(b"\x46" + b"\xf0\x45" + bytes(range(70)))           # literal of 70 bytes, nb = 1
    comps.append(b"\x46" + b"\xfc\x45\x00\x00\x00" + bytes(range(70)))  # nb = 4
    comps.append(b"\x0a" + _lit(b"ab") + _copy(2, 8, wide=True))
    base = list(comps)
    for _ in range(600):
        c = bytearray(base[int(rng.integers(len(base)))])
        for _ in range(int(rng.integers(1, 3))):
            c[int(rng.integers(len(c)))] = int(rng.integers(256))
        if rng.random() < 0.2:
            c = c[: int(rng.integers(1, len(c) + 1))]
        comps.append(bytes(c))
    comps += [c + b"\xfc\xff\xff\xff\xff" for c in base[:40]]
    comps += [bytes.fromhex(v["hex"]) for v in json.loads((GOLDEN / "negative.json").read_text())
              if v["header_ok"] and v["ulen"] <= 1 << 16]
    # padded with larger text bodies so the batch has every path of the fork
    comps += [oracle.compress(text(n)) for n in (3000, 9000, 70000)]
    return comps


def mutate(rng, c: bytes, mode: int) -> bytes:
    """test_large_message_index_fuzz's recipe: mode 0 intact, 1 one to three
    bytes replaced anywhere, 2 truncated, 3 a byte flipped in the last 64."""
    c = bytearray(c)
    if mode == 1:
        for _ in range(int(rng.integers(1, 4))):
            c[int(rng.integers(len(c)))] = int(rng.integers(256))
    elif mode == 2:
        c = c[: int(rng.integers(1, len(c) + 1))]
    elif mode == 3:  # corrupt late in the stream
        c[len(c) - 1 - int(rng.integers(min(64, len(c) - 1)))] ^= 0x5A
    return bytes(c)


def oracle_verdicts(oracle, comps, caps):
    """[(ok, ulen, bytes)] of oracle.uncompress per body: ok None = the slot
    is too small, False = rejected, True = accepted."""
    return [oracle.uncompress(c, cap=int(cap)) for c, cap in zip(comps, caps)]


def check_against_oracle(expect, outs, ol, st):
    """Every slot's status, and the bytes (and length) of the accepted ones,
    against oracle_verdicts' result.  Returns (accepted, rejected) counts."""
    assert len(expect) == len(outs) == len(st)
    n_ok = n_bad = 0
    wrong = []  # (index, status, what)
    for i, ((ok, ulen, ref), o, l, s) in enumerate(zip(expect, outs, ol, st)):
        if ok is None:
            if s != fsg.FSG_SLOT_TOO_SMALL:
                wrong.append((i, int(s), "slot too small for the oracle"))
        elif not ok:
            n_bad += 1
            if s not in (fsg.FSG_CORRUPT, fsg.FSG_BAD_HEADER):
                wrong.append((i, int(s), "rejected by the oracle"))
        else:
            n_ok += 1
            if s != fsg.FSG_OK:
                wrong.append((i, int(s), "accepted by the oracle"))
            elif int(l) != ulen or o[:ulen] != ref:
                wrong.append((i, int(s), f"length {int(l)} for {ulen}" if int(l) != ulen else "bytes differ"))
    assert not wrong, (len(wrong), wrong[:20])
    return n_ok, n_bad
