"""TEST INFRASTRUCTURE ONLY: the inputs behind
tests/golden/lz4f_flags_vectors.json (frames of LZ4F_compressFrame for the
eight combinations of fsg_lz4f_compress_batch_flags' flags), shared by its generator
(tests/golden/make_lz4f_flags_golden.py) and the tests.  The inputs are recipes
kept here; the fixture holds one [frame length, frame FNV] row per (input,
block size id, flags)."""
from __future__ import annotations

import json
from pathlib import Path

from lz4f_cases import build, fnv  # noqa: F401  (fnv: for the users of this module)

GOLDEN = Path(__file__).resolve().parent / "golden"
CSUM, BSUM, NOSIZE = 1, 2, 4   # FSG_LZ4F_FLAG_*
ALL_FLAGS = tuple(range(8))
IDS = (4, 5)
LENGTHS = (0, 1, 15, 16, 17, 65535, 65536, 65537, 300000)
RAW_MIDDLE = 200000            # text | 64 KiB of random bytes | text: at id 4 the middle block is stored raw

_INPUTS = None


def inputs() -> list[bytes]:
    """Text of every length in LENGTHS, then the raw-middle input."""
    global _INPUTS
    if _INPUTS is None:
        xs = [build({"gen": "text", "seed": 200 + i, "size": n}) for i, n in enumerate(LENGTHS)]
        xs.append(build({"gen": "text", "seed": 230, "size": 65536}) +
                  build({"gen": "random", "seed": 231, "size": 65536}) +
                  build({"gen": "text", "seed": 232, "size": RAW_MIDDLE - 131072}))
        assert len(xs[-1]) == RAW_MIDDLE
        _INPUTS = xs
    return _INPUTS


def keys() -> list[tuple[int, int, int]]:
    """(input index, block size id, flags) in the fixture's row order."""
    return [(i, bid, fl) for i in range(len(LENGTHS) + 1) for bid in IDS for fl in ALL_FLAGS]


def load() -> dict:
    """{(input index, block size id, flags): (frame length, frame FNV)}."""
    v = json.loads((GOLDEN / "lz4f_flags_vectors.json").read_text())
    ks = keys()
    assert len(ks) == len(v["frames"])
    return {k: (row[0], row[1]) for k, row in zip(ks, v["frames"])}


def max_frame_length_flags(n: int, bid: int, flags: int) -> int:
    """fsg_lz4f_max_frame_length_flags."""
    nb = (n + (1 << (8 + 2 * bid)) - 1) >> (8 + 2 * bid)
    return n + 4 * nb + 23 + (4 * nb if flags & BSUM else 0)
