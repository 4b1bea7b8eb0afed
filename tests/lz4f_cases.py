"""TEST INFRASTRUCTURE ONLY: the inputs and mutations behind
tests/golden/lz4f_vectors.json, shared by its generator
(tests/golden/make_lz4f_golden.py) and the tests.  The inputs are recipes kept
here, so the fixture holds lengths, digests, verdicts and the mutations only,
as short rows; `load` gives them back as dicts."""
from __future__ import annotations

import json
import struct
from pathlib import Path

import numpy as np

import fsg
from gen_inputs import build_input

GOLDEN = Path(__file__).resolve().parent / "golden"
BOUNDARY = (0, 1, 12, 13, 65535, 65536, 65537, 131072, 131073, 200000)
# sources of the mutated frames: text of 40 B .. 140 KB, and one that is random first and text after
DECODE_SOURCES = [{"gen": "text", "seed": 30 + i, "size": s} for i, s in
                  enumerate((40, 300, 3000, 20000, 70000, 140000))]
DECODE_SOURCES.append({"gen": "random_then_text", "seed": 40, "random": 30000, "size": 100000})
_GOLDEN = None


def golden_specs() -> list[dict]:
    global _GOLDEN
    if _GOLDEN is None:
        _GOLDEN = json.loads((GOLDEN / "vectors.json").read_text())
    return _GOLDEN


def build(spec: dict) -> bytes:
    """gen_inputs.build_input's recipes and three more: "ref" (a golden vector
    by index), "near_raw" (random bytes with 0-3 short repeats: blocks that
    land near the raw-store boundary) and "random_then_text"."""
    g = spec["gen"]
    if g == "ref":
        return build_input(golden_specs()[spec["ref"]])
    if g == "near_raw":
        rng = np.random.default_rng(spec["seed"])
        x = rng.integers(0, 256, spec["size"], dtype=np.uint8)
        for _ in range(spec["repeats"]):
            ln = int(rng.integers(4, 24))
            if spec["size"] < 2 * ln + 2:
                break
            src = int(rng.integers(0, spec["size"] - 2 * ln))
            dst = int(rng.integers(src + ln, min(spec["size"] - ln, src + 60000) + 1))
            x[dst:dst + ln] = x[src:src + ln]
        return x.tobytes()
    if g == "random_then_text":
        a = fsg.make_batch(fsg.KIND_RANDOM, [spec["random"]], first_index=spec["seed"]).item(0)
        return a + fsg.make_batch(fsg.KIND_TEXT, [spec["size"] - spec["random"]], first_index=spec["seed"]).item(0)
    return build_input(spec)


def compress_inputs() -> list[tuple[dict, int]]:
    """(recipe, block size id) behind the `compress` rows, two rows each
    (without and with a content checksum): the golden inputs up to 1 MiB and
    the boundary lengths at id 4, 300,000 B of text and 4 MiB + 17 random
    bytes at ids 4..7, 200 near-raw-boundary inputs (every 20th above 64 KiB,
    at id 5)."""
    out = [({"gen": "ref", "ref": i}, 4) for i in range(len(golden_specs()))]
    out += [({"gen": "text", "seed": 100 + n % 97, "size": n}, 4) for n in BOUNDARY]
    for bid in (4, 5, 6, 7):
        out.append(({"gen": "text", "seed": 5, "size": 300000}, bid))
        out.append(({"gen": "random", "seed": 6, "size": (4 << 20) + 17}, bid))
    for i in range(200):
        big = i % 20 == 19
        size = 65537 + (i * 3739) % 74000 if big else 13 + (i * 7919) % (190 if i % 2 else 4900)
        out.append(({"gen": "near_raw", "seed": 1000 + i, "size": size, "repeats": i % 4}, 5 if big else 4))
    return out


def fnv(b: bytes) -> str:
    return "%016x" % fsg.fnv1a64(b)


def load() -> dict:
    """The fixture with its rows as dicts: compress {input, bid, checksum,
    frame_len, frame_fnv, blocks, raw_blocks[, differs_from_size_rule]};
    decode_ok as stored; decode {src, csum, bsum, set, cut, liblz4_ok, oracle,
    out_len, out_fnv[, liblz4_only]}."""
    v = json.loads((GOLDEN / "lz4f_vectors.json").read_text())
    keys = [(spec, bid, cs) for spec, bid in compress_inputs() for cs in (0, 1)]
    assert len(keys) == len(v["compress"])
    comp = []
    for i, ((spec, bid, cs), (flen, ffnv, blocks, raws)) in enumerate(zip(keys, v["compress"])):
        e = {"input": spec, "bid": bid, "checksum": cs, "frame_len": flen, "frame_fnv": ffnv, "blocks": blocks,
             "raw_blocks": raws}
        if i in v["differs_from_size_rule"]:
            e["differs_from_size_rule"] = True
        comp.append(e)
    dec = []
    for i, (src, flags, sets, cut, ok, st, ln, digest) in enumerate(v["decode"]):
        c = {"src": src, "csum": flags & 1, "bsum": flags >> 1, "set": [sets[k:k + 2] for k in range(0, len(sets), 2)],
             "cut": None if cut < 0 else cut, "liblz4_ok": bool(ok), "oracle": st, "out_len": ln,
             "out_fnv": digest or None}
        if i in v["liblz4_only"]:
            c["liblz4_only"] = True
        dec.append(c)
    return {"liblz4_version": v["liblz4_version"], "compress": comp, "decode_ok": v["decode_ok"], "decode": dec,
            "decode_sources": DECODE_SOURCES}


def mutate(frame: bytes, case: dict) -> bytes:
    """A `decode` entry's frame from its base frame: byte changes, then a cut."""
    b = bytearray(frame)
    for pos, val in case["set"]:
        b[pos] = val
    if case["cut"] is not None:
        b = b[:case["cut"]]
    return bytes(b)


_BASE = {}


def base_frame(o, case: dict) -> bytes:
    """The unmutated frame of a `decode` entry: its source with the entry's
    checksum flags, written by the frame oracle (the generator checks that it
    equals liblz4's)."""
    import lz4f_ref
    key = (case["src"], case["csum"], case["bsum"])
    if key not in _BASE:
        x = build(DECODE_SOURCES[case["src"]])
        _BASE[key] = lz4f_ref.compress_frame(o, x, 4, bool(case["csum"]), bool(case["bsum"]))
    return _BASE[key]


_XXH = {}


def oracle_frame(o, e: dict, x: bytes) -> bytes:
    """The frame oracle's frame of a `compress` entry; the content checksum of
    an input (pure Python) is computed once, whatever the block size."""
    import lz4f_ref as R
    f = R.compress_frame(o, x, e["bid"], False)
    if e["checksum"]:
        key = json.dumps(e["input"], sort_keys=True)
        if key not in _XXH:
            _XXH[key] = R.xxh32(x)
        f = bytearray(f)
        f[4] |= R.F_CSUM
        hl = 15 if x else 7
        f[hl - 1] = (R.xxh32(bytes(f[4:hl - 1])) >> 8) & 0xFF
        f = bytes(f) + struct.pack("<I", _XXH[key])
    return f
