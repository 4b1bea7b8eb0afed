"""The constructed parse family of tests/deflate_parse_cases.py on the CPU:
every case's precondition read from the host model's tokens
(host/deflate_cpu.cc), the coverage floors in one table, every body in the
three formats at both levels through Python's zlib and the host inflate, the
stream reader of tests/deflate_read.py against the writer of
tests/deflate_streams.py, and the family through the stand-alone sanitized
programs of tests/test_deflate.py and tests/test_deflate_level.py (the model
under AddressSanitizer and UBSan, the 64-thread lane emulation of the wide
functions and the 64-lane emulation of level 2's window step).  The device
side is tests/test_deflate_parse_gpu.py."""
import ctypes
import random
import shutil
import struct
import subprocess
import zlib
from pathlib import Path

import pytest

import deflate_cases as C
import deflate_level_cases as V
import deflate_parse_cases as P
import deflate_read as R
import deflate_streams as D

REPO = Path(__file__).resolve().parents[1]
FORMATS = [C.RAW, C.ZLIB, C.GZIP]


def zlib_inflate(fmt, body):
    d = zlib.decompressobj(C.WBITS[fmt])
    out = d.decompress(body)
    assert d.eof and not d.unused_data and not d.unconsumed_tail
    return out


def test_family_shape():
    fam = P.family()
    assert len(fam) < 200 and sum(len(c.data) for c in fam) < 3_000_000
    assert P.cases() == [(c.name, c.level, c.data) for c in fam]
    assert all(c.level in (P.FAST, P.BEST) and c.target in P.TARGETS for c in fam)
    assert all(c.level in P.TARGETS[c.target] for c in fam)
    assert all(len(c.data) <= C.U for c in fam if c.name != "two_units")
    # every combination the chain's carry is asked for
    want = {f"chain_{l}_{m}_{s}" for l in P.CHAIN_LANES for m in (4, 64 - l, 65 - l, 130, 258, 259) if m >= 4
            for s in P.CHAIN_SUFFIX}
    assert want == {c.name for c in fam if c.target == "chain_carry"} and len(want) == 130
    assert {c.name for c in fam if c.target == "same_slot"} == {
        "same_slot_" + t for t in ("0_1", "0_63", "15_16", "14_15", "31_32", "47_48", "62_63", "3_35_60")}
    assert [c.name for c in fam if c.target == "lazy_row_edge"] == ["lazy_lane_15", "lazy_lane_31", "lazy_lane_47",
                                                                   "lazy_lane_16"]


def test_hash_is_the_models():
    """hash4 restated: two strings of one slot are each other's candidates in the model."""
    s1, s2 = P.neighbour_strings()
    assert P.hash4(s1) ^ P.hash4(s2) == 1 and s1 != s2
    assert P.hash4(b"ABCD") == ((0x44434241 * 2654435761) & 0xffffffff) >> 19
    r = random.Random(1)
    seen = {}
    while True:  # a seeded collision: the model must look at the other string, and find 0 common bytes or 4
        s = bytes(r.choice(b"efghijklmnopqrstuvwxyz") for _ in range(4))
        t = seen.setdefault(P.hash4(s), s)
        if t != s and not set(t) & set(s):
            break
    x = V._place([(0, t + b"efgh"), (127, s + b"efgh"), (191, t + b"efgh")], 260, 5)
    assert V.token_starting_at(V.tokens(V.FAST, x), 191) == ("lit", t[0])  # the slot holds s: no match
    assert V.token_starting_at(V.tokens(V.BEST, x), 191) == ("match", 8, 191)  # two candidates: t is the older


def test_every_case_hits_its_target():
    """One test, not one a case: the family is built when the test runs, so
    collecting this file loads no library."""
    missed = [(c.name, c.target) for c in P.family() if not c.hit(c.level)]
    assert not missed, missed
    # the chain and unit-end cases are built once and go through level 2's kernel as well
    # (test_family_at_the_other_level on the device): each of them hits its target there too
    # the level-1 table cases (same slot, neighbouring slots, the repeat in one window) likewise
    both = [c for c in P.family() if c.level == P.FAST and c.target in (
        "chain_carry", "unit_end", "same_slot", "neighbour_slots", "same_window_repeat")]
    assert len(both) == 130 + 8 + 8 + 1 + 1
    missed = [c.name for c in both if not c.hit(P.BEST)]
    assert not missed, missed
    # no case's unit is a stored block, at either level: a copy would hide the parse on the device
    stored = [(c.name, lv) for c in P.family() for lv in (P.FAST, P.BEST) if not P.coded(lv, c.data)]
    assert not stored, stored


def test_coverage_floors():
    """Each target is met at least once at each level at which it applies."""
    fam = P.family()
    table = {(target, level): sum(1 for c in fam if c.target == target and c.hit(level))
             for target, levels in P.TARGETS.items() for level in levels}
    for key, n in table.items():
        print(key, n)
    assert all(n >= 1 for n in table.values()), {k: n for k, n in table.items() if not n}
    # the measured maximum: the named bodies reach it and no long-token body passes it unnoticed
    for level in (P.FAST, P.BEST):
        x = P.by_name(f"{P.LONGEST_TOKEN_BODY}_l{level}").data
        assert P.longest_token(level, x) == P.LONGEST_TOKEN_BITS == 42
        assert 40 <= P.LONGEST_TOKEN_BITS <= 48
    long_cases = [c for c in fam if c.target.startswith("long_token")]
    assert len(long_cases) == 6
    for c in long_cases:
        print(c.name, P.longest_token(c.level, c.data))
        assert P.longest_token(c.level, c.data) <= P.LONGEST_TOKEN_BITS, c.name
    # the lanes that defer at a row's edge, and the one behind it
    assert [at % 64 for at in P.LAZY_AT] == [15, 31, 47, 16]
    # the chain: start lanes and window ends crossed (zero to five), read from the model's
    # tokens of the bodies as built, at both levels
    for level in (P.FAST, P.BEST):
        lanes, crossed = set(), set()
        for c in fam:
            if c.target == "chain_carry":
                lane, m = (int(v) for v in c.name.split("_")[1:3])
                p, length = P.first_match(level, c.data)
                assert (p % 64, length) == (lane, min(m, 258)), c.name
                lanes.add(p % 64)
                crossed.add((p % 64 + length - 1) // 64)
        assert lanes == set(P.CHAIN_LANES) and crossed == {0, 1, 2, 3, 4, 5}, (level, lanes, crossed)


@pytest.mark.parametrize("level", [V.FAST, V.BEST])
@pytest.mark.parametrize("fmt", FORMATS)
def test_family_is_read_by_zlib_and_by_the_host_inflate(fmt, level):
    L = V.host()
    for name, _, x in P.cases():
        body = V.model(fmt, level, x)
        assert zlib_inflate(fmt, body) == x, name
        out = ctypes.create_string_buffer(len(x) + 1)
        ln = ctypes.c_uint64()
        assert L.fsh_cpu_inflate(fmt, body, len(body), out, len(x), ctypes.byref(ln)) == D.OK, name
        assert ln.value == len(x) and out.raw[:len(x)] == x, name
        bound = L.fsh_cpu_deflate_bound(len(x), fmt)
        assert bound == C.bound(len(x), fmt) and len(body) <= bound, name
        n = len(body)
        assert V.deflate_into(fmt, level, x, n) == (D.OK, n, body), name  # exactly the length is enough
        st, ln, buf = V.deflate_into(fmt, level, x, n - 1)  # one byte short: refused, nothing written
        assert (st, ln) == (D.SLOT_TOO_SMALL, 0) and buf == b"\xa5" * (n - 1), name
        if level == V.FAST:
            assert body == C.model(fmt, x), name


def test_two_units_are_independent():
    """The second unit's bytes are those of its input alone: its first 20 bytes
    go on from the first unit's last match, and nothing refers to it."""
    x = P.by_name("two_units").data
    for level in (V.FAST, V.BEST):
        raw = V.model(C.RAW, level, x)
        assert raw.endswith(V.model(C.RAW, level, x[C.U:])) and zlib_inflate(C.RAW, raw) == x
        assert V.unit_types(level, x) == (0, 0, 2)


# ---- the reader against the writer

def _strip(fmt, body):
    if fmt == D.ZLIB:
        return body[2:-4]
    return body


def test_reader_gives_zlibs_bytes_on_the_accept_vectors():
    """Every raw and zlib accept vector up to 6,000 bytes (the reader takes a
    bit at a time): the reader's output is zlib's and it stops where zlib does."""
    seen = types = 0
    for name, fmt, body in D.accept_vectors():
        if fmt == D.GZIP or len(body) > 6000:
            continue
        raw = _strip(fmt, body)
        blocks, out, used = R.read(raw)
        assert out == D.expected()[name], name
        assert (used + 7) // 8 == len(raw) and blocks[-1].final and not any(b.final for b in blocks[:-1]), name
        assert all(len(b.tokens) == len(b.pos) == len(b.nbits) for b in blocks)
        assert all(a.end == b.start for a, b in zip(blocks, blocks[1:])) and blocks[0].start == 0
        seen += 1
        types |= sum(1 << b.btype for b in blocks)
    assert seen >= 100 and types & 7 == 7  # stored, fixed and dynamic blocks were read
    for name, fmt, body, _ in D.reject_streams():
        if fmt == D.RAW and name in ("btype_3", "stored_len_nlen", "symbol_286", "distance_symbol_30",
                                     "distance_before_first_byte", "repeat_with_nothing_before"):
            with pytest.raises(ValueError):
                R.read(body)


def test_reader_gives_the_writers_positions():
    """Seeded token lists through deflate_streams.Deflate with `marks`: the
    reader returns the tokens, every token's first bit, its bits (the next
    mark less this one), the header's length and the end-of-block code."""
    r = random.Random(77)
    for trial in range(20):
        toks = list(D.text(50, trial))
        for _ in range(r.randrange(1, 120)):
            toks.append((r.randint(3, 258), r.randint(1, min(len(toks), 40))) if r.random() < .5 else r.randrange(256))
        used = {t for t in toks if isinstance(t, int)} | {D.length_symbol(t[0])[0] for t in toks if not isinstance(t, int)}
        dused = {D.dist_symbol(t[1])[0] for t in toks if not isinstance(t, int)} | {0, 1}
        ll = D.flat_lengths(used | {256}, 286)
        dl = D.flat_lengths(dused, 30)
        marks = []
        d = D.Deflate().stored(b"xy", final=False)
        d.dynamic(ll, dl, toks, final=False, marks=marks)
        fixed_at = d.b.bitpos
        fmarks = []
        d.header(True, 1)
        d.tokens(toks[:50], D.canonical(D.FIXED_LL), D.canonical(D.FIXED_D), True, fmarks)
        end = d.b.bitpos
        raw = d.raw()
        assert D.zlib_verdict(D.RAW, raw) is not None
        blocks, out, bits = R.read(raw)
        assert [b.btype for b in blocks] == [0, 2, 1] and bits == end
        st, dy, fx = blocks
        assert (st.start, st.header_bits, st.end) == (0, 40, 56)
        (h0, h1), = d.headers
        assert (dy.start, dy.header_bits) == (h0, h1 - h0) and dy.tokens == toks and dy.pos == marks
        assert dy.nbits == [b - a for a, b in zip(marks, marks[1:] + [dy.eob[0]])]
        assert dy.end == fixed_at == dy.eob[0] + dy.eob[1]
        assert (fx.start, fx.header_bits) == (fixed_at, 3) and fx.tokens == toks[:50] and fx.pos == fmarks
        assert fx.eob == (end - 7, 7) and fx.end == end


def test_reader_on_the_models_streams():
    """The model's own raw streams: the tokens the reader finds are the model's
    tokens, block by unit."""
    for name in ("same_slot_0_63", "chain_63_259_4", "tokens_129_l2", "long_token_bits_l1", "one_match_61"):
        c = P.by_name(name)
        blocks, out, _ = R.read(V.model(C.RAW, c.level, c.data))
        assert out == c.data and len(blocks) == 1, name
        want = [t[1] if t[0] == "lit" else (t[1], t[2]) for t in V.tokens(c.level, c.data)]
        assert blocks[0].tokens == want, name
        assert max(blocks[0].nbits) <= 48


# ---- the family through the sanitized stand-alone programs

WIDE = {"long_token_bits_l1", "long_token_three_words_l2", "tokens_64_l1", "tokens_65_l1", "tokens_128_l1",
        "tokens_129_l1", "chain_63_258_0", "chain_0_259_3", "same_slot_3_35_60", "one_match_64", "two_units"}


def _build(tmp_path, source, extra=()):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = tmp_path / source.replace(".cc", "")
    host = REPO / "flare-cpp_amd" / "host"
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        *extra, "-I", str(host), str(REPO / "tests" / "cpp" / source), str(host / "deflate_cpu.cc"),
                        str(host / "inflate_cpu.cc"), "-o", str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return exe


def test_family_through_the_sanitized_model_and_wide_lanes(tmp_path):
    """tests/cpp/deflate_check.cc, as tests/test_deflate.py runs it on its own
    family: the cases go through a file."""
    exe = _build(tmp_path, "deflate_check.cc", ["-pthread"])
    assert WIDE <= {c.name for c in P.family()}
    rec = units = 0
    with open(tmp_path / "vectors.bin", "wb") as f:
        for name, _, x in P.cases():
            for fmt in FORMATS:
                body = C.model(fmt, x)
                flags = 2 if name in WIDE and fmt == C.RAW else 0
                f.write(struct.pack("<4I", fmt, len(x), len(body), flags) + x + body)
                rec += 1
                units += max(1, -(-len(x) // C.U)) if flags & 2 else 0
    r = subprocess.run([str(exe), str(tmp_path / "vectors.bin")], capture_output=True, text=True, timeout=900,
                       env={"ASAN_OPTIONS": "detect_leaks=0"})
    assert r.returncode == 0 and r.stdout.strip() == f"ok {rec} {units}", r.stdout[-2000:] + r.stderr[-3000:]


def test_family_through_the_sanitized_level_2_lanes(tmp_path):
    """tests/cpp/deflate_level_check.cc: the model at levels 0 and 2 and the
    64-lane window step (both candidates, the lazy step from the neighbour's
    record, the chain, one insert a lane) for every unit of every case."""
    exe = _build(tmp_path, "deflate_level_check.cc")
    rec = windows = 0
    with open(tmp_path / "vectors.bin", "wb") as f:
        for name, _, x in P.cases():
            for fmt in FORMATS:
                for level in (V.STORED, V.BEST):
                    body = V.model(fmt, level, x)
                    lanes = fmt == C.RAW and level == V.BEST
                    f.write(struct.pack("<5I", fmt, level, len(x), len(body), 2 if lanes else 0) + x + body)
                    rec += 1
                    if lanes:
                        units = max(1, -(-len(x) // C.U))
                        windows += sum(-(-min(C.U, len(x) - u * C.U) // 64) for u in range(units))
    r = subprocess.run([str(exe), str(tmp_path / "vectors.bin")], capture_output=True, text=True, timeout=900,
                       env={"ASAN_OPTIONS": "detect_leaks=0"})
    assert r.returncode == 0 and r.stdout.strip() == f"ok {rec} {windows}", r.stdout[-2000:] + r.stderr[-3000:]
