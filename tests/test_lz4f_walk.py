"""The one walk over an LZ4 frame's size words (csrc/lz4_frame_format.h:
next_block, end_frame, check_blocks, blocks_decoded_length) on the CPU, under
each reader's rules: the serial decoder's, the lengths call's, those of frames
without a content size on decompress, and the sized fast route's.
tests/cpp/test_lz4f_walk.cc includes only that header; it is built as a
stand-alone program with AddressSanitizer and UBSan and run as a subprocess.

Expected values come from lz4f_nosize_cases.blocks_in (an independent model of
the structure rules) with the per-reader rules written out here, and from
lz4f_nosize_cases.decoded_length.  Every input is a seeded corpus of the other
LZ4 frame tests or built by hand below.

One class the format cannot express: a compressed block of size 0.  Its size
word would be 0, and that is the end mark; `meant_compressed_zero` is such a
frame, and every reader sees bytes after the frame."""
import shutil
import struct
import subprocess
from pathlib import Path

import pytest

import lz4f_linked_cases as K
import lz4f_nosize_cases as C
import lz4f_ref as R
from bind import Lz4Oracle
from lz4f_cases import base_frame, load, mutate

REPO = Path(__file__).resolve().parents[1]
VEC = load()
END = C.END
RULES = ("serial", "lengths", "unsized", "sized")


def word(size: int, raw: bool) -> bytes:
    return struct.pack("<I", size | (R.RAW if raw else 0))


def hand_built():
    """{name: frame}: a case for every rejection class, from R.header and
    struct.pack.  The walk verifies no checksum, so the words are arbitrary."""
    h, hb, hc = R.header(None, 4, False), R.header(None, 4, False, True, True), R.header(None, 4, True)
    raw5, sum4 = word(5, True) + b"hello", b"\x11\x22\x33\x44"
    out = {
        "no_end_mark": h + raw5,
        "half_a_size_word": h + raw5 + b"\0\0",
        "size_above_max": h + word(65537, True) + bytes(65537) + END,
        "block_cut": h + word(10, True) + b"hello",
        "block_cut_with_sums": hb + word(10, True) + b"hello",
        "block_sum_cut": hb + raw5 + sum4[:2],
        "block_sum_absent": hb + raw5,
        "content_sum_absent": hc + raw5 + END,
        "content_sum_cut": hc + raw5 + END + sum4[:3],
        "byte_after_frame": h + raw5 + END + b"\0",
        "word_after_content_sum": hc + raw5 + END + sum4 + sum4,
        "meant_compressed_zero": h + raw5 + word(0, False) + raw5 + END,
        "raw_zero": h + word(0, True) + END,  # (test_decoded_lengths_equal_the_oracle's frame)
        "raw_zero_between": hb + raw5 + sum4 + word(0, True) + sum4 + raw5 + sum4 + END,
        "accepted_with_sums": R.header(None, 5, True, True, True) + raw5 + sum4 + END + sum4,
    }
    full = word(65536, True) + bytes(65536)
    for name, size, blocks in (("sized_ok", 65546, full + word(10, True) + bytes(10)),
                               ("sized_ok_compressed_short", 65546, word(3, False) + b"\x20ab" + word(10, True) + bytes(10)),
                               ("sized_too_few", 65546, full),
                               ("sized_none", 10, b""),
                               ("sized_too_many", 10, word(10, True) + bytes(10) + word(1, True) + b"x"),
                               ("sized_raw_wrong_size", 10, word(9, True) + bytes(9)),
                               ("sized_raw_too_long", 10, word(11, True) + bytes(11)),
                               ("sized_short_nonfinal", 65546, word(65535, True) + bytes(65535) + word(4, False) + b"\x30abc"),
                               ("sized_raw_zero", 10, word(0, True) + word(10, True) + bytes(10))):
        out[name] = R.header(size, 4, False) + blocks + END
    return out


def model(f: bytes):
    """None for a bad descriptor, else (accept, columns, stated xxh, classes):
    accept by rule set, columns [(at, size, raw)] of an accepted frame, and the
    classes the frame belongs to.  blocks_in says whether the structure holds;
    where it stopped, the bytes there say why."""
    st, hl, bmax, flg, size = R.parse_header(f)
    if st != R.OK:
        return None
    ok, bmax, blocks = C.blocks_in(f)
    bsum = 4 if flg & R.F_BSUM else 0
    n, ip, cols, classes = len(f), hl, [], set()
    for b, raw in blocks:
        cols.append((ip + 4, len(b), raw))
        ip += 4 + len(b) + bsum
    if not ok:  # ip: the size word blocks_in stopped at
        left = n - ip - 4
        w = struct.unpack_from("<I", f, ip)[0] if left >= 0 else None
        if w is None:
            classes.add("no_size_word")
        elif w == 0:
            classes.add("no_content_checksum" if flg & R.F_CSUM and left < 4 else "bytes_after_frame")
        elif (w & ~R.RAW) > bmax:
            classes.add("size_above_max")
        elif left < (w & ~R.RAW):
            classes.add("block_past_input_with_sums" if bsum else "block_past_input")
        else:
            assert left < (w & ~R.RAW) + bsum
            classes.add("block_checksum_missing")
        return dict.fromkeys(RULES, False), None, None, classes
    assert all(raw for at, sz, raw in cols if sz == 0)  # a compressed block of size 0 cannot be written
    zero = any(sz == 0 for at, sz, raw in cols)
    accept = {"serial": True, "lengths": True, "unsized": not zero, "sized": False}
    if zero:
        classes.add("raw_zero")
    if size is not R.NO_SIZE:
        want = -(-size // bmax)
        if len(cols) != want:
            classes.add("sized_too_few" if len(cols) < want else "sized_too_many")
        for k, (at, sz, raw) in enumerate(cols[:want]):
            if raw and sz != min(bmax, size - k * bmax):
                classes.add("sized_short_nonfinal" if k + 1 < want else "sized_raw_wrong_size")
        accept["sized"] = not zero and not any(c.startswith("sized_") for c in classes)
    return accept, cols, struct.unpack_from("<I", f, n - 4)[0] if flg & R.F_CSUM else 0, classes


@pytest.fixture(scope="module")
def frames():
    o = Lz4Oracle()
    out = [bytes.fromhex(d["hex"]) for d in VEC["decode_ok"]]
    out += [mutate(base_frame(o, c), c) for c in VEC["decode"]]
    out += C.mutated(o)[0]
    out += [f for _, f, _ in C.routing_edges(o)] + [f for f, _, _ in C.mixed(o)]
    out += K.mutated()[0] + [f for _, f, _ in K.negatives()]
    return out + list(hand_built().values()) + [b""]


@pytest.fixture(scope="module")
def answers(frames, tmp_path_factory):
    """The program's line for each frame."""
    gxx = shutil.which("g++")
    assert gxx, "g++ not found"
    tmp = tmp_path_factory.mktemp("lz4f_walk")
    exe, fin, fout = tmp / "test_lz4f_walk", tmp / "frames.in", tmp / "walk.out"
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-I", str(REPO / "flare-cpp_amd" / "csrc"),
                        str(REPO / "tests" / "cpp" / "test_lz4f_walk.cc"), "-o", str(exe)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    with open(fin, "wb") as fh:
        for f in frames:
            fh.write(struct.pack("<I", len(f)) + f)
    r = subprocess.run([str(exe), str(fin), str(fout)], capture_output=True, text=True, timeout=300,
                       env={"ASAN_OPTIONS": "detect_leaks=0"})
    assert r.returncode == 0, r.stderr[-3000:]
    lines = fout.read_text().splitlines()
    assert len(lines) == len(frames)
    return lines


def expected_field(accept: bool, cols, xxh) -> str:
    if not accept:
        return "reject"
    return " ".join([f"accept {len(cols)} {xxh}"] + [f"{at}:{sz}:{int(raw)}" for at, sz, raw in cols])


def test_every_rule_set_equals_the_model(frames, answers):
    """Accept or reject, the block count, every block's (at, size, raw) and the
    stated checksum, for each frame under each rule set."""
    seen = {(r, a) for r in RULES for a in (False, True)}
    for i, (f, line) in enumerate(zip(frames, answers)):
        m = model(f)
        if m is None:
            assert line == "bad_header", i
            continue
        accept, cols, xxh, _ = m
        got = line.split(" | ")
        sized = R.parse_header(f)[4] is not R.NO_SIZE
        for rule, field in zip(RULES, got):
            want = "-" if rule == "sized" and not sized else expected_field(accept[rule], cols, xxh)
            assert field == want, (i, rule)
            seen.discard((rule, accept[rule]))
    assert not seen, seen


def test_decoded_length_equals_the_oracle(frames, answers):
    seen = set()
    for i, (f, line) in enumerate(zip(frames, answers)):
        if line == "bad_header" or R.parse_header(f)[4] is not R.NO_SIZE:
            assert line == "bad_header" or line.endswith(" | -"), i
            continue
        st, total = C.decoded_length(f)
        assert line.split(" | ")[4] == (f"accept {total}" if st == R.OK else "reject"), i
        seen.add(st)
    assert seen == {R.OK, R.CORRUPT}


def test_every_rejection_class_occurs(frames):
    """By the model alone.  Sized classes count only in frames that are
    otherwise sound, so that the sized rule itself decides."""
    count = {}
    for f in frames:
        m = model(f)
        if m is None:
            count["bad_header"] = count.get("bad_header", 0) + 1
            continue
        for c in m[3]:
            if not c.startswith("sized_") or len(m[3]) == 1:
                count[c] = count.get(c, 0) + 1
    print(sorted(count.items()))
    for c in ("bad_header", "no_size_word", "size_above_max", "block_past_input", "block_past_input_with_sums",
              "block_checksum_missing", "no_content_checksum", "bytes_after_frame", "raw_zero", "sized_too_few",
              "sized_too_many", "sized_raw_wrong_size", "sized_short_nonfinal"):
        assert count.get(c, 0) >= 1, c


def test_hand_built_cases_are_what_their_names_say(frames, answers):
    hb = hand_built()
    line = dict(zip(frames, answers))
    cls = {name: model(f)[3] for name, f in hb.items()}
    for name, want in (("no_end_mark", "no_size_word"), ("half_a_size_word", "no_size_word"),
                       ("size_above_max", "size_above_max"), ("block_cut", "block_past_input"),
                       ("block_cut_with_sums", "block_past_input_with_sums"), ("block_sum_cut", "block_checksum_missing"),
                       ("block_sum_absent", "block_checksum_missing"), ("content_sum_absent", "no_content_checksum"),
                       ("content_sum_cut", "no_content_checksum"), ("byte_after_frame", "bytes_after_frame"),
                       ("word_after_content_sum", "bytes_after_frame"), ("meant_compressed_zero", "bytes_after_frame"),
                       ("raw_zero", "raw_zero"), ("raw_zero_between", "raw_zero"), ("accepted_with_sums", None),
                       ("sized_ok", None), ("sized_ok_compressed_short", None), ("sized_too_few", "sized_too_few"),
                       ("sized_none", "sized_too_few"), ("sized_too_many", "sized_too_many"),
                       ("sized_raw_wrong_size", "sized_raw_wrong_size"), ("sized_raw_too_long", "sized_raw_wrong_size"),
                       ("sized_short_nonfinal", "sized_short_nonfinal"), ("sized_raw_zero", "raw_zero")):
        assert cls[name] >= ({want} if want else set()) and (want or not cls[name]), (name, cls[name])
    # a raw block of size 0: rejected on decompress, accepted by the lengths call and the serial walk
    for name in ("raw_zero", "raw_zero_between"):
        serial, lengths, unsized, sized, length = line[hb[name]].split(" | ")
        assert serial.startswith("accept") and lengths == serial and unsized == "reject" and length.startswith("accept")
    assert line[hb["raw_zero"]].split(" | ")[4] == "accept 0" and line[hb["raw_zero_between"]].endswith("accept 10")
    # what the writer meant as an empty compressed block ends the frame
    assert line[hb["meant_compressed_zero"]] == " | ".join(["reject", "reject", "reject", "-", "reject"])
    assert line[hb["sized_ok"]].split(" | ")[3] == "accept 2 0 19:65536:1 65559:10:1"
    assert line[hb["sized_ok_compressed_short"]].split(" | ")[3] == "accept 2 0 19:3:0 26:10:1"
    assert line[hb["accepted_with_sums"]].split(" | ")[0] == f"accept 1 {0x44332211} 11:5:1"
    assert line[b""] == "bad_header"
