"""The lane walk's advance (csrc/decode_v4_index.h): the step from one tag to
the next is computed in registers from the tag byte (tag_advance), gated by
the iteration's limit (`look`), and the output length is summed apart from the
position.  Every tag byte, at every byte alignment of the ring read, whole and
cut short; every tag type around the limits of an iteration; every tag slot
of the unrolled loop.  Exact: status, out_len and bytes against the oracle.

Every batch has more than 64 bodies, each under kBigIndexMin, and runs on the
four instances of index_kernel (serial, standard, planned, lean: the table in
test_gpu_lane_walk.py, whose launch helpers are used here), with poisoned
side-by-side slots and a 0xFF workspace.

Bodies lie back to back in the input, so a body starts at the sum of the
lengths before it: `ibal`, the start's low four bits, is set through the
lengths (the trailing literal of a body is sized for it), and the alignment of
a tag's ring read, (ip + ibal) & 3, through one- and two-byte literals in front
of the tag.

Where an iteration's limit falls is not computed here.  A limit depends only
on the tags before the iteration it belongs to, so behind an unchanged run of
filler tags a tag that moves one input byte at a time stands at every distance
before each limit it passes: the ring limit (the tags' five bytes must be in
the ring: behind 61-byte fillers every few tags), the kMaxDist clamp (which
binds only where the input's end is in a full ring) and the end of input (a
trailing filler of every length up to 70 bytes).
"""
import numpy as np
import pytest

import fsg
from oracle_codec import OracleCodec
from snappy_batches import check_against_oracle, oracle_verdicts
from test_gpu_lane_walk import BIG_INDEX_MIN, Body, check_walked, decode_two_stream, plan_est_total_in, varint

pytestmark = pytest.mark.gpu

MODES = ["serial", "standard", "planned", "lean"]
PREFIX = 64  # bytes of the literal every body starts with
# one- and two-byte literals in front of the tag (n + 1 input bytes each): every shift modulo 4, twice, so
# that one of them fits where the header's length changes with the output length
PADS = [(), (2,), (1,), (1, 2), (1, 1), (1, 1, 2), (1, 1, 1), (1, 1, 1, 2)]


def tag_size(c: int, long_len: int = 61) -> tuple[int, int]:
    """(input bytes, output bytes) of tag c as put_tag writes it."""
    t, n = c & 3, (c >> 2) + 1
    if t == 0:
        return (1 + n, n) if n <= 60 else (1 + (n - 60) + long_len, long_len)
    if t == 1:
        return 2, 4 + ((c >> 2) & 7)
    return (3 if t == 2 else 5), n


def history_copies(c: int) -> int:
    """Copies of 64 bytes after the prefix, so that a COPY_1 whose tag byte
    carries offset bits (offset >= 256 * (c >> 5)) has that much history."""
    need = ((c >> 5) << 8) + 5 if c & 3 == 1 else 0
    return max(0, -(-(need - PREFIX) // 64))


def put_tag(b: Body, c: int, long_len: int = 61):
    """Tag byte c with valid extra bytes: a literal's bytes (a long literal
    has the length field of the nb bytes c states), a copy's offset."""
    t, n = c & 3, (c >> 2) + 1
    if t == 0:
        ln = n if n <= 60 else long_len
        data = b.rng.integers(0, 256, ln, dtype=np.uint8).tobytes()
        b.tags += bytes([c]) + ((ln - 1).to_bytes(n - 60, "little") if n > 60 else b"") + data
        b.out += data
        return b
    if t == 1:
        ln, off = 4 + ((c >> 2) & 7), ((c >> 5) << 8) + 5
        b.tags += bytes([c, 5])
    elif t == 2:
        ln, off = n, 9
        b.tags += bytes([c, 9, 0])
    else:
        ln, off = n, 11
        b.tags += bytes([c]) + (11).to_bytes(4, "little")
    assert off <= len(b.out)
    for _ in range(ln):
        b.out.append(b.out[-off])
    return b


def front(seed: int, c: int, pad: tuple) -> Body:
    b = Body(seed).lit(PREFIX)
    for _ in range(history_copies(c)):
        b.copy(1, 64)
    for n in pad:
        b.lit(n)
    return b


def aligned_body(seed: int, c: int, residue: int, start: int, length_mod16: int):
    """prefix, history, pad literals, tag c, then a two-byte copy and a
    literal: the tag's ring read has (ip + ibal) & 3 == residue when the body
    starts at `start`, and the body's length is length_mod16 modulo 16."""
    ibal = start & 15
    size_c, out_c = tag_size(c)
    k = history_copies(c)
    for pad in PADS:
        pin, pout = sum(pad) + len(pad), sum(pad)
        for m in range(1, 17):
            ulen = PREFIX + 64 * k + pout + out_c + 4 + m
            ip = len(varint(ulen)) + 2 + PREFIX + 3 * k + pin
            if (ip + ibal) & 3 == residue and (ip + size_c + 2 + 1 + m) % 16 == length_mod16:
                b = put_tag(front(seed, c, pad), c)
                assert len(varint(ulen)) + len(b.tags) - size_c == ip
                body = b.copy(1, 4).lit(m).body()
                assert len(body) % 16 == length_mod16 and len(b.out) == ulen
                return body
    raise AssertionError((c, residue, start, length_mod16))


def every_tag_cases():
    """Set 1: every body a multiple of 16 long (ibal 0).  Set 2: every body
    1 modulo 16 long, so ibal runs through all 16 values."""
    comps, start = [], 0
    for length_mod16 in (0, 1):
        seen = set()
        for c in range(256):
            for r in range(4):
                seen.add(start & 15)
                comps.append(aligned_body(len(comps), c, r, start, length_mod16))
                start += len(comps[-1])
        assert seen == ({0} if length_mod16 == 0 else set(range(16)))
    return comps


def truncated_cases():
    """Tag c last, its extra or literal bytes cut short by 1 up to all of them."""
    comps = []
    for c in range(256):
        for pad in PADS[:4]:
            whole = put_tag(front(5000 + len(comps), c, pad), c).body()
            for cut in range(1, tag_size(c)[0]):
                comps.append(whole[:-cut])
    return comps


def limit_cases():
    """A 60-byte literal, a COPY_1, a COPY_2 and a COPY_4 behind p bytes of
    two-byte and of 61-byte filler tags, for every p of a range longer than
    the ring plus 70, then q bytes of filler up to the end of input, every q
    up to 70 coming up with every tag."""
    kinds = {"lit60": lambda b: b.lit(60), "copy1": lambda b: b.copy(3, 9), "copy2": lambda b: b.copy(2, 37),
             "copy4": lambda b: b.copy(5, 50, wide=True)}
    comps = []
    for dense, top in ((True, 340), (False, 420)):
        for p in [0] + list(range(2, top)):
            for i, put in enumerate(kinds.values()):
                b = Body(9000 + len(comps)).lit(8).fill(p, dense)
                put(b)
                q = (p * 4 + i) % 71
                comps.append(b.fill(0 if q == 1 else q, dense if q % 2 else not dense).body())
    return comps


def slot_cases():
    """k two-byte or five-byte tags, k up to 70 (more than two iterations of
    32 tags), then a long literal (which ends the lane's unrolled part in the
    slot after them) or a short one, so each slot of the 32-, 24- and 16-tag
    loops is the last one used and the first one not."""
    comps = []
    for wide in (False, True):
        for k in range(71):
            for n in (3, 61):
                b = Body(20000 + len(comps)).lit(8)
                for _ in range(k):
                    b.copy(1 + k % 5, 4, wide=wide)
                comps.append(b.lit(n).tail().body())
    return comps


GROUPS = {"every_tag": every_tag_cases, "truncated": truncated_cases, "limit": limit_cases, "slot": slot_cases}


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test run without a visible GPU")
    from gpu_harness import GpuCodec
    return GpuCodec()


@pytest.fixture(scope="module")
def batches():
    """group -> (comps, caps, verdicts), computed once for the four modes."""
    oracle = OracleCodec().o
    out = {}
    for name, make in GROUPS.items():
        comps = make()
        assert len(comps) > 64 and max(map(len, comps)) < BIG_INDEX_MIN
        caps = []
        for c in comps:
            h, ulen = oracle.header(c)
            assert h and ulen <= 1 << 17
            caps.append(ulen)
        expect = oracle_verdicts(oracle, comps, caps)
        # the cases are what they claim to be
        if name == "truncated":
            assert all(e[0] is False for e in expect)
        else:
            assert all(e[0] is True for e in expect), [i for i, e in enumerate(expect) if e[0] is not True][:10]
        out[name] = comps, caps, expect
    return out


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("group", list(GROUPS))
def test_walk_advance(gpu, batches, fsg_opts, group, mode):
    comps, caps, expect = batches[group]
    n = len(comps)
    if mode == "lean":
        assert fsg.get_option("lean_walk") == 1
        outs, ol, st, rep = decode_two_stream(gpu, comps, caps)
    else:
        fsg_opts(decode_fork=1 if mode == "planned" else 0)
        total_in = 20 * 1024 * n if mode == "standard" else sum(len(c) for c in comps)
        if mode != "planned":  # which one-stream walk the plan picks (est_total_in < 16384 n: serial)
            est = plan_est_total_in(n, gpu.codec.lib.fsg_decompress_workspace_bytes(n, total_in))
            assert (est < 16384 * n) == (mode == "serial"), (est, n)
        outs, ol, st = gpu.decompress(comps, caps, ws_fill=0xFF, ws_total_in=total_in)
        rep = gpu.last_report
    check_walked(rep, comps)
    n_ok, n_bad = check_against_oracle(expect, outs, ol, st)
    assert (n_ok, n_bad) == ((0, n) if group == "truncated" else (n, 0))
