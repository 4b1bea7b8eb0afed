"""exec_kernel<5>'s folded instance of exec5_message (whole bodies of at most
big_threshold compressed bytes, one wave each: 16-bit tag ring, 4,096-byte
window, ip0 / op0 / op1 constants; flare-cpp_amd/csrc/decode_v4_exec5.h)
against the oracle: bytes, lengths and statuses, on every route that reaches
it -- one stream, the forked path (walk order) and fsg_decompress_batch_2s."""
import functools
import json
from pathlib import Path

import numpy as np
import pytest

import fsg
from bind import Oracle
from gen_inputs import build_input
from snappy_streams import copy_tag, lit_tag, synthetic_stream
from window_edge_sized import MAX_KEEP_FOLDED, WINDOW_FOLDED, edge_stream

GOLDEN = Path(__file__).resolve().parent / "golden"
pytestmark = pytest.mark.gpu

BIG_MAX = 48 * 1024  # kBigIndexMax: big_threshold's clamp (decode_v4_plan.h)


@pytest.fixture(scope="module")
def codec():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test run without a visible GPU")
    return fsg.SnappyGPU(torch.cuda.current_device())


@pytest.fixture(scope="module")
def oracle():
    return Oracle()


def _route(fsg_opts, route):
    """one: one stream; fork: the forked path with every small body in walk
    order on exec_kernel (no packed pass), twelve waves looping over the batch;
    2s: fsg_decompress_batch_2s.  Returns whether the call is the _2s one."""
    if route == "fork":
        fsg_opts(decode_fork=1, exec_pack=0, small_persist=3)
    else:
        fsg_opts(decode_fork=0)
    return route == "2s"


def _decode(codec, comps, caps, skew=0, fill=0xA5, two_stream=False):
    """Decode into slots laid side by side: slot i starts (i * skew) % 16
    bytes past the next 16-byte boundary after slot i - 1.  The buffer is
    filled with `fill` first; every byte outside the slots must keep it.
    Returns (outputs, lengths, statuses, large_messages of the path report)."""
    import torch
    from gpu_harness import dev
    b = fsg.Batch.from_list(comps)
    n = len(b)
    caps = np.asarray(caps, dtype=np.uint32)
    oo, tot = fsg.slot_offsets(caps.astype(np.uint64) + np.uint64(16 if skew else 0))
    oo = oo + (np.arange(n, dtype=np.uint64) * np.uint64(skew)) % np.uint64(16)
    d_out = torch.full((tot + 64,), fill, dtype=torch.uint8, device="cuda")
    d_ol = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_st = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    ws = codec.decompress_workspace(n, int(b.data.size))
    args = (dev(b.data), dev(b.offsets), dev(b.lens), n, d_out, dev(oo), dev(caps), d_ol, d_st)
    if two_stream:
        s1 = torch.cuda.Stream()
        s1.wait_stream(torch.cuda.current_stream())
        codec.decompress(*args, stream=torch.cuda.current_stream(), workspace=ws, pass1_stream=s1)
    else:
        codec.decompress(*args, workspace=ws)
    torch.cuda.synchronize()
    rep = codec.decompress_report(ws, n, 0)
    out = d_out.cpu().numpy()
    ol = d_ol.cpu().numpy().view(np.uint32)
    st = d_st.cpu().numpy()
    inside = np.zeros(out.size, dtype=bool)
    for i in range(n):
        inside[int(oo[i]):int(oo[i]) + int(caps[i])] = True
    assert (out[~inside] == fill).all(), "a byte outside the slots was written"
    outs = [out[int(oo[i]):int(oo[i]) + int(min(ol[i], caps[i]))].tobytes() for i in range(n)]
    return outs, ol, st, rep["large_messages"]


def _check_against_oracle(oracle, comps, caps, outs, ol, st):
    n_ok = n_bad = 0
    for i, (c, cap, o, l, s) in enumerate(zip(comps, caps, outs, ol, st)):
        ok, ulen, ref = oracle.uncompress(c, cap=int(cap))
        if ok is None:
            assert s == fsg.FSG_SLOT_TOO_SMALL, (i, s)
        elif not ok:
            n_bad += 1
            assert s in (fsg.FSG_CORRUPT, fsg.FSG_BAD_HEADER), (i, len(c), s)
        else:
            n_ok += 1
            assert s == fsg.FSG_OK and l == ulen and o == ref, (i, len(c), s, l, ulen)
    return n_ok, n_bad


# ---------------------------------------------------------------- window edge
@functools.lru_cache(maxsize=None)
def _edge_streams(keep):
    """200 streams of 2-40 KB of output whose copies read from within 24 bytes
    of their group's base in a 4,096-byte window sliding with `keep` bytes of
    history.  Built once per kept history and shared by the routes."""
    rng = np.random.default_rng(4096 + keep)
    comps, raws, edges = [], [], 0
    for _ in range(200):
        c, raw, e = edge_stream(rng, int(rng.integers(2000, 40000)), WINDOW_FOLDED, keep)
        comps.append(c)
        raws.append(raw)
        edges += e
    return comps, raws, edges


@pytest.mark.parametrize("route", ["one", "fork"])
@pytest.mark.parametrize("keep", [512, 1024, 2048, MAX_KEEP_FOLDED])
def test_window_edge_streams_4k_window(codec, oracle, keep, route, fsg_opts):
    """Copies whose sources sit at the edge of the folded instance's window:
    far / near classification, the 16-byte loads that straddle the base, the
    slide's flush rule and the restart after a long literal, at each kept
    history the option admits there (512 .. kMaxKeepWhole = 3,024).  Slots
    side by side, 16-byte aligned and at every alignment, over a zero-filled
    and a 0xA5-filled buffer: a byte the kernel fails to write, or writes from
    a stale window, differs from the oracle's in one of the two."""
    comps, raws, edges = _edge_streams(keep)
    assert edges > 2000  # the generator does put sources across the base
    assert max(len(c) for c in comps) <= BIG_MAX  # every body takes the folded instance
    for c, raw in zip(comps[::20], raws[::20]):
        assert oracle.uncompress(c) == (True, len(raw), raw)
    _route(fsg_opts, route)
    fsg_opts(exec_keep=keep)
    caps = [len(r) for r in raws]
    for skew in (0, 5):
        for fill in (0x00, 0xA5):
            outs, ol, st, large = _decode(codec, comps, caps, skew=skew, fill=fill)
            assert large == 0
            for i, (raw, o, l, s) in enumerate(zip(raws, outs, ol, st)):
                assert s == fsg.FSG_OK and l == len(raw) and o == raw, (keep, route, skew, fill, i, s)


# ------------------------------------------------------------ 16-bit ring edge
def _fill_literals(rng, x):
    """Literal tags of 1..60 bytes taking exactly x >= 2 input bytes."""
    body, out = [], bytearray()
    while x > 0:
        k = min(60, x - 1)
        if x - (k + 1) == 1:
            k -= 1
        d = bytes(rng.integers(0, 256, k, dtype=np.uint8))
        body.append(lit_tag(d))
        out += d
        x -= k + 1
    return b"".join(body), bytes(out)


def _body_of_length(rng, n_in, tail):
    """A valid stream of exactly n_in compressed bytes, almost all of it
    incompressible literals of 1..60 bytes (a tag every <= 61 input bytes up
    to the end) with a few copies between them, ending in `tail`: "copy1" /
    "lit1" (the last tag starts at the last two bytes), "copy2" (the last
    three) or "lit60"."""
    budget = n_in - 3  # a three-byte length header: 16,384 <= output < 2^21
    body, out = [], bytearray()
    used = 0
    while budget - used > 200:
        if len(out) >= 64 and rng.random() < 0.15:
            ln = int(rng.integers(1, 65))
            off = int(rng.integers(16, min(len(out), 0xFFFF) + 1))
            t = copy_tag(off, ln)
            for _ in range(ln):
                out.append(out[-off])
        else:
            d = bytes(rng.integers(0, 256, int(rng.integers(1, 61)), dtype=np.uint8))
            t = lit_tag(d)
            out += d
        body.append(t)
        used += len(t)
    if tail == "copy1":
        last, ln, off = copy_tag(700, 9), 9, 700
    elif tail == "copy2":
        last, ln, off = copy_tag(20000, 64), 64, 20000
    elif tail == "lit1":
        last, ln, off = lit_tag(b"Z"), 0, 0
    else:
        last, ln, off = lit_tag(bytes(rng.integers(0, 256, 60, dtype=np.uint8))), 0, 0
    fb, fo = _fill_literals(rng, budget - used - len(last))
    body.append(fb)
    out += fo
    body.append(last)
    if ln:
        for _ in range(ln):
            out.append(out[-off])
    else:
        out += last[1:]
    assert 16384 <= len(out) < (1 << 21)
    v, hdr = len(out), bytearray()
    while v >= 0x80:
        hdr.append((v & 0x7F) | 0x80)
        v >>= 7
    hdr.append(v)
    comp = bytes(hdr) + b"".join(body)
    assert len(comp) == n_in
    return comp, bytes(out)


@pytest.mark.parametrize("route", ["one", "fork", "2s"])
def test_bodies_at_the_threshold_clamp(codec, oracle, route, fsg_opts):
    """A batch whose mean compressed size puts big_threshold at its 48 KiB
    clamp, of bodies of threshold - 1, threshold and threshold + 1 compressed
    bytes: the first two run on the folded instance with the largest tag
    positions a 16-bit ring entry ever holds there, the last on the general
    one (pass 1b lists it: the path report counts it as large).  Literal-heavy,
    so tags reach the last input bytes, with the last tag at the last two
    bytes, the last three, and 61 from the end."""
    rng = np.random.default_rng(48)
    comps, raws = [], []
    for rep in range(8):
        for n_in in (BIG_MAX - 1, BIG_MAX, BIG_MAX + 1):
            for tail in ("copy1", "lit1", "copy2", "lit60"):
                c, raw = _body_of_length(rng, n_in, tail)
                comps.append(c)
                raws.append(raw)
    # more than a small batch, and four times the mean is far above the clamp
    assert len(comps) > 64 and sum(map(len, comps)) == len(comps) * BIG_MAX
    for c, raw in zip(comps[::7], raws[::7]):
        assert oracle.uncompress(c) == (True, len(raw), raw)
    two = _route(fsg_opts, route)
    outs, ol, st, large = _decode(codec, comps, [len(r) for r in raws], two_stream=two)
    assert large == sum(len(c) > BIG_MAX for c in comps) == 32
    for i, (raw, o, l, s) in enumerate(zip(raws, outs, ol, st)):
        assert s == fsg.FSG_OK and l == len(raw) and o == raw, (route, i, len(comps[i]), s)


# ------------------------------------------------ golden vectors, mixed bodies
def _stream(tags_out):
    body, out = tags_out
    v, hdr = len(out), bytearray()
    while v >= 0x80:
        hdr.append((v & 0x7F) | 0x80)
        v >>= 7
    hdr.append(v)
    return bytes(hdr) + b"".join(body)


@functools.lru_cache(maxsize=None)
def _mixed_bodies():
    """256 bodies: single-literal bodies, pattern copies of every offset 1..15,
    literals of 61..70 and 4,097 bytes between copies, synthetic streams and
    text, and truncated and corrupted copies of those."""
    rng = np.random.default_rng(256)
    rnd = lambda n: bytes(rng.integers(0, 256, n, dtype=np.uint8))  # noqa: E731
    comps = []
    for n in (1, 15, 16, 17, 60, 61, 64, 65, 1000, 4096, 4097, 20000, 40000):  # single literals
        d = rnd(n)
        comps.append(_stream(([lit_tag(d)], d)))
    for off in range(1, 16):  # pattern copies: every length class after a short seed
        body, out = [], bytearray()
        d = rnd(off + 3)
        body.append(lit_tag(d))
        out += d
        for ln in (1, off, 15, 16, 17, 31, 33, 48, 63, 64):
            body.append(copy_tag(off, ln))
            for _ in range(ln):
                out.append(out[-off])
            d = rnd(int(rng.integers(1, 20)))
            body.append(lit_tag(d))
            out += d
        comps.append(_stream((body, bytes(out))))
    for n in list(range(61, 71)) + [4097]:  # literals just past the in-group sizes, between copies
        body, out = [], bytearray()
        for rep in range(6):
            d = rnd(n)
            body.append(lit_tag(d))
            out += d
            for _ in range(int(rng.integers(1, 40))):
                ln = int(rng.integers(4, 65))
                off = int(rng.integers(1, min(len(out), 5000) + 1))
                body.append(copy_tag(off, ln))
                for _ in range(ln):
                    out.append(out[-off])
        comps.append(_stream((body, bytes(out))))
    while len(comps) < 100:
        comps.append(synthetic_stream(rng, int(rng.integers(100, 30000)))[0])
    orc = Oracle()
    for j, n in enumerate(rng.integers(1, 70000, 60)):
        comps.append(orc.compress(fsg.make_batch(fsg.KIND_TEXT, [int(n)], first_index=500 + j).item(0)))
    good = len(comps)
    while len(comps) < 208:  # truncated: cut anywhere, and inside the last tag
        c = comps[int(rng.integers(good))]
        cut = int(rng.integers(1, len(c))) if rng.random() < 0.7 else len(c) - int(rng.integers(1, 4))
        comps.append(c[:max(cut, 1)])
    while len(comps) < 256:  # corrupt: 1-3 changed bytes
        c = bytearray(comps[int(rng.integers(good))])
        for _ in range(int(rng.integers(1, 4))):
            c[int(rng.integers(len(c)))] = int(rng.integers(256))
        comps.append(bytes(c))
    return comps


@pytest.mark.parametrize("route", ["one", "fork", "2s"])
def test_golden_vectors_and_mixed_bodies(codec, oracle, route, fsg_opts):
    """The golden vectors and a 256-body mix of what the folded instance
    treats specially, with truncated and corrupt streams among them: the
    oracle's bytes, lengths and verdicts on every route."""
    vecs = json.loads((GOLDEN / "vectors.json").read_text())
    comps = [oracle.compress(build_input(v)) for v in vecs] + _mixed_bodies()
    caps = []
    for c in comps:
        ok, ulen, _ = oracle.uncompress(c, cap=1 << 21)
        caps.append(ulen if ok else min(ulen, 1 << 17))
    two = _route(fsg_opts, route)
    outs, ol, st, _large = _decode(codec, comps, caps, skew=3, two_stream=two)
    n_ok, n_bad = _check_against_oracle(oracle, comps, caps, outs, ol, st)
    assert n_ok >= 100 + len(vecs) and n_bad >= 40, (n_ok, n_bad)
