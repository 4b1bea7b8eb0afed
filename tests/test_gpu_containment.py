"""Write containment of every batch call (the contract "What a *_batch call
writes" in include/flare_snappy_gpu.h), byte-exact, through every routing:

* no byte of d_out / d_stage outside the slots [off_i, off_i + cap_i) is
  written, whatever the message's status: slots at every alignment with 64
  poison bytes between them ("guarded"), and slots adjacent at byte
  granularity ("tight"), where a spill lands in the neighbour's bytes;
* with cap_i equal to the body's length that is "not one byte past the
  message, not one before it": the valid family's whole buffer must equal the
  image built from the oracle, no byte masked;
* validate-only calls write nothing; result columns get exactly n_msgs
  entries; nothing is written past workspace_bytes; the inputs stay as they
  were.

tests/containment.py is the checker (its own tests: tests/test_containment.py).
The inputs are the smallest at which each path engages: the thresholds are
those of tests/test_gpu_parity.py.

Also here, three calls nothing else runs directly: the device header pass
(fsg_uncompressed_lengths_batch), fsg_gather_blocks at every pair of source
and destination alignments, and the wave encoder with several waves per
workgroup (encode_wave_wg)."""
import ctypes
from dataclasses import dataclass, field

import numpy as np
import pytest

import containment as ct
import fsg
import gpu_harness as gh
from bind import Lz4Oracle, Oracle
from containment import POISON
from snappy_streams import synthetic_stream

pytestmark = pytest.mark.gpu

OK, CORRUPT, BAD_HEADER, TOO_SMALL = fsg.FSG_OK, fsg.FSG_CORRUPT, fsg.FSG_BAD_HEADER, fsg.FSG_SLOT_TOO_SMALL
LAYOUT_NAMES = ["guarded", "tight"]
HUGE = 1 << 20


@pytest.fixture(scope="module")
def codec():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test run without a visible GPU")
    return fsg.SnappyGPU(torch.cuda.current_device())


@pytest.fixture(scope="module")
def oracle():
    return Oracle()


@pytest.fixture(scope="module")
def lz4o():
    return Lz4Oracle()


def _text(n: int) -> bytes:
    return fsg.make_batch(fsg.KIND_TEXT, [n], first_index=n).item(0) if n else b""


# ---------------------------------------------------------------------------
# The decode ladder: (stream, plain bytes) pairs

@pytest.fixture(scope="module")
def plain():
    """The plain inputs behind the ladder (LZ4 compresses the same ones)."""
    rng = np.random.default_rng(12)
    sizes = [0, 1, 15, 16, 17, 31, 33, 64, 65]
    sizes += [48 + r for r in range(16)] + [4100 + r for r in range(16)]  # output ends at every residue
    sizes += [300, 620, 700]                 # compressed 245, 485 (the packed pass: under 512) and 583
    sizes += [3000, 9000]                    # a wave per body
    sizes += [65535, 65536, 65537, 70000]    # 64 KiB segments
    sizes += [120000]                        # compressed over 48 KiB: the wave index pass
    sizes += [HUGE]                          # huge; chunked when chunked_huge=1
    xs = [_text(n) for n in sizes]
    xs += [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in (70, 5000)]  # single literals
    xs += [bytes([n % 251]) * n for n in (700, 769, 20000)]  # runs: small compressed, large output
    return xs


@pytest.fixture(scope="module")
def ladder(plain, oracle):
    rng = np.random.default_rng(2024)
    pairs = [(oracle.compress(x), x) for x in plain]
    clen = {len(x): len(c) for c, x in pairs[:plain.index(_text(HUGE)) + 1]}  # of the text bodies
    assert clen[300] < 512 and 450 < clen[620] < 512 < clen[700]  # either side of the packed pass's limit
    assert 48 * 1024 < clen[120000] and 256 * 1024 < clen[HUGE]   # the wave index pass; huge
    for i in range(100):  # offsets 1..15, COPY_4, long literals, ends at every alignment
        target = int(rng.integers(1, 3000)) if i % 10 else int(rng.integers(20000, 70000))
        pairs.append(synthetic_stream(rng, target))
    return pairs


@dataclass
class Family:
    """Messages, slot capacities and the reference's verdict on each."""
    comps: list
    caps: list
    status: list = field(default_factory=list)  # the oracle's, as FSG_* words
    ulen: list = field(default_factory=list)    # header length (0: bad header)
    body: list = field(default_factory=list)    # the oracle's bytes where status is OK
    _images: dict = field(default_factory=dict)

    def __len__(self):
        return len(self.comps)

    def subset(self, idx):
        pick = lambda a: [a[i] for i in idx]  # noqa: E731
        return Family(pick(self.comps), pick(self.caps), pick(self.status), pick(self.ulen), pick(self.body))

    def image(self, layout_name):
        """(layout, image, mask), built once per layout and left unchanged."""
        if layout_name not in self._images:
            lay = ct.LAYOUTS[layout_name](self.caps)
            img, mask = ct.expected_image(lay, self.caps, self.ulen, self.body, self.status)
            img.setflags(write=False)
            mask.setflags(write=False)
            self._images[layout_name] = (lay, img, mask)
        return self._images[layout_name]


def _snappy_verdicts(fam: Family, oracle):
    for c, cap in zip(fam.comps, fam.caps):
        h, _ = oracle.header(c)
        ok, ulen, ref = oracle.uncompress(c, cap=cap)
        fam.status.append(BAD_HEADER if not h else TOO_SMALL if ok is None else OK if ok else CORRUPT)
        fam.ulen.append(ulen if h else 0)
        fam.body.append(ref)
    return fam


_LZ4_CODE = {1: OK, 0: CORRUPT, -1: BAD_HEADER, -2: TOO_SMALL}


def _lz4_verdicts(fam: Family, lz4o):
    for c, cap in zip(fam.comps, fam.caps):
        r, ulen, ref = lz4o.uncompress(c, cap=cap)
        fam.status.append(_LZ4_CODE[r])
        fam.ulen.append(ulen)
        fam.body.append(ref)
    return fam


def _valid(pairs, verdicts, o):
    """Every body with cap == ulen: all OK by the oracle, no byte masked."""
    fam = verdicts(Family([c for c, _ in pairs], [len(x) for _, x in pairs]), o)
    assert all(s == OK for s in fam.status)
    assert all(b == x for b, (_, x) in zip(fam.body, pairs))
    return fam


def _hostile(pairs, verdicts, o, count=600, seed=5):
    """Round-robin over the ladder, a third each: intact; 1-3 random byte
    flips (30 % of those also truncated) in a slot of the original length;
    intact in a slot of capacity drawn from [0, ulen)."""
    rng = np.random.default_rng(seed)
    comps, caps = [], []
    for k in range(count):
        c, x = pairs[k % len(pairs)]
        kind = (k + k // len(pairs)) % 3  # every ladder entry meets every kind
        cap = len(x)
        if kind == 1:
            c = bytearray(c)
            for _ in range(int(rng.integers(1, 4))):
                c[int(rng.integers(len(c)))] = int(rng.integers(256))
            if rng.random() < 0.3:
                c = c[:int(rng.integers(1, len(c) + 1))]
            c = bytes(c)
        elif kind == 2:
            cap = int(rng.integers(0, len(x))) if x and rng.random() < 0.9 else 0  # capacity 0 now and then
        comps.append(c)
        caps.append(cap)
    fam = verdicts(Family(comps, caps), o)
    # the mix the family is meant to have, by the oracle alone
    n_ok = sum(s == OK for s in fam.status)
    n_bad = sum(s in (CORRUPT, BAD_HEADER) for s in fam.status)
    n_small = sum(s == TOO_SMALL for s in fam.status)
    assert n_ok >= 0.3 * count and n_bad >= 0.1 * count and n_small >= 0.1 * count, (n_ok, n_bad, n_small)
    assert any(cap == 0 and s == TOO_SMALL for cap, s in zip(fam.caps, fam.status))
    return fam


@pytest.fixture(scope="module")
def families(ladder, oracle):
    """valid / hostile over the whole ladder, and without the huge body for
    the routings that do nothing special with it."""
    small = [p for p in ladder if len(p[1]) < HUGE]
    return {"valid": _valid(ladder, _snappy_verdicts, oracle), "hostile": _hostile(ladder, _snappy_verdicts, oracle),
            "valid-small": _valid(small, _snappy_verdicts, oracle),
            "hostile-small": _hostile(small, _snappy_verdicts, oracle)}


# ---------------------------------------------------------------------------
# One guarded decode call

class Call:
    """Device buffers of one decode-shaped call under the guards: a poisoned
    output buffer in the given layout, guarded columns and workspace, inputs
    that are compared after the call."""

    def __init__(self, fam: Family, layout: ct.Layout, columns, ws_bytes, ws_fill=None, extra_inputs=None):
        import torch
        self.torch = torch
        self.n = len(fam)
        self.layout, self.caps = layout, np.array(fam.caps, dtype=np.uint32)
        b = fsg.Batch.from_list(fam.comps)
        self.total_in = int(b.data.size)
        self.ins = gh.Inputs(d_in=b.data, d_in_off=b.offsets, d_in_len=b.lens, d_out_off=layout.offs,
                             d_out_cap=self.caps, **(extra_inputs or {}))
        self.d_out = gh.poisoned(layout.total)
        self.cols = {name: gh.guarded_column(self.n, getattr(torch, dt), fill) for name, (dt, fill) in columns.items()}
        self.ws, self.whole = gh.guarded_workspace(ws_bytes(self.n, self.total_in) if ws_bytes else None, zero=True)
        if self.ws is not None and ws_fill is not None:
            self.ws.fill_(ws_fill)
        torch.cuda.synchronize()

    def args(self):
        i = self.ins
        return i["d_in"], i["d_in_off"], i["d_in_len"], self.n

    def finish(self, what="d_out"):
        """Synchronise; check the guards no routing may touch (outside the
        slots, column tails, past the workspace, inputs); return the host
        copy of the output buffer."""
        self.torch.cuda.synchronize()
        out = self.d_out.cpu().numpy()
        gh.check_call(out, self.layout, self.caps, self.cols, self.n, self.whole, self.ins, what)
        return out

    def col(self, name):
        return self.cols[name].cpu().numpy()[:self.n]


_DECODE_COLS = {"d_out_len": ("int32", None), "d_status": ("int32", -7)}


def _check_decode(call: Call, fam: Family, layout_name):
    """Statuses equal the oracle's, OK bodies equal its bytes, and every byte
    the contract pins -- all of them outside the slots -- is as expected."""
    out = call.finish()
    lay, img, mask = fam.image(layout_name)
    st = call.col("d_status")
    assert list(st) == fam.status, [(i, int(s), w) for i, (s, w) in enumerate(zip(st, fam.status)) if s != w][:8]
    ol = call.col("d_out_len").view(np.uint32)
    for i, s in enumerate(fam.status):
        if s in (OK, TOO_SMALL):
            assert ol[i] == fam.ulen[i], i
    ct.check(out, img, mask, lay, fam.caps)


# routing id -> (library options, decode variant, workspace: "full" | None | "third", huge body in the batch)
_ROUTINGS = {
    "default": ({}, 0, "full", True),
    "variant1": ({}, 1, "full", False),
    "variant3": ({}, 3, "full", False),
    "variant4": ({}, 4, "full", True),
    "variant5": ({}, 5, "full", True),
    "no_workspace": ({}, 0, None, False),
    "third_workspace": ({}, 0, "third", True),
    "fork_pack0": (dict(decode_fork=1, exec_pack=0, small_persist=5), 0, "full", False),
    "fork_pack7": (dict(decode_fork=1, exec_pack=7, small_persist=5), 0, "full", False),
    "fork_pack32": (dict(decode_fork=1, exec_pack=32, small_persist=5), 0, "full", False),
    "fork_chunked_huge": (dict(decode_fork=1, chunked_huge=1), 0, "full", True),
    "fork_whole_huge": (dict(decode_fork=1, chunked_huge=0), 0, "full", True),
    "two_streams": ({}, 0, "full", True),
}


def _ws_bytes(codec, kind):
    if kind is None:
        return None
    lib = codec.lib
    if kind == "third":  # the bitmap of most messages does not fit: pass 3 finishes them
        return lambda n, total_in: lib.fsg_decompress_workspace_bytes(n, max(total_in // 3, 1))
    return lambda n, total_in: lib.fsg_decompress_workspace_bytes(n, total_in)


@pytest.mark.parametrize("layout_name", LAYOUT_NAMES)
@pytest.mark.parametrize("family", ["valid", "hostile"])
@pytest.mark.parametrize("routing", list(_ROUTINGS))
def test_decode_containment(codec, families, routing, family, layout_name, fsg_opts):
    import torch
    opts, variant, ws_kind, huge = _ROUTINGS[routing]
    fam = families[family if huge else family + "-small"]
    lay, _, _ = fam.image(layout_name)
    fsg_opts(**opts)
    call = Call(fam, lay, _DECODE_COLS, _ws_bytes(codec, ws_kind), ws_fill=0xFF if ws_kind == "third" else None)
    i = call.ins
    codec.select_kernels(variant, 0)
    try:
        codec.decompress(*call.args(), call.d_out, i["d_out_off"], i["d_out_cap"], call.cols["d_out_len"],
                         call.cols["d_status"], workspace=call.ws,
                         pass1_stream=torch.cuda.Stream() if routing == "two_streams" else None)
        torch.cuda.synchronize()
        rep = codec.decompress_report(call.ws, call.n)  # (under the call's own options and variant)
    finally:
        codec.select_kernels(0, 0)
    # the routing the case is named after did run
    want_path = fsg.PATH_FORCED if variant in (1, 3) else fsg.PATH_NO_WORKSPACE if ws_kind is None else fsg.PATH_MAIN
    assert rep["path"] == want_path, rep
    if want_path == fsg.PATH_MAIN:
        assert (rep["fallback_bitmap"] > 0) == (ws_kind == "third"), rep
        if ws_kind == "full":  # the 120000-byte body at least is indexed by a wave
            assert rep["large_messages"] + rep["huge_messages"] > 0, rep
    _check_decode(call, fam, layout_name)


@pytest.mark.parametrize("layout_name", LAYOUT_NAMES)
@pytest.mark.parametrize("n_msgs", [1, 63, 65])
def test_decode_column_tails(codec, families, n_msgs, layout_name):
    """Batches of 1, 63 and 65 messages (either side of a wave): d_out_len and
    d_status get exactly n_msgs entries."""
    whole = families["valid"]
    fam = whole.subset([(k * len(whole)) // n_msgs + len(whole) // (2 * n_msgs) for k in range(n_msgs)])
    lay, _, _ = fam.image(layout_name)
    call = Call(fam, lay, _DECODE_COLS, _ws_bytes(codec, "full"))
    i = call.ins
    codec.decompress(*call.args(), call.d_out, i["d_out_off"], i["d_out_cap"], call.cols["d_out_len"],
                     call.cols["d_status"], workspace=call.ws)
    _check_decode(call, fam, layout_name)


@pytest.mark.parametrize("layout_name", LAYOUT_NAMES)
@pytest.mark.parametrize("family", ["valid", "hostile"])
@pytest.mark.parametrize("ws_kind", ["full", None])
def test_validate_only_writes_nothing(codec, oracle, families, ws_kind, family, layout_name):
    """FSG_FLAG_VALIDATE_ONLY: the verdicts of IsValidCompressedBuffer, and
    the whole of d_out still POISON, slots included."""
    fam = families[family]
    lay, _, _ = fam.image(layout_name)
    call = Call(fam, lay, _DECODE_COLS, _ws_bytes(codec, ws_kind))
    i = call.ins
    codec.decompress(*call.args(), call.d_out, i["d_out_off"], i["d_out_cap"], call.cols["d_out_len"],
                     call.cols["d_status"], flags=fsg.FSG_FLAG_VALIDATE_ONLY, workspace=call.ws)
    out = call.finish()
    ct.check(out, np.full(lay.total, POISON, dtype=np.uint8), None, lay, fam.caps)
    st = call.col("d_status")
    for k, c in enumerate(fam.comps):
        want = OK if oracle.is_valid(c) else (CORRUPT if oracle.header(c)[0] else BAD_HEADER)
        assert st[k] == want, (k, st[k], want)


_PARTIAL_CAP = 1 << 18  # the oracle's buffer: above every slot of the -small families


@pytest.fixture(scope="module")
def partial_refs(families, oracle):
    """(family, frag) -> per message (produced, got bytes) of the oracle's
    UncompressAsMuchAsPossible, computed once."""
    cache = {}

    def get(family, frag):
        if (family, frag) not in cache:
            cache[family, frag] = [oracle.uncompress_as_much(c, _PARTIAL_CAP, frag) for c in families[family].comps]
        return cache[family, frag]
    return get


@pytest.mark.parametrize("layout_name", LAYOUT_NAMES)
@pytest.mark.parametrize("family", ["valid-small", "hostile-small"])
@pytest.mark.parametrize("frag", [0, 7, 8160])
def test_partial_containment(codec, oracle, families, partial_refs, frag, family, layout_name):
    """fsg_decompress_batch_partial: [off, off + d_got) holds the oracle's
    as-much-as-possible bytes (after a failed stream too); the rest of the
    slot is free, everything outside the slots untouched."""
    fam = families[family]
    assert max(fam.caps) < _PARTIAL_CAP
    refs = partial_refs(family, frag)
    lay, _, _ = fam.image(layout_name)
    call = Call(fam, lay, {"d_got": ("int32", 0), "d_produced": ("int64", 0), "d_status": ("int32", -7)},
                _ws_bytes(codec, "full"))
    i = call.ins
    codec.decompress_partial(*call.args(), frag, call.d_out, i["d_out_off"], i["d_out_cap"], call.cols["d_got"],
                             call.cols["d_produced"], call.cols["d_status"], workspace=call.ws)
    out = call.finish()
    st, got, prod = call.col("d_status"), call.col("d_got").view(np.uint32), call.col("d_produced")
    pinned, lens, bodies = [], [], []
    for k, (c, (r, rgot)) in enumerate(zip(fam.comps, refs)):
        h, _ = oracle.header(c)
        if not h:
            assert st[k] == BAD_HEADER and prod[k] == 0 and got[k] == 0, k
        elif len(rgot) > fam.caps[k]:
            assert st[k] == TOO_SMALL, k
        else:
            assert prod[k] == r and got[k] == len(rgot), (k, prod[k], r, got[k], len(rgot))
            assert (st[k] == OK) == (fam.status[k] == OK), (k, st[k])
        specified = bool(h) and len(rgot) <= fam.caps[k]
        pinned.append(0 if specified else 1)
        lens.append(len(rgot))
        bodies.append(rgot)
    img, mask = ct.expected_image(lay, fam.caps, lens, bodies, pinned)
    ct.check(out, img, mask, lay, fam.caps)


@pytest.mark.parametrize("layout_name", LAYOUT_NAMES)
@pytest.mark.parametrize("family", ["valid-small", "hostile-small"])
def test_iovec_staging_containment(codec, oracle, families, family, layout_name):
    """fsg_decompress_batch_iovec: the staging slots (d_stage) are scratch,
    every byte outside them untouched; one iovec per message of the slot's
    capacity, 64 poison bytes between them, against the oracle's iovecs."""
    import torch
    fam = families[family]
    lay, _, _ = fam.image(layout_name)
    n = len(fam)
    ilay = ct.guarded(fam.caps)  # the iovecs, in a buffer of their own
    d_iov = gh.poisoned(ilay.total)
    base = (ilay.offs + np.uint64(d_iov.data_ptr())).view(np.int64)
    first = np.arange(n + 1, dtype=np.uint32)
    call = Call(fam, lay, {"d_out_len": ("int32", 0), "d_status": ("int32", -7)}, _ws_bytes(codec, "full"),
                extra_inputs=dict(d_iov_base=base, d_iov_len=np.array(fam.caps, np.int64), d_iov_first=first))
    i = call.ins
    codec.decompress_iovec(*call.args(), i["d_iov_base"], i["d_iov_len"], i["d_iov_first"], call.d_out,
                           i["d_out_off"], i["d_out_cap"], call.cols["d_out_len"], call.cols["d_status"],
                           workspace=call.ws)
    call.finish("d_stage")
    torch.cuda.synchronize()
    mem = d_iov.cpu().numpy()
    ct.check_outside(mem, ilay, fam.caps, "iovec buffer")
    st = call.col("d_status")
    for k, c in enumerate(fam.comps):
        a = int(ilay.offs[k])
        buf = mem[a:a + fam.caps[k]].tobytes()
        h, ulen = oracle.header(c)
        if h and ulen > fam.caps[k]:
            assert st[k] == TOO_SMALL and buf == bytes([POISON]) * fam.caps[k], k
            continue
        ok, rbufs = oracle.uncompress_iovec(c, [fam.caps[k]], fill=POISON)
        assert (st[k] == OK) == ok, (k, st[k])
        assert buf == rbufs[0], k


# ---------------------------------------------------------------------------
# LZ4 decode

@pytest.fixture(scope="module")
def lz4_families(plain, ladder, lz4o):
    from lz4_blocks import random_block
    rng = np.random.default_rng(41)
    xs = [x for x in plain if len(x) < HUGE] + [x for _, x in ladder[len(plain):]]
    pairs = [(lz4o.compress(x), x) for x in xs]
    for t in range(30):
        pairs.append(random_block(rng, int(rng.choice([50, 3000, 40000]))))
    return {"valid": _valid(pairs, _lz4_verdicts, lz4o), "hostile": _hostile(pairs, _lz4_verdicts, lz4o)}


# routing id -> (two-pass, lz4_big_min, workspace sized for a third of the input)
_LZ4_ROUTINGS = {"one_pass": (False, None, False), "lane_walk": (True, 4294967295, False),
                 "wave_walk": (True, 64, False), "third_workspace": (True, None, True)}


@pytest.mark.parametrize("layout_name", LAYOUT_NAMES)
@pytest.mark.parametrize("family", ["valid", "hostile"])
@pytest.mark.parametrize("routing", list(_LZ4_ROUTINGS))
def test_lz4_decode_containment(codec, lz4_families, routing, family, layout_name, fsg_opts):
    two_pass, big_min, third = _LZ4_ROUTINGS[routing]
    if big_min is not None:
        fsg_opts(lz4_big_min=big_min)
    fam = lz4_families[family]
    lay, _, _ = fam.image(layout_name)
    lib = codec.lib
    ws_bytes = None
    if two_pass:
        ws_bytes = lambda n, total_in: lib.fsg_lz4_decompress_workspace_bytes(  # noqa: E731
            n, max(total_in // 3, 1) if third else total_in)
    call = Call(fam, lay, _DECODE_COLS, ws_bytes, ws_fill=0x5A if third else None)
    i = call.ins
    codec.lz4_decompress(*call.args(), call.d_out, i["d_out_off"], i["d_out_cap"], call.cols["d_out_len"],
                         call.cols["d_status"], workspace=call.ws)
    call.torch.cuda.synchronize()
    rep = codec.lz4_decompress_report(call.ws, call.n)
    assert rep["path"] == (fsg.PATH_MAIN if two_pass else fsg.PATH_SINGLE_DESIGN), rep
    if two_pass:
        assert (rep["fallback_messages"] > 0) == third, rep
        if big_min is not None:  # the walk the case is named after indexed the blocks
            assert (rep["large_messages"] > 0) == (routing == "wave_walk"), rep
    _check_decode(call, fam, layout_name)


# ---------------------------------------------------------------------------
# Compress: slots of exactly the max_compressed_length value

_SIZES = [0, 1, 15, 16, 17, 59, 60, 61, 64, 65, 4096, 65535, 65536, 65537, 70000, 131072, 131073, 200000]


def _tag_dense(n: int, rng) -> bytes:
    """Single fresh bytes between 4-byte words repeated from more than 2048
    bytes back: a 1-byte literal and a 3-byte copy for every 5 input bytes,
    the most tags per output byte the format has."""
    out = bytearray(rng.integers(0, 256, min(n, 3000), dtype=np.uint8).tobytes())
    src = 0
    while len(out) < n:
        out.append(int(rng.integers(256)))
        out += out[src:src + 4]
        src += 4
    return bytes(out[:n])


@pytest.fixture(scope="module")
def compress_items():
    rng = np.random.default_rng(8)
    items = []
    for n in _SIZES:
        items.append(rng.integers(0, 256, n, dtype=np.uint8).tobytes())  # the longest output
        items.append(_text(n))
        items.append(bytes(n))
        items.append(rng.integers(0, 2, n, dtype=np.uint8).tobytes())
        items.append(_tag_dense(n, rng))
    return items


def _compress_family(items, compress, max_len):
    comps = [compress(x) for x in items]
    return Family(items, [max_len(len(x)) for x in items], [OK] * len(items), [len(c) for c in comps], comps)


@pytest.fixture(scope="module")
def snappy_compress_family(compress_items, oracle):
    return _compress_family(compress_items, oracle.compress, fsg.max_compressed_length)


@pytest.fixture(scope="module")
def lz4_compress_family(compress_items, lz4o, codec):
    return _compress_family(compress_items, lz4o.compress, codec.lib.fsg_lz4_max_compressed_length)


def _check_compress(call: Call, fam: Family, layout_name):
    """out_len and bytes equal the oracle's; the headroom past out_len is
    free; everything outside the slots untouched."""
    out = call.finish()
    lay, img, mask = fam.image(layout_name)
    assert (call.col("d_status") == OK).all()
    ol = call.col("d_out_len").view(np.uint32)
    assert list(ol) == fam.ulen, [(i, int(a), b) for i, (a, b) in enumerate(zip(ol, fam.ulen)) if a != b][:8]
    ct.check(out, img, mask, lay, fam.caps)


# routing id -> (options, encoder variant, workspace, split region cap)
_ENC_ROUTINGS = {
    "default": ({}, 0, True, None),
    "variant1": ({}, 1, True, None),
    "wave_all": (dict(encode_wave_min=1, encode_wave_all_mb=640), 0, True, None),
    "wave_all_wg2": (dict(encode_wave_min=1, encode_wave_all_mb=640, encode_wave_wg=2), 0, True, None),
    "wave_all_wg5": (dict(encode_wave_min=1, encode_wave_all_mb=640, encode_wave_wg=5), 0, True, None),
    "no_workspace": ({}, 0, False, None),
    "region_cap0": ({}, 0, True, 0),
    "region_cap4096": ({}, 0, True, 4096),  # the whole-message fallback
    "wave_all_region_cap4096": (dict(encode_wave_min=1, encode_wave_all_mb=640), 0, True, 4096),
}


@pytest.mark.parametrize("layout_name", LAYOUT_NAMES)
@pytest.mark.parametrize("routing", list(_ENC_ROUTINGS))
def test_compress_containment(codec, snappy_compress_family, routing, layout_name, fsg_opts):
    opts, variant, use_ws, region_cap = _ENC_ROUTINGS[routing]
    fam = snappy_compress_family
    lay, _, _ = fam.image(layout_name)
    fsg_opts(**opts)
    mx = max(len(x) for x in fam.comps)
    lib = codec.lib
    call = Call(fam, lay, _DECODE_COLS, (lambda n, total_in: lib.fsg_compress_workspace_bytes(n, mx)) if use_ws else None)
    i = call.ins
    codec.select_kernels(0, variant)
    if region_cap is not None:
        codec.set_split_region_cap(region_cap)
    try:
        codec.compress(*call.args(), mx, call.d_out, i["d_out_off"], call.cols["d_out_len"], call.cols["d_status"],
                       workspace=call.ws)
        call.torch.cuda.synchronize()
        rep = codec.compress_report(call.ws, call.n, mx)
    finally:
        codec.select_kernels(0, 0)
        codec.set_split_region_cap(0)
    # the routing the case is named after did run
    want_path = fsg.PATH_FORCED if variant == 1 else fsg.PATH_MAIN if use_ws else fsg.PATH_NO_WORKSPACE
    assert rep["path"] == want_path, rep
    if want_path == fsg.PATH_MAIN:
        n_split = sum(len(x) > 65536 for x in fam.comps)
        assert rep["split_messages"] == n_split > 0, rep
        assert (rep["fallback_messages"] > 0) == (region_cap == 4096), rep
        if "encode_wave_min" in opts:
            assert rep["wave_units"] == rep["units_listed"] > 0, rep
    _check_compress(call, fam, layout_name)


@pytest.mark.parametrize("wg", [2, 3, 5])
def test_wave_encoder_waves_per_workgroup(codec, snappy_compress_family, wg, fsg_opts):
    """encode_wave_wg: 2..5 waves share a workgroup's LDS for their hash
    tables; "every value produces the same bytes" -- at the wave encoder's
    default thresholds too (the all-units setting is in the matrix above)."""
    fsg_opts(encode_wave_wg=wg)
    fam = snappy_compress_family
    lay, _, _ = fam.image("guarded")
    mx = max(len(x) for x in fam.comps)
    lib = codec.lib
    call = Call(fam, lay, _DECODE_COLS, lambda n, total_in: lib.fsg_compress_workspace_bytes(n, mx))
    i = call.ins
    codec.compress(*call.args(), mx, call.d_out, i["d_out_off"], call.cols["d_out_len"], call.cols["d_status"],
                   workspace=call.ws)
    _check_compress(call, fam, "guarded")


@pytest.mark.parametrize("layout_name", LAYOUT_NAMES)
def test_lz4_compress_containment(codec, lz4_compress_family, layout_name):
    fam = lz4_compress_family
    lay, _, _ = fam.image(layout_name)
    lib = codec.lib
    call = Call(fam, lay, _DECODE_COLS, lambda n, total_in: lib.fsg_lz4_compress_workspace_bytes(n))
    i = call.ins
    codec.lz4_compress(*call.args(), call.d_out, i["d_out_off"], call.cols["d_out_len"], call.cols["d_status"],
                       call.ws)
    _check_compress(call, fam, layout_name)


# ---------------------------------------------------------------------------
# fsg_uncompressed_lengths_batch

def _varint(v: int, nbytes: int | None = None) -> bytes:
    """v as a varint; nbytes: padded with continuation bytes to that length
    (non-minimal, legal)."""
    out = bytearray()
    while True:
        b = v & 0x7F
        v >>= 7
        more = v or (nbytes is not None and len(out) + 1 < nbytes)
        out.append(b | (0x80 if more else 0))
        if not more:
            return bytes(out)


def _header_cases():
    cases = [b""]
    values = [0, 1, 127, 128, 300, 16383, 16384, (1 << 21) - 1, 1 << 21, (1 << 28) - 1, 1 << 28, 0x7FFFFFFF,
              0x80000000, (1 << 32) - 1]
    for v in values:
        full = _varint(v)
        cases += [full[:k] for k in range(1, len(full) + 1)]  # truncated at each byte
        cases.append(full + b"\x00tail")
        for nb in range(len(full) + 1, 6):  # every header length up to 5
            padded = _varint(v, nb)
            cases += [padded, padded[:-1]]
    # over 32 bits, and a fifth byte with high bits set
    cases += [_varint(1 << 32), _varint((1 << 35) - 1), _varint(1 << 35), b"\xff\xff\xff\xff\x1f", b"\xff\xff\xff\xff\x7f",
              b"\x80\x80\x80\x80\x70", b"\xff\xff\xff\xff\xff", b"\xff\xff\xff\xff\xff\x01", b"\x80\x80\x80\x80\x80\x00",
              b"\x81\x80\x80\x80\x10", b"\x80\x80\x80\x80\x0f"]
    return cases


@pytest.mark.parametrize("lenient", [True, False])
def test_uncompressed_lengths_batch(codec, oracle, lenient):
    """The device header pass against the host parse and the oracle: header
    lengths 1..5, truncated at each byte, a fifth byte with high bits set,
    empty input, values up to 2^32 - 1 and beyond; in batches of 1, 63, 65 and
    all of them, d_ulen getting exactly n_msgs entries."""
    import torch
    cases = _header_cases()
    assert len(cases) > 65 and {len(c) for c in cases} >= set(range(0, 6))
    want = []
    for c in cases:
        u = ctypes.c_uint32(0)
        h = codec.lib.fsg_get_uncompressed_length(c, len(c), ctypes.byref(u), int(lenient))
        oh, ou = oracle.header(c, lenient=lenient)
        assert h == oh and (not h or u.value == ou), (c.hex(), h, oh, u.value, ou)
        want.append(u.value if h else 0xFFFFFFFF)
    assert sum(w != 0xFFFFFFFF for w in want) > 30 and sum(w == 0xFFFFFFFF for w in want) > 30
    if lenient:  # the fifth byte's high bits are dropped, not rejected
        assert want[cases.index(b"\xff\xff\xff\xff\x7f")] == 0xFFFFFFFF and oracle.header(b"\xff\xff\xff\xff\x7f")[0] == 5
    else:
        assert codec.lib.fsg_get_uncompressed_length(b"\xff\xff\xff\xff\x7f", 5, ctypes.byref(ctypes.c_uint32()), 0) == 0
    for n in (1, 63, 65, len(cases)):
        for b0 in range(0, len(cases), n if n > 1 else 7):
            part = cases[b0:b0 + n]
            b = fsg.Batch.from_list(part)
            ins = gh.Inputs(d_in=b.data, d_in_off=b.offsets, d_in_len=b.lens)
            d_ulen = gh.guarded_column(len(part), torch.int32)
            codec.uncompressed_lengths(ins["d_in"], ins["d_in_off"], ins["d_in_len"], len(part), d_ulen, lenient=lenient)
            torch.cuda.synchronize()
            col = d_ulen.cpu().numpy()
            ct.check_column(col, len(part), "d_ulen")
            ins.check()
            assert list(col[:len(part)].view(np.uint32)) == want[b0:b0 + n], (n, b0)


# ---------------------------------------------------------------------------
# fsg_gather_blocks

def test_gather_blocks_every_alignment(codec):
    """Device-memory sources at every (source mod 16, destination mod 16)
    pair, lengths 0..80 and 8160 (a whole cord_buf block): the destination
    ranges equal a numpy copy, the 64 poison bytes between them untouched."""
    import torch
    rng = np.random.default_rng(3)
    src = rng.integers(0, 256, 1 << 16, dtype=np.uint8)
    src[src == POISON] = 0  # a copied byte never looks like an unwritten one
    lens_all = list(range(81)) + [8160]
    s_off, lens, d_res = [], [], []
    for s in range(16):
        for d in range(16):
            for ln in lens_all:
                s_off.append(s + 16 * int(rng.integers(0, ((1 << 16) - 8160 - 16) // 16)))
                lens.append(ln)
                d_res.append(d)
    n = len(lens)
    offs = np.zeros(n, dtype=np.uint64)
    pos = ct.GUARD
    for k in range(n):
        offs[k] = pos + (d_res[k] - pos) % 16
        pos = int(offs[k]) + lens[k] + ct.GUARD
    lay = ct.Layout("gather", offs, pos - ct.GUARD + ct.TRAIL)
    assert all(int(o) % 16 == d for o, d in zip(offs, d_res))
    d_src = gh.dev(src)
    assert d_src.data_ptr() % 16 == 0
    addr = (np.array(s_off, np.uint64) + np.uint64(d_src.data_ptr())).view(np.int64)
    ins = gh.Inputs(src=src, d_src=addr, d_len=np.array(lens, np.uint32), d_dst_off=offs)
    ins.dev["src"] = d_src
    d_dst = gh.poisoned(lay.total)
    assert d_dst.data_ptr() % 16 == 0
    codec.gather_blocks(ins["d_src"], ins["d_len"], ins["d_dst_off"], n, d_dst)
    torch.cuda.synchronize()
    bodies = [src[a:a + ln].tobytes() for a, ln in zip(s_off, lens)]
    img, mask = ct.expected_image(lay, lens, lens, bodies, [0] * n)
    assert not mask.any()
    ct.check(d_dst.cpu().numpy(), img, None, lay, lens, "d_dst")
    ins.check()
