"""GPU tests of the fast route for LZ4 frames with linked blocks (option
lz4f_linked_fast; flare-cpp_amd/csrc/lz4_frame_decode.hip, and the prefix forms and
lz4_exec_chain_kernel of lz4_decode2.hip), through the C ABI.  Expected
statuses, lengths and bytes are the frame oracle's (tests/lz4f_ref.py,
decode_frame); the frames come from tests/lz4f_linked_cases.py and
tests/golden/lz4f_linked_vectors.json.  Every call goes through
lz4f_harness.Lz4fGpu.decompress, under its write-containment guards."""
import pytest

import lz4f_linked_cases as C
import lz4f_nosize_cases as N
import lz4f_ref as R
from bind import Lz4Oracle

pytestmark = pytest.mark.gpu
BOTH = dict(lz4f_linked_fast=1, lz4f_nosize_fast=1)


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test run without a visible GPU")
    from lz4f_harness import Lz4fGpu
    return Lz4fGpu()


@pytest.fixture(scope="module")
def o():
    return Lz4Oracle()


def sized(f: bytes) -> bool:
    return bool(f[4] & R.F_SIZE)


def check_outputs(frames, caps, got, want):
    """(status, d_out_len) of every case and the bytes of the accepted ones
    against the oracle's `want`; returns the report."""
    outs, ol, st, rep = got
    assert len(outs) == len(want) == len(frames)
    for i, (w, y, l, s) in enumerate(zip(want, outs, ol, st)):
        assert (int(s), int(l)) == w[:2], (i, caps[i])
        if w[0] == R.OK:
            assert y == w[2], i
    return rep


@pytest.fixture(scope="module")
def edges():
    """The case set and the fixture with the oracle's answers at the
    capacities exact, + 1000 (frames without a content size) and - 1."""
    items = C.all_frames()
    frames = [f for _, _, f, _ in items]
    want = {}
    for name, delta in (("exact", 0), ("short", -1)):
        caps = [len(x) + delta for _, x, _, _ in items]
        want[name] = (frames, caps, [R.decode_frame(None, f, c) for f, c in zip(frames, caps)])
    ns = [(x, f) for _, x, f, _ in items if not sized(f)]
    want["roomy"] = ([f for _, f in ns], [len(x) + 1000 for x, _ in ns], [(R.OK, len(x), x) for x, _ in ns])
    for (_, x, _, _), w in zip(items, want["exact"][2]):
        assert w == (R.OK, len(x), x)
    assert all(w[0] in (R.CORRUPT, R.SLOT_TOO_SMALL) for w in want["short"][2])
    return items, want


def check_fast(rep, items):
    assert rep["fast_linked_messages"] == len(items)
    assert rep["fast_linked_blocks"] == sum(nb for _, _, _, nb in items)
    assert rep["serial_linked"] == 0 and rep["serial_rejected"] == 0 and rep["serial_no_size"] == 0
    assert rep["fast_messages"] == 0 and rep["fast_nosize_messages"] == 0


# ---- 1. edges, with and without a content size

def test_edges_sized_and_no_size(gpu, edges, fsg_opts):
    items, want = edges
    assert any(sized(f) for _, _, f, _ in items) and any(not sized(f) for _, _, f, _ in items)
    assert max(len(x) for _, x, _, _ in items) == 300000
    fsg_opts(**BOTH)
    frames, caps, w = want["exact"]
    check_fast(check_outputs(frames, caps, gpu.decompress(frames, caps), w), items)
    frames, caps, w = want["roomy"]
    rep = check_outputs(frames, caps, gpu.decompress(frames, caps), w)
    check_fast(rep, [t for t in items if not sized(t[2])])
    frames, caps, w = want["short"]
    rep = check_outputs(frames, caps, gpu.decompress(frames, caps), w)
    assert rep["serial_rejected"] == len(frames) and rep["fast_linked_messages"] == 0 and rep["serial_linked"] == 0


# ---- 2. both index walkers

@pytest.mark.parametrize("big_min", [0, 0xFFFFFFFF], ids=["wave_walk", "lane_walk"])
def test_both_index_walkers(gpu, edges, fsg_opts, big_min):
    items, want = edges
    fsg_opts(lz4_big_min=big_min, **BOTH)
    frames, caps, w = want["exact"]
    check_fast(check_outputs(frames, caps, gpu.decompress(frames, caps), w), items)


# ---- 3. mutated frames

def test_mutated_frames_against_oracle(gpu, fsg_opts):
    frames, caps = C.mutated()
    want = [R.decode_frame(None, f, c) for f, c in zip(frames, caps)]
    fsg_opts(**BOTH)
    rep = check_outputs(frames, caps, gpu.decompress(frames, caps), want)
    assert rep["fast_linked_messages"] > 0 and rep["serial_rejected"] > 0
    assert rep["serial_linked"] == 0
    for name, f, cap in C.negatives():
        outs, ol, st, rep = gpu.decompress([f], [cap])
        assert (int(st[0]), int(ol[0])) == (R.CORRUPT, 0), name
        assert rep["serial_rejected"] == 1 and rep["fast_linked_messages"] == 0, name


# ---- 4. options

def test_options(gpu, edges, fsg_opts):
    items, want = edges
    frames, caps, w = want["exact"]
    n_sized = sum(sized(f) for f in frames)
    fsg_opts(lz4f_linked_fast=0, lz4f_nosize_fast=0)
    off = gpu.decompress(frames, caps)
    rep = check_outputs(frames, caps, off, w)
    assert rep["serial_linked"] == len(frames) and rep["fast_linked_messages"] == 0 and rep["fast_linked_blocks"] == 0
    assert rep["serial_rejected"] == 0 and rep["fast_messages"] == 0
    fsg_opts(lz4f_linked_fast=0, lz4f_nosize_fast=1)
    rep = check_outputs(frames, caps, gpu.decompress(frames, caps), w)
    assert rep["serial_linked"] == len(frames) and rep["fast_linked_messages"] == 0
    fsg_opts(lz4f_linked_fast=1, lz4f_nosize_fast=0)
    alone = gpu.decompress(frames, caps)
    rep = check_outputs(frames, caps, alone, w)
    assert rep["fast_linked_messages"] == n_sized and rep["serial_linked"] == len(frames) - n_sized
    assert rep["fast_linked_blocks"] == sum(nb for _, _, f, nb in items if sized(f))
    assert rep["serial_rejected"] == 0
    assert alone[0] == off[0] and list(alone[1]) == list(off[1]) and list(alone[2]) == list(off[2])
    fsg_opts(lz4f_force_serial=1, **BOTH)
    rep = check_outputs(frames, caps, gpu.decompress(frames, caps), w)
    assert rep["serial_forced"] == len(frames) and rep["fast_linked_messages"] == 0


# ---- 5. a mixed batch, workspaces, many chains

def test_mixed_batch_and_workspaces(gpu, o, fsg_opts):
    by = {n: (x, f, nb) for n, x, f, nb in C.all_frames()}
    batch = []
    for i, n in enumerate((500, 70000, 200000)):
        x = N.text(n, seed=50 + i)
        batch.append((R.compress_frame(o, x, 4, bool(i % 2)), n, "fast", 0))
        batch.append((N.nosize_frame(o, x, 4, bool(i % 2)), n + (i % 2) * 100, "nosize", 0))
    for name in ("far_sized", "greedy_sized_131073", "sized_200000", "id5_300000"):
        x, f, nb = by[name]
        batch.append((f, len(x), "linked", nb))
    for name in ("hand_sums", "greedy_raw_middle", "no_size_checksums", "pieces_raw_middle"):
        x, f, nb = by[name]
        batch.append((f, len(x) + 7, "linked_nosize", nb))
    batch.append((R.header(None, 4, False, False) + N.END, 0, "empty", 0))
    bad = bytearray(by["hand"][1])
    bad[5] ^= 0x10
    batch.append((bytes(bad), 100, "bad_header", 0))
    frames, caps = [b[0] for b in batch], [b[1] for b in batch]
    kinds = [b[2] for b in batch]
    want = [R.decode_frame(o, f, c) for f, c in zip(frames, caps)]
    assert [w[0] for w, k in zip(want, kinds) if k != "bad_header"] == [R.OK] * (len(batch) - 1)
    fsg_opts(**BOTH)
    full = gpu.decompress(frames, caps)
    rep = check_outputs(frames, caps, full, want)
    assert rep["fast_messages"] == kinds.count("fast") == 3 and rep["fast_nosize_messages"] == kinds.count("nosize") == 3
    assert rep["fast_linked_messages"] == kinds.count("linked") + kinds.count("linked_nosize") == 8
    assert rep["fast_linked_blocks"] == sum(b[3] for b in batch)
    assert rep["empty_messages"] == 1 and rep["serial_linked"] == 0 and rep["serial_rejected"] == 0
    assert rep["serial_no_size"] == 0 and rep["inner_fallback_blocks"] == 0
    assert full[2][kinds.index("bad_header")] == R.BAD_HEADER
    # a workspace for a quarter of the input: some frames' blocks do not fit
    small = gpu.decompress(frames, caps, ws_total_in=sum(map(len, frames)) // 4)
    rep = check_outputs(frames, caps, small, want)
    assert small[0] == full[0] and rep["serial_rejected"] > 0


def test_tight_bitmap_stops_the_chain(gpu, fsg_opts):
    """A workspace sized for 93% of the input: the blocks fit the staging
    area, the block decoder's bitmap does not hold them all, its one-pass
    kernel takes the rest, the chains of those frames stop there, and the
    serial decoder answers with the same bytes."""
    fsg_opts(**BOTH)
    items = [t for t in C.all_frames() if len(t[1]) >= 131073]
    assert len(items) >= 6
    frames, caps = [f for _, _, f, _ in items], [len(x) for _, x, _, _ in items]
    outs, ol, st, rep = gpu.decompress(frames, caps, ws_total_in=sum(map(len, frames)) * 93 // 100)
    assert [int(s) for s in st] == [R.OK] * len(items) and outs == [x for _, x, _, _ in items]
    assert rep["inner_fallback_blocks"] > 0 and rep["serial_rejected"] > 0 and rep["serial_linked"] == 0
    assert rep["fast_linked_messages"] + rep["serial_rejected"] == len(items)


def test_many_chains_side_by_side(gpu, fsg_opts):
    fsg_opts(**BOTH)
    base = N.text(65537 + 299, seed=31)
    xs = [base[i:i + 65537] for i in range(300)]
    frames = [C.frame(C.compress_linked(x, [65536, 1]), x, sized=True) for x in xs[:3]]
    # (the greedy writer is slow: three frames written, each sent 100 times to slots of their own)
    frames, xs = frames * 100, xs[:3] * 100
    outs, ol, st, rep = gpu.decompress(frames, [65537] * 300)
    assert (st == 0).all() and outs == xs and list(ol) == [65537] * 300
    assert rep["fast_linked_messages"] == 300 and rep["fast_linked_blocks"] == 600 and rep["serial_rejected"] == 0


# ---- 6. unaligned, touching slots

def test_unaligned_touching_slots(gpu, fsg_opts, monkeypatch):
    """Slots that touch, at offsets that are no multiples of 16, in a poisoned
    buffer (containment.tight in place of the harness's aligned layout): frame
    k's first block ends k = 1..15 bytes past a 16-byte boundary of the
    buffer, and the slots start at many residues.  Each frame's bytes are
    right, so no frame changed a neighbour's."""
    import containment as ct
    fsg_opts(**BOTH)
    name, hx, hf, _ = C.all_frames()[0]
    assert name == "hand"
    xs = [N.text(3000 + 16 * 40 + k, seed=70 + k) for k in range(1, 16)]
    xs.insert(4, hx)
    caps = [len(x) for x in xs]
    offs = [int(v) for v in ct.tight(caps).offs]
    assert len({v % 16 for v in offs}) >= 8
    frames, ends = [], set()
    for i, (x, at) in enumerate(zip(xs, offs)):
        if x is hx:
            frames.append(hf)
            continue
        k = i + 1 if i < 4 else i  # 1..15
        first = 640 + (k - at - 640) % 16
        ends.add((at + first) % 16)
        frames.append(C.frame(C.compress_linked(x, [first, 1500, len(x) - first - 1500]), x, checksum=k % 3 == 0,
                              bsum=k % 5 == 0))
        assert any(m["k"] == 1 and m["p"] < m["off"] for m in C.matches(frames[-1])), k  # block 1 reads block 0
    assert ends == set(range(1, 16))
    items = list(zip(xs, frames))
    monkeypatch.setattr(ct, "aligned", ct.tight)
    # (blocks of a few hundred stored bytes round their bitmaps up by more than a workspace sized for exactly the
    # input allows for; twice the input holds them all, so no chain stops at a block left to the one-pass kernel)
    outs, ol, st, rep = gpu.decompress(frames, caps, ws_total_in=2 * sum(map(len, frames)))
    monkeypatch.undo()
    assert rep["inner_fallback_blocks"] == 0
    assert (st == 0).all() and list(ol) == caps
    for i, (x, _) in enumerate(items):
        assert outs[i] == x, i
    assert rep["fast_linked_messages"] == len(items) and rep["serial_rejected"] == 0
