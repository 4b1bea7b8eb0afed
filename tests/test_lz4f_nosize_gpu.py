"""GPU tests of the block-parallel route for LZ4 frames without a content size
(option lz4f_nosize_fast; flare-cpp_amd/csrc/lz4_frame_decode.hip, lz4_frame_length.h)
and of fsg_lz4f_decoded_lengths_batch, through the C ABI.  Expected statuses,
lengths and bytes are the frame oracle's (tests/lz4f_ref.py: decode_frame,
block_length); the frames come from tests/lz4f_nosize_cases.py.  Every
decompress call runs under the write-containment guards of
tests/lz4f_harness.py; the lengths call under the same guards here."""
import numpy as np
import pytest

import containment as ct
import fsg
import lz4f_nosize_cases as C
import lz4f_ref as R
from bind import Lz4Oracle
from lz4f_cases import load

pytestmark = pytest.mark.gpu
VEC = load()
NONE = 0xFFFFFFFF  # lz4f_length_wave_min: no block by wave
WALKS = [0, NONE, -1]
WALK_IDS = ["waves", "lanes", "default"]


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


def decoded_lengths(gpu, frames, ws_total_in=None):
    """(lengths, statuses) of fsg_lz4f_decoded_lengths_batch, guarded as
    lz4f_harness guards the other calls: sentinels behind both columns and the
    workspace (filled with 0xFF first), the inputs compared afterwards."""
    from gpu_harness import Inputs, guarded_column, guarded_workspace
    torch = gpu.torch
    b = fsg.Batch.from_list(frames)
    n = len(b)
    ins = Inputs(d_in=b.data, d_in_off=b.offsets, d_in_len=b.lens)
    d_len = guarded_column(n, torch.int64)
    d_st = guarded_column(n, torch.int32, -7)
    total = int(b.data.size) if ws_total_in is None else ws_total_in
    ws, whole = guarded_workspace(gpu.lib.fsg_lz4f_decompress_workspace_bytes(n, total))
    ws.fill_(0xFF)
    gpu.codec.lz4f_decoded_lengths(ins["d_in"], ins["d_in_off"], ins["d_in_len"], n, d_len, d_st, ws)
    torch.cuda.synchronize()
    ct.check_column(d_len.cpu().numpy(), n, "d_length")
    ct.check_column(d_st.cpu().numpy(), n, "d_status")
    ct.check_workspace_guard(whole[-ct.WORKSPACE_GUARD:].cpu().numpy())
    ins.check()
    return d_len.cpu().numpy()[:n].view(np.uint64), d_st.cpu().numpy()[:n]


def check_lengths(gpu, frames, **kw):
    lens, st = decoded_lengths(gpu, frames, **kw)
    for i, (f, l, s) in enumerate(zip(frames, lens, st)):
        assert (int(s), int(l)) == C.decoded_length(f), i


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


# ---- 1. routing edges

@pytest.fixture(scope="module")
def edges(o):
    items = C.routing_edges(o)
    frames = [f for _, f, _ in items]
    want = {}
    for name, delta in (("exact", 0), ("roomy", 1000), ("short", -1)):
        caps = [len(x) + delta for x, _, _ in items]
        want[name] = (caps, [R.decode_frame(o, f, c) for f, c in zip(frames, caps)])
    return items, frames, want


def test_routing_edges_on_the_new_route(gpu, edges, fsg_opts):
    items, frames, want = edges
    assert len(frames) == 64 and sum(len(x) == C.BIG for x, _, _ in items) == 8
    for (x, _, _), w in zip(items, want["exact"][1]):
        assert w == (R.OK, len(x), x)
    assert all(w[:2] == (R.CORRUPT, 0) for w in want["short"][1])
    fsg_opts(lz4f_nosize_fast=1)
    runs = {}
    for name in ("exact", "roomy", "short"):
        caps, w = want[name]
        got = gpu.decompress(frames, caps)
        rep = check_outputs(frames, caps, got, w)
        assert rep["serial_no_size"] == 0 and rep["fast_messages"] == 0 and rep["empty_messages"] == 0
        if name == "short":  # the sum of the lengths exceeds the slot: the serial decoder says what that is
            assert rep["fast_nosize_messages"] == 0 and rep["serial_rejected"] == len(frames)
        else:
            assert rep["fast_nosize_messages"] == len(frames) and rep["serial_rejected"] == 0
            assert rep["fast_nosize_blocks"] == sum(nb for _, _, nb in items)
        runs[name] = got
    fsg_opts(lz4f_nosize_fast=0)
    caps, w = want["exact"]
    got = gpu.decompress(frames, caps)
    rep = check_outputs(frames, caps, got, w)
    assert rep["serial_no_size"] == len(frames) and rep["fast_nosize_messages"] == 0 and rep["fast_nosize_blocks"] == 0
    assert got[0] == runs["exact"][0] and list(got[1]) == list(runs["exact"][1])
    assert list(got[2]) == list(runs["exact"][2])


# ---- 2. free-form blocks

def test_free_form_blocks_and_many_small_frames(gpu, o, fsg_opts):
    fsg_opts(lz4f_nosize_fast=1)
    for items in (C.free_form(o), C.one_block_frames(o, 300)):
        frames = [f for _, f, _ in items]
        caps = [len(x) for x, _, _ in items]
        outs, ol, st, rep = gpu.decompress(frames, caps)
        assert (st == 0).all() and outs == [x for x, _, _ in items] and list(ol) == caps
        assert rep["fast_nosize_messages"] == len(items) and rep["fast_nosize_blocks"] == sum(nb for _, _, nb in items)
        assert rep["serial_rejected"] == 0 and rep["serial_no_size"] == 0 and rep["fast_messages"] == 0
    assert [nb for _, _, nb in C.free_form(o)] == [5, 3, 3, 130]


# ---- 3. both walkers on hard blocks

@pytest.fixture(scope="module")
def hard(o):
    blocks = C.hard_blocks()
    assert len(blocks) >= 120 + 30
    frames = [C.block_frame(b, bid) for b, bid in blocks]
    lens = [R.block_length(b, R.block_bytes(bid)) for b, bid in blocks]
    assert None not in lens
    want = [R.decode_frame(o, f, n) for f, n in zip(frames, lens)]
    assert all(w[0] == R.OK for w in want[:120])
    return frames, lens, want


@pytest.mark.parametrize("wave_min", WALKS, ids=WALK_IDS)
def test_hard_blocks_on_both_walkers(gpu, hard, fsg_opts, wave_min):
    frames, lens, want = hard
    fsg_opts(lz4f_nosize_fast=1, lz4f_length_wave_min=wave_min)
    rep = check_outputs(frames, lens, gpu.decompress(frames, lens), want)
    assert rep["fast_nosize_messages"] == sum(w[0] == R.OK for w in want)
    got, st = decoded_lengths(gpu, frames)
    assert (st == 0).all() and [int(v) for v in got] == lens


# ---- 4. mutated frames

@pytest.fixture(scope="module")
def mutated(o):
    frames, caps, _ = C.mutated(o)
    return frames, caps, [R.decode_frame(o, f, c) for f, c in zip(frames, caps)]


@pytest.mark.parametrize("wave_min", [0, NONE], ids=["waves", "lanes"])
def test_mutated_frames_against_oracle(gpu, mutated, fsg_opts, wave_min):
    frames, caps, want = mutated
    assert len(frames) == 3 * C.MUT_COUNT
    fsg_opts(lz4f_nosize_fast=1, lz4f_length_wave_min=wave_min)
    rep = check_outputs(frames, caps, gpu.decompress(frames, caps), want)
    assert rep["fast_nosize_messages"] > 0 and rep["serial_rejected"] > 0 and rep["serial_no_size"] == 0
    check_lengths(gpu, frames[::3])


# ---- 5. a mixed batch and workspace limits

def test_mixed_batch_and_small_workspace(gpu, o, fsg_opts):
    items = C.mixed(o)
    frames = [f for f, _, _ in items]
    caps = [c for _, c, _ in items]
    kinds = [k for _, _, k in items]
    want = [R.decode_frame(o, f, c) for f, c in zip(frames, caps)]
    assert [w[0] for w, k in zip(want, kinds) if k != "bad_header"] == [R.OK] * (len(items) - 1)
    fsg_opts(lz4f_nosize_fast=1)
    full = gpu.decompress(frames, caps)
    rep = check_outputs(frames, caps, full, want)
    assert rep["fast_messages"] == kinds.count("fast") == 4 and rep["fast_nosize_messages"] == kinds.count("nosize") == 4
    assert rep["serial_linked"] == kinds.count("linked") >= 2 and rep["empty_messages"] == kinds.count("empty") == 2
    assert rep["serial_no_size"] == 0 and rep["serial_rejected"] == 0 and rep["serial_forced"] == 0
    assert full[2][kinds.index("bad_header")] == R.BAD_HEADER
    small = gpu.decompress(frames, caps, ws_total_in=sum(map(len, frames)) // 4)
    rep = check_outputs(frames, caps, small, want)
    assert small[0] == full[0] and rep["serial_rejected"] > 0
    # the workspace size function: the values of the build before this route existed
    sizes = gpu.lib.fsg_lz4f_decompress_workspace_bytes
    assert [sizes(1, 0), sizes(300, 1 << 20), sizes(16, 64 << 20)] == [3072, 1599232, 99880960]


# ---- 6. decoded lengths

def test_decoded_lengths_equal_the_oracle(gpu, o, fsg_opts):
    frames = [f for _, f, _ in C.routing_edges(o)] + [f for _, f, _ in C.free_form(o)]
    frames += [f for f, _, _ in C.mixed(o)] + [bytes.fromhex(d["hex"]) for d in VEC["decode_ok"]]
    frames += [R.header(None, 4, False) + b"\0\0\0\x80" + C.END, b""]  # an empty raw block; no bytes at all
    want = [C.decoded_length(f) for f in frames]
    assert {w[0] for w in want} == {R.OK, R.BAD_HEADER}
    assert any(not (f[4] & R.F_INDEP) and not (f[4] & R.F_SIZE) for f, w in zip(frames, want) if w[0] == R.OK)
    for wave_min in (-1, 0):
        fsg_opts(lz4f_length_wave_min=wave_min)
        check_lengths(gpu, frames)
    # a workspace with room for no blocks but one per frame: the index lane walks what does not fit
    check_lengths(gpu, frames, ws_total_in=0)
