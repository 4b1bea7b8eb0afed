"""GPU parity of the LZ4 frame calls (flare-cpp_amd/csrc/lz4_frame_encode.hip,
lz4_frame_decode.hip) through
the C ABI (include/flare_lz4_gpu.h, "LZ4 frames"): frames byte-equal to the
liblz4 fixtures and to the frame oracle (tests/lz4f_ref.py), every decode
verdict and accepted byte equal to the oracle's on the fast and on the serial
route, the route each frame took as the path report names it.  Every call runs
under the write-containment guards (tests/lz4f_harness.py)."""
import numpy as np
import pytest

import fsg
import lz4f_ref as R
from bind import Lz4Oracle
from lz4f_cases import base_frame, build, fnv, load, mutate, oracle_frame

pytestmark = pytest.mark.gpu
VEC = load()
NONE = 0xFFFFFFFF  # lz4f_block_wave_min: no block on the wave encoder
SERIAL = ("serial_linked", "serial_no_size", "serial_rejected", "serial_forced")


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


@pytest.fixture(scope="module")
def groups(o):
    """The `compress` fixtures by (block size id, checksum): [(entry, input,
    oracle frame)], computed once."""
    out = {}
    for e in VEC["compress"]:
        x = build(e["input"])
        out.setdefault((e["bid"], e["checksum"]), []).append((e, x, oracle_frame(o, e, x)))
    return out


def _check_frames(items, frames, st):
    assert (st == fsg.FSG_OK).all()
    for (e, x, want), f in zip(items, frames):
        assert f == want, e
        if not e.get("differs_from_size_rule"):
            assert len(f) == e["frame_len"] and fnv(f) == e["frame_fnv"], e


@pytest.mark.parametrize("wave_min", [0, NONE, -1], ids=["waves", "lanes", "default"])
def test_compress_matches_fixtures_batches_of_1_65_300(gpu, groups, fsg_opts, wave_min):
    fsg_opts(lz4f_block_wave_min=wave_min)
    items = groups[(4, 0)]
    assert len(items) >= 366 and any(len(x) == 0 for _, x, _ in items[66:366])
    for a, b in ((0, 1), (1, 66), (66, 366)):
        part = items[a:b]
        frames, st, rep = gpu.compress([x for _, x, _ in part], 4, False)
        _check_frames(part, frames, st)
        assert rep["blocks"] == sum(e["blocks"] for e, _, _ in part)
        assert rep["raw_blocks"] == sum(e["raw_blocks"] for e, _, _ in part) and rep["overflow_messages"] == 0
        assert rep["block_wave_min"] == (wave_min if wave_min >= 0 else (8192 if rep["block_entries"] <= 256 else NONE))


def test_compress_every_block_size_and_checksum(gpu, groups):
    for (bid, cs), items in sorted(groups.items()):
        if (bid, cs) == (4, 0):
            items = items[366:]
        frames, st, rep = gpu.compress([x for _, x, _ in items], bid, bool(cs))
        _check_frames(items, frames, st)
        assert rep["raw_blocks"] == sum(e["raw_blocks"] for e, _, _ in items)


def test_no_messages_and_workspace_rules(gpu):
    import torch
    lib = gpu.lib
    assert lib.fsg_lz4f_compress_batch(None, None, None, 0, None, None, None, None, 4, 0, None, 0, None) == 0
    assert lib.fsg_lz4f_decompress_batch(None, None, None, 0, None, None, None, None, None, None, 0, None) == 0
    frames, st, _ = gpu.compress([], 4)
    assert frames == [] and gpu.decompress([], [])[0] == []
    t = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    p = t.data_ptr()
    need_c = lib.fsg_lz4f_compress_workspace_bytes(1, 0, 4)
    need_d = lib.fsg_lz4f_decompress_workspace_bytes(1, 0)
    big = torch.zeros(max(need_c, need_d), dtype=torch.uint8, device="cuda")
    INVALID = -1
    for ws, nbytes in ((None, need_c), (big.data_ptr(), need_c - 1)):  # NULL, undersized
        assert lib.fsg_lz4f_compress_batch(p, p, p, 1, p, p, p, p, 4, 0, ws, nbytes, None) == INVALID
    for ws, nbytes in ((None, need_d), (big.data_ptr(), need_d - 1)):
        assert lib.fsg_lz4f_decompress_batch(p, p, p, 1, p, p, p, p, p, ws, nbytes, None) == INVALID
    for bid in (0, 3, 8):
        assert lib.fsg_lz4f_compress_batch(p, p, p, 1, p, p, p, p, bid, 0, big.data_ptr(), need_c, None) == INVALID
        assert lib.fsg_lz4f_max_frame_length(10, bid) == 0
    assert lib.fsg_lz4f_compress_batch(p, p, p, 1, p, p, p, p, 4, 2, big.data_ptr(), need_c, None) == INVALID
    assert lib.fsg_lz4f_max_frame_length(65537, 4) == R.max_frame_length(65537, 4)
    torch.cuda.synchronize()


def test_compress_workspace_sized_for_fewer_bytes(gpu, o):
    """A workspace sized for less input than the batch: the messages whose
    blocks fit get their frames, the others FSG_CORRUPT with length 0."""
    xs = [fsg.make_batch(fsg.KIND_TEXT, [200000], first_index=i).item(0) for i in range(6)]
    frames, st, rep = gpu.compress(xs, 4, ws_total_in=300000)
    assert rep["overflow_messages"] == int((st != 0).sum()) and 0 < rep["overflow_messages"] < 6
    for x, f, s in zip(xs, frames, st):
        assert (s == fsg.FSG_OK and f == R.compress_frame(o, x, 4)) or (s == fsg.FSG_CORRUPT and f == b"")


@pytest.mark.parametrize("bid", [4, 5, 6, 7])
def test_round_trip_at_the_routing_edges(gpu, o, groups, fsg_opts, bid):
    xs = [fsg.make_batch(fsg.KIND_TEXT, [n], first_index=n).item(0) if n else b""
          for n in (0, 1, 13, 65535, 65536, 65537, 131073, 200000)]
    big = [(x, f) for e, x, f in groups[(bid, 1)] if len(x) == (4 << 20) + 17]
    assert len(big) == 1
    xs.append(big[0][0])
    frames, st, rep = gpu.compress(xs, bid, True)
    assert (st == 0).all() and frames[-1] == big[0][1]
    for x, f in zip(xs[:-1], frames):
        assert f == R.compress_frame(o, x, bid, True), len(x)
    runs = []
    for force in (0, 1):
        fsg_opts(lz4f_force_serial=force)
        outs, ol, st, rep = gpu.decompress(frames, [len(x) for x in xs])
        assert (st == 0).all() and outs == xs and list(ol) == [len(x) for x in xs]
        assert rep["empty_messages"] == 1
        if force:
            assert rep["serial_forced"] == len(xs) - 1 and rep["fast_messages"] == 0
        else:
            assert rep["fast_messages"] == len(xs) - 1 and sum(rep[k] for k in SERIAL) == 0
            assert rep["fast_blocks"] == sum(-(-len(x) // R.block_bytes(bid)) for x in xs)
        runs.append((outs, list(ol), list(st)))
    assert runs[0] == runs[1]


def test_foreign_frames_and_their_routes(gpu, o):
    cases = VEC["decode_ok"]
    frames = [bytes.fromhex(d["hex"]) for d in cases]
    outs, ol, st, rep = gpu.decompress(frames, [d["out_len"] for d in cases])
    for d, y, l, s in zip(cases, outs, ol, st):
        assert s == fsg.FSG_OK and l == d["out_len"] and fnv(y) == d["out_fnv"], d["name"]
    routes = [d["route"] for d in cases]
    assert rep["serial_linked"] == routes.count("serial_linked") >= 2
    assert rep["serial_no_size"] == routes.count("serial_no_size") >= 1
    assert rep["serial_rejected"] == routes.count("serial_rejected") >= 2   # short non-final blocks
    assert rep["fast_messages"] == routes.count("fast") >= 2 and rep["serial_forced"] == 0
    assert rep["checksummed_units"] > 0
    # one frame at a time: the route the fixture names
    for d, f in zip(cases, frames):
        outs, ol, st, rep = gpu.decompress([f], [d["out_len"]])
        assert st[0] == 0 and fnv(outs[0]) == d["out_fnv"]
        assert rep["fast_messages" if d["route"] == "fast" else d["route"]] == 1, d["name"]


@pytest.fixture(scope="module")
def mutated(o):
    """The `decode` fixtures at capacities exact, 0 and too small by one:
    (frames, capacities, the oracle's (status, d_out_len, bytes))."""
    frames, caps, want = [], [], []
    for i, c in enumerate(VEC["decode"]):
        x = build(VEC["decode_sources"][c["src"]])
        f = mutate(base_frame(o, c), c)
        for cap in (len(x), 0, max(len(x) - 1, 0)):
            frames.append(f)
            caps.append(cap)
            want.append(R.decode_frame(o, f, cap))
        assert want[-3][0] == c["oracle"] and want[-3][1] == c["out_len"], i
    return frames, caps, want


@pytest.mark.parametrize("force", [0, 1], ids=["routed", "force_serial"])
def test_mutated_frames_against_oracle(gpu, mutated, fsg_opts, force):
    fsg_opts(lz4f_force_serial=force)
    frames, caps, want = mutated
    outs, ol, st, rep = gpu.decompress(frames, caps)
    for i, (w, y, l, s) in enumerate(zip(want, outs, ol, st)):
        assert (s, l) == w[:2], (i, caps[i])
        if w[0] == R.OK:
            assert y == w[2], i
    assert set(st) == {0, 1, 2, 3}
    if force:
        assert rep["fast_messages"] == 0 and rep["serial_rejected"] == 0
    else:
        assert rep["fast_messages"] > 0 and rep["serial_rejected"] > 0 and rep["serial_forced"] == 0


def test_content_sizes_equal_the_oracle_header_parse(gpu, mutated):
    frames = mutated[0][::3] + [bytes.fromhex(d["hex"]) for d in VEC["decode_ok"]] + [b"", b"\x04\x22\x4d\x18"]
    sizes, st = gpu.content_sizes(frames)
    seen = set()
    for f, sz, s in zip(frames, sizes, st):
        w = R.parse_header(f)
        assert s == w[0] and int(sz) == (fsg.LZ4F_NO_CONTENT_SIZE if w[4] is None else w[4])
        seen.add((w[0], w[4] is None))
    assert len(seen) == 3  # sized, without a size, bad header


def test_inner_decoder_fallback(gpu, o):
    """A decode workspace sized for fewer input bytes than the batch has: the
    blocks still fit the staging area, the block decoder's bitmap does not
    hold them all, and its one-pass kernel finishes the rest -- same bytes,
    and the report counts them."""
    xs = [fsg.make_batch(fsg.KIND_TEXT, [300000], first_index=i).item(0) for i in range(16)]
    frames = [R.compress_frame(o, x, 4) for x in xs]
    total = sum(map(len, frames))
    full = gpu.decompress(frames, [len(x) for x in xs])
    small = gpu.decompress(frames, [len(x) for x in xs], ws_total_in=total * 93 // 100)
    assert full[0] == xs and small[0] == xs and (full[2] == 0).all() and (small[2] == 0).all()
    assert full[3]["inner_fallback_blocks"] == 0 and small[3]["inner_fallback_blocks"] > 0
    for rep in (full[3], small[3]):
        assert rep["fast_messages"] == 16 and sum(rep[k] for k in SERIAL) == 0
    # and one far too small for the batch's blocks: the serial decoder takes what does not fit
    tiny = gpu.decompress(frames, [len(x) for x in xs], ws_total_in=total // 4)
    assert tiny[0] == xs and (tiny[2] == 0).all() and tiny[3]["serial_rejected"] > 0


def test_reports_on_ordinary_frames(gpu, o):
    rng = np.random.default_rng(9)
    xs = [fsg.make_batch(fsg.KIND_TEXT, [n], first_index=n).item(0) for n in (1, 500, 65536, 70000, 300000)]
    xs += [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in (40, 65536, 150000)]
    xs.append(xs[-1][:65536] + xs[4][:100000])  # a raw and two compressed blocks
    frames, st, rep = gpu.compress(xs, 4, True)
    blocks = [R.blocks_of(o, x, 4) for x in xs]
    assert (st == 0).all() and frames == [R.compress_frame(o, x, 4, True) for x in xs]
    assert rep["blocks"] == sum(map(len, blocks)) and rep["overflow_messages"] == 0
    assert rep["raw_blocks"] == sum(r for b in blocks for _, r in b) >= 5
    outs, ol, st, rep = gpu.decompress(frames, [len(x) for x in xs])
    assert (st == 0).all() and outs == xs
    assert sum(rep[k] for k in SERIAL) == 0 and rep["fast_messages"] == len(xs) and rep["empty_messages"] == 0
    assert rep["fast_blocks"] == sum(map(len, blocks)) and rep["checksummed_units"] == len(xs)
    assert rep["inner_fallback_blocks"] == 0
