"""GPU tests of the compress flags of the LZ4 frame calls (content checksum,
block checksums, no content size: flare-cpp_amd/csrc/lz4_frame_encode.hip) and
of the
checksum kernel behind every XXH32 of those calls (csrc/lz4f_xxh.h: a quad of
lanes per unit), alone through fsg_lz4f_xxh32_batch and inside compress and
decompress, through the C ABI.  Expected checksums are tests/lz4f_ref.xxh32,
expected frames the liblz4 fixture tests/golden/lz4f_flags_vectors.json and the
host codec, expected verdicts tests/lz4f_ref.decode_frame and the host codec.
tests/lz4f_harness.py has no flags argument, so the compress and checksum
calls bring their own plumbing here, under the same write-containment guards
(tests/containment.py) and on a workspace filled with 0xFF."""
import ctypes
from pathlib import Path

import numpy as np
import pytest

import containment as ct
import fsg
import lz4f_flags_cases as C
import lz4f_ref as R
from bind import Lz4Oracle
from lz4f_cases import build

pytestmark = pytest.mark.gpu
REPO = Path(__file__).resolve().parents[1]
VEC = C.load()
SEEDS = (0, 0x9E3779B1)


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
def host():
    L = ctypes.CDLL(str(REPO / "flare-cpp_amd" / "lib" / "libflare_rpc_snappy.so"))
    L.fsh_lz4f_max_frame_length_flags.argtypes = [ctypes.c_size_t, ctypes.c_int, ctypes.c_uint32]
    L.fsh_lz4f_max_frame_length_flags.restype = ctypes.c_size_t
    L.fsh_cpu_lz4f_compress_flags.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int,
                                              ctypes.c_uint32]
    L.fsh_cpu_lz4f_compress_flags.restype = ctypes.c_size_t
    L.fsh_cpu_lz4f_uncompress.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t,
                                          ctypes.POINTER(ctypes.c_uint32)]
    return L


def host_compress(L, x: bytes, bid: int, flags: int) -> bytes:
    cap = L.fsh_lz4f_max_frame_length_flags(len(x), bid, flags)
    out = ctypes.create_string_buffer(cap + 1)
    n = L.fsh_cpu_lz4f_compress_flags(ctypes.create_string_buffer(x, max(len(x), 1)), len(x), out, bid, flags)
    assert n <= cap
    return out.raw[:n]


def host_status(L, f: bytes, cap: int):
    out = ctypes.create_string_buffer(max(cap, 1))
    ln = ctypes.c_uint32(0)
    r = L.fsh_cpu_lz4f_uncompress(ctypes.create_string_buffer(f, max(len(f), 1)), len(f), out, cap, ctypes.byref(ln))
    return {1: R.OK, 0: R.CORRUPT, -1: R.BAD_HEADER, -2: R.SLOT_TOO_SMALL}[r], ln.value


# ---- plumbing of the two calls lz4f_harness does not drive

def xxh32_batch(gpu, data: np.ndarray, offs: np.ndarray, lens: np.ndarray, seed: int) -> np.ndarray:
    """fsg_lz4f_xxh32_batch on bodies packed in `data` (the device tensor is
    exactly data.size bytes): a sentinel tail behind the result column, the
    inputs compared afterwards."""
    from gpu_harness import Inputs, guarded_column
    n = len(lens)
    ins = Inputs(d_in=data, d_in_off=offs.astype(np.uint64), d_in_len=lens.astype(np.uint32))
    assert ins["d_in"].numel() == data.size
    d_x = guarded_column(n, gpu.torch.int32)
    gpu.codec.lz4f_xxh32(ins["d_in"], ins["d_in_off"], ins["d_in_len"], n, d_x, seed=seed)
    gpu.torch.cuda.synchronize()
    col = d_x.cpu().numpy()
    ct.check_column(col, n, "d_xxh")
    ins.check()
    return col[:n].view(np.uint32)


def compress(gpu, xs, bid: int, flags: int):
    """(frames, statuses, report) of fsg_lz4f_compress_batch_flags, in
    slots of fsg_lz4f_max_frame_length_flags, guarded as lz4f_harness guards."""
    from gpu_harness import Inputs, check_call, guarded_column, guarded_workspace, poisoned
    torch = gpu.torch
    batch = fsg.Batch.from_list(xs)
    n = len(batch)
    caps = np.array([gpu.lib.fsg_lz4f_max_frame_length_flags(int(x), bid, flags) for x in batch.lens], dtype=np.uint64)
    assert [int(c) for c in caps] == [C.max_frame_length_flags(int(x), bid, flags) for x in batch.lens]
    lay = ct.aligned(caps)
    ins = Inputs(d_in=batch.data, d_in_off=batch.offsets, d_in_len=batch.lens, d_out_off=lay.offs)
    d_out = poisoned(lay.total)
    d_ol = guarded_column(n, torch.int32)
    d_st = guarded_column(n, torch.int32, -7)
    ws, whole = guarded_workspace(gpu.lib.fsg_lz4f_compress_workspace_bytes(n, batch.total, bid))
    ws.fill_(0xFF)
    gpu.codec.lz4f_compress(ins["d_in"], ins["d_in_off"], ins["d_in_len"], n, d_out, ins["d_out_off"], d_ol, d_st, ws,
                            block_size_id=bid, flags=flags)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    check_call(out, lay, caps, {"d_out_len": d_ol, "d_status": d_st}, n, whole, ins)
    ol = d_ol.cpu().numpy()[:n].view(np.uint32)
    st = d_st.cpu().numpy()[:n]
    assert (ol <= caps).all()
    frames = [out[int(lay.offs[i]):int(lay.offs[i]) + int(ol[i])].tobytes() for i in range(n)]
    return frames, st, gpu.codec.lz4f_compress_report(ws, n, bid)


# ---- 1. the checksum kernel alone

def pack(bodies):
    lens = np.array([len(b) for b in bodies], dtype=np.uint32)
    offs = np.zeros(len(bodies), dtype=np.uint64)
    offs[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
    return np.frombuffer(b"".join(bodies), dtype=np.uint8), offs, lens


@pytest.fixture(scope="module")
def edge_bodies():
    """Bodies back to back from offset 0; the 4 MiB + 17 one last, ending where
    the tensor ends.  (bodies, reference words per seed)."""
    rng = np.random.default_rng(71)
    lengths = list(range(81)) + [1023, 1024, 1025, 4095, 4096, 4097, 65535, 65536, 65537, (4 << 20) + 17]
    bodies = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in lengths]
    return bodies, {s: [R.xxh32(b, s) for b in bodies] for s in SEEDS}


@pytest.mark.parametrize("seed", SEEDS)
def test_xxh32_batch_every_alignment_and_length_edge(gpu, edge_bodies, seed):
    bodies, want = edge_bodies
    data, offs, lens = pack(bodies)
    assert {int(v) % 16 for v in offs} == set(range(16))          # every start alignment
    assert int(offs[-1]) + int(lens[-1]) == data.size              # the last body ends the tensor
    got = xxh32_batch(gpu, data, offs, lens, seed)
    assert [int(v) for v in got] == want[seed]


def test_xxh32_batch_many_small_bodies_with_empty_ones(gpu):
    rng = np.random.default_rng(72)
    lens = rng.integers(0, 301, 5000)
    lens[::7] = 0
    lens[-1] = 300
    bodies = [rng.integers(0, 256, int(n), dtype=np.uint8).tobytes() for n in lens]
    data, offs, ln = pack(bodies)
    assert int(offs[-1]) + int(ln[-1]) == data.size
    got = xxh32_batch(gpu, data, offs, ln, 0)
    assert [int(v) for v in got] == [R.xxh32(b) for b in bodies]
    assert R.xxh32(b"") == 0x02CC5D05 and int(got[0]) == 0x02CC5D05


# ---- 2. compress with every flag combination

@pytest.fixture(scope="module")
def bodies():
    """The fixture's inputs (an empty body, a 1-byte body and the raw-middle
    input among them) and nine more: 19 bodies."""
    xs = list(C.inputs())
    xs += [build({"gen": "random", "seed": 240, "size": 70000}), build({"gen": "text", "seed": 241, "size": 131072}),
           build({"gen": "text", "seed": 242, "size": 5000}), build({"gen": "random", "seed": 243, "size": 16}),
           build({"gen": "text", "seed": 244, "size": 196608}), b"", build({"gen": "random", "seed": 245, "size": 1}),
           build({"gen": "text", "seed": 246, "size": 262145}), build({"gen": "text", "seed": 247, "size": 33})]
    return xs


_DEVICE = {}


def device_frames(gpu, bodies, bid, flags):
    key = (bid, flags)
    if key not in _DEVICE:
        _DEVICE[key] = compress(gpu, bodies, bid, flags)
    return _DEVICE[key]


@pytest.mark.parametrize("bid", C.IDS)
@pytest.mark.parametrize("flags", C.ALL_FLAGS)
def test_compress_flags_frames_equal_fixture_and_host_codec(gpu, host, bodies, flags, bid):
    frames, st, rep = device_frames(gpu, bodies, bid, flags)
    assert (st == fsg.FSG_OK).all(), st
    assert rep["overflow_messages"] == 0
    for i, (x, f) in enumerate(zip(bodies, frames)):
        flg = f[4]
        assert bool(flg & R.F_BSUM) == bool(flags & C.BSUM), (i, "B.Checksum")
        assert bool(flg & R.F_SIZE) == bool(x and not flags & C.NOSIZE), (i, "C.Size")
        assert bool(flg & R.F_CSUM) == bool(flags & C.CSUM), (i, "C.Checksum")
        assert f == host_compress(host, x, bid, flags), (i, len(x))
        if i < len(C.LENGTHS) + 1:
            assert (len(f), C.fnv(f)) == VEC[(i, bid, flags)], i
    assert rep["raw_blocks"] >= 3   # the raw-middle input's block among them


def test_compress_rejects_undefined_flag_bits(gpu):
    lib = gpu.lib
    t = gpu.torch.zeros(4096, dtype=gpu.torch.uint8, device="cuda")
    ws = gpu.codec.lz4f_compress_workspace(1, 0, 4)
    p = t.data_ptr()
    args = (ws.data_ptr(), ws.numel(), None)
    for flags in (8, 0x80000000 | C.BSUM):
        assert lib.fsg_lz4f_compress_batch_flags(p, p, p, 1, p, p, p, p, 4, flags, *args) == -1
        assert lib.fsg_lz4f_max_frame_length_flags(10, 4, flags) == 0
    for flags in (C.BSUM, C.NOSIZE, C.CSUM | C.BSUM, 8):   # the older call knows bit 0 alone
        assert lib.fsg_lz4f_compress_batch(p, p, p, 1, p, p, p, p, 4, flags, *args) == -1
    gpu.torch.cuda.synchronize()
    assert int(t.sum().item()) == 0


# ---- 3. decompress what the device wrote

def blocks_in(xs, bid):
    return sum(-(-len(x) // R.block_bytes(bid)) for x in xs)


@pytest.mark.parametrize("nosize_fast", (0, 1))
@pytest.mark.parametrize("flags", C.ALL_FLAGS)
def test_decompress_device_frames_routes_and_checksum_counts(gpu, bodies, fsg_opts, flags, nosize_fast):
    bid = 4
    frames, st, _ = device_frames(gpu, bodies, bid, flags)
    assert (st == fsg.FSG_OK).all()
    if nosize_fast:
        fsg_opts(lz4f_nosize_fast=1)
    outs, ol, dst, rep = gpu.decompress(frames, [len(x) for x in bodies])
    assert (dst == fsg.FSG_OK).all(), dst
    assert [int(v) for v in ol] == [len(x) for x in bodies]
    assert outs == bodies
    full = sum(1 for x in bodies if x)
    assert rep["empty_messages"] == len(bodies) - full
    sized = not flags & C.NOSIZE
    assert rep["fast_messages"] == (full if sized else 0)
    assert rep["fast_blocks"] == (blocks_in(bodies, bid) if sized else 0)
    assert rep["fast_nosize_messages"] == (full if not sized and nosize_fast else 0)
    assert rep["serial_no_size"] == (full if not sized and not nosize_fast else 0)
    assert rep["serial_rejected"] == 0 and rep["serial_linked"] == 0
    assert rep["checksummed_units"] == (blocks_in(bodies, bid) if flags & C.BSUM else 0) + \
        (len(bodies) if flags & C.CSUM else 0)


# ---- 4. checksum failures keep their verdict

def frame_fields(f: bytes):
    """(offsets of the block checksum words, (start, end) of the raw blocks'
    bytes, offset of the content checksum or None) of a well-formed frame."""
    st, hl, _, flg, _ = R.parse_header(f)
    assert st == R.OK
    bsum = 4 if flg & R.F_BSUM else 0
    ip, sums, raws = hl, [], []
    while True:
        word = int.from_bytes(f[ip:ip + 4], "little")
        ip += 4
        if word == 0:
            break
        sz = word & ~R.RAW
        if word & R.RAW:
            raws.append((ip, ip + sz))
        ip += sz
        if bsum:
            sums.append(ip)
            ip += 4
    return sums, raws, (ip if flg & R.F_CSUM else None)


def flip(f: bytes, at: int, bit: int = 3) -> bytes:
    g = bytearray(f)
    g[at] ^= 1 << bit
    return bytes(g)


@pytest.mark.parametrize("fast", (0, 1))
def test_checksum_failures_are_corrupt_by_the_serial_decoder(gpu, host, o, fsg_opts, fast):
    x = C.inputs()[-1]   # the raw-middle input: blocks compressed, raw, compressed, compressed at id 4
    cases = []           # (frame, on a fast route with the options off)
    for flags in (C.BSUM, C.CSUM, C.BSUM | C.CSUM | C.NOSIZE):
        f = host_compress(host, x, 4, flags)
        sums, raws, content = frame_fields(f)
        assert len(raws) == 1 and len(sums) == (4 if flags & C.BSUM else 0)
        muts = [flip(f, (raws[0][0] + raws[0][1]) // 2)]
        if sums:
            muts += [flip(f, sums[0] + 1), flip(f, sums[1] + 2)]   # a compressed block's word, the raw block's
        if content is not None:
            muts.append(flip(f, content))
        cases += [(g, not flags & C.NOSIZE) for g in muts]
    assert len(cases) == 3 + 2 + 4
    frames = [g for g, _ in cases]
    for g in frames:
        assert R.decode_frame(o, g, len(x))[:2] == (R.CORRUPT, 0)
        assert host_status(host, g, len(x)) == (R.CORRUPT, 0)
    if fast:
        fsg_opts(lz4f_nosize_fast=1, lz4f_linked_fast=1)
    outs, ol, st, rep = gpu.decompress(frames, [len(x)] * len(frames))
    assert [int(s) for s in st] == [fsg.FSG_CORRUPT] * len(frames)
    assert [int(v) for v in ol] == [0] * len(frames)
    # it was the serial decoder that judged them: no fast route answered
    assert rep["fast_messages"] == 0 and rep["fast_nosize_messages"] == 0 and rep["fast_linked_messages"] == 0
    pending = len(frames) if fast else sum(1 for _, s in cases if s)
    assert rep["serial_rejected"] == pending
    assert rep["serial_no_size"] == len(frames) - pending
