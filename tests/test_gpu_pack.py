"""fsg_pack_batch on the GPU (flare-cpp_amd/csrc/pack.hip): the offsets, the
total and every destination byte against fsg.pack_offsets and the sources.
The destination is poisoned with 0xA5 and carries 64 guard bytes past the
total: every byte outside the packed ranges must still be 0xA5 afterwards
(alignment padding is not written, nothing is written from the total on)."""
import json
from pathlib import Path

import numpy as np
import pytest

import fsg
from gen_inputs import build_input

pytestmark = pytest.mark.gpu
GOLDEN = Path(__file__).resolve().parent / "golden"
POISON = 0xA5
GUARD = 64
T = fsg.PACK_TILE_BYTES   # a tile of the copy kernel (a wave takes 4 consecutive ones at a time)
B = fsg.PACK_SCAN_BLOCK   # items per workgroup of the offset scan


@pytest.fixture(scope="module")
def codec():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test run without a visible GPU")
    return fsg.SnappyGPU(torch.cuda.current_device())


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.size == 0:
        a = np.zeros(1, a.dtype)
    return torch.from_numpy(a).cuda()


def _expected(src, src_off, lens, status, align):
    """The packed buffer with its guard, from the rule alone."""
    offs, total = fsg.pack_offsets(lens, status, align)
    eff = np.asarray(lens).astype(np.int64)
    if status is not None:
        eff = np.where(np.asarray(status) != fsg.FSG_OK, 0, eff)
    exp = np.full(total + GUARD, POISON, np.uint8)
    k = int(eff.sum())
    if k:
        within = np.arange(k, dtype=np.int64) - np.repeat(np.cumsum(eff) - eff, eff)
        exp[np.repeat(offs.astype(np.int64), eff) + within] = src[np.repeat(src_off.astype(np.int64), eff) + within]
    return offs, total, exp


def _pack(codec, src, src_off, lens, status=None, align=16, copy=True, dst_bytes=None):
    """Runs fsg_pack_batch; returns (pack_off, total, destination with guard or None)."""
    import torch
    n = len(lens)
    d_src = _dev(src) if copy else None
    d_so = _dev(np.asarray(src_off, np.uint64)) if copy else None
    d_len = _dev(np.asarray(lens, np.uint32))
    d_st = None if status is None else _dev(np.asarray(status, np.int32))
    if dst_bytes is None:
        dst_bytes = fsg.pack_offsets(lens, status, align)[1] + GUARD
    d_dst = torch.full((dst_bytes,), POISON, dtype=torch.uint8, device="cuda") if copy else None
    d_po = torch.full((max(n, 1),), -1, dtype=torch.int64, device="cuda")
    d_tot = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    ws = codec.pack_workspace(n)
    ws.fill_(0x5A)  # scratch: nothing may depend on its content
    codec.pack(d_src, d_so, d_len, n, d_dst, d_po, d_tot, ws, d_status=d_st, align=align)
    torch.cuda.synchronize()
    po = d_po.cpu().numpy().view(np.uint64)[:n]
    total = int(d_tot.cpu().numpy().view(np.uint64)[0])
    return po, total, (d_dst.cpu().numpy() if copy else None)


def _check(codec, src, src_off, lens, status=None, align=16):
    offs, total, exp = _expected(src, src_off, lens, status, align)
    po, tot, dst = _pack(codec, src, src_off, lens, status, align)
    assert tot == total
    assert np.array_equal(po, offs)
    assert dst.size == exp.size
    bad = np.flatnonzero(dst != exp)
    assert bad.size == 0, f"first differing byte at {bad[0]} of {total} (+{GUARD} guard): {dst[bad[0]]:#x} != {exp[bad[0]]:#x}"


def _slots(rng, lens, align=1, shift=0):
    """Source slots with some slack each, `align`-aligned, moved by `shift`
    bytes; the source buffer holds random bytes (never the poison value, so a
    copied byte cannot pass for an untouched one)."""
    lens = np.asarray(lens, np.uint32)
    caps = lens.astype(np.uint64) + rng.integers(0, 6, len(lens)).astype(np.uint64)
    offs, tot = fsg.slot_offsets(caps, align=align) if len(lens) else (np.zeros(0, np.uint64), align)
    src = rng.integers(0, POISON, tot + shift + 16, dtype=np.uint8)
    return src, offs + np.uint64(shift)


@pytest.mark.parametrize("n", [0, 1, 2, 64, 65])
@pytest.mark.parametrize("align", [1, 16])
def test_edge_lengths(codec, n, align):
    rng = np.random.default_rng(100 + n)
    for lens in (rng.choice([0, 1, 15, 16, 17, 31, 33], n), np.zeros(n, np.int64)):
        src, so = _slots(rng, lens)
        _check(codec, src, so, lens, align=align)


@pytest.mark.parametrize("align", [1, 4, 16, 64])
def test_alignment_and_source_residues(codec, align):
    """Sources at every residue mod 16 against destinations of every `align`:
    the 16-byte loads are misaligned relative to the stores in most cases."""
    rng = np.random.default_rng(7 + align)
    lens = rng.integers(0, 201, 300)
    for shift in range(16):
        src, so = _slots(rng, lens, align=1, shift=shift)
        _check(codec, src, so, lens, align=align)


@pytest.mark.parametrize("align", [1, 16])
def test_tile_edges(codec, align):
    rng = np.random.default_rng(11)
    for L in (T - 1, T, T + 1, 2 * T - 1, 2 * T + 1, 4 * T - 1, 4 * T, 4 * T + 1):  # a wave takes 4 tiles at a time
        for lens in ([L], [L, L], [3, L, 0, L, 5]):
            src, so = _slots(rng, lens)
            _check(codec, src, so, lens, align=align)
    # one body of 1 MiB + 3 among 500 bodies of 1..40 bytes
    lens = rng.integers(1, 41, 501)
    lens[250] = (1 << 20) + 3
    src, so = _slots(rng, lens)
    _check(codec, src, so, lens, align=align)


@pytest.mark.parametrize("n", [B - 1, B, B + 1, B * B + 1, 1_200_000])
def test_scan_levels(codec, n):
    """One workgroup, two, and (from B * B + 1 items on) the recursive level."""
    rng = np.random.default_rng(n)
    lens = rng.integers(0, 17, n)
    src, so = _slots(rng, lens)
    _check(codec, src, so, lens, align=4 if n == 1_200_000 else 16)


def test_wide_totals(codec):
    """Offsets only (no destination): 4,096 lengths of 0xFFFFFFF0 add up past
    2^43; the total and every offset are exact in u64."""
    lens = np.full(4096, 0xFFFFFFF0, np.uint32)
    offs, total = fsg.pack_offsets(lens, None, 16)
    assert total == 4096 * 0xFFFFFFF0 > 1 << 43
    po, tot, _ = _pack(codec, None, None, lens, None, 16, copy=False)
    assert tot == total
    assert np.array_equal(po, offs)


def test_status_mask(codec):
    rng = np.random.default_rng(5)
    lens = rng.integers(0, 301, 1000)
    status = rng.integers(0, 5, 1000)
    src, so = _slots(rng, lens)
    for align in (1, 16):
        _check(codec, src, so, lens, status, align)
    # every message masked: total 0, nothing written at all
    status = rng.integers(1, 5, 1000)
    po, tot, dst = _pack(codec, src, so, lens, status, 16, dst_bytes=4096)
    assert tot == 0 and not po.any()
    assert (dst == POISON).all()


def _device_compress(codec, items, lz4, stream=None):
    """The batch through fsg_compress_batch / fsg_lz4_compress_batch, results
    left on the device in their worst-case slots."""
    import torch
    b = fsg.Batch.from_list(items)
    n = len(b)
    bound = codec.lib.fsg_lz4_max_compressed_length if lz4 else fsg.max_compressed_length
    caps = np.array([bound(int(x)) for x in b.lens], dtype=np.uint64)
    oo, tot = fsg.slot_offsets(caps)
    d = dict(n=n, oo=oo, tot=tot, d_in=_dev(b.data), d_io=_dev(b.offsets), d_il=_dev(b.lens), d_oo=_dev(oo),
             d_out=torch.full((tot,), POISON, dtype=torch.uint8, device="cuda"),
             d_ol=torch.zeros(n, dtype=torch.int32, device="cuda"),
             d_st=torch.full((n,), -7, dtype=torch.int32, device="cuda"))
    mx = int(b.lens.max())
    d["ws"] = codec.lz4_compress_workspace(n) if lz4 else codec.compress_workspace(n, mx)
    d["d_dst"] = torch.full((tot + GUARD,), POISON, dtype=torch.uint8, device="cuda")
    d["d_po"] = torch.full((n,), -1, dtype=torch.int64, device="cuda")
    d["d_tot"] = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    d["pws"] = codec.pack_workspace(n)
    torch.cuda.synchronize()  # uploads done before any other stream touches them

    def run(stream=None):
        if lz4:
            codec.lz4_compress(d["d_in"], d["d_io"], d["d_il"], n, d["d_out"], d["d_oo"], d["d_ol"], d["d_st"],
                               d["ws"], stream=stream)
        else:
            codec.compress(d["d_in"], d["d_io"], d["d_il"], n, mx, d["d_out"], d["d_oo"], d["d_ol"], d["d_st"],
                           stream=stream, workspace=d["ws"])
        # queued right behind the encoder, no synchronisation in between
        codec.pack(d["d_out"], d["d_oo"], d["d_ol"], n, d["d_dst"], d["d_po"], d["d_tot"], d["pws"],
                   d_status=d["d_st"], align=16, stream=stream)

    d["run"] = run
    return d


def _packed_bodies(d):
    n = d["n"]
    ol = d["d_ol"].cpu().numpy().view(np.uint32)
    st = d["d_st"].cpu().numpy()
    assert (st == fsg.FSG_OK).all()
    po = d["d_po"].cpu().numpy().view(np.uint64)
    offs, total = fsg.pack_offsets(ol, st, 16)
    assert int(d["d_tot"].cpu().numpy().view(np.uint64)[0]) == total
    assert np.array_equal(po, offs)
    dst = d["d_dst"].cpu().numpy()
    assert (dst[total:] == POISON).all()
    for i in range(n):  # the padding behind each body
        assert (dst[int(po[i]) + int(ol[i]):int(po[i]) + (int(ol[i]) + 15) // 16 * 16] == POISON).all(), i
    return [dst[int(po[i]):int(po[i]) + int(ol[i])].tobytes() for i in range(n)], ol


def test_snappy_outputs_pack_and_decode_from_the_packed_buffer(codec):
    """The 171 golden inputs through fsg_compress_batch, then packed: every
    packed body is the reference's compressed stream, and the packed buffer
    (offsets = pack_off) decodes back to the inputs."""
    import torch
    vecs = json.loads((GOLDEN / "vectors.json").read_text())
    assert len(vecs) == 171
    items = [build_input(v) for v in vecs]
    d = _device_compress(codec, items, lz4=False)
    d["run"]()
    torch.cuda.synchronize()
    bodies, ol = _packed_bodies(d)
    for v, c in zip(vecs, bodies):
        assert len(c) == int(v["compressed_len"]), v["name"]
        assert "%016x" % fsg.fnv1a64(c) == v["compressed_fnv"], v["name"]
        if "compressed_hex" in v:
            assert c.hex() == v["compressed_hex"], v["name"]
    # decode straight from the packed buffer
    n = d["n"]
    caps = np.array([len(x) for x in items], np.uint32)
    uo, utot = fsg.slot_offsets(caps.astype(np.uint64))
    d_u = torch.full((utot,), POISON, dtype=torch.uint8, device="cuda")
    d_ul = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_ust = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    total_in = int(d["d_tot"].cpu().numpy()[0])
    ws = codec.decompress_workspace(n, total_in)
    codec.decompress(d["d_dst"], d["d_po"], d["d_ol"], n, d_u, _dev(uo), _dev(caps), d_ul, d_ust, workspace=ws)
    torch.cuda.synchronize()
    assert (d_ust.cpu().numpy() == fsg.FSG_OK).all()
    u = d_u.cpu().numpy()
    for i, x in enumerate(items):
        assert u[int(uo[i]):int(uo[i]) + len(x)].tobytes() == x, vecs[i]["name"]


def test_lz4_outputs_pack_and_decode_from_the_packed_buffer(codec):
    """The same call packs LZ4 bodies (varint length + block) against the
    liblz4 fixtures, and the packed buffer decodes."""
    import torch
    vecs = [v for v in json.loads((GOLDEN / "lz4_vectors.json").read_text())["compress"]
            if int(v["input_len"]) <= 1 << 20]
    items = [build_input(v) for v in vecs]
    d = _device_compress(codec, items, lz4=True)
    d["run"]()
    torch.cuda.synchronize()
    bodies, ol = _packed_bodies(d)
    for v, x, body in zip(vecs, items, bodies):
        blk = body[len(body) - int(v["block_len"]):]
        assert len(body) > int(v["block_len"]), v["name"]
        assert "%016x" % fsg.fnv1a64(blk) == v["block_fnv"], v["name"]
    n = d["n"]
    caps = np.array([len(x) for x in items], np.uint32)
    uo, utot = fsg.slot_offsets(caps.astype(np.uint64))
    d_u = torch.full((utot,), POISON, dtype=torch.uint8, device="cuda")
    d_ul = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_ust = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    codec.lz4_decompress(d["d_dst"], d["d_po"], d["d_ol"], n, d_u, _dev(uo), _dev(caps), d_ul, d_ust)
    torch.cuda.synchronize()
    assert (d_ust.cpu().numpy() == fsg.FSG_OK).all()
    u = d_u.cpu().numpy()
    for i, x in enumerate(items):
        assert u[int(uo[i]):int(uo[i]) + len(x)].tobytes() == x, vecs[i]["name"]


def test_stream_order(codec):
    """Compress and pack queued back to back on one non-default stream: the
    pack sees the encoder's lengths, statuses and bytes without any
    synchronisation in between."""
    import torch
    sizes = [70000, 0, 1, 4096, 65536, 200000, 33, 15] * 8
    items = [fsg.make_batch(fsg.KIND_TEXT, [s], first_index=i).item(0) for i, s in enumerate(sizes)]
    ref = _device_compress(codec, items, lz4=False)
    ref["run"]()
    torch.cuda.synchronize()
    expect, _ = _packed_bodies(ref)
    d = _device_compress(codec, items, lz4=False)
    s = torch.cuda.Stream()
    d["run"](stream=s)
    s.synchronize()
    got, _ = _packed_bodies(d)
    assert got == expect
    from bind import Oracle
    o = Oracle()
    for x, c in zip(items[:8], got[:8]):
        assert c == o.compress(x)
