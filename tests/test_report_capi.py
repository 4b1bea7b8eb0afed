"""Path reports through the C ABI, host side only: the report functions are
pure host code (no HIP call), so the routing rule and the header parsing are
checked here without a GPU."""
import ctypes
import struct

import pytest

import fsg

INVALID_ARG = -1  # FSG_ERR_INVALID_ARG


@pytest.fixture(scope="module")
def lib():
    return fsg.load_gpu_lib()


def decode_report(lib, header, n, ws_bytes, flags=0):
    r = fsg.DecodeReport()
    rc = lib.fsg_decompress_report(header, n, ws_bytes, flags, ctypes.byref(r))
    return rc, {f: int(getattr(r, f)) for f, _ in r._fields_}


def encode_report(lib, header, n, max_in_len, ws_bytes):
    r = fsg.EncodeReport()
    rc = lib.fsg_compress_report(header, n, max_in_len, ws_bytes, ctypes.byref(r))
    return rc, {f: int(getattr(r, f)) for f, _ in r._fields_}


def test_error_code_matches_header():
    assert "#define FSG_ERR_INVALID_ARG -1\n" in fsg.HEADER.read_text()


def test_report_functions_exist(lib):
    for name in ("fsg_decompress_report", "fsg_compress_report", "fsg_lz4_decompress_report"):
        assert hasattr(lib, name), name
        assert name in fsg.header_symbols()
    assert lib.fsg_report_header_bytes() == 256


def test_decode_routing_without_workspace(lib):
    rc, r = decode_report(lib, None, 7, 0)
    assert rc == 0 and r["path"] == 2 and r["single_pass_messages"] == 7
    assert r["fallback_messages"] == 0 and r["bitmap_words_capacity"] == 0
    rc, r = decode_report(lib, None, 7, 0, fsg.FSG_FLAG_VALIDATE_ONLY)
    assert rc == 0 and r["path"] == 1 and r["single_pass_messages"] == 7
    # a workspace below the two-pass minimum (fsg_decompress_workspace_bytes(n, 0)) is none
    rc, r = decode_report(lib, None, 7, lib.fsg_decompress_workspace_bytes(7, 0))
    assert rc == 0 and r["path"] == 2 and r["single_pass_messages"] == 7


def test_decode_routing_forced(lib):
    ws = lib.fsg_decompress_workspace_bytes(7, 1)
    assert lib.fsg_select_kernels(3, 0) == 0
    try:
        for ws_bytes in (0, ws):
            rc, r = decode_report(lib, None, 7, ws_bytes)
            assert rc == 0 and r["path"] == 3 and r["single_pass_messages"] == 7
        # validate-only stays "by design" whatever is forced
        assert decode_report(lib, None, 7, ws, fsg.FSG_FLAG_VALIDATE_ONLY)[1]["path"] == 1
    finally:
        assert lib.fsg_select_kernels(0, 0) == 0
    assert decode_report(lib, None, 7, 0)[1]["path"] == 2


def test_decode_header_required_and_zero_header(lib):
    ws = lib.fsg_decompress_workspace_bytes(7, 1)
    for ws_bytes in (ws, ws + 4096):
        rc, _ = decode_report(lib, None, 7, ws_bytes)
        assert rc == INVALID_ARG
    zero = ctypes.create_string_buffer(256)
    rc, r = decode_report(lib, zero, 7, ws)
    assert rc == 0 and r["path"] == 0
    cap = r.pop("bitmap_words_capacity")
    assert cap >= 1 // 32 + 4 * 7 + 64
    assert all(v == 0 for v in r.values()), r
    # more workspace, more bitmap: 1 MiB of input is 32,768 words more
    rc, r2 = decode_report(lib, zero, 7, lib.fsg_decompress_workspace_bytes(7, 1 << 20))
    assert rc == 0 and r2["bitmap_words_capacity"] >= cap + (1 << 20) // 32 - 4


def test_decode_header_fields(lib):
    """Every field comes from its own slot: a header of distinct words."""
    ws = lib.fsg_decompress_workspace_bytes(1000, 1 << 20)
    words = list(range(1000, 1064))
    rc, r = decode_report(lib, ctypes.create_string_buffer(struct.pack("<64I", *words), 256), 1000, ws)
    assert rc == 0
    got = [r[k] for k in ("bitmap_words_requested", "large_messages", "huge_messages", "fallback_messages",
                          "fallback_bitmap", "fallback_wide_offsets", "fallback_pack_guard")]
    assert len(set(got)) == len(got) and all(1000 <= v < 1064 for v in got), r
    assert r["bitmap_words_requested"] == 1000  # the bump allocator is the first word


def test_encode_routing(lib):
    rc, r = encode_report(lib, None, 9, 4096, 0)
    assert rc == 0 and r["path"] == 2 and r["no_workspace_messages"] == 9
    ws = lib.fsg_compress_workspace_bytes(9, 4096)
    assert encode_report(lib, None, 9, 4096, ws)[0] == INVALID_ARG
    assert lib.fsg_select_kernels(0, 1) == 0
    try:
        rc, r = encode_report(lib, None, 9, 4096, ws)
        assert rc == 0 and r["path"] == 3 and r["no_workspace_messages"] == 9
    finally:
        assert lib.fsg_select_kernels(0, 0) == 0
    rc, r = encode_report(lib, ctypes.create_string_buffer(256), 9, 4096, ws)
    assert rc == 0 and r["path"] == 0 and all(v == 0 for v in r.values()), r


def test_encode_wave_units_follow_wave_quota(lib):
    n, max_in_len = 1000, 65536
    ws = lib.fsg_compress_workspace_bytes(n, max_in_len)
    saved = {k: fsg.get_option(k, lib) for k in ("encode_wave_share", "encode_wave_all_mb", "encode_wave_min")}
    try:
        fsg.set_option("encode_wave_share", 475, lib)
        fsg.set_option("encode_wave_all_mb", 640, lib)
        fsg.set_option("encode_wave_min", 16384, lib)
        bound = 640 << 20

        def header(unit_bytes, fallback=0):
            ctr = [0] * 64
            ctr[1], ctr[2] = 10, 3
            ctr[6], ctr[7] = unit_bytes & 0xffffffff, unit_bytes >> 32
            ctr[8] = fallback
            return ctypes.create_string_buffer(struct.pack("<64I", *ctr), 256)

        rc, r = encode_report(lib, header(bound + 1, fallback=2), n, max_in_len, ws)
        assert rc == 0 and r["path"] == 0
        assert r["units_listed"] == 10 and r["split_messages"] == 3 and r["unit_bytes"] == bound + 1
        assert r["fallback_messages"] == 2
        assert r["wave_units"] == -(-10 * 475 // 1000) == 5
        for below in (bound, bound - 1, 0):
            rc, r = encode_report(lib, header(below), n, max_in_len, ws)
            assert rc == 0 and r["wave_units"] == 10 and r["unit_bytes"] == below
        # 64-bit byte counts
        rc, r = encode_report(lib, header(5 << 32), n, max_in_len, ws)
        assert rc == 0 and r["unit_bytes"] == 5 << 32 and r["wave_units"] == 5
        # the wave encoder off: the lanes take every unit
        fsg.set_option("encode_wave_min", 0, lib)
        rc, r = encode_report(lib, header(0), n, max_in_len, ws)
        assert rc == 0 and r["units_listed"] == 10 and r["wave_units"] == 0
    finally:
        for k, v in saved.items():
            fsg.set_option(k, v, lib)


def test_lz4_routing(lib):
    r = fsg.DecodeReport()
    assert lib.fsg_lz4_decompress_report(None, 5, 0, ctypes.byref(r)) == 0
    assert r.path == 1 and r.single_pass_messages == 5
    ws = lib.fsg_lz4_decompress_workspace_bytes(5, 0)
    assert lib.fsg_lz4_decompress_report(None, 5, ws - 1, ctypes.byref(r)) == 0 and r.path == 1
    assert lib.fsg_lz4_decompress_report(None, 5, ws, ctypes.byref(r)) == INVALID_ARG
    hdr = ctypes.create_string_buffer(struct.pack("<4I", 40, 2, 2, 3), 256)
    assert lib.fsg_lz4_decompress_report(hdr, 5, ws, ctypes.byref(r)) == 0
    assert r.path == 0 and r.bitmap_words_requested == 40 and r.large_messages == 2
    assert r.fallback_messages == r.fallback_bitmap == 3
    assert r.bitmap_words_capacity == 4 * 5 + 4  # the two-pass minimum: 4 words per message + 4


def test_lz4_compress_routing(lib):
    """Route and wave_min are the plan's (csrc/lz4_plan.h): the wave encoder up
    to 256 bodies, the lanes alone on a workspace of the tables."""
    r = fsg.Lz4EncodeReport()
    zero = ctypes.create_string_buffer(256)
    for n, wave_min in ((256, 8192), (257, 0xFFFFFFFF)):
        ws = lib.fsg_lz4_compress_workspace_bytes(n)
        assert ws == 256 + -(-4 * n // 256) * 256 + 16384 * n
        assert lib.fsg_lz4_compress_report(None, n, ws, ctypes.byref(r)) == INVALID_ARG
        assert lib.fsg_lz4_compress_report(zero, n, ws, ctypes.byref(r)) == 0
        assert r.path == 0 and r.wave_min == wave_min and r.lane_messages == n and r.wave_messages == 0
        assert lib.fsg_lz4_compress_report(None, n, ws - 1, ctypes.byref(r)) == 0
        assert r.path == 1 and r.wave_min == 0xFFFFFFFF and r.lane_messages == n


def test_lz4f_block_entries(lib):
    """The frame reports' block_entries is the plan's capacity
    (csrc/lz4_frame_plan.h): 0 and an invalid argument below the size for no
    input, then an entry per message and per block the workspace was sized for."""
    zero = ctypes.create_string_buffer(256)
    d = fsg.Lz4fDecodeReport()
    lo = lib.fsg_lz4f_decompress_workspace_bytes(1, 0)
    assert lo == 3072
    assert lib.fsg_lz4f_decompress_report(zero, 1, lo - 1, ctypes.byref(d)) == INVALID_ARG and d.block_entries == 0
    assert lib.fsg_lz4f_decompress_report(None, 1, lo, ctypes.byref(d)) == INVALID_ARG
    assert lib.fsg_lz4f_decompress_report(zero, 1, lo, ctypes.byref(d)) == 0 and d.block_entries == 1
    ws = lib.fsg_lz4f_decompress_workspace_bytes(1, 1 << 20)
    assert lib.fsg_lz4f_decompress_report(zero, 1, ws, ctypes.byref(d)) == 0 and d.block_entries == 1 + (1 << 20) // 256
    e = fsg.Lz4fEncodeReport()
    for n, total, entries, wave_min in ((1, 255 << 16, 256, 8192), (1, 256 << 16, 257, 0xFFFFFFFF)):
        ws = lib.fsg_lz4f_compress_workspace_bytes(n, total, 4)
        assert lib.fsg_lz4f_compress_report(zero, n, ws, 4, ctypes.byref(e)) == 0
        assert e.block_entries == entries and e.block_wave_min == wave_min
    assert lib.fsg_lz4f_compress_report(zero, 1, lib.fsg_lz4f_compress_workspace_bytes(1, 0, 4) - 1, 4,
                                        ctypes.byref(e)) == INVALID_ARG and e.block_entries == 0
    assert lib.fsg_lz4f_compress_report(zero, 1, 1 << 20, 3, ctypes.byref(e)) == INVALID_ARG


def test_null_out_is_invalid(lib):
    zero = ctypes.create_string_buffer(256)
    assert lib.fsg_decompress_report(zero, 7, 0, 0, None) == INVALID_ARG
    assert lib.fsg_compress_report(zero, 7, 4096, 0, None) == INVALID_ARG
    assert lib.fsg_lz4_decompress_report(zero, 7, 0, None) == INVALID_ARG
