"""C-ABI checks that need no GPU: the library loads, exports every symbol
include/flare_snappy_gpu.h declares, and its host-side helpers agree with the
oracle (no compute calls are made without a GPU)."""
import ctypes
import json
import re
from pathlib import Path

import pytest

import fsg
from bind import Oracle

GOLDEN = Path(__file__).resolve().parent / "golden"


def test_header_declares_expected_entry_points():
    syms = fsg.header_symbols()
    for s in ("fsg_compress_batch", "fsg_decompress_batch", "fsg_max_compressed_length",
              "fsg_get_uncompressed_length", "fsg_init", "fsg_decompress_batch_partial",
              "fsg_decompress_batch_iovec"):
        assert s in syms


def test_library_exports_every_declared_symbol():
    lib = fsg.load_gpu_lib()
    missing = [s for s in fsg.header_symbols() if not hasattr(lib, s)]
    assert not missing, missing
    assert lib.fsg_version().decode().startswith("flare-snappy-gpu")


def test_max_compressed_length_matches_oracle():
    lib = fsg.load_gpu_lib()
    o = Oracle()
    for n in (0, 1, 7, 4096, 65536, 1 << 20, (1 << 32) - 1):
        assert lib.fsg_max_compressed_length(n) == o.max_compressed_length(n) == 32 + n + n // 6


@pytest.mark.parametrize("lenient", [1, 0])
def test_host_header_parse_matches_golden(lenient):
    lib = fsg.load_gpu_lib()
    for v in json.loads((GOLDEN / "negative.json").read_text()):
        b = bytes.fromhex(v["hex"])
        u = ctypes.c_uint32(0)
        buf = ctypes.create_string_buffer(b, max(1, len(b)))
        h = lib.fsg_get_uncompressed_length(buf, len(b), ctypes.byref(u), lenient)
        expect = v["header_ok"] if lenient else v["strict_header_ok"]
        assert bool(h) == expect, v["name"]
        if h and lenient:
            assert u.value == v["ulen"]


def test_invalid_arguments_rejected_without_gpu():
    lib = fsg.load_gpu_lib()
    # null device pointers with n > 0 are rejected before any HIP call
    rc = lib.fsg_compress_batch(None, None, None, 5, 0, None, None, None, None, None, 0, None)
    assert rc == -1
    rc = lib.fsg_decompress_batch(None, None, None, 5, None, None, None, None, None, 0, None, 0, None)
    assert rc == -1
    rc = lib.fsg_decompress_batch_partial(None, None, None, 5, 0, None, None, None, None, None, None, None, 0, None)
    assert rc == -1
    rc = lib.fsg_decompress_batch_iovec(None, None, None, 5, None, None, None, None, None, None, None, None, None,
                                        0, None)
    assert rc == -1


def test_option_calls():
    """fsg_set_option / fsg_get_option / fsg_default_option: known names round
    trip, unknown names and null outputs are rejected, defaults are the
    built-in ones (the environment is read once at load, never per call)."""
    lib = fsg.load_gpu_lib()
    names = ["decode_fork", "split_walk", "split_class", "exec_keep", "chunked_huge", "small_persist",
             "small_batch", "split_huge", "walk_order", "lean_walk", "exec_big_blocks", "exec_prio",
             "exec_big_blocks_fork", "exec_pack", "encode_wave_min", "encode_wave_share",
             "encode_wave_all_mb", "encode_lanes", "encode_wave_per_cu", "encode_wave_wg",
             "lz4_big_min", "lz4_encode_wave_min", "lz4_encode_wave_per_cu", "lz4f_force_serial",
             "lz4f_block_wave_min", "lz4f_nosize_fast", "lz4f_length_wave_min", "lz4f_linked_fast"]
    # every row of the option table (capi.hip kOptDesc: {"name", "FSG_ENV", default}), in its order
    capi = (Path(__file__).resolve().parents[1] / "flare-cpp_amd" / "csrc" / "capi.hip").read_text()
    table = re.findall(r'^\s*\{"([a-z0-9_]+)",\s*"FSG_[A-Z0-9_]+",\s*-?\d+\},', capi, flags=re.M)
    assert table == names
    # ... and the header's list (include/flare_snappy_gpu.h, above fsg_set_option) names each
    header = fsg.HEADER.read_text()
    doc = header[header.index("Process-wide tuning and test options"):header.index("int fsg_set_option(")]
    listed = set(re.findall(r"[a-z][a-z0-9_]+", doc))
    assert not [n for n in names if n not in listed]
    v = ctypes.c_int64(0)
    for n in names:
        assert lib.fsg_default_option(n.encode(), ctypes.byref(v)) == 0, n
        with fsg.options(**{n: 12345}):
            assert fsg.get_option(n) == 12345
        assert fsg.get_option(n) != 12345
    assert lib.fsg_set_option(b"no_such_option", 1) == -1
    assert lib.fsg_get_option(b"no_such_option", ctypes.byref(v)) == -1
    assert lib.fsg_get_option(b"split_walk", None) == -1
    assert lib.fsg_set_option(None, 1) == -1
    assert lib.fsg_default_option(b"split_walk", ctypes.byref(v)) == 0 and v.value == 3
    assert lib.fsg_default_option(b"decode_fork", ctypes.byref(v)) == 0 and v.value == -1


def test_decode_launch_reads_no_environment():
    """The drop-in's launch paths take their knobs from the option table:
    no getenv in the HIP sources or the headers they include outside
    capi.hip's load-time read."""
    src = Path(__file__).resolve().parents[1] / "flare-cpp_amd" / "csrc"
    files = sorted(src.glob("*.hip")) + sorted(src.glob("*.h"))
    assert any(f.name == "capi.hip" for f in files) and any(f.suffix == ".h" for f in files)
    for f in files:
        text = f.read_text()
        if f.name == "capi.hip":
            assert text.count("getenv(") == 2  # env_int (kernel variants) + the option table's one-time read
        else:
            assert "getenv(" not in text, f.name
