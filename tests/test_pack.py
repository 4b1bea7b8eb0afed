"""fsg_pack_batch without a GPU: the layout rule (fsg.pack_offsets), the
argument checks that come before any HIP call, the workspace size, and the
symbols in the header and the library."""
import re
from pathlib import Path

import numpy as np
import pytest

import fsg

REPO = Path(__file__).resolve().parents[1]
P = 0x1000  # a non-null stand-in for a device pointer: rejected calls never touch it


def _loop_offsets(lens, status, align):
    offs, pos = [], 0
    for i, n in enumerate(lens):
        offs.append(pos)
        eff = 0 if status is not None and status[i] != 0 else int(n)
        pos += (eff + align - 1) // align * align
    return offs, pos


@pytest.mark.parametrize("align", [1, 4, 16, 64])
@pytest.mark.parametrize("masked", [False, True])
def test_pack_offsets_matches_a_plain_loop(align, masked):
    rng = np.random.default_rng(align * 2 + masked)
    for n in (0, 1, 2, 17, 1000):
        lens = rng.integers(0, 300, n).astype(np.uint32)
        lens[rng.random(n) < 0.2] = 0
        status = rng.integers(0, 5, n).astype(np.int32) if masked else None
        offs, total = fsg.pack_offsets(lens, status, align)
        eo, et = _loop_offsets(lens, status, align)
        assert offs.dtype == np.uint64 and offs.tolist() == eo and total == et


def test_pack_offsets_is_exact_in_u64():
    lens = np.full(4096, 0xFFFFFFF0, np.uint32)
    offs, total = fsg.pack_offsets(lens, None, 16)
    assert total == 4096 * 0xFFFFFFF0
    assert int(offs[-1]) == 4095 * 0xFFFFFFF0
    assert fsg.pack_offsets(np.array([0xFFFFFFFF], np.uint32), None, 256)[1] == 1 << 32


def test_pack_batch_rejects_bad_arguments_without_gpu():
    lib = fsg.load_gpu_lib()
    ws = lib.fsg_pack_workspace_bytes(5)
    good = [P, P, P, None, 5, 16, P, P, P, P, ws, None]
    # null pointers with n = 5
    assert lib.fsg_pack_batch(None, None, None, None, 5, 16, None, None, None, None, 0, None) == -1
    for k in (0, 1, 2, 7, 8, 9):  # d_src, d_src_off, d_len, d_pack_off, d_total, d_workspace
        args = list(good)
        args[k] = None
        assert lib.fsg_pack_batch(*args) == -1, k
    # align: a power of two from 1 to 256
    for align in (0, 3, 512):
        args = list(good)
        args[5] = align
        assert lib.fsg_pack_batch(*args) == -1, align
    # a short workspace
    n = 5000
    need = lib.fsg_pack_workspace_bytes(n)
    for short in (0, need - 1):
        assert lib.fsg_pack_batch(P, P, P, None, n, 16, P, P, P, P, short, None) == -1


def test_pack_workspace_bytes():
    lib = fsg.load_gpu_lib()
    assert lib.fsg_pack_workspace_bytes(0) >= 8
    sizes = [lib.fsg_pack_workspace_bytes(n) for n in
             (0, 1, 1023, 1024, 1025, 5000, 1 << 20, (1 << 20) + 1, 1 << 24, 1 << 31, (1 << 32) - 1)]
    assert sizes == sorted(sizes)
    assert sizes[-1] > sizes[0]


def test_header_declares_and_library_exports_pack():
    syms = fsg.header_symbols(fsg.HEADER)
    lib = fsg.load_gpu_lib()
    for s in ("fsg_pack_workspace_bytes", "fsg_pack_batch"):
        assert s in syms
        assert hasattr(lib, s)


def test_binding_constants_match_the_kernels():
    """fsg.PACK_SCAN_BLOCK / PACK_TILE_BYTES (the GPU tests size their cases
    around them) are pack.hip's."""
    text = (REPO / "flare-cpp_amd" / "csrc" / "pack.hip").read_text()
    threads = int(re.search(r"kPackScanThreads = (\d+);", text).group(1))
    per = int(re.search(r"kPackScanPerThread = (\d+);", text).group(1))
    assert "kPackScanBlock = kPackScanThreads * kPackScanPerThread;" in text
    assert fsg.PACK_SCAN_BLOCK == threads * per
    assert fsg.PACK_TILE_BYTES == int(re.search(r"kPackTileBytes = (\d+);", text).group(1))
