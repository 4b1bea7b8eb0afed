"""ctypes binding of libflare_snappy_gpu.so (include/flare_snappy_gpu.h) and of
the synthetic-data generator, for the Python test suite and bench.py.

The product path is the C ABI; this module only marshals device pointers
(torch tensors on cuda:N are used as plain device allocations) and never
falls back to anything else: if the HIP library is missing, loading raises.
"""
from __future__ import annotations

import ctypes
import os
from pathlib import Path

import numpy as np

PKG_DIR = Path(__file__).resolve().parents[1]
LIB_DIR = PKG_DIR / "lib"
REPO_DIR = PKG_DIR.parent
HEADER = REPO_DIR / "include" / "flare_snappy_gpu.h"
HEADERS = (HEADER, REPO_DIR / "include" / "flare_lz4_gpu.h", REPO_DIR / "include" / "flare_deflate_gpu.h",
           REPO_DIR / "include" / "flare_deflate_compress_gpu.h", REPO_DIR / "include" / "flare_deflate_level_gpu.h",
           REPO_DIR / "include" / "flare_deflate_index_gpu.h")

FSG_OK, FSG_CORRUPT, FSG_BAD_HEADER, FSG_SLOT_TOO_SMALL, FSG_IOV_TOO_SMALL = 0, 1, 2, 3, 4
FSG_FLAG_VALIDATE_ONLY, FSG_FLAG_STRICT_HEADER = 1, 2

_c = ctypes
_vp, _sz, _u32, _u64, _i32 = _c.c_void_p, _c.c_size_t, _c.c_uint32, _c.c_uint64, _c.c_int32



def _report_struct(name, fields):
    return type(name, (_c.Structure,), {"_fields_": [(f, _u64) for f in fields]})


# struct fsg_decode_report / fsg_encode_report (include/flare_snappy_gpu.h)
DecodeReport = _report_struct("DecodeReport", (
    "path", "single_pass_messages", "fallback_messages", "fallback_bitmap", "fallback_wide_offsets",
    "fallback_pack_guard", "bitmap_words_requested", "bitmap_words_capacity", "large_messages", "huge_messages"))
EncodeReport = _report_struct("EncodeReport", (
    "path", "no_workspace_messages", "units_listed", "split_messages", "unit_bytes", "wave_units",
    "fallback_messages"))
# struct fsg_lz4_encode_report (include/flare_lz4_gpu.h)
Lz4EncodeReport = _report_struct("Lz4EncodeReport", (
    "path", "lane_messages", "wave_messages", "wave_bytes", "wave_min"))
# struct fsg_lz4f_encode_report / fsg_lz4f_decode_report (include/flare_lz4_gpu.h, "LZ4 frames")
Lz4fEncodeReport = _report_struct("Lz4fEncodeReport", (
    "blocks", "raw_blocks", "overflow_messages", "block_entries", "block_wave_min"))
Lz4fDecodeReport = _report_struct("Lz4fDecodeReport", (
    "fast_messages", "fast_blocks", "empty_messages", "serial_linked", "serial_no_size", "serial_rejected",
    "serial_forced", "checksummed_units", "inner_fallback_blocks", "block_entries", "fast_nosize_messages",
    "fast_nosize_blocks", "fast_linked_messages", "fast_linked_blocks"))
LZ4F_NO_CONTENT_SIZE = 0xFFFFFFFFFFFFFFFF
# fsg_lz4f_compress_batch_flags' flags (FSG_LZ4F_FLAG_*)
LZ4F_FLAG_CONTENT_CHECKSUM, LZ4F_FLAG_BLOCK_CHECKSUMS, LZ4F_FLAG_NO_CONTENT_SIZE = 1, 2, 4
# struct fsg_deflate_report (include/flare_deflate_compress_gpu.h)
DeflateReport = _report_struct("DeflateReport", (
    "units", "stored_units", "fixed_units", "dynamic_units", "overflow_messages", "unit_entries"))
# fsg_inflate_batch's and fsg_deflate_batch's formats (FSG_INFLATE_* = FSG_DEFLATE_*, include/flare_deflate_gpu.h)
INFLATE_RAW, INFLATE_ZLIB, INFLATE_GZIP = 0, 1, 2
# fsg_deflate_batch_level's levels (FSG_DEFLATE_LEVEL_*, include/flare_deflate_level_gpu.h)
DEFLATE_LEVEL_STORED, DEFLATE_LEVEL_FAST, DEFLATE_LEVEL_BEST = 0, 1, 2
# fsg_deflate_batch_flags' flag and struct fsg_inflate_units_report (include/flare_deflate_index_gpu.h)
DEFLATE_FLAG_UNIT_INDEX = 1
InflateUnitsReport = _report_struct("InflateUnitsReport", (
    "parallel_messages", "parallel_units", "serial_no_index", "serial_unusable_index", "serial_unit_mismatch",
    "serial_workspace", "unit_entries"))
PATH_MAIN, PATH_SINGLE_DESIGN, PATH_NO_WORKSPACE, PATH_FORCED = 0, 1, 2, 3

_SIGS = {
    "fsg_report_header_bytes": (_sz, []),
    "fsg_decompress_report": (_c.c_int, [_vp, _u32, _sz, _u32, _c.POINTER(DecodeReport)]),
    "fsg_compress_report": (_c.c_int, [_vp, _u32, _u32, _sz, _c.POINTER(EncodeReport)]),
    "fsg_lz4_decompress_report": (_c.c_int, [_vp, _u32, _sz, _c.POINTER(DecodeReport)]),
    "fsg_lz4_compress_report": (_c.c_int, [_vp, _u32, _sz, _c.POINTER(Lz4EncodeReport)]),
    "fsg_version": (_c.c_char_p, []),
    "fsg_init": (_c.c_int, [_c.c_int]),
    "fsg_last_error": (_c.c_char_p, []),
    "fsg_select_kernels": (_c.c_int, [_c.c_int, _c.c_int]),
    "fsg_set_split_region_cap": (_c.c_int, [_u32]),
    "fsg_set_option": (_c.c_int, [_c.c_char_p, _c.c_int64]),
    "fsg_get_option": (_c.c_int, [_c.c_char_p, _c.POINTER(_c.c_int64)]),
    "fsg_default_option": (_c.c_int, [_c.c_char_p, _c.POINTER(_c.c_int64)]),
    "fsg_max_compressed_length": (_sz, [_sz]),
    "fsg_gather_blocks": (_c.c_int, [_vp, _vp, _vp, _u32, _vp, _vp]),
    "fsg_pack_workspace_bytes": (_sz, [_u32]),
    "fsg_pack_batch": (_c.c_int, [_vp, _vp, _vp, _vp, _u32, _u32, _vp, _vp, _vp, _vp, _sz, _vp]),
    "fsg_get_uncompressed_length": (_c.c_int, [_vp, _sz, _c.POINTER(_u32), _c.c_int]),
    "fsg_uncompressed_lengths_batch": (_c.c_int, [_vp, _vp, _vp, _u32, _vp, _c.c_int, _vp]),
    "fsg_compress_workspace_bytes": (_sz, [_u32, _u32]),
    "fsg_decompress_workspace_bytes": (_sz, [_u32, _u64]),
    "fsg_compress_batch": (_c.c_int, [_vp, _vp, _vp, _u32, _u32, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "fsg_decompress_batch": (_c.c_int, [_vp, _vp, _vp, _u32, _vp, _vp, _vp, _vp, _vp, _u32, _vp, _sz, _vp]),
    "fsg_decompress_batch_2s": (_c.c_int, [_vp, _vp, _vp, _u32, _vp, _vp, _vp, _vp, _vp, _u32, _vp, _sz, _vp,
                                           _vp]),
    "fsg_decompress_batch_partial": (_c.c_int, [_vp, _vp, _vp, _u32, _u32, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                                _sz, _vp]),
    "fsg_decompress_batch_iovec": (_c.c_int, [_vp, _vp, _vp, _u32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                              _sz, _vp]),
    "fsg_lz4_max_compressed_length": (_sz, [_sz]),
    "fsg_lz4_compress_workspace_bytes": (_sz, [_u32]),
    "fsg_lz4_compress_batch": (_c.c_int, [_vp, _vp, _vp, _u32, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "fsg_lz4_decompress_batch": (_c.c_int, [_vp, _vp, _vp, _u32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "fsg_lz4_decompress_workspace_bytes": (_sz, [_u32, _u64]),
    "fsg_lz4_decompress_batch_ws": (_c.c_int, [_vp, _vp, _vp, _u32, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "fsg_lz4_decompress_batch_2s": (_c.c_int, [_vp, _vp, _vp, _u32, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp,
                                               _vp]),
    "fsg_lz4f_max_frame_length": (_sz, [_sz, _u32]),
    "fsg_lz4f_max_frame_length_flags": (_sz, [_sz, _u32, _u32]),
    "fsg_lz4f_xxh32_batch": (_c.c_int, [_vp, _vp, _vp, _u32, _u32, _vp, _vp]),
    "fsg_lz4f_compress_workspace_bytes": (_sz, [_u32, _u64, _u32]),
    "fsg_lz4f_compress_batch": (_c.c_int, [_vp, _vp, _vp, _u32, _vp, _vp, _vp, _vp, _u32, _u32, _vp, _sz, _vp]),
    "fsg_lz4f_compress_batch_flags": (_c.c_int, [_vp, _vp, _vp, _u32, _vp, _vp, _vp, _vp, _u32, _u32, _vp, _sz, _vp]),
    "fsg_lz4f_decompress_workspace_bytes": (_sz, [_u32, _u64]),
    "fsg_lz4f_decompress_batch": (_c.c_int, [_vp, _vp, _vp, _u32, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "fsg_lz4f_content_sizes_batch": (_c.c_int, [_vp, _vp, _vp, _u32, _vp, _vp, _vp]),
    "fsg_lz4f_decoded_lengths_batch": (_c.c_int, [_vp, _vp, _vp, _u32, _vp, _vp, _vp, _sz, _vp]),
    "fsg_lz4f_compress_report": (_c.c_int, [_vp, _u32, _sz, _u32, _c.POINTER(Lz4fEncodeReport)]),
    "fsg_lz4f_decompress_report": (_c.c_int, [_vp, _u32, _sz, _c.POINTER(Lz4fDecodeReport)]),
    "fsg_inflate_batch": (_c.c_int, [_vp, _vp, _vp, _u32, _vp, _vp, _vp, _vp, _vp, _u32, _vp]),
    "fsg_inflate_lengths_batch": (_c.c_int, [_vp, _vp, _vp, _u32, _vp, _vp, _u32, _vp]),
    "fsg_crc32_batch": (_c.c_int, [_vp, _vp, _vp, _u32, _vp, _vp]),
    "fsg_adler32_batch": (_c.c_int, [_vp, _vp, _vp, _u32, _vp, _vp]),
    "fsg_deflate_max_length": (_sz, [_sz, _u32]),
    "fsg_deflate_workspace_bytes": (_sz, [_u32, _u64]),
    "fsg_deflate_batch": (_c.c_int, [_vp, _vp, _vp, _u32, _vp, _vp, _vp, _vp, _u32, _vp, _sz, _vp]),
    "fsg_deflate_report": (_c.c_int, [_vp, _u32, _sz, _c.POINTER(DeflateReport)]),
    "fsg_deflate_batch_level": (_c.c_int, [_vp, _vp, _vp, _u32, _vp, _vp, _vp, _vp, _u32, _u32, _vp, _sz, _vp]),
    "fsg_deflate_max_length_flags": (_sz, [_sz, _u32, _u32]),
    "fsg_deflate_batch_flags": (_c.c_int, [_vp, _vp, _vp, _u32, _vp, _vp, _vp, _vp, _u32, _u32, _u32, _vp, _sz, _vp]),
    "fsg_inflate_units_workspace_bytes": (_sz, [_u32, _u64]),
    "fsg_inflate_units_batch": (_c.c_int, [_vp, _vp, _vp, _u32, _vp, _vp, _vp, _vp, _vp, _u32, _vp, _sz, _vp]),
    "fsg_inflate_units_lengths_batch": (_c.c_int, [_vp, _vp, _vp, _u32, _vp, _vp, _u32, _vp, _sz, _vp]),
    "fsg_inflate_units_report": (_c.c_int, [_vp, _u32, _sz, _c.POINTER(InflateUnitsReport)]),
}


def header_symbols(header: Path | None = None) -> list[str]:
    """Every fsg_* function declared in include/flare_snappy_gpu.h,
    include/flare_lz4_gpu.h and include/flare_deflate_gpu.h (or in `header`)."""
    import re
    text = "".join(h.read_text() for h in ((header,) if header else HEADERS))
    return sorted(set(re.findall(r"\b(fsg_[a-z0-9_]+)\s*\(", text)))


# entry points an older library under A/B may lack
_OPTIONAL = {"fsg_decompress_batch_2s", "fsg_decompress_batch_partial", "fsg_decompress_batch_iovec", "fsg_lz4_decompress_batch_2s", "fsg_lz4_decompress_batch_ws",
             "fsg_lz4_decompress_workspace_bytes", "fsg_set_option", "fsg_get_option", "fsg_default_option",
             "fsg_pack_workspace_bytes", "fsg_pack_batch", "fsg_report_header_bytes", "fsg_decompress_report",
             "fsg_compress_report", "fsg_lz4_decompress_report", "fsg_lz4_compress_report",
             "fsg_lz4f_max_frame_length", "fsg_lz4f_compress_workspace_bytes", "fsg_lz4f_compress_batch",
             "fsg_lz4f_decompress_workspace_bytes", "fsg_lz4f_decompress_batch", "fsg_lz4f_content_sizes_batch",
             "fsg_lz4f_compress_report", "fsg_lz4f_decompress_report", "fsg_lz4f_decoded_lengths_batch",
             "fsg_lz4f_max_frame_length_flags", "fsg_lz4f_xxh32_batch", "fsg_lz4f_compress_batch_flags",
             "fsg_inflate_batch", "fsg_inflate_lengths_batch", "fsg_crc32_batch", "fsg_adler32_batch",
             "fsg_deflate_max_length", "fsg_deflate_workspace_bytes", "fsg_deflate_batch", "fsg_deflate_report",
             "fsg_deflate_batch_level", "fsg_deflate_max_length_flags", "fsg_deflate_batch_flags",
             "fsg_inflate_units_workspace_bytes", "fsg_inflate_units_batch", "fsg_inflate_units_lengths_batch",
             "fsg_inflate_units_report"}


def load_gpu_lib(path: Path | None = None) -> ctypes.CDLL:
    path = Path(path or os.environ.get("FSG_LIB", LIB_DIR / "libflare_snappy_gpu.so"))
    if not path.exists():
        raise RuntimeError(f"HIP codec library missing: {path} (run __graft_entry__.build())")
    lib = ctypes.CDLL(str(path))
    for name, (res, args) in _SIGS.items():
        if name in _OPTIONAL and not hasattr(lib, name):
            continue  # an older build under A/B (FSG_LIB)
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


def get_option(name: str, lib: ctypes.CDLL | None = None) -> int:
    """fsg_get_option: a process-wide tuning/test option (include/flare_snappy_gpu.h)."""
    lib = lib or load_gpu_lib()
    v = _c.c_int64(0)
    if lib.fsg_get_option(name.encode(), _c.byref(v)) != 0:
        raise KeyError(name)
    return v.value


def set_option(name: str, value: int, lib: ctypes.CDLL | None = None) -> None:
    lib = lib or load_gpu_lib()
    if lib.fsg_set_option(name.encode(), int(value)) != 0:
        raise KeyError(name)


class options:
    """Context manager: set library options for a block, restore them after.

        with fsg.options(decode_fork=1, split_walk=3): ...
    """

    def __init__(self, **kv):
        self.kv = kv
        self.saved = {}

    def __enter__(self):
        lib = load_gpu_lib()
        for k, v in self.kv.items():
            self.saved[k] = get_option(k, lib)
            set_option(k, v, lib)
        return self

    def __exit__(self, *exc):
        lib = load_gpu_lib()
        for k, v in self.saved.items():
            set_option(k, v, lib)
        return False


def _ptr(t) -> int | None:
    if t is None:
        return None
    return t.data_ptr()


class SnappyGPU:
    """Batched device codec through the C ABI.  Tensors must be on one cuda device."""

    def __init__(self, device: int = 0, lib_path: Path | None = None):
        self.lib = load_gpu_lib(lib_path)
        rc = self.lib.fsg_init(device)
        if rc != 0:
            raise RuntimeError(f"fsg_init({device}) = {rc}: {self.lib.fsg_last_error().decode()}")
        self.device = device

    def select_kernels(self, decode: int = 0, encode: int = 0):
        self._check(self.lib.fsg_select_kernels(decode, encode), "fsg_select_kernels")

    def _check(self, rc: int, what: str):
        if rc != 0:
            raise RuntimeError(f"{what} failed rc={rc}: {self.lib.fsg_last_error().decode()}")

    @staticmethod
    def _stream(stream) -> int | None:
        if stream is None:
            import torch
            return torch.cuda.current_stream().cuda_stream
        return stream.cuda_stream if hasattr(stream, "cuda_stream") else int(stream)

    def decompress_workspace(self, n, total_in=0, device=None):
        import torch
        nbytes = self.lib.fsg_decompress_workspace_bytes(n, total_in)
        return torch.zeros(max(nbytes, 1), dtype=torch.uint8, device=device or f"cuda:{self.device}")

    def set_split_region_cap(self, nbytes: int):
        self._check(self.lib.fsg_set_split_region_cap(nbytes), "fsg_set_split_region_cap")

    def compress_workspace(self, n, max_in_len, device=None):
        """Allocate the device workspace fsg_compress_batch wants (torch uint8)."""
        import torch
        nbytes = self.lib.fsg_compress_workspace_bytes(n, max_in_len)
        return torch.empty(max(nbytes, 1), dtype=torch.uint8, device=device or f"cuda:{self.device}")

    def compress(self, d_in, d_in_off, d_in_len, n, max_in_len, d_out, d_out_off, d_out_len,
                 d_status, stream=None, workspace=None):
        ws = 0 if workspace is None else workspace.numel() * workspace.element_size()
        self._check(self.lib.fsg_compress_batch(
            _ptr(d_in), _ptr(d_in_off), _ptr(d_in_len), n, max_in_len, _ptr(d_out),
            _ptr(d_out_off), _ptr(d_out_len), _ptr(d_status), _ptr(workspace), ws,
            self._stream(stream)), "fsg_compress_batch")

    def decompress(self, d_in, d_in_off, d_in_len, n, d_out, d_out_off, d_out_cap, d_out_len,
                   d_status, flags=0, stream=None, workspace=None, pass1_stream=None):
        """fsg_decompress_batch; with `pass1_stream`, fsg_decompress_batch_2s
        (the tag walk on pass1_stream, the execution on `stream`)."""
        ws = 0 if workspace is None else workspace.numel() * workspace.element_size()
        args = (_ptr(d_in), _ptr(d_in_off), _ptr(d_in_len), n, _ptr(d_out), _ptr(d_out_off),
                _ptr(d_out_cap), _ptr(d_out_len), _ptr(d_status), flags, _ptr(workspace), ws,
                self._stream(stream))
        if pass1_stream is None:
            self._check(self.lib.fsg_decompress_batch(*args), "fsg_decompress_batch")
        else:
            self._check(self.lib.fsg_decompress_batch_2s(*args, self._stream(pass1_stream)),
                        "fsg_decompress_batch_2s")

    def decompress_partial(self, d_in, d_in_off, d_in_len, n, frag, d_out, d_out_off, d_out_cap, d_got,
                           d_produced, d_status, stream=None, workspace=None):
        """fsg_decompress_batch_partial: UncompressAsMuchAsPossible per message
        (d_produced int64 / uint64, d_got int32 / uint32)."""
        ws = 0 if workspace is None else workspace.numel() * workspace.element_size()
        self._check(self.lib.fsg_decompress_batch_partial(
            _ptr(d_in), _ptr(d_in_off), _ptr(d_in_len), n, frag, _ptr(d_out), _ptr(d_out_off), _ptr(d_out_cap),
            _ptr(d_got), _ptr(d_produced), _ptr(d_status), _ptr(workspace), ws, self._stream(stream)),
            "fsg_decompress_batch_partial")

    def decompress_iovec(self, d_in, d_in_off, d_in_len, n, d_iov_base, d_iov_len, d_iov_first, d_stage,
                         d_stage_off, d_stage_cap, d_out_len, d_status, stream=None, workspace=None):
        """fsg_decompress_batch_iovec: RawUncompressToIOVec per message (d_iov_base:
        int64 device addresses, d_iov_len int64, d_iov_first int32 with n + 1 entries)."""
        ws = 0 if workspace is None else workspace.numel() * workspace.element_size()
        self._check(self.lib.fsg_decompress_batch_iovec(
            _ptr(d_in), _ptr(d_in_off), _ptr(d_in_len), n, _ptr(d_iov_base), _ptr(d_iov_len), _ptr(d_iov_first),
            _ptr(d_stage), _ptr(d_stage_off), _ptr(d_stage_cap), _ptr(d_out_len), _ptr(d_status), _ptr(workspace),
            ws, self._stream(stream)), "fsg_decompress_batch_iovec")

    # ---- LZ4 (include/flare_lz4_gpu.h)
    def lz4_compress_workspace(self, n, device=None):
        import torch
        nbytes = self.lib.fsg_lz4_compress_workspace_bytes(n)
        return torch.empty(max(nbytes, 1), dtype=torch.uint8, device=device or f"cuda:{self.device}")

    def lz4_compress(self, d_in, d_in_off, d_in_len, n, d_out, d_out_off, d_out_len, d_status, workspace,
                     stream=None):
        self._check(self.lib.fsg_lz4_compress_batch(
            _ptr(d_in), _ptr(d_in_off), _ptr(d_in_len), n, _ptr(d_out), _ptr(d_out_off), _ptr(d_out_len),
            _ptr(d_status), _ptr(workspace), workspace.numel(), self._stream(stream)), "fsg_lz4_compress_batch")

    def lz4_decompress_workspace(self, n, total_in_bytes, device=None):
        import torch
        if not hasattr(self.lib, "fsg_lz4_decompress_workspace_bytes"):
            return None  # an older library under A/B: the one-pass kernel runs
        nbytes = self.lib.fsg_lz4_decompress_workspace_bytes(n, total_in_bytes)
        return torch.empty(max(nbytes, 1), dtype=torch.uint8, device=device or f"cuda:{self.device}")

    def lz4_decompress(self, d_in, d_in_off, d_in_len, n, d_out, d_out_off, d_out_cap, d_out_len, d_status,
                       stream=None, workspace=None, pass1_stream=None):
        """workspace=None: the one-pass lane kernel; else the two-pass
        decoder (fsg_lz4_decompress_batch_ws; with `pass1_stream`,
        fsg_lz4_decompress_batch_2s: the index pass there, the execution on
        `stream`)."""
        if workspace is None or not hasattr(self.lib, "fsg_lz4_decompress_batch_ws"):
            self._check(self.lib.fsg_lz4_decompress_batch(
                _ptr(d_in), _ptr(d_in_off), _ptr(d_in_len), n, _ptr(d_out), _ptr(d_out_off), _ptr(d_out_cap),
                _ptr(d_out_len), _ptr(d_status), self._stream(stream)), "fsg_lz4_decompress_batch")
            return
        args = (_ptr(d_in), _ptr(d_in_off), _ptr(d_in_len), n, _ptr(d_out), _ptr(d_out_off), _ptr(d_out_cap),
                _ptr(d_out_len), _ptr(d_status), _ptr(workspace), workspace.numel(), self._stream(stream))
        if pass1_stream is None:
            self._check(self.lib.fsg_lz4_decompress_batch_ws(*args), "fsg_lz4_decompress_batch_ws")
        else:
            self._check(self.lib.fsg_lz4_decompress_batch_2s(*args, self._stream(pass1_stream)),
                        "fsg_lz4_decompress_batch_2s")

    # ---- LZ4 frames (include/flare_lz4_gpu.h, "LZ4 frames")
    def lz4f_compress_workspace(self, n, total_in_bytes, block_size_id=4, device=None):
        import torch
        nbytes = self.lib.fsg_lz4f_compress_workspace_bytes(n, total_in_bytes, block_size_id)
        return torch.empty(max(nbytes, 1), dtype=torch.uint8, device=device or f"cuda:{self.device}")

    def lz4f_compress(self, d_in, d_in_off, d_in_len, n, d_out, d_out_off, d_out_len, d_status, workspace,
                      block_size_id=4, checksum=False, stream=None, flags=None):
        """fsg_lz4f_compress_batch: standard LZ4 frames, with a content
        checksum when `checksum`.  With `flags` (LZ4F_FLAG_* bits) it is
        fsg_lz4f_compress_batch_flags, with slots of
        lz4f_max_frame_length_flags(len, block_size_id, flags) bytes."""
        ws = 0 if workspace is None else workspace.numel() * workspace.element_size()
        name = "fsg_lz4f_compress_batch" if flags is None else "fsg_lz4f_compress_batch_flags"
        if flags is None:
            flags = LZ4F_FLAG_CONTENT_CHECKSUM if checksum else 0
        self._check(getattr(self.lib, name)(
            _ptr(d_in), _ptr(d_in_off), _ptr(d_in_len), n, _ptr(d_out), _ptr(d_out_off), _ptr(d_out_len),
            _ptr(d_status), block_size_id, flags, _ptr(workspace), ws, self._stream(stream)), name)

    def lz4f_max_frame_length_flags(self, n, block_size_id=4, flags=0):
        """fsg_lz4f_max_frame_length_flags: the slot size of a compress call
        with `flags` (4 bytes per block more with LZ4F_FLAG_BLOCK_CHECKSUMS)."""
        return self.lib.fsg_lz4f_max_frame_length_flags(n, block_size_id, flags)

    def lz4f_xxh32(self, d_in, d_in_off, d_in_len, n, d_xxh, seed=0, stream=None):
        """fsg_lz4f_xxh32_batch: XXH32 of each body into d_xxh (int32 /
        uint32, n entries), no workspace."""
        self._check(self.lib.fsg_lz4f_xxh32_batch(
            _ptr(d_in), _ptr(d_in_off), _ptr(d_in_len), n, seed, _ptr(d_xxh), self._stream(stream)),
            "fsg_lz4f_xxh32_batch")

    def lz4f_decompress_workspace(self, n, total_in_bytes, device=None):
        import torch
        nbytes = self.lib.fsg_lz4f_decompress_workspace_bytes(n, total_in_bytes)
        return torch.empty(max(nbytes, 1), dtype=torch.uint8, device=device or f"cuda:{self.device}")

    def lz4f_decompress(self, d_in, d_in_off, d_in_len, n, d_out, d_out_off, d_out_cap, d_out_len, d_status,
                        workspace, stream=None):
        ws = 0 if workspace is None else workspace.numel() * workspace.element_size()
        self._check(self.lib.fsg_lz4f_decompress_batch(
            _ptr(d_in), _ptr(d_in_off), _ptr(d_in_len), n, _ptr(d_out), _ptr(d_out_off), _ptr(d_out_cap),
            _ptr(d_out_len), _ptr(d_status), _ptr(workspace), ws, self._stream(stream)),
            "fsg_lz4f_decompress_batch")

    def lz4f_content_sizes(self, d_in, d_in_off, d_in_len, n, d_content_size, d_status, stream=None):
        """fsg_lz4f_content_sizes_batch (d_content_size int64 / uint64:
        LZ4F_NO_CONTENT_SIZE where the frame states none)."""
        self._check(self.lib.fsg_lz4f_content_sizes_batch(
            _ptr(d_in), _ptr(d_in_off), _ptr(d_in_len), n, _ptr(d_content_size), _ptr(d_status),
            self._stream(stream)), "fsg_lz4f_content_sizes_batch")

    def lz4f_decoded_lengths(self, d_in, d_in_off, d_in_len, n, d_length, d_status, workspace, stream=None):
        """fsg_lz4f_decoded_lengths_batch on a decompress workspace (d_length
        int64 / uint64): the content size, or the sum of the blocks' decoded
        lengths for a frame that states none."""
        ws = 0 if workspace is None else workspace.numel() * workspace.element_size()
        self._check(self.lib.fsg_lz4f_decoded_lengths_batch(
            _ptr(d_in), _ptr(d_in_off), _ptr(d_in_len), n, _ptr(d_length), _ptr(d_status), _ptr(workspace), ws,
            self._stream(stream)), "fsg_lz4f_decoded_lengths_batch")

    def lz4f_compress_report(self, workspace, n, block_size_id=4) -> dict:
        head, nbytes = self._report_header(workspace)
        r = Lz4fEncodeReport()
        self._check(self.lib.fsg_lz4f_compress_report(head, n, nbytes, block_size_id, _c.byref(r)),
                    "fsg_lz4f_compress_report")
        return self._report_dict(r)

    def lz4f_decompress_report(self, workspace, n) -> dict:
        head, nbytes = self._report_header(workspace)
        r = Lz4fDecodeReport()
        self._check(self.lib.fsg_lz4f_decompress_report(head, n, nbytes, _c.byref(r)), "fsg_lz4f_decompress_report")
        return self._report_dict(r)

    # ---- inflate (include/flare_deflate_gpu.h)
    def inflate(self, d_in, d_in_off, d_in_len, n, d_out, d_out_off, d_out_cap, d_out_len, d_status,
                fmt=INFLATE_ZLIB, stream=None):
        """fsg_inflate_batch: raw deflate, zlib or gzip bodies (INFLATE_*), no workspace."""
        self._check(self.lib.fsg_inflate_batch(
            _ptr(d_in), _ptr(d_in_off), _ptr(d_in_len), n, _ptr(d_out), _ptr(d_out_off), _ptr(d_out_cap),
            _ptr(d_out_len), _ptr(d_status), fmt, self._stream(stream)), "fsg_inflate_batch")

    def inflate_lengths(self, d_in, d_in_off, d_in_len, n, d_length, d_status, fmt=INFLATE_ZLIB, stream=None):
        """fsg_inflate_lengths_batch (d_length int64 / uint64): the exact
        decoded lengths, no output written, the trailing checksum not judged."""
        self._check(self.lib.fsg_inflate_lengths_batch(
            _ptr(d_in), _ptr(d_in_off), _ptr(d_in_len), n, _ptr(d_length), _ptr(d_status), fmt,
            self._stream(stream)), "fsg_inflate_lengths_batch")

    def crc32(self, d_in, d_in_off, d_in_len, n, d_crc, stream=None):
        """fsg_crc32_batch: zlib.crc32 of each body into d_crc (int32 / uint32, n entries)."""
        self._check(self.lib.fsg_crc32_batch(_ptr(d_in), _ptr(d_in_off), _ptr(d_in_len), n, _ptr(d_crc),
                                             self._stream(stream)), "fsg_crc32_batch")

    def adler32(self, d_in, d_in_off, d_in_len, n, d_adler, stream=None):
        """fsg_adler32_batch: zlib.adler32 of each body into d_adler."""
        self._check(self.lib.fsg_adler32_batch(_ptr(d_in), _ptr(d_in_off), _ptr(d_in_len), n, _ptr(d_adler),
                                               self._stream(stream)), "fsg_adler32_batch")

    # ---- deflate compress (include/flare_deflate_compress_gpu.h)
    def deflate_max_length(self, n, fmt=INFLATE_ZLIB) -> int:
        return self.lib.fsg_deflate_max_length(n, fmt)

    def deflate_workspace_bytes(self, n, total_in_bytes) -> int:
        return self.lib.fsg_deflate_workspace_bytes(n, total_in_bytes)

    def deflate_workspace(self, n, total_in_bytes, device=None):
        import torch
        nbytes = self.deflate_workspace_bytes(n, total_in_bytes)
        return torch.empty(max(nbytes, 1), dtype=torch.uint8, device=device or f"cuda:{self.device}")

    def deflate(self, d_in, d_in_off, d_in_len, n, d_out, d_out_off, d_out_len, d_status, workspace,
                fmt=INFLATE_ZLIB, stream=None, level=None):
        """fsg_deflate_batch: raw deflate, zlib or gzip bodies (INFLATE_*) into
        slots of deflate_max_length(len, fmt) bytes.  level (DEFLATE_LEVEL_*):
        fsg_deflate_batch_level; None calls the level-less entry."""
        ws = 0 if workspace is None else workspace.numel() * workspace.element_size()
        if level is not None:
            self._check(self.lib.fsg_deflate_batch_level(
                _ptr(d_in), _ptr(d_in_off), _ptr(d_in_len), n, _ptr(d_out), _ptr(d_out_off), _ptr(d_out_len),
                _ptr(d_status), fmt, level, _ptr(workspace), ws, self._stream(stream)), "fsg_deflate_batch_level")
            return
        self._check(self.lib.fsg_deflate_batch(
            _ptr(d_in), _ptr(d_in_off), _ptr(d_in_len), n, _ptr(d_out), _ptr(d_out_off), _ptr(d_out_len),
            _ptr(d_status), fmt, _ptr(workspace), ws, self._stream(stream)), "fsg_deflate_batch")

    def deflate_report(self, workspace, n) -> dict:
        head, nbytes = self._report_header(workspace)
        r = DeflateReport()
        self._check(self.lib.fsg_deflate_report(head, n, nbytes, _c.byref(r)), "fsg_deflate_report")
        return self._report_dict(r)

    # ---- the unit index (include/flare_deflate_index_gpu.h)
    def deflate_max_length_flags(self, n, fmt=INFLATE_GZIP, flags=DEFLATE_FLAG_UNIT_INDEX) -> int:
        return self.lib.fsg_deflate_max_length_flags(n, fmt, flags)

    def deflate_flags(self, d_in, d_in_off, d_in_len, n, d_out, d_out_off, d_out_len, d_status, workspace,
                      fmt=INFLATE_GZIP, level=DEFLATE_LEVEL_FAST, flags=DEFLATE_FLAG_UNIT_INDEX, stream=None):
        """fsg_deflate_batch_flags: fsg_deflate_batch_level with a flags word
        (DEFLATE_FLAG_UNIT_INDEX: gzip bodies that carry their units'
        compressed lengths) into slots of deflate_max_length_flags bytes."""
        ws = 0 if workspace is None else workspace.numel() * workspace.element_size()
        self._check(self.lib.fsg_deflate_batch_flags(
            _ptr(d_in), _ptr(d_in_off), _ptr(d_in_len), n, _ptr(d_out), _ptr(d_out_off), _ptr(d_out_len),
            _ptr(d_status), fmt, level, flags, _ptr(workspace), ws, self._stream(stream)), "fsg_deflate_batch_flags")

    def inflate_units_workspace_bytes(self, n, extra_units) -> int:
        return self.lib.fsg_inflate_units_workspace_bytes(n, extra_units)

    def inflate_units_workspace(self, n, extra_units, device=None):
        import torch
        nbytes = self.inflate_units_workspace_bytes(n, extra_units)
        return torch.empty(max(nbytes, 1), dtype=torch.uint8, device=device or f"cuda:{self.device}")

    def inflate_units(self, d_in, d_in_off, d_in_len, n, d_out, d_out_off, d_out_cap, d_out_len, d_status,
                      workspace, fmt=INFLATE_GZIP, stream=None):
        """fsg_inflate_units_batch: fsg_inflate_batch's results, a wave per
        unit for the gzip bodies that carry a usable unit index."""
        ws = 0 if workspace is None else workspace.numel() * workspace.element_size()
        self._check(self.lib.fsg_inflate_units_batch(
            _ptr(d_in), _ptr(d_in_off), _ptr(d_in_len), n, _ptr(d_out), _ptr(d_out_off), _ptr(d_out_cap),
            _ptr(d_out_len), _ptr(d_status), fmt, _ptr(workspace), ws, self._stream(stream)),
            "fsg_inflate_units_batch")

    def inflate_units_lengths(self, d_in, d_in_off, d_in_len, n, d_length, d_status, workspace, fmt=INFLATE_GZIP,
                              stream=None):
        """fsg_inflate_units_lengths_batch: fsg_inflate_lengths_batch's results by units."""
        ws = 0 if workspace is None else workspace.numel() * workspace.element_size()
        self._check(self.lib.fsg_inflate_units_lengths_batch(
            _ptr(d_in), _ptr(d_in_off), _ptr(d_in_len), n, _ptr(d_length), _ptr(d_status), fmt, _ptr(workspace), ws,
            self._stream(stream)), "fsg_inflate_units_lengths_batch")

    def inflate_units_report(self, workspace, n) -> dict:
        head, nbytes = self._report_header(workspace)
        r = InflateUnitsReport()
        self._check(self.lib.fsg_inflate_units_report(head, n, nbytes, _c.byref(r)), "fsg_inflate_units_report")
        return self._report_dict(r)

    # ---- path reports (fsg_decompress_report and its kin)
    def _report_header(self, workspace):
        """(host copy of the workspace's counter header or None, workspace bytes)
        -- after a synchronise, so the last call on it has finished."""
        if workspace is None:
            return None, 0
        import torch
        nbytes = workspace.numel() * workspace.element_size()
        head = self.lib.fsg_report_header_bytes()
        if nbytes < head:
            return None, nbytes  # too short for any workspace path: the routing rule decides
        torch.cuda.synchronize(workspace.device)
        host = workspace.view(torch.uint8)[:head].cpu().numpy().tobytes()
        return _c.create_string_buffer(host, head), nbytes

    @staticmethod
    def _report_dict(r) -> dict:
        return {f: int(getattr(r, f)) for f, _ in r._fields_}

    def decompress_report(self, workspace, n, flags=0) -> dict:
        """fsg_decompress_report of the last decompress call that used
        `workspace` (None: the call had none), as a dict."""
        head, nbytes = self._report_header(workspace)
        r = DecodeReport()
        self._check(self.lib.fsg_decompress_report(head, n, nbytes, flags, _c.byref(r)), "fsg_decompress_report")
        return self._report_dict(r)

    def compress_report(self, workspace, n, max_in_len) -> dict:
        head, nbytes = self._report_header(workspace)
        r = EncodeReport()
        self._check(self.lib.fsg_compress_report(head, n, max_in_len, nbytes, _c.byref(r)), "fsg_compress_report")
        return self._report_dict(r)

    def lz4_decompress_report(self, workspace, n) -> dict:
        head, nbytes = self._report_header(workspace)
        r = DecodeReport()
        self._check(self.lib.fsg_lz4_decompress_report(head, n, nbytes, _c.byref(r)), "fsg_lz4_decompress_report")
        return self._report_dict(r)

    def lz4_compress_report(self, workspace, n) -> dict:
        """fsg_lz4_compress_report of the last fsg_lz4_compress_batch call that
        used `workspace`: which encoder took how many bodies."""
        head, nbytes = self._report_header(workspace)
        r = Lz4EncodeReport()
        self._check(self.lib.fsg_lz4_compress_report(head, n, nbytes, _c.byref(r)), "fsg_lz4_compress_report")
        return self._report_dict(r)

    # ---- pack (fsg_pack_batch)
    def pack_workspace(self, n, device=None):
        """Allocate the device workspace fsg_pack_batch wants (torch uint8)."""
        import torch
        nbytes = self.lib.fsg_pack_workspace_bytes(n)
        return torch.empty(max(nbytes, 1), dtype=torch.uint8, device=device or f"cuda:{self.device}")

    def pack(self, d_src, d_src_off, d_len, n, d_dst, d_pack_off, d_total, workspace, d_status=None, align=16,
             stream=None):
        """fsg_pack_batch: the ranges (d_src + d_src_off[i], d_len[i]) whose status is
        FSG_OK, dense in d_dst at d_pack_off (int64 / uint64), *d_total bytes in all;
        d_dst=None computes d_pack_off and d_total only."""
        self._check(self.lib.fsg_pack_batch(
            _ptr(d_src), _ptr(d_src_off), _ptr(d_len), _ptr(d_status), n, align, _ptr(d_dst), _ptr(d_pack_off),
            _ptr(d_total), _ptr(workspace), workspace.numel() * workspace.element_size(),
            self._stream(stream)), "fsg_pack_batch")

    def gather_blocks(self, d_src, d_len, d_dst_off, n, d_dst, stream=None):
        """fsg_gather_blocks: the n ranges (address d_src[i], d_len[i] bytes) copied to
        d_dst + d_dst_off[i] (d_src int64 / uint64 device-visible addresses)."""
        self._check(self.lib.fsg_gather_blocks(_ptr(d_src), _ptr(d_len), _ptr(d_dst_off), n, _ptr(d_dst),
                                               self._stream(stream)), "fsg_gather_blocks")

    def uncompressed_lengths(self, d_in, d_in_off, d_in_len, n, d_ulen, lenient=True, stream=None):
        self._check(self.lib.fsg_uncompressed_lengths_batch(
            _ptr(d_in), _ptr(d_in_off), _ptr(d_in_len), n, _ptr(d_ulen), int(lenient),
            self._stream(stream)), "fsg_uncompressed_lengths_batch")


# ---------------------------------------------------------------------------
# Batches (host side): one contiguous uint8 buffer + uint64 offsets + uint32 lengths.

class Batch:
    def __init__(self, data: np.ndarray, offsets: np.ndarray, lens: np.ndarray):
        self.data = np.ascontiguousarray(data, dtype=np.uint8)
        self.offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        self.lens = np.ascontiguousarray(lens, dtype=np.uint32)

    def __len__(self):
        return len(self.lens)

    def item(self, i: int) -> bytes:
        o = int(self.offsets[i])
        return self.data[o:o + int(self.lens[i])].tobytes()

    @property
    def total(self) -> int:
        return int(self.lens.astype(np.uint64).sum())

    @staticmethod
    def from_list(items) -> "Batch":
        lens = np.array([len(x) for x in items], dtype=np.uint32)
        offs = np.zeros(len(items), dtype=np.uint64)
        if len(items) > 1:
            offs[1:] = np.cumsum(lens[:-1].astype(np.uint64))
        data = np.frombuffer(b"".join(items), dtype=np.uint8) if items else np.zeros(0, np.uint8)
        if data.size == 0:
            data = np.zeros(1, np.uint8)
        return Batch(data.copy(), offs, lens)


def slot_offsets(caps: np.ndarray, align: int = 16) -> tuple[np.ndarray, int]:
    """Exclusive prefix offsets of slots of the given capacities, `align`-aligned."""
    caps = caps.astype(np.uint64)
    sizes = (caps + np.uint64(align - 1)) // np.uint64(align) * np.uint64(align)
    offs = np.zeros(len(caps), dtype=np.uint64)
    if len(caps) > 1:
        offs[1:] = np.cumsum(sizes[:-1])
    total = int(sizes.sum()) if len(caps) else 0
    return offs, max(total, align)


# fsg_pack_batch's kernels (csrc/pack.hip): items per workgroup of the offset
# scan, destination bytes per wave of the copy.  The tests place their sizes
# around these.
PACK_SCAN_BLOCK = 1024
PACK_TILE_BYTES = 4096


def pack_offsets(lens, status=None, align: int = 16) -> tuple[np.ndarray, int]:
    """fsg_pack_batch's layout rule on the host: messages whose status is not
    FSG_OK take no room, the others round_up(len, align) bytes each, in order.
    Returns the uint64 offsets and the total."""
    eff = np.asarray(lens).astype(np.uint64)
    if status is not None:
        eff = np.where(np.asarray(status) != FSG_OK, np.uint64(0), eff)
    a = np.uint64(align)
    sizes = (eff + (a - np.uint64(1))) // a * a
    ends = np.cumsum(sizes, dtype=np.uint64)
    offs = np.zeros(len(eff), dtype=np.uint64)
    offs[1:] = ends[:-1]
    return offs, int(ends[-1]) if len(eff) else 0


def max_compressed_length(n):
    return 32 + n + n // 6


# ---------------------------------------------------------------------------
# Synthetic data (flare-cpp_amd/tools/datagen.c).

_DG = None


def datagen() -> ctypes.CDLL:
    global _DG
    if _DG is None:
        p = LIB_DIR / "libflare_datagen.so"
        if not p.exists():
            raise RuntimeError(f"datagen library missing: {p}")
        lib = ctypes.CDLL(str(p))
        lib.dg_text_body.argtypes = [_u64, _vp, _sz]
        lib.dg_random_body.argtypes = [_u64, _vp, _sz]
        lib.dg_mixed_sizes.argtypes = [_u64, _vp]
        lib.dg_snappy_message.argtypes = [_u64, _u32, _vp]
        lib.dg_snappy_message.restype = _sz
        lib.dg_fnv1a64.argtypes = [_vp, _sz]
        lib.dg_fnv1a64.restype = _u64
        lib.dg_fill_batch.argtypes = [_c.c_int, _u64, _u64, _vp, _vp, _vp, _vp, _c.c_int]
        lib.dg_digest_batch.argtypes = [_vp, _vp, _vp, _u64, _vp]
        _DG = lib
    return _DG


KIND_TEXT, KIND_RANDOM, KIND_MIXED, KIND_PROTO = 0, 1, 2, 3


def _threads() -> int:
    return max(1, min(16, os.cpu_count() or 1))


def make_batch(kind: int, sizes, first_index: int = 0, threads: int | None = None) -> Batch:
    """Generate message bodies first_index.. with the given sizes (for KIND_PROTO the
    sizes are text lengths and the returned lengths are serialized lengths)."""
    dg = datagen()
    sizes = np.ascontiguousarray(np.asarray(sizes, dtype=np.uint32))
    n = len(sizes)
    if kind == KIND_PROTO:
        lens = np.array([dg.dg_snappy_message(first_index + i, int(s), None) for i, s in enumerate(sizes)],
                        dtype=np.uint32)
    else:
        lens = sizes.copy()
    offs = np.zeros(n, dtype=np.uint64)
    if n > 1:
        offs[1:] = np.cumsum(lens[:-1].astype(np.uint64))
    total = int(lens.astype(np.uint64).sum())
    data = np.zeros(max(total, 1), dtype=np.uint8)
    out_lens = np.zeros(n, dtype=np.uint32)
    dg.dg_fill_batch(kind, first_index, n, sizes.ctypes.data, offs.ctypes.data, data.ctypes.data,
                     out_lens.ctypes.data, threads or _threads())
    return Batch(data, offs, lens)


def mixed_sizes(n: int) -> np.ndarray:
    s = np.zeros(n, dtype=np.uint32)
    datagen().dg_mixed_sizes(n, s.ctypes.data)
    return s


def fnv1a64(b: bytes) -> int:
    buf = np.frombuffer(b, dtype=np.uint8) if b else np.zeros(1, np.uint8)
    return int(datagen().dg_fnv1a64(buf.ctypes.data, len(b)))


def digests(data: np.ndarray, offsets: np.ndarray, lens: np.ndarray) -> np.ndarray:
    out = np.zeros(len(lens), dtype=np.uint64)
    datagen().dg_digest_batch(data.ctypes.data, np.ascontiguousarray(offsets, np.uint64).ctypes.data,
                              np.ascontiguousarray(lens, np.uint32).ctypes.data, len(lens),
                              out.ctypes.data)
    return out
