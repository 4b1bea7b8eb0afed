#!/usr/bin/env python3
"""Records what a built libflare_snappy_gpu.so answers for the LZ4 workspace
sizes, capacities and routes, as the literal tables of
tests/cpp/test_lz4_plan.cc (tests/cpp/lz4_plan_golden.inc).

    python tools/lz4_plan_golden.py [path/to/libflare_snappy_gpu.so] > tests/cpp/lz4_plan_golden.inc

Host code only (the size and report functions make no HIP call).  The tables
in the repository were recorded from the library of the commit before
csrc/lz4_plan.h and csrc/lz4_frame_plan.h existed; run against a later build
the output must not change.
"""
import ctypes
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO / "flare-cpp_amd" / "py"))

import fsg  # noqa: E402

NS = [0, 1, 63, 64, 65, 256, 257, 65536]
TOTALS = [0, 1, 255, 256, 4095, 4096, 65535, 65536, 1 << 20, (1 << 32) + 12345, 1 << 40]
IDS = [4, 5, 6, 7]
WAVE_OPTS = [-1, 0, 8191, 0xFFFFFFFE, 0xFFFFFFFF, (1 << 32) + 5]
ZERO = ctypes.create_string_buffer(256)


def ws_points(size_of):
    """0, around the minimum, and around the size for every total (a size of
    0 = over the limit: no workspace to probe)."""
    lo = size_of(0)
    pts = {0, lo - 1, lo, lo + 1, lo + 255, lo + 256}
    for t in TOTALS:
        s = size_of(t)
        if s:
            pts |= {s - 1, s, s + 1}
    return sorted(p for p in pts if p >= 0)


def rows(name, fmt, data):
    print(f"constexpr {name} k{name}[] = {{")
    for r in data:
        print("    {" + ", ".join(f"{v}{s}" for v, s in zip(r, fmt)) + "},")
    print("};")


def main():
    lib = fsg.load_gpu_lib(sys.argv[1] if len(sys.argv) > 1 else None)
    U, L, I = "u", "ull", ""
    print("// Recorded by tools/lz4_plan_golden.py from the library built at the commit before")
    print("// lz4_plan.h: the C ABI's answers, not this header's.  Do not edit.")

    rows("EncWs", (U, L), [(n, lib.fsg_lz4_compress_workspace_bytes(n)) for n in NS])
    rows("DecWs", (U, L, L), [(n, t, lib.fsg_lz4_decompress_workspace_bytes(n, t))
                              for n in NS for t in TOTALS + [1 << 46]])
    rows("FrameEncWs", (U, L, U, L), [(n, t, i, lib.fsg_lz4f_compress_workspace_bytes(n, t, i))
                                      for n in NS for i in IDS for t in TOTALS + [1 << 46]])
    rows("FrameDecWs", (U, L, L), [(n, t, lib.fsg_lz4f_decompress_workspace_bytes(n, t))
                                   for n in NS for t in TOTALS + [1 << 38]])

    # fsg_lz4_decompress_report: path and bitmap_words_capacity (a zero header)
    out = []
    for n in NS:
        for ws in ws_points(lambda t: lib.fsg_lz4_decompress_workspace_bytes(n, t)):
            r = fsg.DecodeReport()
            assert lib.fsg_lz4_decompress_report(ZERO, n, ws, ctypes.byref(r)) == 0
            out.append((n, ws, r.path, r.bitmap_words_capacity))
    rows("DecCap", (U, L, U, L), out)

    # fsg_lz4_compress_report: path and wave_min under option lz4_encode_wave_min
    out = []
    saved = fsg.get_option("lz4_encode_wave_min", lib)
    for o in WAVE_OPTS:
        fsg.set_option("lz4_encode_wave_min", o, lib)
        for n in NS:
            lo = lib.fsg_lz4_compress_workspace_bytes(n)
            for ws in sorted({0, max(lo - 1, 0), lo, lo + 1, lo + 255, lo + 256}):
                r = fsg.Lz4EncodeReport()
                assert lib.fsg_lz4_compress_report(ZERO, n, ws, ctypes.byref(r)) == 0
                out.append((o, n, ws, r.path, r.wave_min))
    fsg.set_option("lz4_encode_wave_min", saved, lib)
    rows("EncRoute", ("ll", U, L, U, L), out)

    # fsg_lz4f_compress_report: block_entries and block_wave_min (n = 0 answers before either)
    out = []
    for n in NS[1:]:
        for i in IDS:
            for ws in ws_points(lambda t: lib.fsg_lz4f_compress_workspace_bytes(n, t, i)):
                r = fsg.Lz4fEncodeReport()
                rc = lib.fsg_lz4f_compress_report(ZERO, n, ws, i, ctypes.byref(r))
                assert (rc == 0) == (r.block_entries != 0)
                out.append((n, i, ws, r.block_entries, r.block_wave_min))
    rows("FrameEncCap", (U, U, L, U, L), out)
    out = []
    saved = fsg.get_option("lz4f_block_wave_min", lib)
    for o in WAVE_OPTS:
        fsg.set_option("lz4f_block_wave_min", o, lib)
        for n, t in ((1, 255 * 65536), (1, 256 * 65536), (256, 0), (257, 0)):  # 256, 257, 256, 257 entries
            ws = lib.fsg_lz4f_compress_workspace_bytes(n, t, 4)
            r = fsg.Lz4fEncodeReport()
            assert lib.fsg_lz4f_compress_report(ZERO, n, ws, 4, ctypes.byref(r)) == 0
            out.append((o, n, ws, r.block_entries, r.block_wave_min))
    fsg.set_option("lz4f_block_wave_min", saved, lib)
    rows("FrameEncWave", ("ll", U, L, U, L), out)

    # fsg_lz4f_decompress_report: block_entries
    out = []
    for n in NS[1:]:
        for ws in ws_points(lambda t: lib.fsg_lz4f_decompress_workspace_bytes(n, t)):
            r = fsg.Lz4fDecodeReport()
            rc = lib.fsg_lz4f_decompress_report(ZERO, n, ws, ctypes.byref(r))
            assert (rc == 0) == (r.block_entries != 0)
            out.append((n, ws, r.block_entries))
    rows("FrameDecCap", (U, L, U), out)


if __name__ == "__main__":
    main()
