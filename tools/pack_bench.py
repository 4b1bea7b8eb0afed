#!/usr/bin/env python3
"""fsg_pack_batch against a plain device-to-device copy of the same bytes.

Packs the compress layout of a benchmark configuration -- worst-case slots
(fsg_max_compressed_length of each input) holding the compressed lengths
recorded in tests/golden/full_<CONFIG>.npz -- and times it with HIP events
over --launches launches after --warmup warm-up ones, then times
hipMemcpyAsync device-to-device of `total` bytes the same way in the same
process.  The slot contents are whatever the allocation holds: the kernels'
time does not depend on the byte values.

  python tools/pack_bench.py [--configs C3,CM] [--launches 20] [--warmup 3] [--align 16]

Prints one JSON line per configuration:
  pack_ms / copy_ms (medians), scan_only_ms (the call without a destination:
  offsets and total), ratio = pack_ms / copy_ms, the slot and packed
  bytes, and d2h_saved_ms = (slot bytes - packed bytes) / 57 GB/s, the pinned
  D2H time the handler no longer spends; pack_share =
  pack_ms / d2h_saved_ms has to stay at or below 0.10.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO / "flare-cpp_amd" / "py"))
import fsg  # noqa: E402

D2H_GBPS = 57.0  # pinned D2H, DESIGN.md §5


def layout(config: str):
    f = np.load(REPO / "tests" / "golden" / f"full_{config}.npz")
    lens = f["compressed_len"].astype(np.uint32)
    n = len(lens)
    sizes = np.full(n, 65536, np.uint32) if config == "C3" else fsg.mixed_sizes(n)
    caps = fsg.max_compressed_length(sizes.astype(np.uint64))
    assert (lens <= caps).all()
    offs, slot_bytes = fsg.slot_offsets(caps)
    return lens, offs, slot_bytes


def timed(torch, fn, launches, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(launches):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C3,CM")
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--align", type=int, default=16)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("pack_bench needs a GPU")
    codec = fsg.SnappyGPU(torch.cuda.current_device())
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    for config in args.configs.split(","):
        lens, offs, slot_bytes = layout(config)
        n = len(lens)
        poffs, total = fsg.pack_offsets(lens, None, args.align)
        d_src = torch.empty(slot_bytes, dtype=torch.uint8, device="cuda")
        d_dst = torch.empty(total + 64, dtype=torch.uint8, device="cuda")
        d_so = torch.from_numpy(offs.view(np.int64)).cuda()
        d_len = torch.from_numpy(lens.view(np.int32)).cuda()
        d_po = torch.zeros(n, dtype=torch.int64, device="cuda")
        d_tot = torch.zeros(1, dtype=torch.int64, device="cuda")
        ws = codec.pack_workspace(n)
        stream = torch.cuda.current_stream().cuda_stream

        def pack():
            codec.pack(d_src, d_so, d_len, n, d_dst, d_po, d_tot, ws, align=args.align)

        def scan():  # offsets and total only
            codec.pack(None, None, d_len, n, None, d_po, d_tot, ws, align=args.align)

        def copy():
            rc = hip.hipMemcpyAsync(d_dst.data_ptr(), d_src.data_ptr(), total, 3, stream)  # hipMemcpyDeviceToDevice
            assert rc == 0, rc

        pack_ms = timed(torch, pack, args.launches, args.warmup)
        assert int(d_tot.cpu().numpy().view(np.uint64)[0]) == total
        assert np.array_equal(d_po.cpu().numpy().view(np.uint64), poffs)
        scan_ms = timed(torch, scan, args.launches, args.warmup)
        copy_ms = timed(torch, copy, args.launches, args.warmup)
        p, c = float(np.median(pack_ms)), float(np.median(copy_ms))
        saved = (slot_bytes - total) / (D2H_GBPS * 1e6)
        print(json.dumps({
            "config": config, "messages": n, "align": args.align, "slot_bytes": int(slot_bytes),
            "packed_bytes": int(total), "launches": args.launches,
            "pack_ms": round(p, 4), "pack_ms_min": round(min(pack_ms), 4), "pack_ms_max": round(max(pack_ms), 4),
            "copy_ms": round(c, 4), "copy_ms_min": round(min(copy_ms), 4), "copy_ms_max": round(max(copy_ms), 4),
            "scan_only_ms": round(float(np.median(scan_ms)), 4), "ratio": round(p / c, 3), "pack_gb_s": round(2 * total / p / 1e6, 1),
            "d2h_saved_ms": round(saved, 2), "pack_share": round(p / saved, 4)}), flush=True)
        del d_src, d_dst
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
