#!/usr/bin/env python3
"""Which device path a bench workload takes: builds the batch the way bench.py
does (bodies from the generator, compressed inputs from the GPU encoder in
their worst-case slots, the decode workspace sized from the slot total), runs
ONE call at default options and prints its path report
(fsg_decompress_report / fsg_compress_report, include/flare_snappy_gpu.h;
fsg_lz4_compress_report, include/flare_lz4_gpu.h, for the lz4-* workloads) as
one JSON line.  The round trip is checked first (zero statuses, decoded bytes
equal to the raw batch).

    python tools/path_report.py --workload cm-decompress
"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO / "flare-cpp_amd" / "py"))
import fsg  # noqa: E402

# name: (op, kind, messages, body size or None = the mixed size stream)
WORKLOADS = {
    "c3-decompress": ("decompress", fsg.KIND_TEXT, 65536, 65536),
    "c2-decompress": ("decompress", fsg.KIND_RANDOM, 65536, 4096),
    "cm-decompress": ("decompress", fsg.KIND_MIXED, 1 << 20, None),
    "c3-compress": ("compress", fsg.KIND_TEXT, 65536, 65536),
    "c5-compress": ("compress", fsg.KIND_PROTO, 262144, None),
    # LZ4 compress: which encoder took the bodies (lanes, or the wave encoder)
    "lz4-c3-compress": ("lz4-compress", fsg.KIND_TEXT, 65536, 65536),
    "lz4-256x64k-compress": ("lz4-compress", fsg.KIND_TEXT, 256, 65536),
    "lz4-16x4m-compress": ("lz4-compress", fsg.KIND_TEXT, 16, 4 << 20),
}


def lz4_compress(args, torch, codec, b, n, H):
    """One fsg_lz4_compress_batch call, the bodies decoded back, its report."""
    lib = codec.lib
    d_raw, d_off, d_len = H(b.data), H(b.offsets), H(b.lens)
    caps = np.array([lib.fsg_lz4_max_compressed_length(int(x)) for x in b.lens], np.uint64)
    c_off, c_tot = fsg.slot_offsets(caps)
    d_c = torch.zeros(c_tot, dtype=torch.uint8, device="cuda")
    d_coff = H(c_off)
    d_cl = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_st = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    ws = codec.lz4_compress_workspace(n)
    codec.lz4_compress(d_raw, d_off, d_len, n, d_c, d_coff, d_cl, d_st, ws)
    rep = codec.lz4_compress_report(ws, n)
    del ws
    errors = int((d_st != 0).sum().item())
    comp_total = int(d_cl.sum(dtype=torch.int64).item())
    d_out = torch.full((max(b.total, 1),), 0xA5, dtype=torch.uint8, device="cuda")
    d_ol = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_st.fill_(-7)
    codec.lz4_decompress(d_c, d_coff, d_cl, n, d_out, d_off, d_len, d_ol, d_st)
    torch.cuda.synchronize()
    errors += int((d_st != 0).sum().item())
    line = {
        "workload": args.workload, "n_msgs": n, "raw_bytes": b.total, "compressed_bytes": comp_total,
        "status_errors": errors, "roundtrip_ok": bool(torch.equal(d_out[:b.total], d_raw[:b.total])),
        "report": rep,
    }
    print(json.dumps(line))
    return 0 if errors == 0 and line["roundtrip_ok"] else 1


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workload", required=True, choices=sorted(WORKLOADS))
    ap.add_argument("--n-msgs", type=int, default=0, help="messages (default: the workload's full size)")
    args = ap.parse_args()
    import torch
    torch.cuda.set_device(0)
    op, kind, n_default, size = WORKLOADS[args.workload]
    n = args.n_msgs or n_default
    sizes = np.full(n, size, np.uint32) if size else fsg.mixed_sizes(n)
    b = fsg.make_batch(kind, sizes)

    def H(a):
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()

    codec = fsg.SnappyGPU(0)
    if op == "lz4-compress":
        return lz4_compress(args, torch, codec, b, n, H)
    d_raw, d_off, d_len = H(b.data), H(b.offsets), H(b.lens)
    caps = np.array([fsg.max_compressed_length(int(x)) for x in b.lens], np.uint64)
    c_off, c_tot = fsg.slot_offsets(caps)
    d_c = torch.zeros(c_tot, dtype=torch.uint8, device="cuda")
    d_coff = H(c_off)
    d_cl = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_st = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    max_len = int(b.lens.max())
    ws = codec.compress_workspace(n, max_len)
    codec.compress(d_raw, d_off, d_len, n, max_len, d_c, d_coff, d_cl, d_st, workspace=ws)
    enc = codec.compress_report(ws, n, max_len)
    del ws
    errors = int((d_st != 0).sum().item())
    comp_total = int(d_cl.sum(dtype=torch.int64).item())
    d_out = torch.full((max(b.total, 1),), 0xA5, dtype=torch.uint8, device="cuda")
    d_ol = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_st.fill_(-7)
    dws = codec.decompress_workspace(n, c_tot)
    codec.decompress(d_c, d_coff, d_cl, n, d_out, d_off, d_len, d_ol, d_st, workspace=dws)
    dec = codec.decompress_report(dws, n)
    errors += int((d_st != 0).sum().item())
    line = {
        "workload": args.workload, "n_msgs": n, "raw_bytes": b.total, "compressed_bytes": comp_total,
        "status_errors": errors, "roundtrip_ok": bool(torch.equal(d_out[:b.total], d_raw[:b.total])),
        "report": dec if op == "decompress" else enc,
    }
    print(json.dumps(line))
    return 0 if errors == 0 and line["roundtrip_ok"] else 1


if __name__ == "__main__":
    sys.exit(main())
