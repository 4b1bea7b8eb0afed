"""Deflate compress on the device against zlib's deflate on the host
(include/flare_deflate_compress_gpu.h; DESIGN.md section 5, "Deflate compress").

Batches of text bodies, device resident.  Per batch, HIP events around single
fsg_deflate_batch calls (zlib format: every kernel of the call), the median of
--launches after two warm-up launches; the outputs are then inflated on the
device (fsg_inflate_batch) and compared with the inputs before the row is
reported.  Beside them zlib's compress at level 1 and level 6 on the same
bodies on this machine's host, one thread and --threads threads (zlib releases
the GIL), on at most --host-sample bodies, and the compression ratio of all
three.  One JSON line per row.  A row above 8,192 bodies repeats 8,192
distinct ones.

The split parse / code build / emit.  `make deflate_phases` builds two more
copies of the library whose unit kernel stops after phase 1 and after phase 2
(their outputs are not streams).  FSG_LIB=<that library> with --time-only
times the call under one of them, nothing checked; the differences between
the three times are the phases.

--level 0 or 2 times fsg_deflate_batch_level (include/flare_deflate_level_gpu.h)
at that level; the rows then carry a "level" key.

    python tools/deflate_bench.py [--rows 1x64k,c3] [--launches 10] [--time-only] [--level 2]
"""
import argparse
import json
import os
import sys
import time
import zlib
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO / "flare-cpp_amd" / "py"))
import fsg  # noqa: E402

GIB = float(1 << 30)
MATRIX = {"1x64k": (1, 64 << 10), "64x16k": (64, 16 << 10), "256x64k": (256, 64 << 10), "16x4m": (16, 4 << 20),
          "c3": (65536, 64 << 10)}
DISTINCT = 8192


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="", help="comma-separated rows (default: all of " + ",".join(MATRIX) + ")")
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--host-sample", type=int, default=2048)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--time-only", action="store_true", help="the call's median ms per row, nothing checked")
    ap.add_argument("--level", type=int, default=1, choices=(0, 1, 2),
                    help="fsg_deflate_batch_level's level; 1 (the default) times the level-less call")
    a = ap.parse_args()
    import torch
    dev = torch.device("cuda", 0)
    codec = fsg.SnappyGPU(0)
    s = torch.cuda.current_stream()
    H = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    pool = ThreadPoolExecutor(a.threads)
    fmt = fsg.INFLATE_ZLIB
    lvl = None if a.level == 1 else a.level
    tag = {} if lvl is None else {"level": lvl}

    def timed(fn):
        ms = []
        for k in range(2 + a.launches):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            fn()
            e1.record(s)
            torch.cuda.synchronize()
            if k >= 2:
                ms.append(e0.elapsed_time(e1))
        return float(np.median(ms))

    for name in (a.rows.split(",") if a.rows else MATRIX):
        n, size = MATRIX[name]
        distinct = min(n, DISTINCT)
        batch = fsg.make_batch(fsg.KIND_TEXT, np.full(distinct, size, np.uint32))
        rep = n // distinct
        raw_bytes = n * size
        slot = codec.deflate_max_length(size, fmt)
        d_in = H(batch.data[:distinct * size])
        d_io = H(np.tile(np.arange(distinct, dtype=np.uint64) * np.uint64(size), rep))
        d_il = H(np.full(n, size, np.uint32))
        d_oo = H(np.arange(n, dtype=np.uint64) * np.uint64(slot))
        d_out = torch.full((n * slot,), 0xA5, dtype=torch.uint8, device=dev)
        d_ol = torch.zeros(n, dtype=torch.int32, device=dev)
        d_st = torch.zeros(n, dtype=torch.int32, device=dev)
        ws = codec.deflate_workspace(n, raw_bytes)
        t_call = timed(lambda: codec.deflate(d_in, d_io, d_il, n, d_out, d_oo, d_ol, d_st, ws, fmt=fmt, stream=s,
                                            level=lvl))
        if a.time_only:
            print(json.dumps({"row": name, **tag, "lib": os.environ.get("FSG_LIB", ""), "call_ms": round(t_call, 4)}),
                  flush=True)
            continue
        report = codec.deflate_report(ws, n)
        ok = int((d_st != 0).sum().item()) == 0
        out_bytes = int(d_ol.cpu().numpy().view(np.uint32).astype(np.uint64).sum())
        # the round trip: the call's outputs through the device inflate
        d_back = torch.full((raw_bytes,), 0x5A, dtype=torch.uint8, device=dev)
        d_bo = H(np.arange(n, dtype=np.uint64) * np.uint64(size))
        d_bl = torch.zeros(n, dtype=torch.int32, device=dev)
        d_bs = torch.zeros(n, dtype=torch.int32, device=dev)
        codec.inflate(d_out, d_oo, d_ol, n, d_back, d_bo, d_il, d_bl, d_bs, fmt=fmt, stream=s)
        torch.cuda.synchronize()
        back = d_back.view(rep, distinct * size)
        ok = ok and int((d_bs != 0).sum().item()) == 0 and all(bool(torch.equal(back[r], d_in)) for r in range(rep))
        # and zlib itself on the first body
        first = bytes(d_out[:int(d_ol[0].item())].cpu().numpy())
        ok = ok and zlib.decompress(first) == batch.item(0)
        # the host: zlib's compress on the same bodies
        k = min(distinct, a.host_sample)
        items = [batch.item(i) for i in range(k)]
        host = {}
        for level in (1, 6):
            t = time.perf_counter()
            comp = [zlib.compress(x, level) for x in items]
            t1 = time.perf_counter() - t
            t = time.perf_counter()
            list(pool.map(lambda x: zlib.compress(x, level), items))
            tn = time.perf_counter() - t
            host[f"host_zlib{level}_ratio"] = round(k * size / sum(map(len, comp)), 3)
            host[f"host_zlib{level}_1thread_gib_s"] = round(k * size / t1 / GIB, 4)
            host[f"host_zlib{level}_{a.threads}threads_gib_s"] = round(k * size / tn / GIB, 4)
            host[f"host_zlib{level}_1thread_ms_whole_batch"] = round(t1 / k * n * 1e3, 2)
            host[f"host_zlib{level}_{a.threads}threads_ms_whole_batch"] = round(tn / k * n * 1e3, 2)
        row = {"row": name, **tag, "n": n, "size": size, "distinct": distinct, "launches": a.launches,
               "call_ms": round(t_call, 4), "call_gib_s": round(raw_bytes / (t_call / 1e3) / GIB, 4),
               "ratio": round(raw_bytes / out_bytes, 3), "units": report["units"],
               "stored_units": report["stored_units"], "fixed_units": report["fixed_units"],
               "dynamic_units": report["dynamic_units"], "workspace_mib": round(ws.numel() / 2 ** 20, 1), "ok": bool(ok),
               "host_sample_bodies": k, **host}
        print(json.dumps(row), flush=True)
        del d_in, d_out, d_back, ws
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
