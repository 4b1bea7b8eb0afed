"""Inflate on the device against zlib's own inflate on the host
(include/flare_deflate_gpu.h; DESIGN.md section 5, "Deflate").

Batches of text bodies compressed by zlib at level 6 (zlib format), device
resident.  Per batch, HIP events around single launches, the median of
--launches after two warm-up launches, separately for
  decode    fsg_inflate_batch on the raw streams (the decode kernel alone)
  checksum  fsg_adler32_batch on the decoded bytes (the checksum kernel alone)
  zlib      fsg_inflate_batch on the zlib bodies (both kernels)
  lengths   fsg_inflate_lengths_batch (the symbol phase alone: no execute phase)
and beside them zlib's inflate on the same bodies on this machine's host, one
thread and 16 threads (zlib releases the GIL), on at most --host-sample bodies.
One JSON line per row.  A row above 8,192 bodies repeats 8,192 distinct ones.

    python tools/inflate_bench.py [--rows 1x64k,c3] [--launches 10]
"""
import argparse
import json
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
    ap.add_argument("--host-sample", type=int, default=4096)
    ap.add_argument("--threads", type=int, default=16)
    a = ap.parse_args()
    import torch
    dev = torch.device("cuda", 0)
    codec = fsg.SnappyGPU(0)
    s = torch.cuda.current_stream()
    H = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    pool = ThreadPoolExecutor(a.threads)

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
        items = [batch.item(i) for i in range(distinct)]
        comp = list(pool.map(lambda x: zlib.compress(x, 6), items))
        cb = fsg.Batch.from_list(comp)
        rep = n // distinct
        c_off = np.tile(cb.offsets, rep)
        c_len = np.tile(cb.lens, rep)
        raw_bytes = n * size
        d_c, d_co, d_cl = H(cb.data), H(c_off), H(c_len)
        d_ro, d_rl = H(c_off + np.uint64(2)), H(c_len - np.uint32(6))  # the raw streams inside the zlib bodies
        o_off = np.arange(n, dtype=np.uint64) * np.uint64(size)
        d_oo, d_cap = H(o_off), H(np.full(n, size, np.uint32))
        d_out = torch.full((raw_bytes,), 0xA5, dtype=torch.uint8, device=dev)
        d_ol = torch.zeros(n, dtype=torch.int32, device=dev)
        d_st = torch.zeros(n, dtype=torch.int32, device=dev)
        d_len = torch.zeros(n, dtype=torch.int64, device=dev)
        d_sum = torch.zeros(n, dtype=torch.int32, device=dev)
        want = H(batch.data[:distinct * size])

        def check(what):
            ok = int((d_st != 0).sum().item()) == 0
            out = d_out.view(rep, distinct * size)
            return ok and all(bool(torch.equal(out[r], want)) for r in range(rep)), what

        t_dec = timed(lambda: codec.inflate(d_c, d_ro, d_rl, n, d_out, d_oo, d_cap, d_ol, d_st, fmt=fsg.INFLATE_RAW,
                                            stream=s))
        ok_dec = check("decode")[0]
        d_out.fill_(0xA5)
        t_zlib = timed(lambda: codec.inflate(d_c, d_co, d_cl, n, d_out, d_oo, d_cap, d_ol, d_st, fmt=fsg.INFLATE_ZLIB,
                                             stream=s))
        ok_zlib = check("zlib")[0]
        t_sum = timed(lambda: codec.adler32(d_out, d_oo, d_cap, n, d_sum, stream=s))
        ok_sum = int(d_sum.cpu().numpy().view(np.uint32)[0]) == zlib.adler32(items[0])
        t_len = timed(lambda: codec.inflate_lengths(d_c, d_co, d_cl, n, d_len, d_st, fmt=fsg.INFLATE_ZLIB, stream=s))
        ok_len = int((d_st != 0).sum().item()) == 0 and bool((d_len == size).all().item())
        # the host: zlib's inflate on the same bodies
        k = min(distinct, a.host_sample)
        sample = comp[:k]
        t = time.perf_counter()
        for c in sample:
            zlib.decompress(c)
        t1 = time.perf_counter() - t
        t = time.perf_counter()
        list(pool.map(zlib.decompress, sample))
        t16 = time.perf_counter() - t
        g = lambda ms: round(raw_bytes / (ms / 1e3) / GIB, 3)  # noqa: E731
        print(json.dumps({
            "row": name, "n": n, "size": size, "distinct": distinct, "launches": a.launches,
            "compressed_bytes": int(c_len.astype(np.uint64).sum()),
            "decode_ms": round(t_dec, 4), "decode_gib_s": g(t_dec),
            "checksum_ms": round(t_sum, 4), "checksum_gib_s": g(t_sum),
            "zlib_call_ms": round(t_zlib, 4), "zlib_call_gib_s": g(t_zlib),
            "lengths_ms": round(t_len, 4), "lengths_gib_s": g(t_len),
            "ok": bool(ok_dec and ok_zlib and ok_sum and ok_len),
            "host_sample_bodies": k,
            "host_zlib_1thread_gib_s": round(k * size / t1 / GIB, 3),
            f"host_zlib_{a.threads}threads_gib_s": round(k * size / t16 / GIB, 3),
            "host_zlib_1thread_ms_whole_batch": round(t1 / k * n * 1e3, 3),
            f"host_zlib_{a.threads}threads_ms_whole_batch": round(t16 / k * n * 1e3, 3)}), flush=True)
        del d_c, d_out, want
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
