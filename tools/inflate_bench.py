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

Indexed rows (include/flare_deflate_index_gpu.h; the names with an i): gzip
bodies written on the device by fsg_deflate_batch_flags at level 1 with the
unit index.  Per row fsg_inflate_units_batch and fsg_inflate_units_lengths_batch
against fsg_inflate_batch and fsg_inflate_lengths_batch on the same bodies --
those of --baseline-lib (another build of the library, the parent commit's
for an A/B; this build's serial calls are then timed beside them) or, without
it, this build's -- and host zlib as above.  The calls
alternate within each of --rounds rounds; a row gives the median over the
rounds of each call's per-round median, and the lowest and highest per-round
median as its spread.  i256x64k and i4096x64k have one unit per body: what
they show is the cost of the classify, plan, list and resolve launches.

    python tools/inflate_bench.py --rows i16x4m,i1x4m,i256x64k,i4096x64k [--baseline-lib PATH]
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
INDEXED = {"i16x4m": (16, 4 << 20), "i1x4m": (1, 4 << 20), "i256x64k": (256, 64 << 10), "i4096x64k": (4096, 64 << 10)}
DISTINCT = 8192


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="", help="comma-separated rows (default: all of " + ",".join(MATRIX) + ")")
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--host-sample", type=int, default=4096)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=5, help="indexed rows: rounds of alternating calls")
    ap.add_argument("--baseline-lib", default="", help="indexed rows: the library whose serial calls are the baseline")
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

    def indexed_row(name):
        n, size = INDEXED[name]
        base = fsg.SnappyGPU(0, Path(a.baseline_lib)) if a.baseline_lib else codec
        batch = fsg.make_batch(fsg.KIND_TEXT, np.full(n, size, np.uint32))
        items = [batch.item(i) for i in range(n)]
        caps = np.array([codec.deflate_max_length_flags(size)] * n, dtype=np.uint64)
        b_off = np.concatenate([[0], np.cumsum(caps)[:-1]]).astype(np.uint64)
        d_in, d_io, d_il = H(batch.data[:n * size]), H(batch.offsets[:n]), H(batch.lens[:n])
        d_body = torch.zeros(int(caps.sum()), dtype=torch.uint8, device=dev)
        d_bo, d_bl = H(b_off), torch.zeros(n, dtype=torch.int32, device=dev)
        d_st = torch.zeros(n, dtype=torch.int32, device=dev)
        codec.deflate_flags(d_in, d_io, d_il, n, d_body, d_bo, d_bl, d_st, codec.deflate_workspace(n, n * size), stream=s)
        torch.cuda.synchronize()
        assert int((d_st != 0).sum().item()) == 0
        blen = d_bl.cpu().numpy().view(np.uint32)
        body = d_body.cpu().numpy()
        bodies = [body[int(o):int(o) + int(k)].tobytes() for o, k in zip(b_off, blen)]
        units = -(-size // 65472)
        ws = codec.inflate_units_workspace(n, n * (units - 1))
        o_off = np.arange(n, dtype=np.uint64) * np.uint64(size)
        d_oo, d_cap = H(o_off), H(np.full(n, size, np.uint32))
        d_out = torch.full((n * size,), 0xA5, dtype=torch.uint8, device=dev)
        d_ol = torch.zeros(n, dtype=torch.int32, device=dev)
        d_len = torch.zeros(n, dtype=torch.int64, device=dev)
        G = fsg.INFLATE_GZIP
        calls = {
            "units": lambda: codec.inflate_units(d_body, d_bo, d_bl, n, d_out, d_oo, d_cap, d_ol, d_st, ws, fmt=G,
                                                 stream=s),
            "serial": lambda: base.inflate(d_body, d_bo, d_bl, n, d_out, d_oo, d_cap, d_ol, d_st, fmt=G, stream=s),
            "units_lengths": lambda: codec.inflate_units_lengths(d_body, d_bo, d_bl, n, d_len, d_st, ws, fmt=G,
                                                                 stream=s),
            "serial_lengths": lambda: base.inflate_lengths(d_body, d_bo, d_bl, n, d_len, d_st, fmt=G, stream=s),
        }
        if base is not codec:  # the A/B of the serial calls themselves
            calls["serial_this_build"] = lambda: codec.inflate(d_body, d_bo, d_bl, n, d_out, d_oo, d_cap, d_ol, d_st,
                                                               fmt=G, stream=s)
            calls["serial_lengths_this_build"] = lambda: codec.inflate_lengths(d_body, d_bo, d_bl, n, d_len, d_st,
                                                                               fmt=G, stream=s)
        ok = {}
        for what, fn in calls.items():  # the answers, before any timing
            d_out.fill_(0xA5)
            d_len.zero_()
            fn()
            torch.cuda.synchronize()
            good = int((d_st != 0).sum().item()) == 0
            if "lengths" in what:
                ok[what] = good and bool((d_len == size).all().item())
            else:
                ok[what] = good and bool(torch.equal(d_out, d_in))
        codec.inflate_units(d_body, d_bo, d_bl, n, d_out, d_oo, d_cap, d_ol, d_st, ws, fmt=G, stream=s)
        report = codec.inflate_units_report(ws, n)
        per_round = {what: [] for what in calls}
        for _ in range(a.rounds):
            for what, fn in calls.items():
                per_round[what].append(timed(fn))
        t = time.perf_counter()
        for c in bodies:
            zlib.decompress(c, 31)
        t1 = time.perf_counter() - t
        t = time.perf_counter()
        list(pool.map(lambda c: zlib.decompress(c, 31), bodies))
        t16 = time.perf_counter() - t
        row = {"row": name, "n": n, "size": size, "units_per_body": units, "launches": a.launches, "rounds": a.rounds,
               "compressed_bytes": int(blen.astype(np.uint64).sum()),
               "baseline": a.baseline_lib or "this build", "ok": ok, "report": report}
        for what, ms in per_round.items():
            row[what + "_ms"] = round(float(np.median(ms)), 4)
            row[what + "_ms_spread"] = [round(min(ms), 4), round(max(ms), 4)]
        row["units_over_serial"] = round(row["serial_ms"] / row["units_ms"], 3)
        row["units_lengths_over_serial_lengths"] = round(row["serial_lengths_ms"] / row["units_lengths_ms"], 3)
        row["host_zlib_1thread_ms"] = round(t1 * 1e3, 3)
        row[f"host_zlib_{a.threads}threads_ms"] = round(t16 * 1e3, 3)
        row[f"host_{a.threads}threads_over_units"] = round(t16 * 1e3 / row["units_ms"], 3)
        print(json.dumps(row), flush=True)

    for name in (a.rows.split(",") if a.rows else MATRIX):
        if name in INDEXED:
            indexed_row(name)
            continue
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
