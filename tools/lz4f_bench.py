"""LZ4 frames beside the single-block LZ4 bodies, device-resident: the same
text bodies through fsg_lz4f_compress_batch / fsg_lz4f_decompress_batch and
through fsg_lz4_compress_batch / fsg_lz4_decompress_batch_ws in one process,
the two alternating launch by launch, each launch timed with HIP events on the
launch stream after warm-up launches of both; the median, minimum and maximum
per call.  One JSON line per row.

    python tools/lz4f_bench.py [--rows 16x4m,c3] [--launches 7] [--warmup 2] [--bid 4]
    python tools/lz4f_bench.py --no-size [--rows 16x4m@7,16x4m@7c,c3,1x64k] [--bid 4] [--checksum 1]
    python tools/lz4f_bench.py --length-pass
    python tools/lz4f_bench.py --linked [--rows 16x4m@4,16x4m@7,4096x128k@4,1x128k@4] [--sys-linked 1]
    python tools/lz4f_bench.py --sums [--rows 16x4m@4,16x4m@7,c3@4]
    python tools/lz4f_bench.py --xxh [--rows 1x4m,16x4m,1024x64k,c3]

Rows: 16x4m (16 x 4 MiB: 64 independent blocks a body, where the format adds
parallelism) and c3 (65,536 x 64 KiB: one block a body, the cost of the plan,
stage, assemble and finish passes).  Round trips are checked untimed, frames of
a sample against the frame oracle.  `staging_bytes`: what the decompressor's
stage pass copies (one read and one write of the compressed blocks).

--no-size: the rows' frames with the content size field taken out (what the
lz4 command and LZ4F_compressFrame with contentSize 0 write) through
fsg_lz4f_decompress_batch with option lz4f_nosize_fast at 0 (the serial
decoder) and at 1 (the block decoders), alternating; a library without the
option gives the serial figure alone.  --length-pass: the length pass by
itself (fsg_lz4f_decoded_lengths_batch on one-block frames without a content
size), one lane per block against one wave per block, by block size and batch.

--linked: the rows' frames with B.Indep cleared in FLG and HC recomputed on
the host -- valid linked frames with the same bytes, which take the routes of
linked frames but hold no copy that reaches into an earlier block -- each with
and without a content size, through fsg_lz4f_decompress_batch with options
lz4f_linked_fast and lz4f_nosize_fast both 0 (the serial decoder) and both 1
(a wave per frame), alternating; a library without the option gives the
serial figure alone.  --sys-linked 1: one more row, 16 x 4 MiB at id 4 written
by the system liblz4 with LZ4F_blockLinked (copies into history included);
reported as missing where liblz4 is not installed.

--sums: the rows' sized frames written without checksums, with a content
checksum, with block checksums and with both (fsg_lz4f_compress_batch_flags'
flags), compress and then decompress, the variants alternating launch by launch
in one process, so a checksum's share is a difference of two figures of one
line.  --xxh: fsg_lz4f_xxh32_batch alone, in ms and GiB/s.
"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[1]
for p in (REPO / "flare-cpp_amd" / "py", REPO / "oracle", REPO / "tests"):
    sys.path.insert(0, str(p))
import fsg  # noqa: E402

ROWS = {"16x4m": (16, 4 << 20), "c3": (65536, 64 << 10), "256x256k": (256, 256 << 10), "1x64k": (1, 64 << 10),
        "4096x128k": (4096, 128 << 10), "1x128k": (1, 128 << 10)}
NONE = 0xFFFFFFFF


def stats(ms):
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def alternate(torch, s, fns, warmup, launches):
    """Times each of `fns` launches times, alternating them, after `warmup`
    untimed rounds of all."""
    ms = [[] for _ in fns]
    for k in range(warmup + launches):
        for i, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            fn()
            e1.record(s)
            torch.cuda.synchronize()
            if k >= warmup:
                ms[i].append(e0.elapsed_time(e1))
    return [stats(m) for m in ms]


def row(torch, codec, name, bid, warmup, launches):
    dev = torch.device("cuda", 0)
    lib = codec.lib
    n, size = ROWS[name]
    batch = fsg.make_batch(fsg.KIND_TEXT, np.full(n, size, np.uint32))
    raw = batch.total
    H = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    s = torch.cuda.current_stream()
    d_raw, d_ro, d_rl = H(batch.data), H(batch.offsets), H(batch.lens)
    # single-block bodies
    b_off, b_tot = fsg.slot_offsets(np.array([lib.fsg_lz4_max_compressed_length(int(x)) for x in batch.lens], np.uint64))
    d_b, d_bo = torch.zeros(b_tot, dtype=torch.uint8, device=dev), H(b_off)
    d_bl = torch.zeros(n, dtype=torch.int32, device=dev)
    d_bst = torch.zeros(n, dtype=torch.int32, device=dev)
    b_ws = codec.lz4_compress_workspace(n)
    # frames
    f_off, f_tot = fsg.slot_offsets(np.array([lib.fsg_lz4f_max_frame_length(int(x), bid) for x in batch.lens], np.uint64))
    d_f, d_fo = torch.zeros(f_tot, dtype=torch.uint8, device=dev), H(f_off)
    d_fl = torch.zeros(n, dtype=torch.int32, device=dev)
    d_fst = torch.zeros(n, dtype=torch.int32, device=dev)
    f_ws = codec.lz4f_compress_workspace(n, raw, bid)

    def enc_block():
        codec.lz4_compress(d_raw, d_ro, d_rl, n, d_b, d_bo, d_bl, d_bst, b_ws, stream=s)

    def enc_frame():
        codec.lz4f_compress(d_raw, d_ro, d_rl, n, d_f, d_fo, d_fl, d_fst, f_ws, block_size_id=bid, stream=s)

    enc = alternate(torch, s, (enc_block, enc_frame), warmup, launches)
    enc_rep = codec.lz4f_compress_report(f_ws, n, bid)
    body_bytes = int(d_bl.cpu().numpy().view(np.uint32).astype(np.uint64).sum())
    frame_len = d_fl.cpu().numpy().view(np.uint32)
    frame_bytes = int(frame_len.astype(np.uint64).sum())
    enc_ok = int((d_bst != 0).sum().item()) == 0 and int((d_fst != 0).sum().item()) == 0
    from bind import Lz4Oracle
    import lz4f_ref
    o = Lz4Oracle()
    host_f = d_f.cpu().numpy()
    sample_ok = all(host_f[int(f_off[i]):int(f_off[i]) + int(frame_len[i])].tobytes() ==
                    lz4f_ref.compress_frame(o, batch.item(int(i)), bid)
                    for i in np.linspace(0, n - 1, 8).astype(np.int64))
    del b_ws, f_ws, host_f
    torch.cuda.empty_cache()
    # decode: both into slots of the input layout
    d_out_b = torch.full((raw,), 0xA5, dtype=torch.uint8, device=dev)
    d_out_f = torch.full((raw,), 0xA5, dtype=torch.uint8, device=dev)
    d_ol = torch.zeros(n, dtype=torch.int32, device=dev)
    bd_ws = codec.lz4_decompress_workspace(n, int(b_tot))
    fd_ws = codec.lz4f_decompress_workspace(n, frame_bytes)  # sized for the frames' bytes, as a caller would

    def dec_block():
        codec.lz4_decompress(d_b, d_bo, d_bl, n, d_out_b, d_ro, d_rl, d_ol, d_bst, stream=s, workspace=bd_ws)

    def dec_frame():
        codec.lz4f_decompress(d_f, d_fo, d_fl, n, d_out_f, d_ro, d_rl, d_ol, d_fst, fd_ws, stream=s)

    dec = alternate(torch, s, (dec_block, dec_frame), warmup, launches)
    dec_rep = codec.lz4f_decompress_report(fd_ws, n)
    dec_ok = (int((d_bst != 0).sum().item()) == 0 and int((d_fst != 0).sum().item()) == 0 and
              bool(torch.equal(d_out_b, d_raw)) and bool(torch.equal(d_out_f, d_raw)))
    out = {"row": name, "n": n, "size": size, "block_size_id": bid, "launches": launches, "warmup": warmup,
           "raw_bytes": raw, "body_bytes": body_bytes, "frame_bytes": frame_bytes,
           "ratio_bodies": round(raw / body_bytes, 4), "ratio_frames": round(raw / frame_bytes, 4),
           "compress_block_call": enc[0], "compress_frame_call": enc[1],
           "compress_gain": round(enc[0]["median_ms"] / enc[1]["median_ms"], 3),
           "decompress_block_call": dec[0], "decompress_frame_call": dec[1],
           "decompress_gain": round(dec[0]["median_ms"] / dec[1]["median_ms"], 3),
           "staging_bytes": frame_bytes, "compress_report": enc_rep, "decompress_report": dec_rep,
           "status_ok": enc_ok, "frames_equal_oracle_sample": sample_ok, "roundtrip_ok": dec_ok}
    print(json.dumps(out), flush=True)


def has_option(name):
    try:
        fsg.get_option(name)
        return True
    except Exception:
        return False


def nosize_frames(torch, codec, batch, bid, checksum):
    """(bytes, offsets, lengths as host arrays) of the batch's frames without
    a content size: compressed on the device, the 8-byte field cut out and the
    descriptor's check byte made right on the host."""
    import lz4f_ref
    dev = torch.device("cuda", 0)
    lib = codec.lib
    n = len(batch)
    H = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    f_off, f_tot = fsg.slot_offsets(np.array([lib.fsg_lz4f_max_frame_length(int(x), bid) for x in batch.lens], np.uint64))
    d_f = torch.zeros(f_tot, dtype=torch.uint8, device=dev)
    d_fl = torch.zeros(n, dtype=torch.int32, device=dev)
    d_st = torch.zeros(n, dtype=torch.int32, device=dev)
    ws = codec.lz4f_compress_workspace(n, batch.total, bid)
    codec.lz4f_compress(H(batch.data), H(batch.offsets), H(batch.lens), n, d_f, H(f_off), d_fl, d_st, ws,
                        block_size_id=bid, checksum=checksum)
    torch.cuda.synchronize()
    assert int((d_st != 0).sum().item()) == 0
    host = d_f.cpu().numpy()
    flen = d_fl.cpu().numpy().view(np.uint32).astype(np.uint64)
    lens = (flen - 8).astype(np.uint32)
    offs, total = fsg.slot_offsets(lens.astype(np.uint64))
    out = np.zeros(total, np.uint8)
    for i in range(n):
        a, b = int(f_off[i]), int(offs[i])
        head = bytes(host[a:a + 6])
        assert head[4] & lz4f_ref.F_SIZE
        d = bytes([head[4] & ~lz4f_ref.F_SIZE, head[5]])
        out[b:b + 4] = host[a:a + 4]
        out[b + 4:b + 7] = np.frombuffer(d + bytes([(lz4f_ref.xxh32(d) >> 8) & 0xFF]), np.uint8)
        out[b + 7:b + int(lens[i])] = host[a + 15:a + int(flen[i])]
    return out, offs, lens


def nosize_row(torch, codec, name, bid, checksum, warmup, launches):
    dev = torch.device("cuda", 0)
    n, size = ROWS[name]
    batch = fsg.make_batch(fsg.KIND_TEXT, np.full(n, size, np.uint32))
    H = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    s = torch.cuda.current_stream()
    data, offs, lens = nosize_frames(torch, codec, batch, bid, checksum)
    torch.cuda.empty_cache()
    d_f, d_fo, d_fl = H(data), H(offs), H(lens)
    d_raw, d_ro, d_rl = H(batch.data), H(batch.offsets), H(batch.lens)
    d_out = torch.full((batch.total,), 0xA5, dtype=torch.uint8, device=dev)
    d_ol = torch.zeros(n, dtype=torch.int32, device=dev)
    d_st = torch.zeros(n, dtype=torch.int32, device=dev)
    ws = codec.lz4f_decompress_workspace(n, int(data.size))
    routed = has_option("lz4f_nosize_fast")
    out = {"mode": "no_size", "row": name, "n": n, "size": size, "block_size_id": bid, "checksum": int(checksum),
           "launches": launches, "warmup": warmup, "raw_bytes": batch.total, "frame_bytes": int(lens.sum()),
           "has_option": routed}

    def call(fast):
        def fn():
            if routed:
                fsg.set_option("lz4f_nosize_fast", fast)
            codec.lz4f_decompress(d_f, d_fo, d_fl, n, d_out, d_ro, d_rl, d_ol, d_st, ws, stream=s)
        return fn

    def check():
        return int((d_st != 0).sum().item()) == 0 and bool(torch.equal(d_out, d_raw))

    if routed:
        saved = fsg.get_option("lz4f_nosize_fast")
        ms = alternate(torch, s, (call(0), call(1)), warmup, launches)
        out["serial_call"], out["fast_call"] = ms
        out["gain"] = round(ms[0]["median_ms"] / ms[1]["median_ms"], 3)
        d_out.fill_(0xA5)
        call(1)()
        torch.cuda.synchronize()
        out["fast_ok"] = check()
        out["fast_report"] = codec.lz4f_decompress_report(ws, n)
        length_mode = fsg.get_option("lz4f_length_wave_min")
        out["length_wave_min_option"] = length_mode
        d_out.fill_(0xA5)
        call(0)()
        torch.cuda.synchronize()
        out["serial_ok"] = check()
        fsg.set_option("lz4f_nosize_fast", saved)
    else:
        out["serial_call"] = alternate(torch, s, (call(0),), warmup, launches)[0]
        out["serial_ok"] = check()
    out["serial_report"] = codec.lz4f_decompress_report(ws, n)
    print(json.dumps(out), flush=True)


def linked_frames(torch, codec, batch, bid, sized):
    """(bytes, offsets, lengths as host arrays) of the batch's frames as linked
    frames: compressed on the device, B.Indep cleared and the descriptor's
    check byte made right on the host; without the content size field unless
    `sized`."""
    import lz4f_ref
    dev = torch.device("cuda", 0)
    lib = codec.lib
    n = len(batch)
    H = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    f_off, f_tot = fsg.slot_offsets(np.array([lib.fsg_lz4f_max_frame_length(int(x), bid) for x in batch.lens], np.uint64))
    d_f = torch.zeros(f_tot, dtype=torch.uint8, device=dev)
    d_fl = torch.zeros(n, dtype=torch.int32, device=dev)
    d_st = torch.zeros(n, dtype=torch.int32, device=dev)
    ws = codec.lz4f_compress_workspace(n, batch.total, bid)
    codec.lz4f_compress(H(batch.data), H(batch.offsets), H(batch.lens), n, d_f, H(f_off), d_fl, d_st, ws,
                        block_size_id=bid, checksum=False)
    torch.cuda.synchronize()
    assert int((d_st != 0).sum().item()) == 0
    host = d_f.cpu().numpy()
    flen = d_fl.cpu().numpy().view(np.uint32).astype(np.uint64)
    cut = 0 if sized else 8
    lens = (flen - cut).astype(np.uint32)
    offs, total = fsg.slot_offsets(lens.astype(np.uint64))
    out = np.zeros(total, np.uint8)
    for i in range(n):
        a, b = int(f_off[i]), int(offs[i])
        head = bytes(host[a:a + 14])
        assert head[4] & lz4f_ref.F_SIZE and head[4] & lz4f_ref.F_INDEP
        flg = head[4] & ~lz4f_ref.F_INDEP & (0xFF if sized else ~lz4f_ref.F_SIZE)
        d = bytes([flg, head[5]]) + (head[6:14] if sized else b"")
        hl = 7 + len(d) - 2
        out[b:b + 4] = host[a:a + 4]
        out[b + 4:b + hl] = np.frombuffer(d + bytes([(lz4f_ref.xxh32(d) >> 8) & 0xFF]), np.uint8)
        out[b + hl:b + int(lens[i])] = host[a + 15:a + int(flen[i])]
    return out, offs, lens


def sys_linked_frames(batch, bid):
    """The batch's frames written by the system liblz4 with linked blocks and a
    content size, or None where it is not installed."""
    import lz4f_sys
    L = lz4f_sys.load()
    if L is None:
        return None
    z = lz4f_sys.SysLz4F(L)
    frames = [z.compress_frame(batch.item(i), bid, mode=lz4f_sys.LINKED) for i in range(len(batch))]
    lens = np.array([len(f) for f in frames], np.uint32)
    offs, total = fsg.slot_offsets(lens.astype(np.uint64))
    out = np.zeros(total, np.uint8)
    for f, at in zip(frames, offs):
        out[int(at):int(at) + len(f)] = np.frombuffer(f, np.uint8)
    return out, offs, lens


def linked_row(torch, codec, name, bid, sized, warmup, launches, from_sys=False):
    dev = torch.device("cuda", 0)
    n, size = ROWS[name]
    batch = fsg.make_batch(fsg.KIND_TEXT, np.full(n, size, np.uint32))
    H = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    s = torch.cuda.current_stream()
    routed = has_option("lz4f_linked_fast")
    out = {"mode": "linked", "row": name, "n": n, "size": size, "block_size_id": bid, "sized": int(sized),
           "frames": "liblz4" if from_sys else "device", "launches": launches, "warmup": warmup,
           "raw_bytes": batch.total, "has_option": routed}
    made = sys_linked_frames(batch, bid) if from_sys else linked_frames(torch, codec, batch, bid, sized)
    if made is None:
        out["missing"] = "no system liblz4"
        print(json.dumps(out), flush=True)
        return
    data, offs, lens = made
    torch.cuda.empty_cache()
    out["frame_bytes"] = int(lens.sum())
    d_f, d_fo, d_fl = H(data), H(offs), H(lens)
    d_raw, d_ro, d_rl = H(batch.data), H(batch.offsets), H(batch.lens)
    d_out = torch.full((batch.total,), 0xA5, dtype=torch.uint8, device=dev)
    d_ol = torch.zeros(n, dtype=torch.int32, device=dev)
    d_st = torch.zeros(n, dtype=torch.int32, device=dev)
    ws = codec.lz4f_decompress_workspace(n, int(data.size))
    names = ("lz4f_linked_fast", "lz4f_nosize_fast")

    def call(fast):
        def fn():
            if routed:
                for k in names:
                    fsg.set_option(k, fast)
            codec.lz4f_decompress(d_f, d_fo, d_fl, n, d_out, d_ro, d_rl, d_ol, d_st, ws, stream=s)
        return fn

    def check():
        return int((d_st != 0).sum().item()) == 0 and bool(torch.equal(d_out, d_raw))

    if routed:
        saved = [fsg.get_option(k) for k in names]
        ms = alternate(torch, s, (call(0), call(1)), warmup, launches)
        out["serial_call"], out["fast_call"] = ms
        out["gain"] = round(ms[0]["median_ms"] / ms[1]["median_ms"], 3)
        d_out.fill_(0xA5)
        call(1)()
        torch.cuda.synchronize()
        out["fast_ok"] = check()
        out["fast_report"] = codec.lz4f_decompress_report(ws, n)
        d_out.fill_(0xA5)
        call(0)()
        torch.cuda.synchronize()
        out["serial_ok"] = check()
        for k, v in zip(names, saved):
            fsg.set_option(k, v)
    else:
        out["serial_call"] = alternate(torch, s, (call(0),), warmup, launches)[0]
        out["serial_ok"] = check()
    out["serial_report"] = codec.lz4f_decompress_report(ws, n)
    print(json.dumps(out), flush=True)


def length_pass(torch, codec, warmup, launches, limit_bytes=2 << 30):
    """Lane against wave for the length pass alone."""
    dev = torch.device("cuda", 0)
    H = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    s = torch.cuda.current_stream()
    saved = fsg.get_option("lz4f_length_wave_min")
    for size in (4 << 10, 16 << 10, 64 << 10, 256 << 10, 1 << 20, 4 << 20):
        for count in (1, 64, 4096):
            if size * count > limit_bytes:
                print(json.dumps({"mode": "length_pass", "block_bytes": size, "blocks": count, "skipped": "too large"}),
                      flush=True)
                continue
            batch = fsg.make_batch(fsg.KIND_TEXT, np.full(count, size, np.uint32))
            data, offs, lens = nosize_frames(torch, codec, batch, 7, False)
            d_f, d_fo, d_fl = H(data), H(offs), H(lens)
            d_len = torch.zeros(count, dtype=torch.int64, device=dev)
            d_st = torch.zeros(count, dtype=torch.int32, device=dev)
            ws = codec.lz4f_decompress_workspace(count, int(data.size))

            def call(wave_min):
                def fn():
                    fsg.set_option("lz4f_length_wave_min", wave_min)
                    codec.lz4f_decoded_lengths(d_f, d_fo, d_fl, count, d_len, d_st, ws, stream=s)
                return fn
            ms = alternate(torch, s, (call(NONE), call(0)), warmup, launches)
            ok = int((d_st != 0).sum().item()) == 0 and bool((d_len == size).all().item())
            print(json.dumps({"mode": "length_pass", "block_bytes": size, "blocks": count,
                              "stored_bytes_mean": int(lens.mean()) - 15, "lane_call": ms[0], "wave_call": ms[1],
                              "lane_over_wave": round(ms[0]["median_ms"] / ms[1]["median_ms"], 3), "ok": ok}),
                  flush=True)
            del d_f, ws
            torch.cuda.empty_cache()
    fsg.set_option("lz4f_length_wave_min", saved)


SUM_FLAGS = {"none": 0, "content": 1, "block": 2, "both": 3}


def sums_row(torch, codec, name, bid, warmup, launches, only=None, time_compress=True):
    """The row's sized frames without checksums, with a content checksum, with
    block checksums and with both, compress and decompress, the variants
    alternating launch by launch in one process: a checksum's share is the
    difference of two figures of this line.  A library without
    fsg_lz4f_max_frame_length_flags gives "none" and "content" alone."""
    dev = torch.device("cuda", 0)
    lib = codec.lib
    n, size = ROWS[name]
    batch = fsg.make_batch(fsg.KIND_TEXT, np.full(n, size, np.uint32))
    raw = batch.total
    H = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    s = torch.cuda.current_stream()
    d_raw, d_ro, d_rl = H(batch.data), H(batch.offsets), H(batch.lens)
    flagged = hasattr(lib, "fsg_lz4f_max_frame_length_flags")
    kinds = [k for k, f in SUM_FLAGS.items() if (flagged or f < 2) and (only is None or k in only)]
    bound = (lambda x: lib.fsg_lz4f_max_frame_length_flags(x, bid, 3)) if flagged else \
        (lambda x: lib.fsg_lz4f_max_frame_length(x, bid))
    f_off, f_tot = fsg.slot_offsets(np.array([bound(int(x)) for x in batch.lens], np.uint64))
    d_fo = H(f_off)
    ws = codec.lz4f_compress_workspace(n, raw, bid)
    bufs = {k: (torch.zeros(f_tot, dtype=torch.uint8, device=dev), torch.zeros(n, dtype=torch.int32, device=dev),
                torch.zeros(n, dtype=torch.int32, device=dev)) for k in kinds}

    def enc(k):
        d_f, d_fl, d_st = bufs[k]
        if flagged:
            return lambda: codec.lz4f_compress(d_raw, d_ro, d_rl, n, d_f, d_fo, d_fl, d_st, ws, block_size_id=bid,
                                               flags=SUM_FLAGS[k], stream=s)
        return lambda: codec.lz4f_compress(d_raw, d_ro, d_rl, n, d_f, d_fo, d_fl, d_st, ws, block_size_id=bid,
                                           checksum=bool(SUM_FLAGS[k]), stream=s)

    out = {"mode": "sums", "row": name, "n": n, "size": size, "block_size_id": bid, "launches": launches,
           "warmup": warmup, "raw_bytes": raw, "has_flags": flagged}
    if time_compress:
        for k, m in zip(kinds, alternate(torch, s, [enc(k) for k in kinds], warmup, launches)):
            out["compress_" + k] = m
    else:  # (the frames are needed all the same)
        for k in kinds:
            enc(k)()
        torch.cuda.synchronize()
    ok = all(int((bufs[k][2] != 0).sum().item()) == 0 for k in kinds)
    del ws
    torch.cuda.empty_cache()
    d_out = torch.full((raw,), 0xA5, dtype=torch.uint8, device=dev)
    d_ol = torch.zeros(n, dtype=torch.int32, device=dev)
    d_st = torch.zeros(n, dtype=torch.int32, device=dev)
    dws = codec.lz4f_decompress_workspace(n, int(f_tot))

    def dec(k):
        d_f, d_fl, _ = bufs[k]
        return lambda: codec.lz4f_decompress(d_f, d_fo, d_fl, n, d_out, d_ro, d_rl, d_ol, d_st, dws, stream=s)

    for k, m in zip(kinds, alternate(torch, s, [dec(k) for k in kinds], warmup, launches)):
        out["decompress_" + k] = m
    for k in kinds:
        d_out.fill_(0xA5)
        dec(k)()
        torch.cuda.synchronize()
        ok = ok and int((d_st != 0).sum().item()) == 0 and bool(torch.equal(d_out, d_raw))
        out["checksummed_units_" + k] = codec.lz4f_decompress_report(dws, n)["checksummed_units"]
    out["ok"] = ok
    print(json.dumps(out), flush=True)


XXH_ROWS = {"1x4m": (1, 4 << 20), "16x4m": (16, 4 << 20), "1024x64k": (1024, 64 << 10), "c3": (65536, 64 << 10)}


def xxh_row(torch, codec, name, warmup, launches):
    """fsg_lz4f_xxh32_batch alone on the row's bodies."""
    dev = torch.device("cuda", 0)
    n, size = XXH_ROWS[name]
    batch = fsg.make_batch(fsg.KIND_TEXT, np.full(n, size, np.uint32))
    H = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    s = torch.cuda.current_stream()
    d_raw, d_ro, d_rl = H(batch.data), H(batch.offsets), H(batch.lens)
    d_x = torch.zeros(n, dtype=torch.int32, device=dev)
    m = alternate(torch, s, [lambda: codec.lz4f_xxh32(d_raw, d_ro, d_rl, n, d_x, stream=s)], warmup, launches)[0]
    import lz4f_ref
    got = d_x.cpu().numpy().view(np.uint32)
    sample = [0, n - 1] if size > (1 << 20) else list(np.linspace(0, n - 1, 4).astype(np.int64))
    ok = all(int(got[i]) == lz4f_ref.xxh32(batch.item(int(i))) for i in set(int(v) for v in sample))
    print(json.dumps({"mode": "xxh", "row": name, "n": n, "size": size, "launches": launches, "warmup": warmup,
                      "call": m, "gib_per_s": round(batch.total / 2**30 / (m["median_ms"] / 1e3), 2),
                      "sample_equals_oracle": ok}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sums", action="store_true",
                    help="sized frames without / with content / block / both checksums (rows as row[@id])")
    ap.add_argument("--kinds", default="", help="--sums: a subset of none,content,block,both")
    ap.add_argument("--decompress-only", action="store_true", help="--sums: compress once, untimed")
    ap.add_argument("--xxh", action="store_true", help="fsg_lz4f_xxh32_batch alone (rows of XXH_ROWS)")
    ap.add_argument("--rows", default="16x4m,c3")
    ap.add_argument("--no-size", action="store_true", help="frames without a content size: serial against routed")
    ap.add_argument("--checksum", type=int, default=0, help="--no-size: frames with a content checksum")
    ap.add_argument("--length-pass", action="store_true", help="the length pass alone: lane against wave")
    ap.add_argument("--linked", action="store_true", help="linked frames, sized and not: serial against a wave per frame")
    ap.add_argument("--sys-linked", type=int, default=0, help="--linked: also 16x4m at id 4 written by the system liblz4")
    ap.add_argument("--bid", type=int, default=4, help="block size id 4..7")
    ap.add_argument("--launches", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("lz4f_bench needs a GPU")
    codec = fsg.SnappyGPU(0)
    if a.length_pass:
        length_pass(torch, codec, a.warmup, a.launches)
        return
    if a.xxh:
        for name in ("1x4m,16x4m,1024x64k,c3" if a.rows == "16x4m,c3" else a.rows).split(","):
            xxh_row(torch, codec, name, a.warmup, a.launches)
            torch.cuda.empty_cache()
        return
    if a.sums:
        for item in ("16x4m@4,16x4m@7" if a.rows == "16x4m,c3" else a.rows).split(","):
            name, _, spec = item.partition("@")
            sums_row(torch, codec, name, int(spec) if spec else a.bid, a.warmup, a.launches,
                     only=a.kinds.split(",") if a.kinds else None, time_compress=not a.decompress_only)
            torch.cuda.empty_cache()
        return
    if a.linked:
        rows = "16x4m@4,16x4m@7,4096x128k@4,1x128k@4" if a.rows == "16x4m,c3" else a.rows
        for item in rows.split(","):
            name, _, spec = item.partition("@")
            for sized in (True, False):
                linked_row(torch, codec, name, int(spec) if spec else a.bid, sized, a.warmup, a.launches)
                torch.cuda.empty_cache()
        if a.sys_linked:
            linked_row(torch, codec, "16x4m", 4, True, a.warmup, a.launches, from_sys=True)
        return
    for name in a.rows.split(","):
        if a.no_size:  # row[@id[c]]: a block size id and a content checksum of the row's own
            name, _, spec = name.partition("@")
            bid = int(spec.rstrip("c")) if spec.rstrip("c") else a.bid
            nosize_row(torch, codec, name, bid, spec.endswith("c") or bool(a.checksum), a.warmup, a.launches)
        else:
            row(torch, codec, name, a.bid, a.warmup, a.launches)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
