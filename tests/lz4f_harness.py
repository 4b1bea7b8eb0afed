"""GPU-test plumbing of the LZ4 frame calls (include/flare_lz4_gpu.h, "LZ4
frames"), in the manner of gpu_harness.GpuCodec: every call runs under the
write-containment guards of tests/containment.py, on a workspace filled with
0xFF first (the calls must not rely on a zeroed one), and comes back with the
call's path report."""
from __future__ import annotations

import numpy as np

import containment as ct
import fsg
from gpu_harness import GpuCodec, Inputs, check_call, guarded_column, guarded_workspace, poisoned


class Lz4fGpu:
    def __init__(self):
        self.g = GpuCodec()
        self.codec, self.lib, self.torch = self.g.codec, self.g.codec.lib, self.g.torch

    def compress(self, xs: list[bytes], bid: int = 4, checksum: bool = False, ws_total_in: int | None = None):
        """(frames, statuses, report) of fsg_lz4f_compress_batch."""
        torch = self.torch
        batch = fsg.Batch.from_list(xs)
        n = len(batch)
        caps = np.array([self.lib.fsg_lz4f_max_frame_length(int(x), bid) for x in batch.lens], dtype=np.uint64)
        lay = ct.aligned(caps)
        ins = Inputs(d_in=batch.data, d_in_off=batch.offsets, d_in_len=batch.lens, d_out_off=lay.offs)
        d_out = poisoned(lay.total)
        d_ol = guarded_column(n, torch.int32)
        d_st = guarded_column(n, torch.int32, -7)
        total = batch.total if ws_total_in is None else ws_total_in
        ws, whole = guarded_workspace(self.lib.fsg_lz4f_compress_workspace_bytes(n, total, bid))
        ws.fill_(0xFF)
        self.codec.lz4f_compress(ins["d_in"], ins["d_in_off"], ins["d_in_len"], n, d_out, ins["d_out_off"], d_ol, d_st,
                                 ws, block_size_id=bid, checksum=checksum)
        torch.cuda.synchronize()
        out = d_out.cpu().numpy()
        check_call(out, lay, caps, {"d_out_len": d_ol, "d_status": d_st}, n, whole, ins)
        ol = d_ol.cpu().numpy()[:n].view(np.uint32)
        st = d_st.cpu().numpy()[:n]
        assert (ol <= caps).all()
        frames = [out[int(lay.offs[i]):int(lay.offs[i]) + int(ol[i])].tobytes() for i in range(n)]
        return frames, st, (self.codec.lz4f_compress_report(ws, n, bid) if n else None)

    def decompress(self, frames: list[bytes], caps, ws_total_in: int | None = None):
        """(outputs, d_out_len, statuses, report) of fsg_lz4f_decompress_batch."""
        torch = self.torch
        b = fsg.Batch.from_list(frames)
        n = len(b)
        caps = np.array(caps, dtype=np.uint32)
        lay = ct.aligned(caps)
        ins = Inputs(d_in=b.data, d_in_off=b.offsets, d_in_len=b.lens, d_out_off=lay.offs, d_out_cap=caps)
        d_out = poisoned(lay.total)
        d_ol = guarded_column(n, torch.int32)
        d_st = guarded_column(n, torch.int32, -7)
        total = int(b.data.size) if ws_total_in is None else ws_total_in
        ws, whole = guarded_workspace(self.lib.fsg_lz4f_decompress_workspace_bytes(n, total))
        ws.fill_(0xFF)
        self.codec.lz4f_decompress(ins["d_in"], ins["d_in_off"], ins["d_in_len"], n, d_out, ins["d_out_off"],
                                   ins["d_out_cap"], d_ol, d_st, ws)
        torch.cuda.synchronize()
        out = d_out.cpu().numpy()
        check_call(out, lay, caps, {"d_out_len": d_ol, "d_status": d_st}, n, whole, ins)
        ol = d_ol.cpu().numpy()[:n].view(np.uint32)
        st = d_st.cpu().numpy()[:n]
        outs = [out[int(lay.offs[i]):int(lay.offs[i]) + int(min(ol[i], caps[i]))].tobytes() for i in range(n)]
        return outs, ol, st, (self.codec.lz4f_decompress_report(ws, n) if n else None)

    def content_sizes(self, frames: list[bytes]):
        """(sizes as uint64, statuses) of fsg_lz4f_content_sizes_batch."""
        torch = self.torch
        b = fsg.Batch.from_list(frames)
        n = len(b)
        ins = Inputs(d_in=b.data, d_in_off=b.offsets, d_in_len=b.lens)
        d_sz = guarded_column(n, torch.int64)
        d_st = guarded_column(n, torch.int32, -7)
        self.codec.lz4f_content_sizes(ins["d_in"], ins["d_in_off"], ins["d_in_len"], n, d_sz, d_st)
        torch.cuda.synchronize()
        ct.check_column(d_sz.cpu().numpy(), n, "d_content_size")
        ct.check_column(d_st.cpu().numpy(), n, "d_status")
        ins.check()
        return d_sz.cpu().numpy()[:n].view(np.uint64), d_st.cpu().numpy()[:n]
