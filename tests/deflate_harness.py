"""GPU-test plumbing for fsg_deflate_batch (include/flare_deflate_compress_gpu.h),
on the write-containment guards of tests/containment.py as
tests/inflate_harness.py uses them: slots of fsg_deflate_max_length bytes in a
POISON buffer under the named layout, result columns with a sentinel tail, a
workspace with a poison guard behind it, inputs compared after the call."""
from __future__ import annotations

import numpy as np

import containment as ct
import fsg
from gpu_harness import Inputs, check_call, guarded_column, guarded_workspace, poisoned
from inflate_harness import skewed_batch


class DeflateGpu:
    def __init__(self):
        import torch
        self.torch = torch
        self.codec = fsg.SnappyGPU(torch.cuda.current_device())
        self.lib = self.codec.lib

    def deflate(self, datas, fmt, layout="guarded", ws_fill=None, ws_total=None, keep_device=False):
        """fsg_deflate_batch on the inputs (skewed_batch: every input alignment).
        Returns (bodies, lengths, statuses, report[, device state for a round trip])."""
        torch = self.torch
        n = len(datas)
        data, offs, lens = skewed_batch(datas)
        caps = np.array([self.lib.fsg_deflate_max_length(len(x), fmt) for x in datas], dtype=np.uint64)
        lay = ct.LAYOUTS[layout](caps)
        ins = Inputs(d_in=data, d_in_off=offs, d_in_len=lens, d_out_off=lay.offs)
        d_out = poisoned(lay.total)
        d_ol = guarded_column(n, torch.int32)
        d_st = guarded_column(n, torch.int32, -7)
        total = int(lens.sum()) if ws_total is None else ws_total
        ws, whole = guarded_workspace(self.lib.fsg_deflate_workspace_bytes(n, total))
        if ws_fill is not None:
            ws.fill_(ws_fill)
        self.codec.deflate(ins["d_in"], ins["d_in_off"], ins["d_in_len"], n, d_out, ins["d_out_off"], d_ol, d_st, ws,
                           fmt=fmt)
        torch.cuda.synchronize()
        out = d_out.cpu().numpy()
        check_call(out, lay, caps, {"d_out_len": d_ol, "d_status": d_st}, n, whole, ins)
        ol = d_ol.cpu().numpy()[:n].view(np.uint32)
        st = d_st.cpu().numpy()[:n]
        assert (ol <= caps).all()
        bodies = [out[int(lay.offs[i]):int(lay.offs[i]) + int(ol[i])].tobytes() for i in range(n)]
        report = self.codec.deflate_report(ws, n) if n else None
        if keep_device:
            return bodies, ol, st, report, (d_out, ins["d_out_off"], d_ol)
        return bodies, ol, st, report

    def check_image(self, datas, fmt, layout, bodies_want):
        """The whole output buffer against the model: the slots hold the
        model's bytes, the slot tails and everything outside are POISON."""
        torch = self.torch
        n = len(datas)
        data, offs, lens = skewed_batch(datas)
        caps = np.array([self.lib.fsg_deflate_max_length(len(x), fmt) for x in datas], dtype=np.uint64)
        lay = ct.LAYOUTS[layout](caps)
        ins = Inputs(d_in=data, d_in_off=offs, d_in_len=lens, d_out_off=lay.offs)
        d_out = poisoned(lay.total)
        d_ol = guarded_column(n, torch.int32)
        d_st = guarded_column(n, torch.int32, -7)
        ws, whole = guarded_workspace(self.lib.fsg_deflate_workspace_bytes(n, int(lens.sum())))
        self.codec.deflate(ins["d_in"], ins["d_in_off"], ins["d_in_len"], n, d_out, ins["d_out_off"], d_ol, d_st, ws,
                           fmt=fmt)
        torch.cuda.synchronize()
        out = d_out.cpu().numpy()
        check_call(out, lay, caps, {"d_out_len": d_ol, "d_status": d_st}, n, whole, ins)
        st = d_st.cpu().numpy()[:n]
        assert (st == fsg.FSG_OK).all(), st
        ol = d_ol.cpu().numpy()[:n].view(np.uint32)
        assert [int(v) for v in ol] == [len(b) for b in bodies_want]
        image, _ = ct.expected_image(lay, caps, ol, bodies_want, st)
        # the call writes only the bytes below d_out_len: the slot tails stay POISON too
        bad = np.nonzero(out != image)[0]
        assert bad.size == 0, f"{layout}: first difference at byte {int(bad[0])} of the output buffer"
        return d_out, ins["d_out_off"], d_ol, lay

    def inflate_device(self, d_bodies, d_body_off, d_body_len, datas, fmt):
        """The feature's own round trip: the compress call's output buffer,
        still on the device, through fsg_inflate_batch."""
        torch = self.torch
        n = len(datas)
        caps = np.array([len(x) for x in datas], dtype=np.uint32)
        lay = ct.aligned(caps)
        d_out = poisoned(lay.total)
        d_cap = torch.from_numpy(caps.view(np.int32)).cuda()
        d_off = torch.from_numpy(lay.offs.view(np.int64)).cuda()
        d_ol = guarded_column(n, torch.int32)
        d_st = guarded_column(n, torch.int32, -7)
        self.codec.inflate(d_bodies, d_body_off, d_body_len, n, d_out, d_off, d_cap, d_ol, d_st, fmt=fmt)
        torch.cuda.synchronize()
        out = d_out.cpu().numpy()
        st = d_st.cpu().numpy()[:n]
        ol = d_ol.cpu().numpy()[:n].view(np.uint32)
        outs = [out[int(lay.offs[i]):int(lay.offs[i]) + int(ol[i])].tobytes() for i in range(n)]
        return outs, st
