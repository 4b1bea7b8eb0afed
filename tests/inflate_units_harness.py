"""GPU-test plumbing for the unit-index calls (include/flare_deflate_index_gpu.h),
beside tests/inflate_harness.py and on the same containment guards: the output
buffer is POISON, slots lie under the named layout, result columns carry a
sentinel tail, inputs are compared after the call -- and the workspace has a
poison guard behind it, which must be as it was."""
from __future__ import annotations

import numpy as np

import containment as ct
import fsg
from gpu_harness import Inputs, check_call, guarded_column, guarded_workspace, poisoned
from inflate_harness import skewed_batch


class InflateUnitsGpu:
    def __init__(self):
        import torch
        self.torch = torch
        self.codec = fsg.SnappyGPU(torch.cuda.current_device())
        self.lib = self.codec.lib

    def workspace(self, n, extra_units, fill=0x5C):
        ws, whole = guarded_workspace(self.lib.fsg_inflate_units_workspace_bytes(n, extra_units))
        ws.fill_(fill)  # any bytes on entry
        return ws, whole

    def inflate(self, bodies, caps, fmt, layout="guarded", extra_units=4096):
        """fsg_inflate_units_batch.  Returns (slot contents up to min(length,
        capacity), lengths, statuses, report)."""
        torch = self.torch
        n = len(bodies)
        data, offs, lens = skewed_batch(bodies)
        caps = np.array(caps, dtype=np.uint32)
        lay = ct.LAYOUTS[layout](caps)
        ins = Inputs(d_in=data, d_in_off=offs, d_in_len=lens, d_out_off=lay.offs, d_out_cap=caps)
        d_out = poisoned(lay.total)
        d_ol = guarded_column(n, torch.int32)
        d_st = guarded_column(n, torch.int32, -7)
        ws, whole = self.workspace(n, extra_units)
        self.codec.inflate_units(ins["d_in"], ins["d_in_off"], ins["d_in_len"], n, d_out, ins["d_out_off"],
                                 ins["d_out_cap"], d_ol, d_st, ws, fmt=fmt)
        torch.cuda.synchronize()
        out = d_out.cpu().numpy()
        check_call(out, lay, caps, {"d_out_len": d_ol, "d_status": d_st}, n, whole, ins)
        ol = d_ol.cpu().numpy()[:n].view(np.uint32)
        st = d_st.cpu().numpy()[:n]
        oo = lay.offs
        outs = [out[int(oo[i]):int(oo[i]) + int(min(ol[i], caps[i]))].tobytes() for i in range(n)]
        return outs, ol, st, self.codec.inflate_units_report(ws, n)

    def lengths(self, bodies, fmt, extra_units=4096):
        """fsg_inflate_units_lengths_batch: (lengths, statuses, report)."""
        torch = self.torch
        n = len(bodies)
        data, offs, lens = skewed_batch(bodies)
        ins = Inputs(d_in=data, d_in_off=offs, d_in_len=lens)
        d_len = guarded_column(n, torch.int64)
        d_st = guarded_column(n, torch.int32, -7)
        ws, whole = self.workspace(n, extra_units)
        self.codec.inflate_units_lengths(ins["d_in"], ins["d_in_off"], ins["d_in_len"], n, d_len, d_st, ws, fmt=fmt)
        torch.cuda.synchronize()
        ct.check_column(d_len.cpu().numpy(), n, "d_length")
        ct.check_column(d_st.cpu().numpy(), n, "d_status")
        ct.check_workspace_guard(whole[-ct.WORKSPACE_GUARD:].cpu().numpy())
        ins.check()
        return (d_len.cpu().numpy()[:n].view(np.uint64), d_st.cpu().numpy()[:n],
                self.codec.inflate_units_report(ws, n))

    def deflate_flags(self, datas, fmt, level, flags, layout="guarded"):
        """fsg_deflate_batch_flags into slots of fsg_deflate_max_length_flags
        bytes.  Returns (bodies, statuses, the whole output image check done)."""
        torch = self.torch
        n = len(datas)
        data, offs, lens = skewed_batch(datas)
        caps = np.array([self.lib.fsg_deflate_max_length_flags(len(x), fmt, flags) for x in datas], dtype=np.uint64)
        lay = ct.LAYOUTS[layout](caps)
        ins = Inputs(d_in=data, d_in_off=offs, d_in_len=lens, d_out_off=lay.offs)
        d_out = poisoned(lay.total)
        d_ol = guarded_column(n, torch.int32)
        d_st = guarded_column(n, torch.int32, -7)
        ws, whole = guarded_workspace(self.lib.fsg_deflate_workspace_bytes(n, int(lens.sum())))
        self.codec.deflate_flags(ins["d_in"], ins["d_in_off"], ins["d_in_len"], n, d_out, ins["d_out_off"], d_ol, d_st,
                                 ws, fmt=fmt, level=level, flags=flags)
        torch.cuda.synchronize()
        out = d_out.cpu().numpy()
        check_call(out, lay, caps, {"d_out_len": d_ol, "d_status": d_st}, n, whole, ins)
        ol = d_ol.cpu().numpy()[:n].view(np.uint32)
        st = d_st.cpu().numpy()[:n]
        assert (ol <= caps).all()
        bodies = [out[int(lay.offs[i]):int(lay.offs[i]) + int(ol[i])].tobytes() for i in range(n)]
        # the call writes only the bytes below d_out_len: the slot tails stay POISON too
        image, _ = ct.expected_image(lay, caps, ol, bodies, st)
        bad = np.nonzero(out != image)[0]
        assert bad.size == 0, f"{layout}: first difference at byte {int(bad[0])} of the output buffer"
        return bodies, st
