"""GPU-test plumbing for fsg_deflate_batch_level
(include/flare_deflate_level_gpu.h): tests/deflate_harness.py's calls with a
level, on the same write-containment guards (tests/containment.py) -- slots
of fsg_deflate_max_length bytes in a POISON buffer under the named layout,
result columns with a sentinel tail, a workspace with a poison guard behind
it, inputs compared after the call."""
from __future__ import annotations

import numpy as np

import containment as ct
import fsg
from deflate_harness import DeflateGpu
from gpu_harness import Inputs, check_call, guarded_column, guarded_workspace, poisoned
from inflate_harness import skewed_batch


class DeflateLevelGpu(DeflateGpu):
    def run(self, datas, fmt, level, layout="guarded", ws_fill=None, ws_total=None):
        """One call (level None: the level-less entry).  Returns the output
        buffer's host copy, the layout, the capacities, lengths, statuses, the
        report and the device state for a round trip; the guards are checked."""
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
                           fmt=fmt, level=level)
        torch.cuda.synchronize()
        out = d_out.cpu().numpy()
        check_call(out, lay, caps, {"d_out_len": d_ol, "d_status": d_st}, n, whole, ins)
        ol = d_ol.cpu().numpy()[:n].view(np.uint32)
        st = d_st.cpu().numpy()[:n]
        assert (ol <= caps).all()
        report = self.codec.deflate_report(ws, n)
        return out, lay, caps, ol, st, report, (d_out, ins["d_out_off"], d_ol)

    def bodies(self, datas, fmt, level, **kw):
        """(bodies, lengths, statuses, report)."""
        out, lay, _, ol, st, report, _ = self.run(datas, fmt, level, **kw)
        return [out[int(lay.offs[i]):int(lay.offs[i]) + int(ol[i])].tobytes() for i in range(len(datas))], ol, st, report

    def check_image(self, datas, fmt, level, layout, bodies_want):
        """The whole output buffer against the model: the slots hold the
        model's bytes, the slot tails and everything outside are POISON.
        Returns the output buffer's host copy and the device state."""
        out, lay, caps, ol, st, _, dev = self.run(datas, fmt, level, layout=layout)
        assert (st == fsg.FSG_OK).all(), st
        assert [int(v) for v in ol] == [len(b) for b in bodies_want]
        image, _ = ct.expected_image(lay, caps, ol, bodies_want, st)
        bad = np.nonzero(out != image)[0]
        assert bad.size == 0, f"{layout}, level {level}: first difference at byte {int(bad[0])} of the output buffer"
        return out, dev
