"""GPU-test plumbing for the inflate calls (include/flare_deflate_gpu.h), on
the write-containment guards of tests/containment.py as tests/gpu_harness.py
uses them: the output buffer is POISON before the call, slots are laid out with
poison guards between them (or adjacent, or skewed to every alignment), the
result columns carry a sentinel tail, and after the call every byte outside
the slots, the column tails and the input arrays must be as they were."""
from __future__ import annotations

import numpy as np

import containment as ct
import fsg
from gpu_harness import Inputs, check_call, guarded_column, poisoned


def skewed_batch(bodies):
    """The bodies in one buffer with body i at residue (5 * i) % 16, so inputs
    of every alignment, with a poison byte or more between neighbours."""
    offs, pos = [], 3
    for i, b in enumerate(bodies):
        pos += ((5 * i) % 16 - pos) % 16
        offs.append(pos)
        pos += len(b) + 1
    data = np.full(pos + 16, ct.POISON, dtype=np.uint8)
    for o, b in zip(offs, bodies):
        data[o:o + len(b)] = np.frombuffer(b, dtype=np.uint8)
    return data, np.array(offs, dtype=np.uint64), np.array([len(b) for b in bodies], dtype=np.uint32)


class InflateGpu:
    def __init__(self):
        import torch
        self.torch = torch
        self.codec = fsg.SnappyGPU(torch.cuda.current_device())

    def inflate(self, bodies, caps, fmt, layout="guarded"):
        """fsg_inflate_batch on the bodies with the given capacities; slots by
        the named containment layout ("guarded" covers every alignment 0..15).
        Returns (slot contents up to min(length, capacity), lengths, statuses)."""
        torch = self.torch
        n = len(bodies)
        data, offs, lens = skewed_batch(bodies)
        caps = np.array(caps, dtype=np.uint32)
        lay = ct.LAYOUTS[layout](caps)
        ins = Inputs(d_in=data, d_in_off=offs, d_in_len=lens, d_out_off=lay.offs, d_out_cap=caps)
        d_out = poisoned(lay.total)
        d_ol = guarded_column(n, torch.int32)
        d_st = guarded_column(n, torch.int32, -7)
        self.codec.inflate(ins["d_in"], ins["d_in_off"], ins["d_in_len"], n, d_out, ins["d_out_off"],
                           ins["d_out_cap"], d_ol, d_st, fmt=fmt)
        torch.cuda.synchronize()
        out = d_out.cpu().numpy()
        check_call(out, lay, caps, {"d_out_len": d_ol, "d_status": d_st}, n, None, ins)
        ol = d_ol.cpu().numpy()[:n].view(np.uint32)
        st = d_st.cpu().numpy()[:n]
        oo = lay.offs
        outs = [out[int(oo[i]):int(oo[i]) + int(min(ol[i], caps[i]))].tobytes() for i in range(n)]
        return outs, ol, st

    def lengths(self, bodies, fmt):
        torch = self.torch
        n = len(bodies)
        data, offs, lens = skewed_batch(bodies)
        ins = Inputs(d_in=data, d_in_off=offs, d_in_len=lens)
        d_len = guarded_column(n, torch.int64)
        d_st = guarded_column(n, torch.int32, -7)
        self.codec.inflate_lengths(ins["d_in"], ins["d_in_off"], ins["d_in_len"], n, d_len, d_st, fmt=fmt)
        torch.cuda.synchronize()
        ct.check_column(d_len.cpu().numpy(), n, "d_length")
        ct.check_column(d_st.cpu().numpy(), n, "d_status")
        ins.check()
        return d_len.cpu().numpy()[:n].view(np.uint64), d_st.cpu().numpy()[:n]

    def checksums(self, data: np.ndarray, offs, lens, adler: bool):
        """fsg_crc32_batch / fsg_adler32_batch over ranges of one buffer."""
        torch = self.torch
        n = len(lens)
        ins = Inputs(d_in=data, d_in_off=np.asarray(offs, dtype=np.uint64), d_in_len=np.asarray(lens, dtype=np.uint32))
        d_sum = guarded_column(n, torch.int32)
        (self.codec.adler32 if adler else self.codec.crc32)(ins["d_in"], ins["d_in_off"], ins["d_in_len"], n, d_sum)
        torch.cuda.synchronize()
        ct.check_column(d_sum.cpu().numpy(), n, "d_sum")
        ins.check()
        return d_sum.cpu().numpy()[:n].view(np.uint32)
