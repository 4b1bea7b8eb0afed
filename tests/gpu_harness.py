"""Shared GPU-test plumbing: move host batches to the device, run the C ABI,
bring results back.  torch is used only for device allocations/streams.

Output slots are filled with POISON (0xA5) before every call, never zeros: an
output byte a kernel fails to write then shows up as 0xA5 instead of passing
whenever its true value happens to be 0.

Every call here also runs under the write-containment guards of
tests/containment.py ("What a *_batch call writes" in
include/flare_snappy_gpu.h): the slots keep their 16-byte-aligned starts with
64 poison bytes after each, the result columns carry a sentinel tail, the
workspace is a view of an allocation 256 bytes longer, and after the call
every byte outside the slots, the column tails, the bytes past the workspace
and the input arrays must be as they were."""
from __future__ import annotations

import numpy as np

import containment as ct
import fsg

POISON = ct.POISON


def dev(a: np.ndarray, device="cuda"):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def poisoned(total: int, device="cuda"):
    """An output buffer of `total` POISON bytes."""
    import torch
    return torch.full((max(int(total), 1),), POISON, dtype=torch.uint8, device=device)


def guarded_column(n: int, dtype, fill=None, device="cuda"):
    """A result column of n entries (`fill`, default the sentinel) followed by
    ct.COLUMN_TAIL sentinel entries."""
    import torch
    col = torch.full((n + ct.COLUMN_TAIL,), ct.SENTINEL, dtype=dtype, device=device)
    if fill is not None:
        col[:n] = fill
    return col


def guarded_workspace(nbytes, zero: bool = False, device="cuda"):
    """(view, whole): a workspace of max(nbytes, 1) bytes as the first bytes
    of an allocation ct.WORKSPACE_GUARD bytes longer, the surplus POISON.  The
    call is given the view (the binding passes numel() as workspace_bytes).
    nbytes None: no workspace."""
    import torch
    if nbytes is None:
        return None, None
    nbytes = max(int(nbytes), 1)
    whole = (torch.zeros if zero else torch.empty)(nbytes + ct.WORKSPACE_GUARD, dtype=torch.uint8, device=device)
    whole[nbytes:] = POISON
    return whole[:nbytes], whole


class Inputs:
    """Device copies of a call's input arrays, compared with their host
    originals after the call (item 5 of the contract: never written)."""

    def __init__(self, **arrays):
        self.host = {k: np.ascontiguousarray(v) for k, v in arrays.items()}
        self.dev = {k: dev(v) for k, v in self.host.items()}

    def __getitem__(self, k):
        return self.dev[k]

    def check(self):
        for k, h in self.host.items():
            ct.check_unwritten(self.dev[k].cpu().numpy(), h, k)


def check_call(out, layout, caps, columns, n, whole_ws, inputs, what="d_out"):
    """After a synchronised call: every byte outside the slots, each column's
    tail, the bytes past the workspace, the inputs."""
    ct.check_outside(out, layout, caps, what)
    for name, col in columns.items():
        ct.check_column(col.cpu().numpy(), n, name)
    if whole_ws is not None:
        ct.check_workspace_guard(whole_ws[-ct.WORKSPACE_GUARD:].cpu().numpy())
    inputs.check()


class GpuCodec:
    def __init__(self, use_workspace: bool = True):
        import torch
        self.use_workspace = use_workspace
        self.torch = torch
        self.codec = fsg.SnappyGPU(torch.cuda.current_device())
        # the path report of the last compress / decompress call
        # (fsg_compress_report / fsg_decompress_report), as a dict
        self.last_report = None

    def compress(self, batch: fsg.Batch):
        torch = self.torch
        n = len(batch)
        caps = np.array([fsg.max_compressed_length(int(x)) for x in batch.lens], dtype=np.uint64)
        lay = ct.aligned(caps)
        oo = lay.offs
        ins = Inputs(d_in=batch.data, d_in_off=batch.offsets, d_in_len=batch.lens, d_out_off=oo)
        d_out = poisoned(lay.total)
        d_ol = guarded_column(n, torch.int32)
        d_st = guarded_column(n, torch.int32, -7)
        mx = int(batch.lens.max()) if n else 0
        ws, whole = guarded_workspace(self.codec.lib.fsg_compress_workspace_bytes(n, mx) if self.use_workspace else None)
        self.codec.compress(ins["d_in"], ins["d_in_off"], ins["d_in_len"], n, mx, d_out, ins["d_out_off"], d_ol, d_st,
                            workspace=ws)
        torch.cuda.synchronize()
        self.last_report = self.codec.compress_report(ws, n, mx)
        out = d_out.cpu().numpy()
        check_call(out, lay, caps, {"d_out_len": d_ol, "d_status": d_st}, n, whole, ins)
        ol = d_ol.cpu().numpy()[:n].view(np.uint32)
        st = d_st.cpu().numpy()[:n]
        return [out[int(oo[i]):int(oo[i]) + int(ol[i])].tobytes() for i in range(n)], st

    def decompress(self, comps: list[bytes], caps: list[int], flags: int = 0,
                   ws_total_in: int | None = None, ws_fill: int | None = None, slot_skew: int = 0):
        """ws_total_in: input size the workspace is sized for (default: the
        real packed size; smaller values force the v4 fallback path).
        ws_fill: byte the workspace is filled with before the call (the
        decoder must not rely on a zeroed workspace).
        slot_skew: output slot i starts (i * slot_skew) % 16 bytes past its
        16-byte-aligned place (slots of every alignment)."""
        torch = self.torch
        b = fsg.Batch.from_list(comps)
        n = len(b)
        caps = np.array(caps, dtype=np.uint32)
        lay = ct.aligned(caps.astype(np.uint64) + (16 if slot_skew else 0))
        if slot_skew:  # the 16 spare bytes around a skewed slot are guard too
            lay = ct.Layout("aligned+skew", lay.offs + (np.arange(n, dtype=np.uint64) * slot_skew) % 16, lay.total)
        oo = lay.offs
        ins = Inputs(d_in=b.data, d_in_off=b.offsets, d_in_len=b.lens, d_out_off=oo, d_out_cap=caps)
        d_out = poisoned(lay.total)
        d_ol = guarded_column(n, torch.int32)
        d_st = guarded_column(n, torch.int32, -7)
        total_in = int(b.data.size) if ws_total_in is None else ws_total_in
        ws, whole = guarded_workspace(self.codec.lib.fsg_decompress_workspace_bytes(n, total_in) if self.use_workspace
                                      else None, zero=True)
        if ws is not None and ws_fill is not None:
            ws.fill_(ws_fill)
        self.codec.decompress(ins["d_in"], ins["d_in_off"], ins["d_in_len"], n, d_out, ins["d_out_off"],
                              ins["d_out_cap"], d_ol, d_st, flags=flags, workspace=ws)
        torch.cuda.synchronize()
        self.last_report = self.codec.decompress_report(ws, n, flags)
        out = d_out.cpu().numpy()
        check_call(out, lay, caps, {"d_out_len": d_ol, "d_status": d_st}, n, whole, ins)
        if flags & fsg.FSG_FLAG_VALIDATE_ONLY:
            assert (out == POISON).all(), "validate-only call wrote to d_out"
        ol = d_ol.cpu().numpy()[:n].view(np.uint32)
        st = d_st.cpu().numpy()[:n]
        outs = [out[int(oo[i]):int(oo[i]) + int(min(ol[i], caps[i]))].tobytes() for i in range(n)]
        return outs, ol, st

    # ---- LZ4 bodies (include/flare_lz4_gpu.h)
    def lz4_compress(self, batch: fsg.Batch):
        torch = self.torch
        n = len(batch)
        caps = np.array([self.codec.lib.fsg_lz4_max_compressed_length(int(x)) for x in batch.lens], dtype=np.uint64)
        lay = ct.aligned(caps)
        oo = lay.offs
        ins = Inputs(d_in=batch.data, d_in_off=batch.offsets, d_in_len=batch.lens, d_out_off=oo)
        d_out = poisoned(lay.total)
        d_ol = guarded_column(n, torch.int32)
        d_st = guarded_column(n, torch.int32, -7)
        ws, whole = guarded_workspace(self.codec.lib.fsg_lz4_compress_workspace_bytes(n))
        self.codec.lz4_compress(ins["d_in"], ins["d_in_off"], ins["d_in_len"], n, d_out, ins["d_out_off"], d_ol, d_st,
                                ws)
        torch.cuda.synchronize()
        out = d_out.cpu().numpy()
        check_call(out, lay, caps, {"d_out_len": d_ol, "d_status": d_st}, n, whole, ins)
        ol = d_ol.cpu().numpy()[:n].view(np.uint32)
        st = d_st.cpu().numpy()[:n]
        return [out[int(oo[i]):int(oo[i]) + int(ol[i])].tobytes() for i in range(n)], st

    def lz4_decompress(self, bodies: list[bytes], caps: list[int], two_pass: bool = True,
                       ws_total_in: int | None = None, ws_fill: int | None = None):
        """two_pass: fsg_lz4_decompress_batch_ws with a workspace sized for
        ws_total_in input bytes (default: the real size; smaller values send
        messages to the one-pass fallback), filled with ws_fill first."""
        torch = self.torch
        b = fsg.Batch.from_list(bodies)
        n = len(b)
        caps = np.array(caps, dtype=np.uint32)
        lay = ct.aligned(caps)
        oo = lay.offs
        ins = Inputs(d_in=b.data, d_in_off=b.offsets, d_in_len=b.lens, d_out_off=oo, d_out_cap=caps)
        d_out = poisoned(lay.total)
        d_ol = guarded_column(n, torch.int32)
        d_st = guarded_column(n, torch.int32, -7)
        ws = whole = None
        if two_pass:
            lib = self.codec.lib  # (an older library under A/B has no two-pass decoder: the one-pass kernel runs)
            if hasattr(lib, "fsg_lz4_decompress_workspace_bytes"):
                ws, whole = guarded_workspace(lib.fsg_lz4_decompress_workspace_bytes(
                    n, int(b.data.size) if ws_total_in is None else ws_total_in))
            if ws is not None and ws_fill is not None:
                ws.fill_(ws_fill)
        self.codec.lz4_decompress(ins["d_in"], ins["d_in_off"], ins["d_in_len"], n, d_out, ins["d_out_off"],
                                  ins["d_out_cap"], d_ol, d_st, workspace=ws)
        torch.cuda.synchronize()
        out = d_out.cpu().numpy()
        check_call(out, lay, caps, {"d_out_len": d_ol, "d_status": d_st}, n, whole, ins)
        ol = d_ol.cpu().numpy()[:n].view(np.uint32)
        st = d_st.cpu().numpy()[:n]
        outs = [out[int(oo[i]):int(oo[i]) + int(min(ol[i], caps[i]))].tobytes() for i in range(n)]
        return outs, ol, st
