"""Write-containment checker for the batch calls (pure numpy, no GPU).

The contract (include/flare_snappy_gpu.h, "What a *_batch call writes"): a
call writes no byte of its output buffer outside the union of the slots
[off_i, off_i + cap_i); inside a slot, bytes at and past the reported length
are unspecified, as is the whole slot of a message whose status is not FSG_OK;
result columns get exactly n_msgs entries; nothing is written past
workspace_bytes.

A test lays its slots out with one of the layouts below in a buffer filled
with POISON, builds the expected image of the whole buffer from the reference
(`expected_image`) and compares every byte the contract specifies (`check`).
Guards are never masked: a store that spills out of a slot -- one byte or a
whole 16-byte piece, before the slot or after it -- changes a POISON byte and
is reported with the slot edge it lies nearest to.

GUARD is 64 bytes: the widest single spill in the kernels is the encoder's
64-byte literal chunk."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

POISON = 0xA5
GUARD = 64            # poison between consecutive slots, and before the first
TRAIL = 256           # poison after the last slot (guarded / tight)
COLUMN_TAIL = 64      # sentinel entries after a result column's n_msgs
SENTINEL = -0x5A5A5A5B  # 0xA5A5A5A5 as an int32
WORKSPACE_GUARD = 256  # bytes after the workspace a call is told about


@dataclass
class Layout:
    name: str
    offs: np.ndarray  # uint64 slot starts
    total: int        # bytes of the whole buffer, guards included


def _caps(caps) -> np.ndarray:
    return np.asarray(caps, dtype=np.uint64).reshape(-1)


def aligned(caps) -> Layout:
    """16-byte-aligned slot starts (the layout fsg.slot_offsets gives, the
    first slot at 0) with GUARD bytes of poison after every slot."""
    caps = _caps(caps)
    offs = np.zeros(len(caps), dtype=np.uint64)
    pos = 0
    for i, c in enumerate(caps):
        offs[i] = pos
        pos = (pos + int(c) + GUARD + 15) // 16 * 16
    return Layout("aligned", offs, max(pos, 16))


def guarded(caps) -> Layout:
    """Slot i starts at residue (7 * i) % 16, so 16 consecutive slots cover
    every residue; at least GUARD poison bytes between slots, GUARD before
    the first and TRAIL after the last."""
    caps = _caps(caps)
    offs = np.zeros(len(caps), dtype=np.uint64)
    pos = GUARD
    for i, c in enumerate(caps):
        start = pos + ((7 * i) % 16 - pos) % 16
        offs[i] = start
        pos = start + int(c) + GUARD
    end = pos - GUARD
    return Layout("guarded", offs, end + TRAIL)


def tight(caps) -> Layout:
    """Slots adjacent at byte granularity, no gaps; GUARD before the first
    and TRAIL after the last."""
    caps = _caps(caps)
    offs = np.zeros(len(caps), dtype=np.uint64)
    if len(caps):
        offs[:] = GUARD
        offs[1:] += np.cumsum(caps[:-1])
    end = GUARD + int(caps.sum())
    return Layout("tight", offs, end + TRAIL)


LAYOUTS = {"aligned": aligned, "guarded": guarded, "tight": tight}


def outside_index(layout: Layout, caps) -> np.ndarray:
    """Offsets of every byte of the buffer that lies in no slot, ascending
    (slots in ascending order, as every layout here makes them)."""
    caps = _caps(caps).astype(np.int64)
    offs = layout.offs.astype(np.int64)
    starts = np.concatenate([[0], offs + caps])        # gap k starts after slot k - 1
    ends = np.concatenate([offs, [layout.total]])      # and ends where slot k starts
    lens = ends - starts
    assert (lens >= 0).all(), "slots overlap or are out of order"
    first = np.cumsum(lens) - lens
    return np.repeat(starts - first, lens) + np.arange(int(lens.sum()), dtype=np.int64)


def expected_image(layout: Layout, caps, lens, bodies, statuses):
    """(image, mask) of the whole buffer.  Everything starts as POISON;
    [off_i, off_i + len_i) holds bodies[i] where statuses[i] == 0 (FSG_OK).
    mask is True on the bytes the contract leaves unspecified: the tail of an
    OK slot from len_i on, and the whole slot of a message that is not OK.
    Bytes outside the slots are never masked."""
    caps = _caps(caps)
    image = np.full(layout.total, POISON, dtype=np.uint8)
    mask = np.zeros(layout.total, dtype=bool)
    for i, c in enumerate(caps):
        a, c = int(layout.offs[i]), int(c)
        if statuses[i] != 0:
            mask[a:a + c] = True
            continue
        n = int(lens[i])
        assert n <= c and len(bodies[i]) == n, f"slot {i}: reference body of {n} bytes in a slot of {c}"
        image[a:a + n] = np.frombuffer(bodies[i], dtype=np.uint8)
        mask[a + n:a + c] = True
    return image, mask


class ContainmentError(AssertionError):
    """A byte the contract pins came back different.  offset: the first such
    byte; slot / edge: the nearest slot edge ("start" or "end"); distance:
    offset - start, or offset - (last byte of the slot), so -1 is the byte just
    before a slot, +1 the byte just past it and 0 a slot's own first or last
    byte; found / expected: the byte values."""

    def __init__(self, what, offset, slot, edge, distance, found, expected):
        self.offset, self.slot, self.edge, self.distance = offset, slot, edge, distance
        self.found, self.expected = found, expected
        if slot is None:
            where = "no slots in the buffer"
        else:
            side = {True: "past the end", False: "before the end"}[distance > 0] if edge == "end" else \
                {True: "before the start", False: "past the start"}[distance < 0]
            where = f"{abs(distance)} byte(s) {side} of slot {slot}"
        super().__init__(f"{what}: byte at offset {offset} is 0x{found:02x}, expected 0x{expected:02x} ({where})")


def nearest_edge(offset: int, layout: Layout, caps):
    """(slot, edge, signed distance) of the slot edge nearest to `offset`; a
    slot of capacity 0 has only its start."""
    caps = _caps(caps).astype(np.int64)
    if not len(caps):
        return None, None, 0
    offs = layout.offs.astype(np.int64)
    d_start = offset - offs
    d_end = np.where(caps > 0, offset - (offs + caps - 1), np.iinfo(np.int64).max // 2)
    i, j = int(np.abs(d_start).argmin()), int(np.abs(d_end).argmin())
    de, ds = int(d_end[j]), int(d_start[i])
    if abs(de) < abs(ds) or (abs(de) == abs(ds) and de > 0 and ds >= 0):  # past a 1-byte slot: its end
        return j, "end", de
    return i, "start", int(d_start[i])


def _fail(what, offset, found, expected, layout, caps):
    slot, edge, dist = nearest_edge(offset, layout, caps)
    raise ContainmentError(what, offset, slot, edge, dist, int(found), int(expected))


def check(out, image, mask, layout: Layout, caps, what: str = "output buffer"):
    """Every unmasked byte of `out` equals `image` (mask None: every byte)."""
    out = np.asarray(out, dtype=np.uint8)
    assert out.size >= layout.total and image.size == layout.total, (out.size, image.size, layout.total)
    bad = out[:layout.total] != image
    if mask is not None:
        bad &= ~mask
    if bad.any():
        at = int(bad.argmax())
        _fail(what, at, out[at], image[at], layout, caps)
    if out.size > layout.total and (out[layout.total:] != POISON).any():
        at = layout.total + int((out[layout.total:] != POISON).argmax())
        _fail(what, at, out[at], POISON, layout, caps)


def check_outside(out, layout: Layout, caps, what: str = "output buffer"):
    """Only the bytes outside every slot (item 1 of the contract): all POISON.
    For buffers too large to build an image of."""
    out = np.asarray(out, dtype=np.uint8)
    assert out.size >= layout.total, (out.size, layout.total)
    idx = outside_index(layout, caps)
    if out.size > layout.total:
        idx = np.concatenate([idx, np.arange(layout.total, out.size, dtype=np.int64)])
    bad = out[idx] != POISON
    if bad.any():
        at = int(idx[int(bad.argmax())])
        _fail(what, at, out[at], POISON, layout, caps)


# ---- result columns: n entries for the call, COLUMN_TAIL sentinel entries behind them

def sentinel(dtype):
    """SENTINEL in a column's dtype (wrapped for the unsigned ones)."""
    return np.array(SENTINEL, dtype=np.int64).astype(dtype)[()]


def column(n: int, dtype, fill=SENTINEL) -> np.ndarray:
    """A host image of a guarded result column: n entries of `fill`, then
    COLUMN_TAIL entries of SENTINEL."""
    col = np.full(n + COLUMN_TAIL, sentinel(dtype), dtype=dtype)
    col[:n] = np.array(fill, dtype=np.int64).astype(dtype)
    return col


def check_column(col, n: int, name: str):
    """The sentinel tail of a column that was sized column(n, ...) is intact:
    the call wrote exactly n entries, or fewer."""
    col = np.asarray(col)
    assert col.size == n + COLUMN_TAIL, (name, col.size, n)
    bad = col[n:] != sentinel(col.dtype)
    if bad.any():
        k = n + int(bad.argmax())
        raise AssertionError(f"{name}: entry {k} written, {k - n + 1} past its {n} entries (value {int(col[k])})")


def check_workspace_guard(tail, name: str = "workspace"):
    """The WORKSPACE_GUARD bytes after the workspace the call was given."""
    tail = np.asarray(tail, dtype=np.uint8)
    assert tail.size == WORKSPACE_GUARD, tail.size
    bad = tail != POISON
    if bad.any():
        k = int(bad.argmax())
        raise AssertionError(f"{name}: byte {k} past workspace_bytes written (0x{int(tail[k]):02x})")


def check_unwritten(after, before, name: str):
    """An input array (d_in, the offset and length columns) is as it was."""
    after, before = np.asarray(after), np.asarray(before)
    if after.shape != before.shape or (after != before).any():
        k = int((after.reshape(-1) != before.reshape(-1)).argmax()) if after.shape == before.shape else -1
        raise AssertionError(f"{name}: input written by the call (first change at element {k})")
