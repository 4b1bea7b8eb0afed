"""The write-containment checker (tests/containment.py) on simulated outputs:
every kind of spill a kernel could make must be reported, at the right offset
and against the right slot edge; a clean image must pass.  This is what shows
that the GPU tests built on the checker would fail if a kernel wrote one byte
outside its slot.  No GPU."""
import numpy as np
import pytest

import containment as ct
from containment import POISON

CAPS = [0, 1, 15, 16, 17, 0, 33, 100, 5, 64, 0, 7, 300, 2, 48, 31, 19, 0, 1000, 3]


def _case(layout_name, caps=CAPS, seed=1):
    """A layout, reference bodies / statuses (every third message not OK, the
    OK ones shorter than their slot now and then) and the clean output: the
    image, with garbage where the contract allows any byte."""
    rng = np.random.default_rng(seed)
    lay = ct.LAYOUTS[layout_name](caps)
    statuses = [1 if i % 3 == 2 else 0 for i in range(len(caps))]
    lens = [c if i % 4 else c - c // 3 for i, c in enumerate(caps)]
    bodies = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in lens]
    image, mask = ct.expected_image(lay, caps, lens, bodies, statuses)
    out = image.copy()
    out[mask] = rng.integers(0, 256, int(mask.sum()), dtype=np.uint8)
    return lay, image, mask, out, lens, statuses


@pytest.mark.parametrize("name", ["aligned", "guarded", "tight"])
def test_layout_properties(name):
    caps = np.array(CAPS * 3, dtype=np.uint64)
    lay = ct.LAYOUTS[name](caps)
    offs = lay.offs.astype(np.int64)
    ends = offs + caps.astype(np.int64)
    assert (offs[1:] >= ends[:-1]).all()  # ascending, no overlap
    assert lay.total >= ends[-1]
    gaps = offs[1:] - ends[:-1]
    if name == "aligned":
        assert (offs % 16 == 0).all() and offs[0] == 0
        assert (gaps >= ct.GUARD).all() and lay.total - ends[-1] >= ct.GUARD
        # the guards aside, the layout the tests always had
        assert (gaps < ct.GUARD + 16).all()
    elif name == "guarded":
        assert set(int(x) for x in offs % 16) == set(range(16))
        assert [int(x) for x in offs[:16] % 16] == [(7 * i) % 16 for i in range(16)]
        assert (gaps >= ct.GUARD).all() and (gaps < ct.GUARD + 16).all()
        assert offs[0] >= ct.GUARD and lay.total - ends[-1] == ct.TRAIL
    else:
        assert (gaps == 0).all()
        assert offs[0] == ct.GUARD and lay.total - ends[-1] == ct.TRAIL
    # outside_index is exactly the complement of the slots
    inside = np.zeros(lay.total, dtype=bool)
    for a, b in zip(offs, ends):
        assert not inside[a:b].any()
        inside[a:b] = True
    assert np.array_equal(ct.outside_index(lay, caps), np.flatnonzero(~inside))


@pytest.mark.parametrize("name", ["aligned", "guarded", "tight"])
def test_empty_batch_layout(name):
    lay = ct.LAYOUTS[name]([])
    assert lay.total > 0 and len(lay.offs) == 0
    out = np.full(lay.total, POISON, dtype=np.uint8)
    ct.check_outside(out, lay, [])
    out[3] = 0
    with pytest.raises(ct.ContainmentError) as e:
        ct.check_outside(out, lay, [])
    assert e.value.offset == 3 and e.value.slot is None


@pytest.mark.parametrize("name", ["aligned", "guarded", "tight"])
def test_clean_image_passes(name):
    lay, image, mask, out, _, _ = _case(name)
    ct.check(out, image, mask, lay, CAPS)
    ct.check_outside(out, lay, CAPS)
    # masked bytes are only ever inside slots
    assert not mask[ct.outside_index(lay, CAPS)].any()


def _both(out, image, mask, lay, caps=CAPS):
    """The two checkers' errors for a spill outside the slots (they must agree)."""
    with pytest.raises(ct.ContainmentError) as a:
        ct.check(out, image, mask, lay, caps)
    with pytest.raises(ct.ContainmentError) as b:
        ct.check_outside(out, lay, caps)
    for f in ("offset", "slot", "edge", "distance", "found", "expected"):
        assert getattr(a.value, f) == getattr(b.value, f), f
    return a.value


@pytest.mark.parametrize("name", ["aligned", "guarded"])
@pytest.mark.parametrize("slot", [1, 4, 7, 12, 18])
def test_one_byte_past_a_slot(name, slot):
    lay, image, mask, out, _, _ = _case(name)
    at = int(lay.offs[slot]) + CAPS[slot]
    out[at] = 0x00
    e = _both(out, image, mask, lay)
    assert (e.offset, e.slot, e.edge, e.distance) == (at, slot, "end", 1)
    assert (e.found, e.expected) == (0, POISON)
    assert f"offset {at}" in str(e) and f"slot {slot}" in str(e) and "past the end" in str(e)


@pytest.mark.parametrize("name", ["aligned", "guarded"])
@pytest.mark.parametrize("slot", [1, 4, 7, 12, 18])
def test_one_byte_before_a_slot(name, slot):
    lay, image, mask, out, _, _ = _case(name)
    at = int(lay.offs[slot]) - 1
    out[at] = 0x11
    e = _both(out, image, mask, lay)
    assert (e.offset, e.slot, e.edge, e.distance) == (at, slot, "start", -1)
    assert (e.found, e.expected) == (0x11, POISON)
    assert "before the start" in str(e)


def test_spill_in_tight_layout_hits_the_neighbour():
    """With adjacent slots a spill past slot i lands in slot i + 1: caught
    when that neighbour's bytes are pinned (an OK body), at its first byte."""
    lay, image, mask, out, lens, statuses = _case("tight")
    i = 6  # OK, full; slot 7 is OK with 100 pinned bytes
    assert statuses[i] == 0 and statuses[i + 1] == 0 and lens[i + 1] > 0
    at = int(lay.offs[i]) + CAPS[i]
    assert at == int(lay.offs[i + 1])
    out[at] ^= 0xFF
    with pytest.raises(ct.ContainmentError) as e:
        ct.check(out, image, mask, lay, CAPS)
    assert e.value.offset == at and abs(e.value.distance) <= 1 and e.value.slot in (i, i + 1)


@pytest.mark.parametrize("name", ["aligned", "guarded"])
def test_sixteen_byte_store_straddling_a_slot_end(name):
    """A whole 16-byte piece stored 9 bytes before the end of a short body:
    the first 9 bytes stay inside the slot (here equal to the body), 7 spill."""
    lay, image, mask, out, _, _ = _case(name)
    slot = 7
    end = int(lay.offs[slot]) + CAPS[slot]
    piece = np.concatenate([out[end - 9:end], np.arange(7, dtype=np.uint8) + 1])
    out[end - 9:end + 7] = piece
    e = _both(out, image, mask, lay)
    assert (e.offset, e.slot, e.edge, e.distance) == (end, slot, "end", 1)
    assert e.found == 1


@pytest.mark.parametrize("name", ["guarded", "tight"])
def test_write_into_leading_and_trailing_guard(name):
    lay, image, mask, out, _, _ = _case(name)
    first, last = 0, len(CAPS) - 1
    spoiled = out.copy()
    spoiled[5] = 0
    e = _both(spoiled, image, mask, lay)
    assert (e.offset, e.slot, e.edge, e.distance) == (5, first, "start", 5 - int(lay.offs[0]))
    spoiled = out.copy()
    at = lay.total - 1
    spoiled[at] = 0
    e = _both(spoiled, image, mask, lay)
    assert (e.offset, e.slot, e.edge) == (at, last, "end")
    assert e.distance == at - (int(lay.offs[last]) + CAPS[last] - 1) == ct.TRAIL
    # the first byte of the trailing guard, too
    spoiled = out.copy()
    at = lay.total - ct.TRAIL
    spoiled[at] = 0
    assert _both(spoiled, image, mask, lay).distance == 1


def test_write_past_the_layout_total():
    """A buffer allocated larger than the layout: its surplus is guard too."""
    lay, image, mask, out, _, _ = _case("guarded")
    big = np.concatenate([out, np.full(40, POISON, dtype=np.uint8)])
    ct.check(big, image, mask, lay, CAPS)
    ct.check_outside(big, lay, CAPS)
    big[lay.total + 17] = 1
    assert _both(big, image, mask, lay).offset == lay.total + 17


@pytest.mark.parametrize("name", ["aligned", "guarded", "tight"])
def test_ok_body_with_one_byte_left_as_poison(name):
    lay, image, mask, out, lens, statuses = _case(name)
    slot = 12
    assert statuses[slot] == 0
    a = int(lay.offs[slot])
    for k in (0, 137, lens[slot] - 1):
        spoiled = out.copy()
        expect = int(spoiled[a + k])
        spoiled[a + k] = POISON if expect != POISON else 0
        with pytest.raises(ct.ContainmentError) as e:
            ct.check(spoiled, image, mask, lay, CAPS)
        assert e.value.offset == a + k and e.value.expected == expect
        if k == 0:
            assert (e.value.slot, e.value.edge, e.value.distance) == (slot, "start", 0)
    # a short body's last byte: the slot's tail past it stays free
    slot = 4
    assert lens[slot] < CAPS[slot] and statuses[slot] == 0
    spoiled = out.copy()
    spoiled[int(lay.offs[slot]) + lens[slot] - 1] ^= 0x40
    with pytest.raises(ct.ContainmentError):
        ct.check(spoiled, image, mask, lay, CAPS)


@pytest.mark.parametrize("name", ["guarded", "aligned"])
@pytest.mark.parametrize("slot", [0, 5, 10, 17])
def test_write_into_a_capacity_zero_slot(name, slot):
    assert CAPS[slot] == 0
    lay, image, mask, out, _, _ = _case(name)
    at = int(lay.offs[slot])
    out[at] = 0x77
    e = _both(out, image, mask, lay)
    assert (e.offset, e.slot, e.edge, e.distance) == (at, slot, "start", 0)


def test_masked_bytes_are_free_and_only_those():
    lay, image, mask, out, lens, statuses = _case("guarded", seed=2)
    # a not-OK slot: anything goes inside, nothing outside
    slot = 8
    assert statuses[slot] != 0
    a = int(lay.offs[slot])
    out[a:a + CAPS[slot]] = 0
    ct.check(out, image, mask, lay, CAPS)
    out[a + CAPS[slot]] = 0
    with pytest.raises(ct.ContainmentError) as e:
        ct.check(out, image, mask, lay, CAPS)
    assert (e.value.slot, e.value.distance) == (slot, 1)
    # mask None (validate-only: nothing at all may be written)
    clean = np.full(lay.total, POISON, dtype=np.uint8)
    ct.check(clean, clean.copy(), None, lay, CAPS)
    clean[a] = 0
    with pytest.raises(ct.ContainmentError):
        ct.check(clean, np.full(lay.total, POISON, dtype=np.uint8), None, lay, CAPS)


def test_expected_image_rejects_a_body_longer_than_its_slot():
    lay = ct.guarded([4])
    with pytest.raises(AssertionError):
        ct.expected_image(lay, [4], [5], [b"abcde"], [0])


@pytest.mark.parametrize("dtype", [np.int32, np.uint32, np.int64, np.uint64])
@pytest.mark.parametrize("n", [0, 1, 63, 65])
def test_column_tail(dtype, n):
    col = ct.column(n, dtype, fill=-7)
    assert col.size == n + ct.COLUMN_TAIL
    col[:n] = 3  # what a call writes
    ct.check_column(col, n, "d_status")
    for k in (n, n + 1, n + ct.COLUMN_TAIL - 1):
        bad = col.copy()
        bad[k] = 0
        with pytest.raises(AssertionError, match=rf"d_status: entry {k} written, {k - n + 1} past its {n} entries"):
            ct.check_column(bad, n, "d_status")


def test_workspace_guard_and_inputs():
    tail = np.full(ct.WORKSPACE_GUARD, POISON, dtype=np.uint8)
    ct.check_workspace_guard(tail)
    tail[9] = 0
    with pytest.raises(AssertionError, match="byte 9 past workspace_bytes"):
        ct.check_workspace_guard(tail)
    a = np.arange(10, dtype=np.uint64)
    ct.check_unwritten(a.copy(), a, "d_in_off")
    b = a.copy()
    b[4] = 0
    with pytest.raises(AssertionError, match="d_in_off: input written by the call .*element 4"):
        ct.check_unwritten(b, a, "d_in_off")
