"""The device-only code of the deflate writer (csrc/deflate_unit.h and the
plan, list, place and copy kernels of csrc/deflate.hip) against the host model
(host/deflate_cpu.cc, the definition of the bytes): the constructed family of
tests/deflate_parse_cases.py at its level and at the other one under two slot
layouts with the whole output buffer compared, the device-resident round trip,
each alignment body at all sixteen source addresses mod 16, a call with more
units than the persistent grid has waves, bodies of 66 and 130 units (with the
unit index and back through the unit-parallel inflate) and a batch whose unit
bases cross the plan kernel's 64-lane passes.  tests/test_deflate_parse.py
checks on the CPU that every constructed case hits what it aims at."""
import numpy as np
import pytest

import containment as ct
import deflate_cases as C
import deflate_level_cases as V
import deflate_parse_cases as P
import deflate_streams as D
import fsg
import gzip_index_cases as G
from inflate_harness import skewed_batch

pytestmark = pytest.mark.gpu

FORMATS = [C.RAW, C.ZLIB, C.GZIP]
U = C.U


@pytest.fixture(scope="module")
def gpu():
    from deflate_level_harness import DeflateLevelGpu
    return DeflateLevelGpu()


@pytest.fixture(scope="module")
def units_gpu():
    from inflate_units_harness import InflateUnitsGpu
    return InflateUnitsGpu()


def family(level):
    return [x for _, lv, x in P.cases() if lv == level]


# ---- the family

@pytest.mark.parametrize("layout", ["guarded", "tight"])
@pytest.mark.parametrize("level", [V.FAST, V.BEST])
@pytest.mark.parametrize("fmt", FORMATS)
def test_family_equals_host_model(gpu, fmt, level, layout):
    datas = family(level)
    assert len(datas) > 20
    want = [V.model(fmt, level, x) for x in datas]
    _, (d_out, d_off, d_len) = gpu.check_image(datas, fmt, level, layout, want)
    if layout == "guarded" and fmt == C.ZLIB:  # both directions device-resident, once a level
        outs, st = gpu.inflate_device(d_out, d_off, d_len, datas, fmt)
        assert (st == fsg.FSG_OK).all(), st
        assert all(o == x for o, x in zip(outs, datas))


@pytest.mark.parametrize("level", [V.FAST, V.BEST])
def test_family_at_the_other_level(gpu, level):
    """The cases built for one level through the other level's kernel against
    that level's model: other bytes, the same route."""
    datas = family(V.FAST + V.BEST - level)
    gpu.check_image(datas, C.GZIP, level, "tight", [V.model(C.GZIP, level, x) for x in datas])


def test_level_less_call_on_the_family(gpu):
    datas = family(V.FAST)
    out, _, _, ol, st, _, _ = gpu.run(datas, C.RAW, None, layout="tight")
    new, _ = gpu.check_image(datas, C.RAW, V.FAST, "tight", [C.model(C.RAW, x) for x in datas])
    assert (st == fsg.FSG_OK).all() and np.array_equal(out, new)


@pytest.mark.parametrize("level", [V.FAST, V.BEST])
def test_every_source_alignment(gpu, level):
    """Each alignment body sixteen times in a row: skewed_batch places body i at
    residue 5 * i mod 16, so the sixteen copies lie at sixteen different source
    addresses mod 16."""
    bodies = P.alignment_bodies()
    datas = [x for x in bodies for _ in range(16)]
    _, offs, _ = skewed_batch(datas)
    for k in range(len(bodies)):
        assert sorted(int(o) % 16 for o in offs[16 * k:16 * k + 16]) == list(range(16))
    want = [V.model(C.ZLIB, level, x) for x in datas]
    gpu.check_image(datas, C.ZLIB, level, "guarded", want)


# ---- one wave, several units; more than 64 units in a body

def small_bodies(count=1100):
    """test_deflate_gpu.small_bodies' recipe, the types mixed: text (dynamic),
    noise (stored) and bodies short enough for the fixed code follow each other."""
    rng = np.random.default_rng(15)
    sizes = rng.integers(0, 301, count)
    return [D.noise(int(n), i) if i % 3 == 0 else D.text(int(n) if i % 3 == 1 else int(n) % 24, i)
            for i, n in enumerate(sizes)]


TEXT_UNITS_66 = (0, 63, 64)  # and unit 65, the short last one
TEXT_UNITS_130 = (0, 63, 64, 65, 127, 128)
_BIG = {}


def big_body(units):
    """`units` units: noise everywhere (stored units, cheap on both sides)
    except text at units 0, 63, 64, 65, 127, 128 where there are as many, and a
    short last unit of text."""
    if units not in _BIG:
        text_at = TEXT_UNITS_66 if units == 66 else TEXT_UNITS_130
        rng = np.random.default_rng(units)
        parts = [D.text(U, 500 + k) if k in text_at else rng.integers(0, 256, U, dtype=np.uint8).tobytes()
                 for k in range(units - 1)]
        parts.append(D.text(777, units))
        _BIG[units] = b"".join(parts)
        assert len(_BIG[units]) == (units - 1) * U + 777
    return _BIG[units]


def n_units(x):
    return max(1, -(-len(x) // U))


_MODEL = {}


def big_model(fmt, level, units):
    """The model's bytes of a big body, computed once for the tests that share it."""
    key = ("model", fmt, level, units)
    if key not in _MODEL:
        _MODEL[key] = V.model(fmt, level, big_body(units))
    return _MODEL[key]


def big_types(level, units):
    key = ("types", level, units)
    if key not in _MODEL:
        _MODEL[key] = V.unit_types(level, big_body(units))
    return _MODEL[key]


@pytest.mark.parametrize("level", [V.STORED, V.FAST, V.BEST])
def test_one_wave_takes_several_units(gpu, level):
    """More units than the 1,024 waves of the persistent grid, on a workspace
    full of 0xFF: a wave's second unit starts from the first one's table,
    counts and bit window unless they are set up again."""
    datas = small_bodies() + [big_body(66), big_body(130)]
    units = sum(n_units(x) for x in datas)
    assert units == 1100 + 66 + 130 > 1024
    total = sum(len(x) for x in datas)
    lib = gpu.lib
    # the workspace holds a token region a wave, and no more than 1,024 of them
    per_wave = (U + 64) * 4
    assert (lib.fsg_deflate_workspace_bytes(2048, 0) - lib.fsg_deflate_workspace_bytes(1024, 0)
            < per_wave < lib.fsg_deflate_workspace_bytes(1024, 0) - lib.fsg_deflate_workspace_bytes(1023, 0))
    assert lib.fsg_deflate_workspace_bytes(len(datas), total) > 1024 * per_wave
    bodies, ol, st, rep = gpu.bodies(datas, C.GZIP, level, layout="tight", ws_fill=0xFF)
    assert (st == fsg.FSG_OK).all(), st[st != fsg.FSG_OK]
    small = len(datas) - 2
    want = [V.model(C.GZIP, level, x) for x in datas[:small]] + [big_model(C.GZIP, level, 66),
                                                                big_model(C.GZIP, level, 130)]
    for i, (b, w) in enumerate(zip(bodies, want)):
        assert b == w, (level, i, len(datas[i]))
    assert rep["units"] == units > 1024 and rep["overflow_messages"] == 0
    want = np.sum([V.unit_types(level, x) for x in datas[:small]] + [big_types(level, 66), big_types(level, 130)],
                  axis=0)
    assert [rep["stored_units"], rep["fixed_units"], rep["dynamic_units"]] == list(want)
    if level != V.STORED:
        assert all(v > 100 for v in want)  # the three kinds follow each other


@pytest.mark.parametrize("level", [V.FAST, V.BEST])
def test_a_waves_second_unit_starts_from_an_empty_table(gpu, level):
    """2,200 bodies, the two of deflate_parse_cases.same_window_repeat in a
    seeded mix: more than twice the grid's 1,024 waves, so some wave takes the
    second body behind the first, whichever way the units fall.  At level 1 a
    table left over from text does no visible harm (a stale position is a
    candidate only where the new unit has the same four bytes at it, and then
    the slot has been filled again); these two bodies are built so that it does."""
    x, _ = P.same_window_repeat()
    a = P.same_window_repeat(first=True)
    rng = np.random.default_rng(8)
    datas = [x if v else a for v in rng.integers(0, 2, 2200)]
    assert 900 < sum(1 for d in datas if d is x) < 1300
    bodies, ol, st, rep = gpu.bodies(datas, C.RAW, level, layout="tight", ws_fill=0xFF)
    assert (st == fsg.FSG_OK).all() and rep["units"] == 2200
    want = {id(x): V.model(C.RAW, level, x), id(a): V.model(C.RAW, level, a)}
    wrong = [i for i, (b, d) in enumerate(zip(bodies, datas)) if b != want[id(d)]]
    assert not wrong, (len(wrong), wrong[:8])


@pytest.mark.parametrize("fmt,layout", [(C.ZLIB, "guarded"), (C.GZIP, "tight")])
@pytest.mark.parametrize("level", [V.FAST, V.BEST])
def test_more_than_64_units_in_a_body(gpu, fmt, layout, level):
    datas = [big_body(66), b"abc", big_body(130)]
    want = [big_model(fmt, level, 66), V.model(fmt, level, b"abc"), big_model(fmt, level, 130)]
    out, lay, caps, ol, st, rep, _ = gpu.run(datas, fmt, level, layout=layout)
    assert (st == fsg.FSG_OK).all() and [int(v) for v in ol] == [len(b) for b in want]
    image, _ = ct.expected_image(lay, caps, ol, want, st)  # the whole output buffer, as check_image has it
    bad = np.nonzero(out != image)[0]
    assert bad.size == 0, (f"first difference at byte {int(bad[0])} of the output buffer; the bodies start at "
                           f"{[int(o) for o in lay.offs]}, a stored unit is {U + 5} bytes")
    types = np.sum([big_types(level, 66), V.unit_types(level, b"abc"), big_types(level, 130)], axis=0)
    assert [rep["stored_units"], rep["fixed_units"], rep["dynamic_units"]] == list(types) and rep["units"] == 197
    assert big_types(level, 130) == (123, 0, 7) and big_types(level, 66) == (62, 0, 4)


@pytest.mark.parametrize("level", [V.FAST, V.BEST])
def test_130_units_with_the_unit_index_and_back(units_gpu, level):
    x = big_body(130)
    bodies, st = units_gpu.deflate_flags([x], D.GZIP, level, G.FLAG, layout="tight")
    assert (st == G.OK).all()
    body = bodies[0]
    want = G.own(x, level)
    assert len(body) == len(want)
    bad = np.nonzero(np.frombuffer(body, dtype=np.uint8) != np.frombuffer(want, dtype=np.uint8))[0]
    assert bad.size == 0, f"first difference at byte {int(bad[0])}"
    state, chlen, chcnt, starts = G.index(body)
    assert (state, chlen, chcnt) == (G.INDEX_USABLE, U, 130)
    assert G.route(body, len(x)) == (G.PARALLEL, 130)
    # back by units, and the lengths by units; fsg_inflate_batch gives the same
    outs, ol, st, rep = units_gpu.inflate([body], [len(x)], D.GZIP)
    assert (st == G.OK).all() and int(ol[0]) == len(x) and outs[0] == x
    assert rep["parallel_messages"] == 1 and rep["parallel_units"] == 130
    assert sum(rep[k] for k in rep if k.startswith("serial")) == 0
    lens, st, rep = units_gpu.lengths([body], D.GZIP)
    assert (st == G.OK).all() and int(lens[0]) == len(x) and rep["parallel_units"] == 130
    from inflate_harness import InflateGpu
    outs2, ol2, st2 = InflateGpu().inflate([body], [len(x)], D.GZIP)
    assert (st2 == G.OK).all() and outs2[0] == x


def test_plan_pass_edges(gpu):
    """130 bodies, three units in bodies 63, 64 and 127 and one in the others:
    the unit bases and the staging granules are carried over the plan
    kernel's 64-lane passes with a multi-unit body on either side of an edge."""
    datas = [D.text(200 + i, i) if i % 2 else D.noise(100 + i, i) for i in range(130)]
    for i in (63, 64, 127):
        datas[i] = D.text(2 * U + 100 + i, i)
    assert [n_units(x) for x in datas] == [3 if i in (63, 64, 127) else 1 for i in range(130)]
    for level in (V.FAST, V.BEST):
        want = [V.model(C.ZLIB, level, x) for x in datas]
        gpu.check_image(datas, C.ZLIB, level, "tight", want)
        _, _, st, rep = gpu.bodies(datas, C.ZLIB, level)
        assert (st == fsg.FSG_OK).all() and rep["units"] == 136 and rep["overflow_messages"] == 0
