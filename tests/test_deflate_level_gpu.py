"""fsg_deflate_batch_level on the device (include/flare_deflate_level_gpu.h)
against the host model at the level (host/deflate_cpu.cc, the definition of
the bytes): the family of tests/deflate_cases.py and the constructed bodies of
tests/deflate_level_cases.py per format at levels 0 and 2 under two slot
layouts with the whole output buffer compared, level 1 against the level-less
call, the device-resident round trip through fsg_inflate_batch, the batch
shapes, a dirty workspace, an undersized workspace and the unit report."""
import numpy as np
import pytest

import containment as ct
import deflate_cases as C
import deflate_level_cases as V
import deflate_streams as D
import fsg

pytestmark = pytest.mark.gpu

FORMATS = [C.RAW, C.ZLIB, C.GZIP]


@pytest.fixture(scope="module")
def gpu():
    from deflate_level_harness import DeflateLevelGpu
    return DeflateLevelGpu()


def family():
    return [x for _, x in C.cases()] + [x for _, x in V.constructed()]


@pytest.mark.parametrize("layout", ["guarded", "tight"])
@pytest.mark.parametrize("level", [V.STORED, V.BEST])
@pytest.mark.parametrize("fmt", FORMATS)
def test_family_equals_host_model(gpu, fmt, level, layout):
    datas = family()
    want = [V.model(fmt, level, x) for x in datas]
    _, (d_out, d_off, d_len) = gpu.check_image(datas, fmt, level, layout, want)
    if layout == "guarded" and level == V.BEST:  # both directions device-resident
        outs, st = gpu.inflate_device(d_out, d_off, d_len, datas, fmt)
        assert (st == fsg.FSG_OK).all(), st
        assert all(o == x for o, x in zip(outs, datas))


@pytest.mark.parametrize("fmt", FORMATS)
def test_level_1_is_the_level_less_call(gpu, fmt):
    datas = family()
    old, _, _, ol0, st0, rep0, _ = gpu.run(datas, fmt, None, layout="tight")
    new, _ = gpu.check_image(datas, fmt, V.FAST, "tight", [C.model(fmt, x) for x in datas])
    assert (st0 == fsg.FSG_OK).all() and np.array_equal(old, new)


def small_bodies():
    rng = np.random.default_rng(6)
    return [D.text(int(n), i) if i % 3 else D.noise(int(n), i) for i, n in enumerate(rng.integers(0, 130, 300))]


@pytest.mark.parametrize("name,datas", [
    ("one_byte", lambda: [b"q"]),
    ("two_units_and_a_byte", lambda: [D.text(2 * C.U + 1, 3)]),
    ("three_hundred_small", small_bodies),
    ("large_among_small", lambda: [D.text(n, n) for n in range(32)] + [D.text(300000, 4)]
                                   + [D.noise(n, n) for n in range(98, 130)]),
])
def test_batch_shapes(gpu, name, datas):
    datas = datas()
    assert name != "large_among_small" or len(datas) == 65
    for level in (V.STORED, V.BEST):
        bodies, ol, st, rep = gpu.bodies(datas, C.ZLIB, level, layout="tight")
        assert (st == fsg.FSG_OK).all(), (name, level, st)
        assert bodies == [V.model(C.ZLIB, level, x) for x in datas], (name, level)
        assert rep["units"] == sum(max(1, -(-len(x) // C.U)) for x in datas) and rep["overflow_messages"] == 0


def test_dirty_workspace_gives_the_same_bytes(gpu):
    datas = [D.text(70000, 8), b"", D.noise(300, 1), D.text(129, 2), V.two_candidates()]
    bodies, _, st, _ = gpu.bodies(datas, C.ZLIB, V.BEST, ws_fill=0xFF)
    assert (st == fsg.FSG_OK).all() and bodies == [V.model(C.ZLIB, V.BEST, x) for x in datas]


@pytest.mark.parametrize("level", [V.STORED, V.BEST])
def test_workspace_sized_for_less_answers_corrupt(gpu, level):
    """The lengths are on the device only: a workspace sized for fewer bytes
    holds a prefix of the batch; the other slots are not touched."""
    datas = [D.text(1000, 1), D.text(3 * C.U, 2), D.text(1000, 3)]
    out, lay, caps, ol, st, rep, _ = gpu.run(datas, C.ZLIB, level, ws_total=0)
    assert list(st) == [fsg.FSG_OK, fsg.FSG_CORRUPT, fsg.FSG_CORRUPT] and list(ol[1:]) == [0, 0]
    want = [V.model(C.ZLIB, level, datas[0]), b"", b""]
    assert int(ol[0]) == len(want[0])
    image, _ = ct.expected_image(lay, caps, ol, want, st)  # POISON in the slots of the bodies not held
    bad = np.nonzero(out != image)[0]
    assert bad.size == 0, f"first difference at byte {int(bad[0])} of the output buffer"
    assert rep["overflow_messages"] == 2 and rep["unit_entries"] == 3


def test_report_counts_units_by_type(gpu):
    datas = [C.block_choice(), b"abcde", D.noise(5000, 1), D.text(5000, 1)]
    _, _, st, rep = gpu.bodies(datas, C.RAW, V.STORED)
    assert (st == fsg.FSG_OK).all()
    assert [rep["stored_units"], rep["fixed_units"], rep["dynamic_units"]] == [6, 0, 0] and rep["units"] == 6
    assert V.unit_types(V.BEST, C.block_choice()) == (1, 0, 2)  # dynamic, stored, dynamic
    _, _, st, rep = gpu.bodies([C.block_choice()], C.RAW, V.BEST)
    assert (st == fsg.FSG_OK).all()
    assert [rep["stored_units"], rep["fixed_units"], rep["dynamic_units"]] == [1, 0, 2] and rep["units"] == 3
    want = np.sum([V.unit_types(V.BEST, x) for x in datas], axis=0)
    _, _, st, rep = gpu.bodies(datas, C.RAW, V.BEST)
    assert [rep["stored_units"], rep["fixed_units"], rep["dynamic_units"]] == list(want)
