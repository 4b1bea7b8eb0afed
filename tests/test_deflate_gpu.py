"""fsg_deflate_batch on the device (include/flare_deflate_compress_gpu.h)
against the host model (host/deflate_cpu.cc, the definition of the bytes):
the family of tests/deflate_cases.py per format under two slot layouts, the
device-resident round trip through fsg_inflate_batch, the batch shapes, a
dirty workspace, the argument errors and the unit report."""
import numpy as np
import pytest

import deflate_cases as C
import deflate_streams as D
import fsg

pytestmark = pytest.mark.gpu

FORMATS = [C.RAW, C.ZLIB, C.GZIP]


@pytest.fixture(scope="module")
def gpu():
    from deflate_harness import DeflateGpu
    return DeflateGpu()


def family():
    return [x for _, x in C.cases()]


@pytest.mark.parametrize("layout", ["guarded", "tight"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_family_equals_host_model(gpu, fmt, layout):
    datas = family()
    want = [C.model(fmt, x) for x in datas]
    d_out, d_off, d_len, _ = gpu.check_image(datas, fmt, layout, want)
    if layout == "guarded":  # both directions device-resident
        outs, st = gpu.inflate_device(d_out, d_off, d_len, datas, fmt)
        assert (st == fsg.FSG_OK).all(), st
        assert all(o == x for o, x in zip(outs, datas))


def small_bodies():
    rng = np.random.default_rng(5)
    return [D.text(int(n), i) if i % 3 else D.noise(int(n), i) for i, n in enumerate(rng.integers(0, 301, 1000))]


@pytest.mark.parametrize("name,datas", [
    ("one", lambda: [D.text(5000, 2)]),
    ("thousand_small", small_bodies),
    ("empty_64", lambda: [b""] * 64),
    ("large_between_small", lambda: [D.text(100, 1), b"", D.text(300000, 4), D.noise(70, 2), D.text(64, 3)]),
])
def test_batch_shapes(gpu, name, datas):
    datas = datas()
    for fmt in (C.ZLIB, C.GZIP) if name != "thousand_small" else (C.GZIP,):
        bodies, ol, st, rep = gpu.deflate(datas, fmt, layout="tight")
        assert (st == fsg.FSG_OK).all(), (name, st)
        assert bodies == [C.model(fmt, x) for x in datas], name
        assert rep["units"] == sum(max(1, -(-len(x) // C.U)) for x in datas) and rep["overflow_messages"] == 0


def test_empty_batch_launches_nothing(gpu):
    lib = gpu.lib
    assert lib.fsg_deflate_batch(None, None, None, 0, None, None, None, None, C.ZLIB, None, 0, None) == 0


def test_dirty_workspace_gives_the_same_bytes(gpu):
    datas = [D.text(70000, 8), b"", D.noise(300, 1), D.text(129, 2)]
    for fill in (0xFF, 0x00):
        bodies, _, st, _ = gpu.deflate(datas, C.ZLIB, ws_fill=fill)
        assert (st == fsg.FSG_OK).all() and bodies == [C.model(C.ZLIB, x) for x in datas], fill


def test_workspace_sized_for_less_answers_corrupt(gpu):
    """The lengths are on the device only: a workspace sized for fewer bytes
    is accepted by the host check and holds a prefix of the batch."""
    datas = [D.text(1000, 1), D.text(3 * C.U, 2), D.text(1000, 3)]
    bodies, ol, st, rep = gpu.deflate(datas, C.ZLIB, ws_total=0)
    assert list(st) == [fsg.FSG_OK, fsg.FSG_CORRUPT, fsg.FSG_CORRUPT] and list(ol[1:]) == [0, 0]
    assert bodies[0] == C.model(C.ZLIB, datas[0])
    assert rep["overflow_messages"] == 2 and rep["unit_entries"] == 3


def test_argument_errors(gpu):
    import torch
    lib = gpu.lib
    n = 3
    need = lib.fsg_deflate_workspace_bytes(n, 0)
    ws = torch.empty(need + 64, dtype=torch.uint8, device="cuda")
    col = torch.zeros(16, dtype=torch.int64, device="cuda")
    p, w = col.data_ptr(), ws.data_ptr()
    call = lambda *a: lib.fsg_deflate_batch(*a)
    assert call(p, p, p, n, p, p, p, p, C.ZLIB, w, need - 1, None) == -1   # one byte too small
    assert call(p, p, p, n, p, p, p, p, 3, w, need, None) == -1             # an unknown format
    assert call(p, p, p, n, p, p, p, p, C.ZLIB, None, need, None) == -1     # no workspace
    assert call(p, p, p, n, p, p, p, p, C.ZLIB, w + 4, need, None) == -1    # a misaligned one
    for hole in range(7):                                                   # a NULL column
        a = [p] * 7
        a[hole] = None
        a.insert(3, n)
        assert call(*a, C.ZLIB, w, need, None) == -1, hole
    torch.cuda.synchronize()


def test_report_counts_units_by_type(gpu):
    datas = [C.block_choice(), b"abcde", D.noise(5000, 1), D.text(5000, 1)]
    want = np.sum([C.unit_types(x) for x in datas], axis=0)
    assert list(want) == [2, 1, 3]
    _, _, st, rep = gpu.deflate(datas, C.RAW)
    assert (st == fsg.FSG_OK).all()
    assert [rep["stored_units"], rep["fixed_units"], rep["dynamic_units"]] == list(want) and rep["units"] == 6
