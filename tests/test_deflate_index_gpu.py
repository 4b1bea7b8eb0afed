"""GPU tests of fsg_deflate_batch_flags (include/flare_deflate_index_gpu.h):
the device's flagged gzip bodies are the host model's (fsh_cpu_deflate_flags)
byte for byte at every level, inside slots of fsg_deflate_max_length_flags
bytes and under the containment guards of tests/inflate_units_harness.py; with
no flag the call is fsg_deflate_batch_level; the flag with raw or zlib is
refused; and the bodies come back through fsg_inflate_units_batch with every
one of them decoded by units."""
import pytest

import deflate_level_cases as V
import deflate_streams as D
import gzip_index_cases as G

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test run without a visible GPU")
    from inflate_units_harness import InflateUnitsGpu
    return InflateUnitsGpu()


def datas():
    out = [D.text(n, 3) for n in G.OWN_SIZES]
    out += [D.noise(G.U + 100, 4), D.noise(100, 5) + D.text(G.U, 6) + D.noise(G.U, 7)]
    return out


@pytest.mark.parametrize("level", [0, 1, 2])
@pytest.mark.parametrize("layout", ["guarded", "tight"])
def test_flagged_bodies_are_the_host_models(gpu, level, layout):
    xs = datas()
    bodies, st = gpu.deflate_flags(xs, D.GZIP, level, G.FLAG, layout=layout)
    assert (st == G.OK).all(), st
    for x, b in zip(xs, bodies):
        assert b == G.own(x, level), len(x)
        assert D.zlib_verdict(D.GZIP, b) == x


@pytest.mark.parametrize("fmt", [D.RAW, D.ZLIB, D.GZIP])
def test_without_the_flag_it_is_the_level_call(gpu, fmt):
    xs = datas()[:6]
    bodies, st = gpu.deflate_flags(xs, fmt, 1, 0)
    assert (st == G.OK).all() and bodies == [V.model(fmt, 1, x) for x in xs]


def test_the_flag_with_zlib_or_raw_is_refused(gpu):
    for fmt, flags in ((D.RAW, 1), (D.ZLIB, 1), (D.GZIP, 2)):
        assert gpu.lib.fsg_deflate_max_length_flags(100, fmt, flags) == 0
        with pytest.raises(Exception):
            gpu.deflate_flags([b"abc"], fmt, 1, flags)


def test_round_trip_by_units(gpu):
    xs = [x for x in datas() if x]
    bodies, st = gpu.deflate_flags(xs, D.GZIP, 1, G.FLAG)
    outs, ol, st, rep = gpu.inflate(bodies, [len(x) for x in xs], D.GZIP)
    assert (st == G.OK).all() and outs == xs
    units = sum(-(-len(x) // G.U) for x in xs)
    assert rep["parallel_messages"] == len(xs) and rep["parallel_units"] == units
    assert sum(rep[k] for k in rep if k.startswith("serial")) == 0
