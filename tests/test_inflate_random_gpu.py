"""GPU tests of the inflate calls over the seeded family of
tests/deflate_random.py: random hand-built streams (every block type, random
complete code sets, run-length encoded headers, copies placed against the
decoder's 64-symbol groups) and the worst-case code sets that fill the LDS
decode tables to their last entry.  tests/test_inflate.py checks the family
itself against Python's zlib on the CPU; here status, length and bytes of the
device are zlib's, at exact capacities, at capacities inside the body
(count-only mode from the capacity on) and in the lengths call, and 2,000
single-bit flips of family streams get zlib's verdict.  Every call runs under
the write-containment guards of tests/inflate_harness.py."""
import numpy as np
import pytest

import deflate_random as R
import deflate_streams as D

pytestmark = pytest.mark.gpu
FORMATS = [D.RAW, D.ZLIB, D.GZIP]


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test run without a visible GPU")
    from inflate_harness import InflateGpu
    return InflateGpu()


@pytest.mark.parametrize("fmt", FORMATS)
def test_random_family_matches_zlib(gpu, fmt):
    fam = R.random_family()
    outs, ol, st = gpu.inflate([s.body(fmt) for s in fam], [len(s.expected) for s in fam], fmt, layout="guarded")
    for i, s in enumerate(fam):
        assert (st[i], ol[i]) == (D.OK, len(s.expected)), (s.name, int(st[i]), int(ol[i]))
        assert outs[i] == s.expected, s.name


@pytest.mark.parametrize("fmt", FORMATS)
def test_random_family_count_only(gpu, fmt):
    """Capacities 0, n - 1 and one inside each body: FSG_SLOT_TOO_SMALL with
    the whole length, nothing written past the capacity (tight slots: an
    overrun lands in a neighbour's slot, which the harness compares)."""
    fam = R.random_family()
    bodies, caps, want, inside = [], [], [], {"copy": 0, "stored": 0, "lit": 0}
    for s in fam:
        n = len(s.expected)
        inner, kind = R.inner_capacity(s, fmt)
        if inner is not None:
            inside[kind] += 1
        for cap in sorted({0, n - 1, inner} - {None, -1, n}):
            bodies.append(s.body(fmt))
            caps.append(cap)
            want.append((s.name, n))
    assert inside["copy"] >= 100 and inside["stored"] >= 20, inside
    outs, ol, st = gpu.inflate(bodies, caps, fmt, layout="tight")
    for i, (name, n) in enumerate(want):
        assert (st[i], ol[i]) == (D.SLOT_TOO_SMALL, n), (name, caps[i], int(st[i]), int(ol[i]))


@pytest.mark.parametrize("fmt", FORMATS)
def test_random_family_lengths(gpu, fmt):
    fam = R.random_family()
    lens, st = gpu.lengths([s.body(fmt) for s in fam], fmt)
    assert (st == D.OK).all(), [fam[i].name for i in np.nonzero(st != D.OK)[0]]
    assert [int(v) for v in lens] == [len(s.expected) for s in fam]


@pytest.mark.parametrize("fmt", FORMATS)
def test_hand_built_flips_match_zlib(gpu, fmt):
    muts = R.hand_flip_set(fmt)
    caps = [len(w) if w is not None else 8192 for _, w in muts]
    outs, ol, st = gpu.inflate([b for b, _ in muts], caps, fmt, layout="tight")
    for i, (body, want) in enumerate(muts):
        assert (st[i] == D.OK) == (want is not None), (i, int(st[i]))
        if want is not None:
            assert ol[i] == len(want) and outs[i] == want, i
        elif st[i] != D.SLOT_TOO_SMALL:
            assert ol[i] == 0, i
