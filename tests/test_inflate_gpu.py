"""GPU tests of the inflate calls (include/flare_deflate_gpu.h,
flare-cpp_amd/csrc/inflate.hip) through the C ABI: the CPU vector set of
tests/test_inflate.py (tests/deflate_streams.py) with Python's zlib as the
judge, the three sets of 2,000 single-bit flips, FSG_SLOT_TOO_SMALL, the
lengths call, the two checksum calls and the batch shapes.  Every call runs
under the write-containment guards of tests/inflate_harness.py."""
import zlib

import numpy as np
import pytest

import deflate_streams as D

pytestmark = pytest.mark.gpu
FORMATS = [D.RAW, D.ZLIB, D.GZIP]
CHECKSUM_CASES = ("zlib_adler", "gzip_crc", "gzip_isize")


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test run without a visible GPU")
    from inflate_harness import InflateGpu
    return InflateGpu()


def vectors(fmt):
    """(name, body, zlib's bytes or None, status) of the CPU vector set in one format."""
    exp = D.expected()
    out = [(n, b, exp[n], D.OK) for n, f, b in D.accept_vectors() if f == fmt]
    out += [(n, b, None, st) for n, f, b, st in D.reject_streams() if f == fmt]
    return out


@pytest.mark.parametrize("fmt", FORMATS)
def test_parity_with_zlib(gpu, fmt):
    vec = vectors(fmt)
    caps = [len(w) if w is not None else 4096 for _, _, w, _ in vec]
    outs, ol, st = gpu.inflate([b for _, b, _, _ in vec], caps, fmt, layout="guarded")
    for i, (name, body, want, status) in enumerate(vec):
        assert st[i] == status, (name, int(st[i]))
        assert ol[i] == (len(want) if want is not None else 0), name
        if want is not None:
            assert outs[i] == want, name


@pytest.mark.parametrize("fmt", FORMATS)
def test_bit_flips_match_zlib(gpu, fmt):
    muts = D.mutation_set(fmt)
    caps = [len(w) if w is not None else 8192 for _, w in muts]
    outs, ol, st = gpu.inflate([b for b, _ in muts], caps, fmt, layout="tight")
    for i, (body, want) in enumerate(muts):
        assert (st[i] == D.OK) == (want is not None), (i, int(st[i]))
        if want is not None:
            assert ol[i] == len(want) and outs[i] == want, i
        elif st[i] != D.SLOT_TOO_SMALL:
            assert ol[i] == 0, i


def test_slot_too_small(gpu):
    exp = D.expected()
    names = ("text_5000_l6_f1", "random_1000_l6_f1", "text_70000_l9_f1", "fixed_every_length_f1", "sync_flush_f1")
    by_name = {n: b for n, f, b in D.accept_vectors()}
    bodies, caps, want = [], [], []
    for name in names:
        n = len(exp[name])
        for cap in (0, 1, n - 1, n):
            bodies.append(by_name[name])
            caps.append(cap)
            want.append((D.SLOT_TOO_SMALL if cap < n else D.OK, n, exp[name]))
    for layout in ("tight", "guarded"):  # the guards around every slot are checked by the harness
        outs, ol, st = gpu.inflate(bodies, caps, D.ZLIB, layout=layout)
        for i, (status, n, data) in enumerate(want):
            assert (st[i], ol[i]) == (status, n), (i, caps[i])
            if status == D.OK:
                assert outs[i] == data, i


@pytest.mark.parametrize("fmt", FORMATS)
def test_lengths_call(gpu, fmt):
    vec = vectors(fmt)
    data = D.text(4000, 21)
    raw = D.compress(D.RAW, data)
    wrong = {D.RAW: [], D.ZLIB: [D.wrap(D.ZLIB, raw, data, adler=1)],
             D.GZIP: [D.wrap(D.GZIP, raw, data, crc=7), D.wrap(D.GZIP, raw, data, isize=3)]}[fmt]
    bodies = [b for _, b, _, _ in vec] + wrong
    lens, st = gpu.lengths(bodies, fmt)
    for i, (name, body, want, status) in enumerate(vec):
        if name in CHECKSUM_CASES:  # a correct stream with a wrong trailer
            assert (st[i], lens[i]) == (D.OK, 2000), name
        else:
            assert (st[i], lens[i]) == (status, len(want) if want is not None else 0), name
    if wrong:
        k = len(vec)
        assert (st[k:] == D.OK).all() and (lens[k:] == len(data)).all()
        _, ol, st2 = gpu.inflate(wrong, [len(data)] * len(wrong), fmt)
        assert (st2 == D.CORRUPT).all() and (ol == 0).all()


@pytest.mark.parametrize("adler", [False, True])
def test_checksum_calls(gpu, adler):
    sizes = list(range(0, 301)) + [4095, 4096, 4097, 65536, 1000003]
    buf = np.frombuffer(D.noise(1000003 + 1024, 17), dtype=np.uint8).copy()
    buf[5000:9000] = 0xff  # the largest Adler sums
    offs, lens = [], []
    for k, n in enumerate(sizes):
        for a in range(16):
            offs.append(16 * ((k * 7) % 61) + a)
            lens.append(n)
    got = gpu.checksums(buf, offs, lens, adler)
    f = zlib.adler32 if adler else zlib.crc32
    raw = buf.tobytes()
    for i, (o, n) in enumerate(zip(offs, lens)):
        assert got[i] == f(raw[o:o + n]), (o, n)


def test_batch_shapes(gpu):
    # one body
    data = D.text(3000, 31)
    outs, ol, st = gpu.inflate([D.compress(D.GZIP, data)], [len(data)], D.GZIP)
    assert st[0] == D.OK and outs[0] == data
    # 4,096 bodies of 1,000 bytes
    texts = [D.text(1000, 100 + k) for k in range(64)]
    comp = [D.compress(D.ZLIB, t) for t in texts]
    outs, ol, st = gpu.inflate([comp[i % 64] for i in range(4096)], [1000] * 4096, D.ZLIB, layout="tight")
    assert (st == D.OK).all() and (ol == 1000).all()
    assert all(outs[i] == texts[i % 64] for i in range(4096))
    # 64 bodies of 300,000 bytes
    texts = [D.text(300000, 200 + k) for k in range(4)]
    comp = [D.compress(D.RAW, t) for t in texts]
    outs, ol, st = gpu.inflate([comp[i % 4] for i in range(64)], [300000] * 64, D.RAW, layout="tight")
    assert (st == D.OK).all() and all(outs[i] == texts[i % 4] for i in range(64))


def test_corrupt_bodies_leave_their_neighbours_alone(gpu):
    big, small = D.text(300000, 41), D.text(40, 42)
    good = [b"", D.compress(D.ZLIB, small), D.compress(D.ZLIB, big), D.compress(D.ZLIB, b"")]
    want = [None, small, big, b""]
    bad = [b for n, f, b, s in D.reject_streams() if f == D.ZLIB] + [good[2][:-9], good[2][:5000] + good[2][5001:]]
    bodies, expect = [], []
    for k in range(24):
        bodies.append(good[k % 4])
        expect.append(want[k % 4])
        bodies.append(bad[k % len(bad)])
        expect.append(D.zlib_verdict(D.ZLIB, bodies[-1]))
    caps = [len(w) if w is not None else 300000 for w in expect]
    outs, ol, st = gpu.inflate(bodies, caps, D.ZLIB, layout="tight")
    for i, w in enumerate(expect):
        assert (st[i] == D.OK) == (w is not None), i
        if w is not None:
            assert outs[i] == w and ol[i] == len(w), i
