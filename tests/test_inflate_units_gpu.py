"""GPU tests of fsg_inflate_units_batch and fsg_inflate_units_lengths_batch
(include/flare_deflate_index_gpu.h, flare-cpp_amd/csrc/inflate_units.hip).

The rule under test: for every body and capacity, status, length and bytes are
exactly what fsg_inflate_batch gives -- the index changes the route, never the
result -- and the route each body took (fsg_inflate_units_report) is the one
the host model (fsh_cpu_inflate_units_route) names.  Python's zlib judges the
bytes.  Bodies: tests/gzip_index_cases.py (this project's flagged bodies and
foreign ones written by zlib with a full flush per chunk) and the hand-built
units of tests/deflate_random.py.  Every call runs under the containment
guards of tests/inflate_units_harness.py."""
import numpy as np
import pytest

import deflate_random as R
import deflate_streams as D
import gzip_index_cases as G

pytestmark = pytest.mark.gpu
FORMATS = [D.RAW, D.ZLIB, D.GZIP]
ROUTE_FIELD = {G.PARALLEL: "parallel_messages", G.NO_INDEX: "serial_no_index", G.UNUSABLE: "serial_unusable_index",
               G.MISMATCH: "serial_unit_mismatch"}


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test run without a visible GPU")
    from inflate_harness import InflateGpu
    from inflate_units_harness import InflateUnitsGpu
    return InflateUnitsGpu(), InflateGpu()


def model_report(bodies, caps, fmt, extra_units, store=True):
    """What fsg_inflate_units_report must say: the host model's route per body,
    and the workspace rule (indexed bodies keep their units while the units
    beyond one per body of all indexed bodies so far fit extra_units)."""
    rep = {f: 0 for f in ("parallel_messages", "parallel_units", "serial_no_index", "serial_unusable_index",
                          "serial_unit_mismatch", "serial_workspace")}
    rep["unit_entries"] = len(bodies) + extra_units
    run = 0
    for b, cap in zip(bodies, caps):
        r, units = G.route(b, int(cap), fmt, store)
        if r in (G.PARALLEL, G.MISMATCH):
            run += units - 1
            if run > extra_units:
                rep["serial_workspace"] += 1
                continue
        rep[ROUTE_FIELD[r]] += 1
        if r == G.PARALLEL:
            rep["parallel_units"] += units
    return rep


def check_parity(gpu, bodies, caps, fmt, layout="guarded", extra_units=4096, wants=None):
    units, plain = gpu
    outs, ol, st, rep = units.inflate(bodies, caps, fmt, layout=layout, extra_units=extra_units)
    outs0, ol0, st0 = plain.inflate(bodies, caps, fmt, layout=layout)
    for i in range(len(bodies)):
        assert (int(st[i]), int(ol[i])) == (int(st0[i]), int(ol0[i])), (i, len(bodies[i]), int(caps[i]))
        assert outs[i] == outs0[i], i
        if wants is not None:  # zlib's verdict, capacity aside
            want = wants[i]
            if want is None:  # a slot too small is answered before the trailer is judged
                assert st[i] != G.OK and (st[i] == G.SLOT_TOO_SMALL or ol[i] == 0), i
            elif caps[i] >= len(want):
                assert st[i] == G.OK and outs[i] == want, i
            else:
                assert (st[i], ol[i]) == (G.SLOT_TOO_SMALL, len(want)) and outs[i] == want[:caps[i]], i
    assert rep == model_report(bodies, caps, fmt, extra_units)
    return rep


def all_bodies(fmt):
    """Every fixture as it is (in raw and zlib they are corrupt or bad-header
    bodies), and the format's own vector set up to 100,000 decoded bytes."""
    out = [b for _, b, _ in G.fixtures()]
    exp = D.expected()
    out += [b for n, f, b in D.accept_vectors() if f == fmt and len(exp[n]) <= 100000]
    out += [b for n, f, b, _ in D.reject_streams() if f == fmt]
    return out


@pytest.mark.parametrize("fmt", FORMATS)
def test_parity_with_the_existing_call_and_report(gpu, fmt):
    bodies = all_bodies(fmt)
    wants = [D.zlib_verdict(fmt, b) for b in bodies]
    caps = [len(w) if w is not None else 4096 for w in wants]
    rep = check_parity(gpu, bodies, caps, fmt, wants=wants)
    if fmt == D.GZIP:
        par = [G.route(b)[1] for _, b, r in G.fixtures() if r == G.PARALLEL]
        assert rep["parallel_messages"] >= len(par) and rep["parallel_units"] >= sum(par)
        assert rep["serial_unit_mismatch"] >= len(G.mismatch_bodies())
        assert rep["serial_unusable_index"] >= len(G.unusable_bodies()) - 1
    else:
        assert rep["serial_no_index"] == len(bodies)


def test_mixed_batch_tight_slots(gpu):
    fx = G.fixtures()
    rej = [b for n, f, b, _ in D.reject_streams() if f == D.GZIP]
    bodies = []
    for i, (_, b, _) in enumerate(fx):  # indexed, plain, corrupt and bad-header bodies interleaved
        bodies.append(b)
        bodies.append(rej[i % len(rej)])
        if i % 5 == 0:
            bodies.append(b"\x1f\x8b\x09" + b[3:])
    wants = [D.zlib_verdict(D.GZIP, b) for b in bodies]
    caps = [len(w) if w is not None else 100 for w in wants]
    check_parity(gpu, bodies, caps, D.GZIP, layout="tight", wants=wants)


def test_bit_flips_over_an_indexed_body(gpu):
    muts = G.flip_set()
    base = G.foreign(G.TEXT5K, 1000)
    bodies = [b for b, _ in muts]
    wants = [w for _, w in muts]
    caps = [len(w) if w is not None else 8192 for w in wants]
    rep = check_parity(gpu, bodies, caps, D.GZIP, layout="tight", extra_units=4 * len(bodies), wants=wants)
    in_index = 0
    for b, w in muts:  # flips inside the index's data still decode, through the fallback
        at = next(i for i, (x, y) in enumerate(zip(b, base)) if x != y)
        if 16 <= at < 32:
            in_index += 1
            assert w == G.TEXT5K, at
    assert in_index >= 3
    assert rep["parallel_messages"] > 0 and rep["serial_unit_mismatch"] > 0 and rep["serial_unusable_index"] > 0
    assert rep["serial_workspace"] == 0


def test_hand_built_units(gpu):
    """40 bodies of 2 to 6 units made of random blocks of every type, each
    unit in front of the last closed by an empty stored block: one wave per
    unit.  In 5 of them a unit copies from below its first byte, so the body
    is walked as one stream.  Either way the bytes are zlib's."""
    cases = R.unit_bodies()
    bodies = [b for b, _, _ in cases]
    wants = [D.zlib_verdict(D.GZIP, b) for b in bodies]
    for (_, data, parallel), body, want in zip(cases, bodies, wants):
        assert want == data
        assert G.route(body, len(data))[0] == (G.PARALLEL if parallel else G.MISMATCH)
    rep = check_parity(gpu, bodies, [len(w) for w in wants], D.GZIP, layout="tight", wants=wants)
    assert rep["parallel_messages"] == 35 and rep["serial_unit_mismatch"] == 5
    assert rep["parallel_units"] == sum(G.route(b)[1] for b, _, p in cases if p)


def test_capacities(gpu):
    bodies, caps, wants = [], [], []
    for body, data, chlen in ((G.foreign(G.TEXT5K, 1000), G.TEXT5K, 1000),
                              (G.own(D.text(2 * G.U + 77, 6)), D.text(2 * G.U + 77, 6), G.U)):
        n = len(data)
        for cap in (0, 1, chlen - 1, chlen, chlen + 1, n - 1, n, n + 1):
            bodies.append(body)
            caps.append(cap)
            wants.append(data)
    for layout in ("tight", "guarded"):
        rep = check_parity(gpu, bodies, caps, D.GZIP, layout=layout, wants=wants)
        assert rep["parallel_messages"] == 4 and rep["serial_unit_mismatch"] == len(bodies) - 4


def test_a_workspace_that_holds_fewer_units_than_the_batch_has(gpu):
    five = G.foreign(G.TEXT5K, 1000)  # 5 units: 4 beyond one per body
    plain = D.compress(D.GZIP, G.TEXT5K)
    bodies = [five, plain, five, five, plain, G.foreign(G.TEXT5K[:1500], 1000), five]
    caps = [5000, 5000, 5000, 5000, 5000, 1500, 5000]
    wants = [D.zlib_verdict(D.GZIP, b) for b in bodies]
    for extra, serial in ((0, 5), (3, 5), (4, 4), (8, 3), (12, 2), (13, 1), (16, 1), (17, 0)):
        rep = check_parity(gpu, bodies, caps, D.GZIP, extra_units=extra, wants=wants)
        assert rep["serial_workspace"] == serial and rep["unit_entries"] == len(bodies) + extra, extra
        assert rep["parallel_messages"] == 5 - serial


@pytest.mark.parametrize("fmt", FORMATS)
def test_lengths_call(gpu, fmt):
    units, plain = gpu
    bodies = all_bodies(fmt)
    if fmt == D.GZIP:
        bodies += [b for b, _ in G.flip_set()[:300]]
    ln, st, rep = units.lengths(bodies, fmt)
    ln0, st0 = plain.lengths(bodies, fmt)
    assert np.array_equal(st, st0) and np.array_equal(ln, ln0)
    assert rep == model_report(bodies, [0] * len(bodies), fmt, 4096, store=False)
    ln, st, rep = units.lengths(bodies, fmt, extra_units=2)  # a small workspace: the same answers
    assert np.array_equal(st, st0) and np.array_equal(ln, ln0)
    assert rep == model_report(bodies, [0] * len(bodies), fmt, 2, store=False)
