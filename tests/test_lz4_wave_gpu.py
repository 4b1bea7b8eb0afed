"""The LZ4 wave encoder (flare-cpp_amd/csrc/lz4_encode_wave.hip: one wave per
body, position table in LDS) through fsg_lz4_compress_batch: bytes equal to
the oracle's whichever encoder a body is routed to, the routing options, the
path report, the old-size workspace and write containment."""
import json
from pathlib import Path

import numpy as np
import pytest

import containment as ct
import fsg
import gpu_harness as gh
from bind import Lz4Oracle
from gen_inputs import build_input
from lz4_wave_cases import boundary_family, shaped

pytestmark = pytest.mark.gpu
GOLDEN = Path(__file__).resolve().parent / "golden"
VEC = json.loads((GOLDEN / "lz4_vectors.json").read_text())
NONE = 0xFFFFFFFF  # lz4_encode_wave_min: no body on the waves


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test run without a visible GPU")
    return gh.GpuCodec()


@pytest.fixture(scope="module")
def o():
    return Lz4Oracle()


@pytest.fixture(scope="module")
def family(o):
    """(names, inputs, the oracle's bodies), computed once."""
    fam = boundary_family()
    return [n for n, _ in fam], [x for _, x in fam], [o.compress(x) for _, x in fam]


def run(gpu, xs, layout="aligned", ws_bytes=None, ws_fill=None):
    """fsg_lz4_compress_batch on `xs` under the containment guards; returns
    (bodies, statuses, fsg_lz4_compress_report as a dict)."""
    torch = gpu.torch
    lib = gpu.codec.lib
    batch = fsg.Batch.from_list(xs)
    n = len(batch)
    caps = np.array([lib.fsg_lz4_max_compressed_length(int(x)) for x in batch.lens], dtype=np.uint64)
    lay = ct.LAYOUTS[layout](caps)
    oo = lay.offs
    ins = gh.Inputs(d_in=batch.data, d_in_off=batch.offsets, d_in_len=batch.lens, d_out_off=oo)
    d_out = gh.poisoned(lay.total)
    d_ol = gh.guarded_column(n, torch.int32)
    d_st = gh.guarded_column(n, torch.int32, -7)
    ws, whole = gh.guarded_workspace(lib.fsg_lz4_compress_workspace_bytes(n) if ws_bytes is None else ws_bytes)
    if ws_fill is not None:
        ws.fill_(ws_fill)
    gpu.codec.lz4_compress(ins["d_in"], ins["d_in_off"], ins["d_in_len"], n, d_out, ins["d_out_off"], d_ol, d_st, ws)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    gh.check_call(out, lay, caps, {"d_out_len": d_ol, "d_status": d_st}, n, whole, ins)
    ol = d_ol.cpu().numpy()[:n].view(np.uint32)
    st = d_st.cpu().numpy()[:n]
    assert (ol.astype(np.uint64) <= caps).all()
    rep = gpu.codec.lz4_compress_report(ws, n)
    return [out[int(oo[i]):int(oo[i]) + int(ol[i])].tobytes() for i in range(n)], st, rep


def _same(names, got, want):
    for name, g, w in zip(names, got, want):
        assert g == w, name


# ---- 1. ABI
def test_abi_report_and_options(gpu):
    lib = gpu.codec.lib
    assert hasattr(lib, "fsg_lz4_compress_report")
    assert "fsg_lz4_compress_report" in fsg.header_symbols()
    import ctypes
    for name, dflt in (("lz4_encode_wave_min", -1), ("lz4_encode_wave_per_cu", 0)):
        v = ctypes.c_int64(99)
        assert lib.fsg_default_option(name.encode(), ctypes.byref(v)) == 0 and v.value == dflt
        saved = fsg.get_option(name, lib)
        try:
            for x in (0, 4096, NONE, -1):
                fsg.set_option(name, x, lib)
                assert fsg.get_option(name, lib) == x
        finally:
            fsg.set_option(name, saved, lib)
    # the report without a device: an old-size workspace is path 1 whatever the header
    r = fsg.Lz4EncodeReport()
    assert lib.fsg_lz4_compress_report(None, 5, 5 * 16384, ctypes.byref(r)) == 0
    assert (r.path, r.lane_messages, r.wave_messages, r.wave_bytes) == (1, 5, 0, 0)
    assert lib.fsg_lz4_compress_report(None, 5, 5 * 16384, None) != 0


# ---- 2. every body on the wave kernel
def test_fixtures_on_the_waves(gpu, o, fsg_opts):
    fsg_opts(lz4_encode_wave_min=0)
    vecs = [v for v in VEC["compress"] if v["input_len"] <= 1 << 20]
    xs = [build_input(v) for v in vecs]
    bodies, st, rep = run(gpu, xs)
    assert (st == fsg.FSG_OK).all()
    for v, x, body in zip(vecs, xs, bodies):
        want = o.compress(x)
        blk = body[len(want) - v["block_len"]:]
        assert len(blk) == v["block_len"] and "%016x" % fsg.fnv1a64(blk) == v["block_fnv"], v["name"]
        assert body == want, v["name"]
    assert rep["path"] == 0 and rep["wave_messages"] == len(xs) and rep["lane_messages"] == 0
    assert rep["wave_bytes"] == sum(len(x) for x in xs) and rep["wave_min"] == 0
    outs, ol, st = gpu.lz4_decompress(bodies, [len(x) for x in xs], two_pass=True)
    assert (st == fsg.FSG_OK).all()
    assert all(y == x for y, x in zip(outs, xs))


# ---- 3. the boundary family, on the waves and on the lanes
@pytest.mark.parametrize("wave_min", [0, NONE], ids=["waves", "lanes"])
def test_boundary_family(gpu, family, fsg_opts, wave_min):
    fsg_opts(lz4_encode_wave_min=wave_min)
    names, xs, want = family
    bodies, st, rep = run(gpu, xs)
    assert (st == fsg.FSG_OK).all()
    _same(names, bodies, want)
    assert rep["path"] == 0 and rep["wave_min"] == wave_min
    assert rep["wave_messages"] == (len(xs) if wave_min == 0 else 0)
    assert rep["lane_messages"] == len(xs) - rep["wave_messages"]


# ---- 4. a mixed batch with an explicit threshold
def test_mixed_batch_threshold(gpu, o, fsg_opts):
    fsg_opts(lz4_encode_wave_min=4096)
    rng = np.random.default_rng(17)
    xs = []
    for t in range(300):  # test_lz4_randomized_against_oracle's sizes and alphabets
        n = int(rng.choice([rng.integers(0, 40), rng.integers(0, 5000), rng.integers(60000, 70000),
                            rng.integers(0, 200000)]))
        alpha = int(rng.choice([1, 2, 4, 40, 256]))
        xs.append(rng.integers(0, alpha, n, dtype=np.uint8).tobytes())
    bodies, st, rep = run(gpu, xs)
    assert (st == fsg.FSG_OK).all()
    for i, (x, b) in enumerate(zip(xs, bodies)):
        assert b == o.compress(x), (i, len(x))
    big = [len(x) for x in xs if len(x) >= 4096]
    assert 0 < len(big) < len(xs)
    assert rep["path"] == 0 and rep["wave_min"] == 4096
    assert rep["wave_messages"] == len(big) and rep["lane_messages"] == len(xs) - len(big)
    assert rep["wave_bytes"] == sum(big)


# ---- 5. more bodies than resident waves
def test_more_bodies_than_waves(gpu, o, fsg_opts):
    fsg_opts(lz4_encode_wave_min=0, lz4_encode_wave_per_cu=1)
    rng = np.random.default_rng(51)
    xs = [rng.integers(0, int(rng.choice([2, 4, 40, 256])), int(rng.integers(100, 301)), dtype=np.uint8).tobytes()
          for _ in range(3000)]
    want = [o.compress(x) for x in xs]
    for n in (3000, 1, 63, 65):
        bodies, st, rep = run(gpu, xs[:n])
        assert (st == fsg.FSG_OK).all()
        _same(range(n), bodies, want)
        assert rep["wave_messages"] == n and rep["lane_messages"] == 0


# ---- 6. the old-size workspace; a workspace full of garbage
def test_old_size_workspace_and_garbage(gpu, family, fsg_opts):
    names, xs, want = family
    names, xs, want = names[-40:], xs[-40:], want[-40:]
    n = len(xs)
    for wave_min in (0, -1):
        fsg_opts(lz4_encode_wave_min=wave_min)
        bodies, st, rep = run(gpu, xs, ws_bytes=16384 * n, ws_fill=0xFF)
        assert (st == fsg.FSG_OK).all()
        _same(names, bodies, want)
        assert rep["path"] == 1 and rep["wave_messages"] == 0 and rep["lane_messages"] == n
    for wave_min in (0, 1000, NONE):
        fsg_opts(lz4_encode_wave_min=wave_min)
        for fill in (0x00, 0xFF):
            bodies, st, rep = run(gpu, xs, ws_fill=fill)
            assert (st == fsg.FSG_OK).all()
            _same(names, bodies, want)
            assert rep["path"] == 0
            assert rep["wave_messages"] == sum(len(x) >= wave_min for x in xs)
    # one byte short of the old size: refused as before
    lib = gpu.codec.lib
    ws = gpu.torch.zeros(16384 * n - 1, dtype=gpu.torch.uint8, device="cuda")
    d = gh.dev(np.zeros(64, dtype=np.uint8))
    assert lib.fsg_lz4_compress_batch(d.data_ptr(), d.data_ptr(), d.data_ptr(), n, d.data_ptr(), d.data_ptr(),
                                      d.data_ptr(), d.data_ptr(), ws.data_ptr(), ws.numel(), None) != 0
    assert lib.fsg_lz4_compress_batch(d.data_ptr(), d.data_ptr(), d.data_ptr(), n, d.data_ptr(), d.data_ptr(),
                                      d.data_ptr(), d.data_ptr(), None, 0, None) != 0


# ---- 7. write containment, every body on the waves
@pytest.mark.parametrize("layout", ["guarded", "tight"])
def test_wave_write_containment(gpu, o, fsg_opts, layout):
    fsg_opts(lz4_encode_wave_min=0)
    fam = shaped()
    rng = np.random.default_rng(77)
    for n in (0, 1, 12, 13, 70, 300, 5000, 65546, 65547, 70001):
        fam.append((f"text-{n}", fsg.make_batch(fsg.KIND_TEXT, [n], first_index=n % 91).item(0) if n else b""))
        fam.append((f"random-{n}", rng.integers(0, 256, n, dtype=np.uint8).tobytes()))
        fam.append((f"zeros-{n}", bytes(n)))
    names, xs = [a for a, _ in fam], [b for _, b in fam]
    assert len(xs) >= 32  # two rounds of the guarded layout's 16 residues
    bodies, st, rep = run(gpu, xs, layout=layout)
    assert (st == fsg.FSG_OK).all()
    _same(names, bodies, [o.compress(x) for x in xs])
    assert rep["wave_messages"] == len(xs)
