"""Path reports on the GPU: every batch's bytes and statuses are checked
against the oracle (as test_gpu_parity.py does), then the report of the call
(fsg_decompress_report / fsg_compress_report / fsg_lz4_decompress_report) is
checked against the route the batch was built to take.  The tests keep the
workspace tensor, so they do their own device plumbing."""
import numpy as np
import pytest

import fsg
from bind import Lz4Oracle, Oracle

pytestmark = pytest.mark.gpu
POISON = 0xA5


@pytest.fixture(scope="module")
def codec():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test run without a visible GPU")
    return fsg.SnappyGPU(torch.cuda.current_device())


@pytest.fixture(scope="module")
def oracle():
    return Oracle()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def bitmap_words(n_bytes: int) -> int:
    """index_prologue's / lz4_index_kernel's allocation for n_bytes of input."""
    return (((n_bytes + 31) >> 5) + 3) & ~3


def run_decode(codec, comps, caps, ws_total_in=None, workspace="sized", flags=0):
    """One fsg_decompress_batch; returns (outputs, statuses, report).
    workspace: "sized" (for ws_total_in bytes of input; default the real
    size), None, or a tensor."""
    import torch
    b = fsg.Batch.from_list(comps)
    n = len(b)
    caps = np.array(caps, dtype=np.uint32)
    oo, tot = fsg.slot_offsets(caps.astype(np.uint64))
    d_out = torch.full((max(tot, 1),), POISON, dtype=torch.uint8, device="cuda")
    d_ol = torch.empty(max(n, 1), dtype=torch.int32, device="cuda")
    d_st = torch.full((max(n, 1),), -7, dtype=torch.int32, device="cuda")
    ws = workspace
    if isinstance(workspace, str):
        ws = codec.decompress_workspace(n, int(b.data.size) if ws_total_in is None else ws_total_in)
        ws.fill_(0x5A)  # the counters must not rely on a zeroed workspace
    codec.decompress(_dev(b.data), _dev(b.offsets), _dev(b.lens), n, d_out, _dev(oo), _dev(caps), d_ol, d_st,
                     flags=flags, workspace=ws)
    rep = codec.decompress_report(ws, n, flags)
    out = d_out.cpu().numpy()
    ol = d_ol.cpu().numpy()[:n].view(np.uint32)
    st = d_st.cpu().numpy()[:n]
    outs = [out[int(oo[i]):int(oo[i]) + int(min(ol[i], caps[i]))].tobytes() for i in range(n)]
    return outs, st, rep


def run_encode(codec, items, workspace="sized"):
    """One fsg_compress_batch; returns (compressed bodies, statuses, report)."""
    import torch
    batch = fsg.Batch.from_list(items)
    n = len(batch)
    caps = np.array([fsg.max_compressed_length(int(x)) for x in batch.lens], dtype=np.uint64)
    oo, tot = fsg.slot_offsets(caps)
    d_out = torch.full((max(tot, 1),), POISON, dtype=torch.uint8, device="cuda")
    d_ol = torch.empty(max(n, 1), dtype=torch.int32, device="cuda")
    d_st = torch.full((max(n, 1),), -7, dtype=torch.int32, device="cuda")
    mx = int(batch.lens.max())
    ws = workspace
    if isinstance(workspace, str):
        ws = codec.compress_workspace(n, mx)
        ws[:256] = 0x5A
    codec.compress(_dev(batch.data), _dev(batch.offsets), _dev(batch.lens), n, mx, d_out, _dev(oo), d_ol, d_st,
                   workspace=ws)
    rep = codec.compress_report(ws, n, mx)
    out = d_out.cpu().numpy()
    ol = d_ol.cpu().numpy()[:n].view(np.uint32)
    st = d_st.cpu().numpy()[:n]
    return [out[int(oo[i]):int(oo[i]) + int(ol[i])].tobytes() for i in range(n)], st, rep


def check_decoded(oracle, items, comps, outs, st):
    for i, (x, c, o, s) in enumerate(zip(items, comps, outs, st)):
        ok, _, ref = oracle.uncompress(c, cap=len(x))
        assert (s == fsg.FSG_OK) == bool(ok), (i, s)
        if ok:
            assert o == ref == x, i


def bodies(kind, sizes, first_index=0):
    b = fsg.make_batch(kind, sizes, first_index=first_index)
    return [b.item(i) for i in range(len(b))]


# ---- inputs shared by the tests (built and compressed by the oracle once)
@pytest.fixture(scope="module")
def batches(oracle):
    mixed = bodies(fsg.KIND_MIXED, fsg.mixed_sizes(3000)) + \
        [fsg.make_batch(fsg.KIND_TEXT if i % 2 else fsg.KIND_RANDOM, [s], first_index=9000 + i).item(0)
         for i, s in enumerate((70000, 300000, 1200000))]
    sets = {
        "random4k": bodies(fsg.KIND_RANDOM, [4096] * 256),
        "text64k": bodies(fsg.KIND_TEXT, [65536] * 128),
        "mixed": mixed,
    }
    return {k: (v, [oracle.compress(x) for x in v]) for k, v in sets.items()}


@pytest.fixture(scope="module")
def small_text(oracle):
    """300 text bodies of 4 KiB, each under 4096 bytes compressed."""
    items = bodies(fsg.KIND_TEXT, [4096] * 300, first_index=500)
    comps = [oracle.compress(x) for x in items]
    assert all(0 < len(c) < 4096 for c in comps)
    return items, comps


def assert_causes_sum(rep):
    assert rep["fallback_bitmap"] + rep["fallback_wide_offsets"] + rep["fallback_pack_guard"] == \
        rep["fallback_messages"], rep


# ---- 1. nothing falls back at defaults
@pytest.mark.parametrize("name,fork", [("random4k", -1), ("text64k", -1), ("mixed", 0), ("mixed", 1)])
def test_decode_defaults_report_zero(codec, oracle, batches, fsg_opts, name, fork):
    items, comps = batches[name]
    fsg_opts(decode_fork=fork)
    outs, st, rep = run_decode(codec, comps, [len(x) for x in items])
    check_decoded(oracle, items, comps, outs, st)
    assert rep["path"] == 0 and rep["single_pass_messages"] == 0, rep
    assert rep["fallback_messages"] == 0, rep
    assert_causes_sum(rep)
    assert 0 < rep["bitmap_words_requested"] <= rep["bitmap_words_capacity"], rep


@pytest.mark.parametrize("name", ["random4k", "text64k", "mixed"])
def test_encode_defaults_report_zero(codec, batches, name):
    """No message takes the encoder's whole-message fallback at default
    options.  The mixed batch holds 12 split messages, three of them
    incompressible with a short last fragment (bodies 1663 and 1899 of the
    mixed size stream, 105,135 and 161,891 bytes, and the 70,000-byte random
    body): with the slot split evenly among the fragments these three
    overflowed their regions (two of 40,832 bytes for 70,000) and fell back;
    split_region (snappy_device.h) gives every full fragment its own worst
    case."""
    items, comps = batches[name]
    got, st, rep = run_encode(codec, items)
    print(name, rep)
    assert (st == fsg.FSG_OK).all()
    assert got == comps  # the oracle's bytes
    assert rep["path"] == 0 and rep["no_workspace_messages"] == 0, rep
    assert rep["fallback_messages"] == 0, rep


# ---- 2. bitmap overflow, exact count
def test_bitmap_overflow_exact_count(codec, oracle):
    n = 200
    x = fsg.make_batch(fsg.KIND_TEXT, [4096], first_index=3).item(0)
    c = oracle.compress(x)
    w = bitmap_words(len(c))
    items, comps = [x] * n, [c] * n
    outs, st, rep = run_decode(codec, comps, [len(x)] * n, ws_total_in=1)
    check_decoded(oracle, items, comps, outs, st)
    assert (st == fsg.FSG_OK).all()
    assert rep["path"] == 0, rep
    assert rep["bitmap_words_requested"] == n * w, rep
    expect = n - rep["bitmap_words_capacity"] // w
    assert expect > 0, rep
    assert rep["fallback_bitmap"] == rep["fallback_messages"] == expect, rep
    assert rep["fallback_wide_offsets"] == 0 and rep["fallback_pack_guard"] == 0, rep
    # a workspace sized for the real input: nothing falls back
    outs, st, rep = run_decode(codec, comps, [len(x)] * n)
    check_decoded(oracle, items, comps, outs, st)
    assert rep["fallback_messages"] == 0 and rep["fallback_bitmap"] == 0, rep
    assert rep["bitmap_words_requested"] == n * w, rep


# ---- 3. bitmap overflow, mixed sizes (test_two_pass_workspace_fallback's batch)
def test_bitmap_overflow_mixed_sizes(codec, oracle):
    rng = np.random.default_rng(77)
    items = [fsg.make_batch(fsg.KIND_TEXT if i % 3 else fsg.KIND_RANDOM,
                            [int(rng.integers(0, 70000))], first_index=i).item(0) for i in range(200)]
    comps = [oracle.compress(x) for x in items]
    comps[5] = comps[5][:-2]
    outs, st, rep = run_decode(codec, comps, [len(x) for x in items], ws_total_in=4096)
    check_decoded(oracle, items, comps, outs, st)
    assert rep["path"] == 0, rep
    assert 0 < rep["fallback_messages"] < len(items), rep
    assert_causes_sum(rep)
    assert rep["bitmap_words_requested"] > rep["bitmap_words_capacity"], rep


# ---- 4. single-pass paths
def test_single_pass_paths(codec, oracle, small_text):
    items, comps = small_text
    n = len(items)
    ws = codec.decompress_workspace(n, 0)
    assert ws.numel() == 256
    for workspace in (ws, None):
        outs, st, rep = run_decode(codec, comps, [len(x) for x in items], workspace=workspace)
        check_decoded(oracle, items, comps, outs, st)
        assert rep["path"] == 2 and rep["single_pass_messages"] == n, rep
        assert rep["fallback_messages"] == 0, rep


# ---- 5. the packed pass's 32-bit offset check
def test_wide_offsets_fall_back(codec, oracle, small_text, fsg_opts):
    import torch
    items, comps = small_text
    n = len(items)
    fsg_opts(decode_fork=1)
    caps = np.array([len(x) for x in items], dtype=np.uint32)
    oo, tot = fsg.slot_offsets(caps.astype(np.uint64))
    tail = 2 << 20
    assert tot <= tail
    # the same batch in an ordinary output buffer first: the packed pass keeps it
    outs, st, rep = run_decode(codec, comps, caps)
    check_decoded(oracle, items, comps, outs, st)
    assert rep["fallback_messages"] == 0 and rep["fallback_wide_offsets"] == 0, rep
    base = 1 << 32
    try:
        d_out = torch.empty(base + tail, dtype=torch.uint8, device="cuda")
    except RuntimeError as e:  # torch.cuda.OutOfMemoryError is one
        pytest.skip(f"torch cannot allocate the {base + tail}-byte output buffer: {e}")
    d_out[base:].fill_(POISON)
    oo = oo + np.uint64(base)  # 16-aligned: slot_offsets aligns, and so is the base
    b = fsg.Batch.from_list(comps)
    d_ol = torch.empty(n, dtype=torch.int32, device="cuda")
    d_st = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    ws = codec.decompress_workspace(n, int(b.data.size))
    codec.decompress(_dev(b.data), _dev(b.offsets), _dev(b.lens), n, d_out, _dev(oo), _dev(caps), d_ol, d_st,
                     workspace=ws)
    rep = codec.decompress_report(ws, n)
    out = d_out[base:].cpu().numpy()
    del d_out
    st = d_st.cpu().numpy()
    outs = [out[int(oo[i]) - base:int(oo[i]) - base + int(caps[i])].tobytes() for i in range(n)]
    check_decoded(oracle, items, comps, outs, st)
    assert (st == fsg.FSG_OK).all()
    assert rep["path"] == 0, rep
    assert rep["fallback_wide_offsets"] == rep["fallback_messages"] == n, rep
    assert rep["fallback_bitmap"] == 0 and rep["fallback_pack_guard"] == 0, rep


# ---- 6. encoder fallback, exact count
def test_encoder_fallback_exact_count(codec, oracle):
    """Regions capped at 4,096 bytes: every fragment of the four long random
    bodies overflows, so all four are re-encoded whole.  With the cap lifted
    none is: an incompressible 64 KiB fragment (65,539 bytes) fits the region
    split_region gives it whatever the message length (70,000, 131,073 and
    200,000 bytes are far from a multiple of 64 KiB)."""
    sizes =[70000, 131073, 200000, 1048576, 5, 65536]
    items = bodies(fsg.KIND_RANDOM, sizes, first_index=40)
    want = [oracle.compress(x) for x in items]
    codec.set_split_region_cap(4096)
    try:
        got, st, rep = run_encode(codec, items)
        assert (st == fsg.FSG_OK).all() and got == want
        assert rep["path"] == 0, rep
        assert rep["split_messages"] == 4 and rep["fallback_messages"] == 4, rep
        codec.set_split_region_cap(0)
        got, st, rep = run_encode(codec, items)
        print("cap 0:", rep)
        assert (st == fsg.FSG_OK).all() and got == want
        assert rep["split_messages"] == 4 and rep["fallback_messages"] == 0, rep
    finally:
        codec.set_split_region_cap(0)


# ---- 7. encoder routing
def test_encoder_routing(codec, oracle, fsg_opts):
    items = bodies(fsg.KIND_TEXT, [8192] * 40, first_index=70)
    want = [oracle.compress(x) for x in items]
    got, st, rep = run_encode(codec, items)
    assert (st == fsg.FSG_OK).all() and got == want
    assert rep["path"] == 0 and rep["wave_units"] == rep["units_listed"] == 40, rep
    got, st, rep = run_encode(codec, items, workspace=None)
    assert (st == fsg.FSG_OK).all() and got == want
    assert rep["path"] == 2 and rep["no_workspace_messages"] == 40, rep
    items = bodies(fsg.KIND_TEXT, [32768] * 200, first_index=120)
    want = [oracle.compress(x) for x in items]
    fsg_opts(encode_wave_min=0)
    got, st, rep = run_encode(codec, items)
    assert (st == fsg.FSG_OK).all() and got == want
    assert rep["path"] == 0 and rep["units_listed"] == 0 and rep["wave_units"] == 0, rep


# ---- 8. large-message counts
def test_large_message_counts(codec, oracle, small_text):
    items, comps = small_text
    assert fsg.get_option("small_batch") == 64
    outs, st, rep = run_decode(codec, comps[:40], [len(x) for x in items[:40]])
    check_decoded(oracle, items[:40], comps[:40], outs, st)
    assert rep["large_messages"] + rep["huge_messages"] == 40, rep
    outs, st, rep = run_decode(codec, comps, [len(x) for x in items])
    check_decoded(oracle, items, comps, outs, st)
    assert rep["large_messages"] == 0 and rep["huge_messages"] == 0, rep


# ---- 9. LZ4
def test_lz4_fallback_exact_count(codec):
    import torch
    lz = Lz4Oracle()
    n = 200
    x = fsg.make_batch(fsg.KIND_TEXT, [4096], first_index=11).item(0)
    body = lz.compress(x)
    hdr = 2  # varint32 of 4096
    w = bitmap_words(len(body) - hdr)
    b = fsg.Batch.from_list([body] * n)
    caps = np.full(n, len(x), dtype=np.uint32)
    oo, tot = fsg.slot_offsets(caps.astype(np.uint64))

    def run(ws):
        d_out = torch.full((tot,), POISON, dtype=torch.uint8, device="cuda")
        d_ol = torch.empty(n, dtype=torch.int32, device="cuda")
        d_st = torch.full((n,), -7, dtype=torch.int32, device="cuda")
        if ws is not None:
            ws.fill_(0x5A)
        codec.lz4_decompress(_dev(b.data), _dev(b.offsets), _dev(b.lens), n, d_out, _dev(oo), _dev(caps), d_ol,
                             d_st, workspace=ws)
        rep = codec.lz4_decompress_report(ws, n)
        out = d_out.cpu().numpy()
        assert (d_st.cpu().numpy() == fsg.FSG_OK).all()
        assert (d_ol.cpu().numpy().view(np.uint32) == len(x)).all()
        for i in range(n):
            assert out[int(oo[i]):int(oo[i]) + len(x)].tobytes() == x, i
        return rep

    assert lz.uncompress(body, len(x))[2] == x
    rep = run(codec.lz4_decompress_workspace(n, 0))  # the two-pass minimum
    assert rep["path"] == 0, rep
    expect = n - rep["bitmap_words_capacity"] // w
    assert 0 < expect < n, rep
    assert rep["bitmap_words_requested"] == n * w, rep
    assert rep["fallback_messages"] == rep["fallback_bitmap"] == expect, rep
    rep = run(codec.lz4_decompress_workspace(n, int(b.data.size)))
    assert rep["path"] == 0 and rep["fallback_messages"] == 0, rep
    rep = run(None)
    assert rep["path"] == 1 and rep["single_pass_messages"] == n, rep
