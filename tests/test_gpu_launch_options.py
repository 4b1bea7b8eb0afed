"""Launch options on the GPU: include/flare_snappy_gpu.h promises of
fsg_set_option that "every value produces the same bytes and statuses".  The
loops of the production launches -- one wave or lane carrying its LDS,
register or table state from one work item into the next -- only run with
these options at non-default values, or at full workload size.  Each test
here sets them so that, by pigeonhole on the path report's counters, some
wave or lane MUST take several items, and compares every status and every
accepted byte with the oracle (oracle/bind.py).  Exact: no tolerance.

Every call goes through gpu_harness.GpuCodec, under the write-containment
guards (the two-stream test, like the test it copies, does its own plumbing:
GpuCodec has no second stream).

Where each option of csrc/options.h meets a non-default value on the GPU:

  option                  test                                            values
  ----------------------  ----------------------------------------------  ------------------
  decode_fork             every decode test here                          0, 1
  split_walk              test_walk_and_split_knobs_forked                2 (parity: 0..2)
  split_class             test_walk_and_split_knobs_forked                0, 1, 7, 8, 15
  exec_keep               test_gpu_parity.test_window_slide_flush_rule    512..2000
  chunked_huge            test_few_large_message_blocks_forked            0
  small_persist           test_gpu_parity.test_decode_fuzz_against_oracle 5, 1792
  small_batch             test_gpu_parity.test_small_batch_verdicts       0
  split_huge              test_few_large_message_blocks_forked            0
  walk_order              test_walk_and_split_knobs_forked                0
  lean_walk               test_two_stream_without_lean_walk               0
  exec_big_blocks         test_few_large_message_blocks_one_stream        1, 3
  exec_prio               test_few_large_message_blocks_one_stream        0
  exec_big_blocks_fork    test_few_large_message_blocks_forked            1
  exec_pack               test_walk_and_split_knobs_forked                0 (parity: 1, 7, 64)
  encode_wave_min         test_few_encode_lanes                           0
  encode_wave_share       test_encode_wave_share                          0, 1, 500, 999, 1000
  encode_wave_all_mb      test_encode_wave_share                          0
  encode_lanes            test_few_encode_lanes                           64, 256
  encode_wave_per_cu      test_more_units_than_waves                      1
  encode_wave_wg          test_more_units_than_waves                      5
  lz4_big_min             test_lz4_gpu                                    0 .. 1 << 20
  lz4_encode_wave_min     test_lz4_wave_gpu                               0, 4096, ...
  lz4_encode_wave_per_cu  test_lz4_wave_gpu.test_more_bodies_than_waves   1
  lz4f_force_serial       test_lz4f_gpu                                   1
  lz4f_block_wave_min     test_lz4f_gpu                                   0, ...
  lz4f_nosize_fast        test_lz4f_nosize_gpu                            1
  lz4f_length_wave_min    test_lz4f_nosize_gpu                            0, ...
  lz4f_linked_fast        test_lz4f_linked_gpu                            1
"""
import numpy as np
import pytest

import fsg
from bind import Oracle
from snappy_batches import (check_against_oracle, mutate, oracle_verdicts, rand, small_bodies_forked_batch, text)

pytestmark = pytest.mark.gpu

# csrc/decode_v4_plan.h
BIG_INDEX_MIN = 8 * 1024     # kBigIndexMin: the large-message threshold's floor
HUGE_BYTES = 256 * 1024      # kHugeIndexBytes
WAVES_PER_BLOCK = 4          # kWavesPerBlock
INDEX_BIG_WAVES = 1024 * 4   # index_big_grid <= 1024 blocks of 4 waves


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test run without a visible GPU")
    from gpu_harness import GpuCodec
    return GpuCodec()


@pytest.fixture(scope="module")
def oracle():
    return Oracle()


# ---- decode_v4_plan's arithmetic, restated (csrc/decode_v4_plan.h)
def plan_est_total_in(n: int, ws_bytes: int) -> int:
    """est_total_in: the batch's compressed bytes as the launch estimates
    them from the workspace size (decode_v4_bitmap_capacity_words)."""
    base_bytes = (4 * n + 255) & ~255
    chunk_bytes = (ws_bytes // 64) & ~255
    chunk_off = (ws_bytes - chunk_bytes) & ~255
    cap_words = min((chunk_off - 256 - 11 * base_bytes) // 4, 0x7FFFFFFF)
    return (cap_words - 4 * n - 64) * 32 if cap_words > 4 * n + 64 else 0


def plan_big_threshold(n: int, ws_bytes: int) -> int:
    """big_threshold for a batch of more than small_batch messages."""
    return min(max(4 * plan_est_total_in(n, ws_bytes) // n, BIG_INDEX_MIN), 48 * 1024)


def real_workspace_bytes(gpu, comps) -> int:
    return gpu.codec.lib.fsg_decompress_workspace_bytes(len(comps), sum(len(c) for c in comps))


# =========================================================================
# Decode 1 / 2: few large-message blocks
# =========================================================================
@pytest.fixture(scope="module")
def large_batch(oracle):
    """Large bodies of every kind of pass 2's large-message role, each kind
    intact, bit-flipped, truncated and late-corrupted in turn
    (snappy_batches.mutate, test_large_message_index_fuzz's recipe), so a
    valid item follows a corrupt one in list order:
      3 huge ones (over 256 KiB compressed: intact, late-corrupted, bit-flipped),
      160 large bodies of 9-40 KiB compressed (text and random),
       14 text bodies of 150-300 KB, whose output runs as 64 KiB segments,
    spread among tiny text bodies (20-200 B), as many as keep four times the
    mean compressed size under 8 KiB: the large-message threshold then sits
    at its floor, kBigIndexMin, and every body over it is listed."""
    rng = np.random.default_rng(2027)
    srcs = [rand(300000, first_index=600), text(1 << 20, first_index=601), rand(270000, first_index=602)]
    for i in range(160):
        if i % 2:
            srcs.append(rand(int(rng.integers(9300, 40000)), first_index=300 + i))
        else:  # text compresses to about a half
            srcs.append(text(int(rng.integers(26000, 80000)), first_index=300 + i))
    for i in range(14):
        srcs.append(text(int(rng.integers(150000, 300000)), first_index=500 + i))
    big = [oracle.compress(s) for s in srcs]
    assert all(BIG_INDEX_MIN < len(c) for c in big)
    assert sum(len(c) > HUGE_BYTES for c in big) == 3
    big_comps = [mutate(rng, c, (0, 3, 1)[i] if i < 3 else i % 4) for i, c in enumerate(big)]
    assert sum(len(c) > HUGE_BYTES for c in big_comps) == 3
    big_caps = [len(s) for s in srcs]
    n_tiny = max(200, sum(len(c) for c in big_comps) // 1700)
    tiny_src = [text(int(rng.integers(20, 201)), first_index=1000 + i) for i in range(n_tiny)]
    tiny = [oracle.compress(s) for s in tiny_src]
    # interleave: a large body every few tiny ones, in list order
    comps, caps, is_big = [], [], []
    step = n_tiny // len(big_comps)
    for i, (c, cap) in enumerate(zip(big_comps, big_caps)):
        comps.append(c); caps.append(cap); is_big.append(True)
        for j in range(i * step, (i + 1) * step):
            comps.append(tiny[j]); caps.append(len(tiny_src[j])); is_big.append(False)
    for j in range(len(big_comps) * step, n_tiny):
        comps.append(tiny[j]); caps.append(len(tiny_src[j])); is_big.append(False)
    expect = oracle_verdicts(oracle, comps, caps)
    # a valid large item follows a corrupt one, and the reverse
    verdicts = [bool(e[0]) for e, b in zip(expect, is_big) if b]
    assert any(a and not b for a, b in zip(verdicts, verdicts[1:]))
    assert any(b and not a for a, b in zip(verdicts, verdicts[1:]))
    return comps, caps, expect, sum(len(c) > BIG_INDEX_MIN for c in comps), sum(verdicts)


def check_large_batch(gpu, large_batch, blocks):
    comps, caps, expect, n_big, n_big_ok = large_batch
    # the threshold at its floor: every large body is listed for pass 1b
    assert plan_big_threshold(len(comps), real_workspace_bytes(gpu, comps)) == BIG_INDEX_MIN
    outs, ol, st = gpu.decompress(comps, caps)
    rep = gpu.last_report
    print(rep)
    n_ok, n_bad = check_against_oracle(expect, outs, ol, st)
    assert n_ok > len(comps) - n_big and n_bad >= n_big // 4
    assert n_big >= 10 * WAVES_PER_BLOCK * 3  # (bodies over the threshold; a bad header is not listed)
    assert rep["path"] == fsg.PATH_MAIN and rep["fallback_messages"] == 0, rep
    # pigeonhole: blocks * 4 waves share the listed messages, ten each at least
    assert rep["large_messages"] + rep["huge_messages"] <= n_big, rep
    assert rep["large_messages"] + rep["huge_messages"] >= 10 * WAVES_PER_BLOCK * blocks, rep
    assert rep["huge_messages"] == 3, rep
    # ... and the accepted ones alone (each at least one execution item) outnumber the waves
    assert n_big_ok >= 4 * WAVES_PER_BLOCK * blocks
    return rep


@pytest.mark.parametrize("prio", [0, 1])
@pytest.mark.parametrize("blocks", [1, 3])
def test_few_large_message_blocks_one_stream(gpu, large_batch, fsg_opts, blocks, prio):
    """exec_kernel's large-message role on one stream with 1 or 3 blocks (4 or
    12 waves) for some 170 listed messages: every wave draws whole messages and
    64 KiB segments from exec_next one after another, corrupt and valid ones
    mixed, reusing its tag ring and output window; with and without the
    priority raise around round-A loads."""
    fsg_opts(decode_fork=0, exec_big_blocks=blocks, exec_prio=prio)
    check_large_batch(gpu, large_batch, blocks)


@pytest.mark.parametrize("chunked_huge", [0, 1])
@pytest.mark.parametrize("split_huge", [0, 1])
def test_few_large_message_blocks_forked(gpu, large_batch, fsg_opts, split_huge, chunked_huge):
    """The same batch on the forked path with one large-message block per
    launch: the huge bodies on the one side stream (split_huge 0, pass 1b
    mode 0) or on their own (1), walked by a wave each or in chunks."""
    fsg_opts(decode_fork=1, exec_big_blocks_fork=1, split_huge=split_huge, chunked_huge=chunked_huge)
    check_large_batch(gpu, large_batch, 1)


# =========================================================================
# Decode 3: more large messages than pass-1b waves
# =========================================================================
@pytest.fixture(scope="module")
def many_large(oracle):
    """4,200 large bodies (two distinct random bodies of 9 KiB with a
    repeated tail, and the first with a byte changed near its end so that the
    oracle rejects it, in rotation) before, between and after 16,000 bodies of
    about 20 bytes: the mean compressed size stays under 2 KiB, the threshold
    at 8 KiB."""
    rng = np.random.default_rng(4200)
    a = rng.integers(0, 256, 9216, dtype=np.uint8).tobytes()
    b = rng.integers(0, 256, 9216, dtype=np.uint8).tobytes()
    a, b = a + a[:300], b + b[100:350]  # the streams end in copies
    ca, cb = oracle.compress(a), oracle.compress(b)
    assert len(ca) > BIG_INDEX_MIN and len(cb) > BIG_INDEX_MIN
    cc = None
    for back in range(1, 32):  # a byte near the end whose change the oracle rejects
        for x in (0xFF, 0x5A, 0x80):
            t = bytearray(ca)
            t[len(t) - back] ^= x
            if oracle.uncompress(bytes(t), cap=len(a))[0] is False:
                cc = bytes(t)
                break
        if cc:
            break
    assert cc is not None
    tiny_src = text(20, first_index=3)
    tiny = oracle.compress(tiny_src)
    three = [(ca, len(a)), (cb, len(b)), (cc, len(a))]
    comps, caps = [], []
    n_large, n_tiny = 4200, 16000
    for i in range(n_large):
        c, cap = three[i % 3]
        comps.append(c); caps.append(cap)
        k = n_tiny // n_large + (1 if i < n_tiny % n_large else 0)
        comps += [tiny] * k
        caps += [len(tiny_src)] * k
    assert len(comps) == n_large + n_tiny
    verdict = {c: oracle.uncompress(c, cap=cap) for c, cap in three + [(tiny, len(tiny_src))]}
    assert verdict[ca][0] and verdict[cb][0] and verdict[cc][0] is False and verdict[tiny][0]
    return comps, caps, [verdict[c] for c in comps], n_large


@pytest.mark.parametrize("fork", [0, 1])
def test_more_large_messages_than_index_waves(gpu, many_large, fsg_opts, fork):
    """index_big_kernel runs at most 1,024 blocks of 4 waves: with more than
    4,096 listed messages some wave takes a second one from big_next (its
    staging buffer and window state reused), valid after corrupt.  (38 MB of
    output: most of the test's time is the containment check's copy-back.)"""
    comps, caps, expect, n_large = many_large
    fsg_opts(decode_fork=fork)
    assert plan_big_threshold(len(comps), real_workspace_bytes(gpu, comps)) == BIG_INDEX_MIN
    outs, ol, st = gpu.decompress(comps, caps)
    rep = gpu.last_report
    print(rep)
    assert rep["path"] == fsg.PATH_MAIN and rep["fallback_messages"] == 0, rep
    assert rep["large_messages"] == n_large > INDEX_BIG_WAVES and rep["huge_messages"] == 0, rep
    n_ok, n_bad = check_against_oracle(expect, outs, ol, st)
    assert n_bad == n_large // 3 and n_ok == len(comps) - n_bad


# =========================================================================
# Decode 4: walk and split knobs on the forked path
# =========================================================================
@pytest.fixture(scope="module")
def forked_mixed(oracle):
    """test_small_bodies_forked's batch plus 40 bodies of 2-40 KiB compressed
    (text and random, every fourth one mutated): every size class of the
    planned walk is populated, on both sides of every split point.  Slots are
    exactly the stated length (64 bytes where the header is bad)."""
    rng = np.random.default_rng(404)
    comps = small_bodies_forked_batch(oracle)
    mid = []
    for i in range(40):
        want = int(2048 * (20.0 ** (i / 39.0)))  # 2 KiB .. 40 KiB compressed, evenly in log size
        src = rand(want, first_index=700 + i) if i % 3 == 0 else text(int(want * 2.6), first_index=700 + i)
        c = oracle.compress(src)
        mid.append(mutate(rng, c, 1 + i % 3) if i % 4 == 3 else c)
    assert min(len(c) for c in mid) < 4096 and max(len(c) for c in mid) > 32768
    # spread among the short ones
    for i, c in enumerate(mid):
        comps.insert((i * 37 + 11) % len(comps), c)
    classes = {15 - min(max(len(c), 1).bit_length() - 1, 15) for c in comps}
    assert classes >= set(range(0, 16)), sorted(classes)
    caps = []
    for c in comps:
        h, ulen = oracle.header(c)
        caps.append(ulen if h and ulen <= 1 << 17 else 64)
    return comps, caps, oracle_verdicts(oracle, comps, caps)


_FORKED_KNOBS = ([dict(), dict(walk_order=0)] +
                 [dict(split_class=c, exec_pack=p) for c in (0, 1, 7, 8, 15) for p in (32, 0)] +
                 [dict(split_walk=2, split_class=0)])


@pytest.mark.parametrize("skew", [0, 7])
@pytest.mark.parametrize("knobs", _FORKED_KNOBS, ids=lambda k: "-".join(f"{a}{b}" for a, b in k.items()) or "defaults")
def test_walk_and_split_knobs_forked(gpu, forked_mixed, fsg_opts, knobs, skew):
    """The forked path at default options (with the path report, which
    test_small_bodies_forked does not read), without the walk permutation (walk_order 0: planned
    walk and execution in message order), with the boundary between the
    packed pass and the one-wave-per-body pass at every kind of size class
    (split_class 0 hands the packed pass every body up to the large-message
    threshold, 15 almost none), packed and unpacked, and in one launch in walk
    order (split_walk 2); output slots aligned and of every alignment."""
    comps, caps, expect = forked_mixed
    fsg_opts(decode_fork=1, **knobs)
    # a workspace sized for 13 KiB per body puts the large-message threshold
    # at its ceiling: the bodies of up to 40 KiB stay on the walk and its
    # execution passes (with the real size, 8 KiB: test_small_bodies_forked's case)
    total_in = 13 * 1024 * len(comps)
    assert plan_big_threshold(len(comps), gpu.codec.lib.fsg_decompress_workspace_bytes(len(comps), total_in)) == 48 * 1024
    outs, ol, st = gpu.decompress(comps, caps, slot_skew=skew, ws_total_in=total_in)
    rep = gpu.last_report
    print({k: v for k, v in rep.items() if k.startswith("fallback")})
    n_ok, n_bad = check_against_oracle(expect, outs, ol, st)
    assert n_ok > 700 and n_bad > 100
    # nothing goes to pass 3: the workspace holds every bitmap, and the packed
    # pass ends a batch whose last body carries tags after its output is
    # complete (the trailing zero-length literals here) without its guard
    assert rep["path"] == fsg.PATH_MAIN and rep["fallback_messages"] == 0 and rep["fallback_pack_guard"] == 0, rep


# =========================================================================
# Decode 5: the two-stream form without the lean walk
# =========================================================================
@pytest.fixture(scope="module")
def two_stream_batches(oracle):
    """Two batches of more than 64 bodies (so the lane walk, not pass 1b,
    indexes most of them), with mutated and truncated streams among the
    valid ones: "short" with a mean compressed size well under 16 KiB
    (lean_walk 0: kWalkSerial), "long" well over (kWalkStandard)."""
    rng = np.random.default_rng(55)
    out = {}
    for name, sizes in (("short", rng.integers(1, 30000, 96)), ("long", rng.integers(60000, 130000, 72))):
        srcs = [text(int(s), first_index=2000 + j) if j % 4 else rand(int(s) // 2 + 1, first_index=2000 + j)
                for j, s in enumerate(sizes)]
        srcs.append(text(200000, first_index=7))  # the segment path
        comps = [oracle.compress(s) for s in srcs]
        comps = [mutate(rng, c, 1 + (i // 5) % 3) if i % 5 == 2 else c for i, c in enumerate(comps)]
        caps = [len(s) for s in srcs]
        out[name] = (comps, caps, oracle_verdicts(oracle, comps, caps))
    return out


@pytest.mark.parametrize("lean_walk", [0, 1])
def test_two_stream_without_lean_walk(gpu, two_stream_batches, fsg_opts, lean_walk):
    """test_two_stream_decode_stream_of_batches' pattern (pass 1 on a second
    stream, two buffer sets reused behind an event) over six batches
    alternating "short" and "long", each buffer set's workspace sized for its
    own batch: with lean_walk 0 the two-stream form runs the serial walk on
    one and the standard walk on the other; with 1 the lean walk on both."""
    import torch
    from gpu_harness import dev
    fsg_opts(lean_walk=lean_walk)
    codec = gpu.codec
    names = ["short", "long"]
    sets = []
    for name in names:
        comps, caps, expect = two_stream_batches[name]
        b = fsg.Batch.from_list(comps)
        caps = np.array(caps, dtype=np.uint32)
        oo, tot = fsg.slot_offsets(caps.astype(np.uint64))
        ws = codec.decompress_workspace(len(b), int(b.data.size))
        sets.append(dict(n=len(b), d_in=dev(b.data), d_io=dev(b.offsets), d_il=dev(b.lens), oo=oo, d_oo=dev(oo),
                         d_cap=dev(caps), caps=caps, expect=expect, ws=ws,
                         out=torch.full((tot,), 0xA5, dtype=torch.uint8, device="cuda"),
                         ol=torch.zeros(len(b), dtype=torch.int32, device="cuda"),
                         st=torch.full((len(b),), -7, dtype=torch.int32, device="cuda"), done=None))
    # which walk lean_walk 0 selects (decode_v4_plan: est_total_in < 16384 n: serial)
    est = [plan_est_total_in(s["n"], s["ws"].numel()) for s in sets]
    assert all(s["n"] > 64 for s in sets)
    assert est[0] < 16384 * sets[0]["n"] and est[1] >= 16384 * sets[1]["n"], est
    s_main = torch.cuda.current_stream()
    s1 = torch.cuda.Stream()
    torch.cuda.synchronize()
    results = []

    def collect(k):
        s = sets[k % 2]
        torch.cuda.synchronize()
        out = s["out"].cpu().numpy()
        ol = s["ol"].cpu().numpy().view(np.uint32).copy()
        st = s["st"].cpu().numpy().copy()
        outs = [out[int(s["oo"][i]):int(s["oo"][i]) + int(min(ol[i], s["caps"][i]))].tobytes()
                for i in range(s["n"])]
        results.append((k, outs, ol, st, codec.decompress_report(s["ws"], s["n"])))
        # poison again: the next batch on this set must write every byte itself
        s["out"].fill_(0xA5)
        s["st"].fill_(-7)
        s["ws"].fill_(0x5A)
        torch.cuda.synchronize()

    for k in range(6):
        s = sets[k % 2]
        if s["done"] is not None:
            collect(k - 2)  # (also orders: the set is free again)
            s1.wait_event(s["done"])
        codec.decompress(s["d_in"], s["d_io"], s["d_il"], s["n"], s["out"], s["d_oo"], s["d_cap"], s["ol"],
                         s["st"], stream=s_main, workspace=s["ws"], pass1_stream=s1)
        ev = torch.cuda.Event()
        ev.record(s_main)
        s["done"] = ev
    collect(4)
    collect(5)
    assert sorted(r[0] for r in results) == list(range(6))
    for k, outs, ol, st, rep in results:
        n_ok, n_bad = check_against_oracle(sets[k % 2]["expect"], outs, ol, st)
        assert n_ok > 40 and n_bad >= 5, (k, n_ok, n_bad)
        assert rep["path"] == fsg.PATH_MAIN and rep["fallback_messages"] == 0, (k, rep)


# =========================================================================
# Encode
# =========================================================================
def check_encoded(gpu, oracle, items, want=None):
    """Compress on the device: the oracle's bytes; then decode them back on
    the device.  Returns the compress call's report."""
    want = want or [oracle.compress(x) for x in items]
    comps, st = gpu.compress(fsg.Batch.from_list(items))
    rep = gpu.last_report
    print(rep)
    assert (st == fsg.FSG_OK).all()
    for i, (x, c, w) in enumerate(zip(items, comps, want)):
        assert c == w, (i, len(x))
    assert rep["path"] == fsg.PATH_MAIN and rep["no_workspace_messages"] == 0, rep
    assert rep["fallback_messages"] == 0, rep
    outs, ol, st = gpu.decompress(comps, [len(x) for x in items])
    assert (st == fsg.FSG_OK).all() and all(o == x for o, x in zip(outs, items))
    return rep


@pytest.fixture(scope="module")
def lane_items(oracle):
    """1,500 bodies drawn as test_randomized_against_oracle draws them (0 B
    to 140 KB, alphabets 2 to 256), the sizes either side of every
    table_size_for step (256 .. 16,384 entries) and of the 64 KiB fragment
    edge, and 1,100 short bodies (0-300 B); ordered so that short bodies
    (small tables) follow long ones (large tables) and the reverse all
    through the list."""
    rng = np.random.default_rng(606)
    drawn = []
    for t in range(1500):
        n = int(rng.choice([rng.integers(0, 100), rng.integers(0, 5000), rng.integers(0, 140000)]))
        alpha = int(rng.choice([2, 3, 8, 40, 256]))
        drawn.append(rng.integers(0, alpha, n, dtype=np.uint8).tobytes())
    edges = []
    for k in range(8, 15):
        for n in ((1 << k) - 1, 1 << k, (1 << k) + 1):
            edges.append(text(n, first_index=800 + n) if k % 2 else
                         rng.integers(0, 8, n, dtype=np.uint8).tobytes())
    for i, n in enumerate((65535, 65536, 65537, 131073)):
        edges.append(text(n, first_index=900 + i))
    short = [rng.integers(0, int(rng.choice([2, 8, 256])), int(rng.integers(0, 301)), dtype=np.uint8).tobytes()
             for _ in range(1100)]
    longs = sorted(drawn + edges, key=len, reverse=True)
    # long, short, long, ... : the longest beside the shortest first, so the
    # table size swings both ways between neighbours
    items = []
    for i, x in enumerate(longs):
        items.append(x)
        if i < len(short):
            items.append(short[i])
    assert len(items) == len(drawn) + len(edges) + len(short)
    return items, [oracle.compress(x) for x in items]


@pytest.mark.parametrize("wave_min", [0, None], ids=["lanes_only", "defaults"])
@pytest.mark.parametrize("lanes", [64, 256])
def test_few_encode_lanes(gpu, oracle, lane_items, fsg_opts, lanes, wave_min):
    """encode_pipe_kernel with 64 or 256 lanes for 2,600 bodies: every lane
    draws unit after unit from ctr[0], its hash table in the workspace
    changing size (table_size_for) from one to the next; alone
    (encode_wave_min 0) and beside the wave encoder."""
    items, want = lane_items
    fsg_opts(encode_lanes=lanes)
    if wave_min is not None:
        fsg_opts(encode_wave_min=wave_min)
    rep = check_encoded(gpu, oracle, items, want)
    assert rep["split_messages"] == sum(len(x) > 65536 for x in items) > 100, rep
    if wave_min == 0:
        assert rep["wave_units"] == 0, rep
    else:
        assert rep["wave_units"] == rep["units_listed"] > 0, rep
    # pigeonhole: a wave-encoder unit is at most one message, the lanes take every other
    assert (len(items) - rep["wave_units"]) / lanes >= 5, rep


@pytest.mark.parametrize("wg", [1, 5])
def test_more_units_than_waves(gpu, oracle, fsg_opts, wg):
    """encode_wave_kernel with one wave per CU (256 waves; 260 in 52
    workgroups of five) and more units than that: 800 text and random bodies
    of 4-8 KiB, all on the wave encoder by the short-bodies rule
    (max_in_len <= 8192), and 300 bodies of 64 KiB with the all-on-wave bound
    raised.  Every wave takes a second unit from ctr[5], its LDS table
    refilled."""
    fsg_opts(encode_wave_per_cu=1, encode_wave_wg=wg)
    waves = (256 + wg - 1) // wg * wg
    rng = np.random.default_rng(700 + wg)
    items = [text(int(n), first_index=1200 + i) if i % 3 else rand(int(n), first_index=1200 + i)
             for i, n in enumerate(rng.integers(4096, 8193, 800))]
    assert max(map(len, items)) <= 8192
    rep = check_encoded(gpu, oracle, items)
    assert rep["wave_units"] == rep["units_listed"] == len(items) > 256, rep
    assert rep["wave_units"] >= 2 * waves, rep
    fsg_opts(encode_wave_all_mb=1 << 20)
    items = [text(65536, first_index=1300 + i) if i % 4 else rand(65536, first_index=1300 + i) for i in range(300)]
    rep = check_encoded(gpu, oracle, items)
    assert rep["wave_units"] == rep["units_listed"] == len(items) > 256, rep
    assert rep["wave_units"] > waves, rep


@pytest.fixture(scope="module")
def share_items(oracle):
    items = [text(32768, first_index=1400 + i) for i in range(200)]
    items[50:50] = [text(70000, first_index=1), rand(131073, first_index=2)]
    items += [text(200000, first_index=3), text(65537, first_index=4)]
    return items, [oracle.compress(x) for x in items]


@pytest.mark.parametrize("share", [0, 1, 500, 999, 1000])
def test_encode_wave_share(gpu, oracle, share_items, fsg_opts, share):
    """The long units split between the wave encoder and the lanes at every
    kind of share (wave_quota_of with all_bytes 0): none, one unit, half, all
    but one, all -- 200 whole units of 32 KiB and the fragments of four split
    bodies."""
    items, want = share_items
    fsg_opts(encode_wave_all_mb=0, encode_wave_share=share)
    rep = check_encoded(gpu, oracle, items, want)
    units = 200 + sum((len(x) + 65535) // 65536 for x in items if len(x) > 65536)
    assert rep["units_listed"] == units and rep["split_messages"] == 4, rep
    # wave_quota_of restated: ceil(units * share / 1000)
    assert rep["wave_units"] == (rep["units_listed"] * share + 999) // 1000, rep
