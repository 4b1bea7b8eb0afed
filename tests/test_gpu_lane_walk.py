"""The lane walk's tag step (csrc/decode_v4_index.h): tag bytes read one at a
time from the input ring, one packed advance/length accumulator per
iteration, long literals handled after the unrolled loop.  Hand-built streams
put long literals wherever that split can go wrong; every status, out_len and
accepted byte is compared with the oracle.  Exact: no tolerance.

Every batch here has more than 64 bodies (smaller ones go to pass 1b, not to
the lane walk) and runs on each instance of index_kernel:

  mode        launch                                     tags per iteration
  ----------  -----------------------------------------  ------------------
  serial      decode_fork 0, mean compressed < 16 KiB    32 (four waves per workgroup)
  standard    decode_fork 0, workspace sized for 20 KiB  32
              per body (raises the estimated mean)
  planned     decode_fork 1                              24
  lean        the two-stream entry                       16

Slots are side by side and poisoned with 0xA5, the workspace is filled with
0xFF, and the bytes outside the slots are checked (gpu_harness, containment).

Where a long literal's tag byte lands is not computed here: the sweeps move it
one input byte at a time behind fillers of two-byte tags (every tag slot of an
iteration and every byte alignment, whatever the geometry) and of 61-byte tags
(every position around the bit groups of 128 input bytes, the super-groups of
512 and the 256 bytes the ring covers).  Bodies with a 65,535- or 65,536-byte
literal are larger than any large-message threshold and are indexed by pass
1b; their truncated forms stay on the lane walk.
"""
import numpy as np
import pytest

import containment as ct
import fsg
from oracle_codec import OracleCodec
from snappy_batches import check_against_oracle, oracle_verdicts
from snappy_streams import copy_tag, synthetic_stream

pytestmark = pytest.mark.gpu

BIG_INDEX_MIN = 8 * 1024  # kBigIndexMin (csrc/decode_v4_plan.h)


def varint(n: int) -> bytes:
    out = bytearray()
    while n >= 0x80:
        out.append((n & 0x7F) | 0x80)
        n >>= 7
    out.append(n)
    return bytes(out)


class Body:
    """A tag stream under construction, with the output it stands for."""

    def __init__(self, seed: int = 0):
        self.tags = bytearray()
        self.out = bytearray()
        self.rng = np.random.default_rng(seed)

    def lit(self, n: int, nb: int | None = None):
        """A literal of n fresh bytes; nb asks for a length field of at least
        nb bytes (1..4: a long-literal tag whatever n is)."""
        data = self.rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        if nb is None and n <= 60:
            self.tags += bytes([(n - 1) << 2])
        else:
            nb = max(nb or 1, ((n - 1).bit_length() + 7) // 8)
            self.tags += bytes([(59 + nb) << 2]) + (n - 1).to_bytes(nb, "little")
        self.tags += data
        self.out += data
        return self

    def copy(self, off: int, ln: int, wide: bool = False):
        self.tags += copy_tag(off, ln, wide)
        for _ in range(ln):
            self.out.append(self.out[-off])
        return self

    def fill(self, p: int, dense: bool):
        """Tags that take exactly p input bytes (p == 0 or p >= 2): two-byte
        tags (a one-byte literal, then copies of 4 at offset 1; one three-byte
        literal tag when p is odd), or literals of up to 60 bytes."""
        assert p == 0 or p >= 2
        if dense and p:
            first = 2 if p % 2 else 1
            self.lit(first)
            for _ in range((p - first - 1) // 2):
                self.copy(1, 4)
        elif p:
            while p >= 63:
                self.lit(60)
                p -= 61
            if p == 62:
                self.lit(30)
                p -= 31
            self.lit(p - 1)
        return self

    def tail(self):
        """Tags after the case's literal, so the walk goes on past it."""
        return self.copy(1, 4).lit(3).copy(5, 7)

    def body(self, ulen: int | None = None) -> bytes:
        return varint(len(self.out) if ulen is None else ulen) + bytes(self.tags)


def long_literal_cases():
    cases = []  # (name, compressed bytes)
    seed = [0]

    def new():
        seed[0] += 1
        return Body(seed[0])

    def add(name, b, with_tail):
        if with_tail:
            b.tail()
        cases.append((name, b.body()))

    # the tag byte on every tag slot and byte alignment: two-byte tags before it
    dense = [0] + list(range(2, 331))
    for p in dense:
        add(f"dense{p}-61", new().fill(p, True).lit(61), p % 3 == 0)
        add(f"dense{p}-300", new().fill(p, True).lit(300), p % 3 == 1)
    for p in [0] + list(range(2, 90)):
        add(f"dense{p}-70nb4", new().fill(p, True).lit(70, nb=4), p % 2 == 0)
    # around the bit groups (128), the ring's 256 bytes, the super-groups (512)
    sparse = list(range(90, 140)) + list(range(230, 290)) + list(range(480, 530)) + list(range(1000, 1040))
    for p in sparse:
        add(f"sparse{p}-61", new().fill(p, False).lit(61), p % 2 == 0)
        add(f"sparse{p}-257", new().fill(p, False).lit(257), p % 2 == 1)
    # every length, with the shortest and with longer length fields
    spots = (0, 2, 3, 4, 5, 37, 126, 127, 128, 129, 510, 511, 512, 513)
    for p in spots:
        for n, nbs in ((61, (1, 2, 4)), (64, (1, 3)), (65, (1,)), (255, (1, 2)), (256, (1, 4)), (257, (2, 3)),
                       (1, (1, 4)), (60, (1,))):
            for nb in nbs:
                add(f"at{p}-{n}nb{nb}", new().fill(p, p % 2 == 0).lit(n, nb=nb), (p + nb) % 2 == 0)
    for p in (0, 3, 126, 513):
        for n, nb in ((65535, 2), (65536, 3), (65536, 4)):
            b = new().fill(p, True).lit(n, nb=nb)
            whole = b.body()
            cases.append((f"at{p}-{n}nb{nb}", whole))
            cases.append((f"at{p}-{n}nb{nb}-cut", whole[:5000 + p]))  # the literal runs past the input
    return cases


def run_cases():
    cases = []
    b = Body(101)
    for _ in range(120):
        b.lit(61)
    cases.append(("run-61x120", b.body()))
    for k in (26, 110):
        b = Body(102 + k)
        for _ in range(k):
            b.lit(300)
        cases.append((f"run-300x{k}", b.body()))
    b = Body(103)
    for _ in range(110):
        b.lit(61).copy(1, 1)
    cases.append(("alt-61", b.body()))
    b = Body(104)
    for _ in range(24):
        b.lit(300).copy(7, 1)
    cases.append(("alt-300", b.body()))
    b = Body(105)
    for i in range(40):  # long literals between runs of two-byte tags of every length up to 39
        b.lit(62 + i)
        for _ in range(i):
            b.copy(1, 4)
    cases.append(("ll-between-dense", b.body()))
    # packed accumulator bounds: the largest advance and the largest length on every tag
    b = Body(106)
    for _ in range(130):
        b.lit(60)
    cases.append(("max-advance", b.body()))
    b = Body(107).lit(1)
    for _ in range(2000):
        b.copy(1, 64)
    cases.append(("max-length", b.body()))
    b = Body(108).lit(4)
    for i in range(1500):
        b.copy(1 + i % 4, 64, wide=i % 2 == 0)
    cases.append(("max-length-copy4", b.body()))
    b = Body(109).lit(1)
    for _ in range(3000):
        b.copy(1, 11)
    cases.append(("dense-copy1", b.body()))
    return cases


def corrupt_cases():
    cases = []
    fills = (0, 2, 3, 4, 5, 57, 58, 59, 60, 61, 125, 251, 509)
    for k, p in enumerate(fills):
        d = k % 2 == 0
        # a long literal's length past the input by one byte
        for n, nb in ((61, 1), (300, 2), (70, 4)):
            cases.append((f"past1-{p}-{n}", Body(200 + k).fill(p, d).lit(n, nb=nb).body()[:-1]))
        # 0xFFFFFFFF wraps to length 0; huge lengths whose ip + len wraps
        for val in (0xFFFFFFFF, 0xFFFFFFFA, 0xFFFFFFF9, 0xFFFFFFF0, 0x80000000, 0x7FFFFFFF, 0xFFFFFF00):
            b = Body(300 + k).fill(p, d)
            b.tags += b"\xfc" + val.to_bytes(4, "little")
            for rest in (b"", bytes(range(40))):
                cases.append((f"wrap-{p}-{val:x}-{len(rest)}", b.body(len(b.out) + 40) + rest))
        # a tag cut by the end of input at each of its bytes
        for tag in (b"\xfc\x45\x00\x00\x00", b"\xf8\x45\x00\x00", b"\xf4\x45\x00", b"\xf0\x45",
                    copy_tag(1, 9, wide=True), copy_tag(1, 30), copy_tag(1, 5), b"\x0c"):
            for cut in range(1, len(tag) + 1):
                b = Body(400 + k).fill(p or 2, d)
                cases.append((f"cut-{p}-{tag[0]:02x}-{cut}", b.body(len(b.out) + 70) + tag[:cut]))
        # the header's length one under and one over the output
        for n in (61, 300):
            for t in (False, True):
                b = Body(500 + k).fill(p, d).lit(n)
                if t:
                    b.tail()
                for delta in (-1, 1):
                    cases.append((f"ulen{delta:+d}-{p}-{n}-{int(t)}", b.body(len(b.out) + delta)))
    return cases


def fuzz_cases():
    rng = np.random.default_rng(77)
    cases = []
    for i in range(160):
        b = Body(1000 + i)
        b.lit(int(rng.integers(1, 70)))
        target = int(rng.integers(200, 7000))
        while len(b.tags) < target:
            r = rng.random()
            if r < 0.35:
                b.lit(int(rng.choice([61, 62, 64, 65, 100, 255, 256, 257, 300, 1000])),
                      nb=int(rng.integers(1, 5)) if rng.random() < 0.3 else None)
            elif r < 0.5:
                b.lit(int(rng.integers(1, 61)))
            else:
                for _ in range(int(rng.integers(1, 40))):
                    b.copy(int(rng.integers(1, min(len(b.out), 2000) + 1)), int(rng.integers(1, 65)),
                           wide=rng.random() < 0.1)
        cases.append((f"fuzz{i}", b.body()))
    for i in range(40):
        cases.append((f"synthetic{i}", synthetic_stream(rng, int(rng.integers(100, 12000)))[0]))
    base = [c for _, c in cases]
    for i in range(240):
        c = bytearray(base[int(rng.integers(len(base)))])
        for _ in range(int(rng.integers(1, 3))):
            c[int(rng.integers(len(c)))] = int(rng.choice([0xF0, 0xF4, 0xF8, 0xFC, 0xFF, int(rng.integers(256))]))
        if rng.random() < 0.25:
            c = c[: int(rng.integers(1, len(c) + 1))]
        cases.append((f"mutated{i}", bytes(c)))
    return cases


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test run without a visible GPU")
    from gpu_harness import GpuCodec
    return GpuCodec()


@pytest.fixture(scope="module")
def oracle():
    return OracleCodec().o


@pytest.fixture(scope="module")
def batch(oracle):
    """(names, comps, caps, verdicts) of every case, valid and corrupt ones
    interleaved.  A slot has the header's length (64 bytes where the header
    is bad or claims more than 1 << 17)."""
    valid = long_literal_cases() + run_cases()
    bad = corrupt_cases() + fuzz_cases()
    cases = []
    for i in range(max(len(valid), len(bad))):
        cases += valid[i:i + 1] + bad[i:i + 1]
    names = [n for n, _ in cases]
    assert len(set(names)) == len(names)
    comps = [c for _, c in cases]
    caps = []
    for c in comps:
        h, ulen = oracle.header(c)
        caps.append(ulen if h and ulen <= 1 << 17 else 64)
    expect = oracle_verdicts(oracle, comps, caps)
    # the cases are what they claim to be
    ok = {n: e[0] for n, e in zip(names, expect)}
    for n, _ in long_literal_cases() + run_cases():
        assert ok[n] is True or n.endswith("-cut"), n
    for n, _ in corrupt_cases():
        assert ok[n] is False, n
    return names, comps, caps, expect


def plan_est_total_in(n: int, ws_bytes: int) -> int:
    """est_total_in of decode_v4_plan (csrc/decode_v4_plan.h): the batch's
    compressed bytes as the launch estimates them from the workspace size."""
    base_bytes = (4 * n + 255) & ~255
    chunk_bytes = (ws_bytes // 64) & ~255
    chunk_off = (ws_bytes - chunk_bytes) & ~255
    cap_words = min((chunk_off - 256 - 11 * base_bytes) // 4, 0x7FFFFFFF)
    return (cap_words - 4 * n - 64) * 32 if cap_words > 4 * n + 64 else 0


def decode_two_stream(gpu, comps, caps):
    """fsg_decompress_batch_2s (the lean walk on a second stream) with
    GpuCodec.decompress's layout: poisoned slots side by side, a 0xFF-filled
    workspace, the bytes outside the slots checked."""
    import torch
    from gpu_harness import Inputs, guarded_column, guarded_workspace, poisoned
    b = fsg.Batch.from_list(comps)
    n = len(b)
    caps = np.array(caps, dtype=np.uint32)
    lay = ct.aligned(caps.astype(np.uint64))
    ins = Inputs(d_in=b.data, d_in_off=b.offsets, d_in_len=b.lens, d_out_off=lay.offs, d_out_cap=caps)
    d_out = poisoned(lay.total)
    d_ol = guarded_column(n, torch.int32)
    d_st = guarded_column(n, torch.int32, -7)
    ws, whole = guarded_workspace(gpu.codec.lib.fsg_decompress_workspace_bytes(n, int(b.data.size)))
    ws.fill_(0xFF)
    s1 = torch.cuda.Stream()
    torch.cuda.synchronize()
    gpu.codec.decompress(ins["d_in"], ins["d_in_off"], ins["d_in_len"], n, d_out, ins["d_out_off"], ins["d_out_cap"],
                         d_ol, d_st, stream=torch.cuda.current_stream(), workspace=ws, pass1_stream=s1)
    torch.cuda.synchronize()
    rep = gpu.codec.decompress_report(ws, n)
    out = d_out.cpu().numpy()
    ct.check_outside(out, lay, caps, "d_out")
    ct.check_column(d_ol.cpu().numpy(), n, "d_out_len")
    ct.check_column(d_st.cpu().numpy(), n, "d_status")
    ct.check_workspace_guard(whole[-ct.WORKSPACE_GUARD:].cpu().numpy())
    ins.check()
    ol = d_ol.cpu().numpy()[:n].view(np.uint32)
    st = d_st.cpu().numpy()[:n]
    outs = [out[int(lay.offs[i]):int(lay.offs[i]) + int(min(ol[i], caps[i]))].tobytes() for i in range(n)]
    return outs, ol, st, rep


def check_walked(rep, comps):
    """The main path, nothing to the fallback, and pass 1b took no more than
    the bodies over the large-message threshold's floor."""
    assert rep["path"] == fsg.PATH_MAIN and rep["fallback_messages"] == 0, rep
    assert rep["large_messages"] + rep["huge_messages"] <= sum(len(c) > BIG_INDEX_MIN for c in comps), rep


@pytest.mark.parametrize("mode", ["serial", "standard", "planned", "lean"])
def test_lane_walk_cases(gpu, batch, fsg_opts, mode):
    """Every case on every instance of the lane walk, against the oracle."""
    names, comps, caps, expect = batch
    n = len(comps)
    assert n > 64
    if mode == "lean":
        assert fsg.get_option("lean_walk") == 1
        outs, ol, st, rep = decode_two_stream(gpu, comps, caps)
    else:
        fsg_opts(decode_fork=1 if mode == "planned" else 0)
        total_in = 20 * 1024 * n if mode == "standard" else sum(len(c) for c in comps)
        if mode != "planned":  # which one-stream walk the plan picks (est_total_in < 16384 n: serial)
            est = plan_est_total_in(n, gpu.codec.lib.fsg_decompress_workspace_bytes(n, total_in))
            assert (est < 16384 * n) == (mode == "serial"), (est, n)
        outs, ol, st = gpu.decompress(comps, caps, ws_fill=0xFF, ws_total_in=total_in)
        rep = gpu.last_report
    check_walked(rep, comps)
    try:
        n_ok, n_bad = check_against_oracle(expect, outs, ol, st)
    except AssertionError as e:
        wrong = e.args[0][1] if e.args and isinstance(e.args[0], tuple) else []
        raise AssertionError(f"{mode}: {[(names[i], s, w) for i, s, w in wrong]}") from e
    assert n_ok > 1500 and n_bad > 700, (n_ok, n_bad)


@pytest.mark.parametrize("fork", [0, 1])
@pytest.mark.parametrize("n", [63, 64, 65])
def test_corrupt_beside_valid(gpu, batch, fsg_opts, n, fork):
    """Batches of 63, 64 and 65 bodies (a partial wave, a whole one, one lane
    of a second; up to 64 bodies pass 1b indexes them, from 65 the lane walk),
    corrupt streams of every kind between valid ones: every valid neighbour's
    slot comes out whole, and nothing outside the slots is written."""
    names, comps, caps, expect = batch
    small = [i for i, c in enumerate(comps) if len(c) <= BIG_INDEX_MIN]
    bad = [i for i in small if expect[i][0] is False]
    good = [i for i in small if expect[i][0] is True]
    step_b, step_g = len(bad) // 32, len(good) // 33
    pick = []
    for k in range(33):
        pick.append(good[k * step_g + n % 7])
        if k < 32:
            pick.append(bad[k * step_b + n % 5])
    pick = pick[:n]
    fsg_opts(decode_fork=fork)
    outs, ol, st = gpu.decompress([comps[i] for i in pick], [caps[i] for i in pick], ws_fill=0xFF)
    n_ok, n_bad = check_against_oracle([expect[i] for i in pick], outs, ol, st)
    assert n_ok >= 31 and n_bad >= 31
