"""CPU tests for LZ4 frames with linked blocks: the case set of
tests/lz4f_linked_cases.py and liblz4's own frames
(tests/golden/lz4f_linked_vectors.json) against the frame oracle, the host
codec and, where it is installed, liblz4; what the case set contains, by the
sequence walker; the negative and the mutated cases' composition; the path
report's two new fields and option lz4f_linked_fast; and lz4f::linked_prefix
under AddressSanitizer and UBSan in a stand-alone program
(tests/cpp/lz4f_linked_check.cc)."""
import ctypes
import json
import shutil
import struct
import subprocess
from pathlib import Path

import pytest

import fsg
import lz4f_linked_cases as C
import lz4f_ref as R
import lz4f_sys
from lz4f_cases import fnv

REPO = Path(__file__).resolve().parent.parent
_HOST_ST = {1: R.OK, 0: R.CORRUPT, -1: R.BAD_HEADER, -2: R.SLOT_TOO_SMALL}


@pytest.fixture(scope="module")
def host():
    lib = REPO / "flare-cpp_amd" / "lib" / "libflare_rpc_snappy.so"
    if not lib.exists():
        subprocess.run(["make", "-C", str(REPO), "host"], check=True, capture_output=True)
    L = ctypes.CDLL(str(lib))
    L.fsh_cpu_lz4f_uncompress.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t,
                                          ctypes.POINTER(ctypes.c_uint32)]
    return L


def host_uncompress(L, f: bytes, cap: int):
    out = ctypes.create_string_buffer(max(cap, 1))
    ln = ctypes.c_uint32(0)
    r = L.fsh_cpu_lz4f_uncompress(ctypes.create_string_buffer(f, max(len(f), 1)), len(f), out, cap, ctypes.byref(ln))
    return _HOST_ST[r], ln.value, (out.raw[:ln.value] if r == 1 else None)


def test_every_frame_decodes_to_its_input(host):
    items = C.all_frames()
    assert len(C.fixture()) == 7 and len(items) >= 18
    for name, x, f, nb in items:
        st, hl, bmax, flg, size = R.parse_header(f)
        assert st == R.OK and not flg & R.F_INDEP, name
        assert R.decode_frame(None, f, len(x)) == (R.OK, len(x), x), name
        assert host_uncompress(host, f, len(x)) == (R.OK, len(x), x), name
        assert len(C.blocks_in(f)[2]) == nb, name
    v = {e["name"]: e for e in json.loads(C.GOLDEN.read_text())["frames"]}
    for name, x, f, nb in C.fixture():
        assert fnv(x) == v[name]["out_fnv"], name
    # what liblz4 writes: FLG 0x48 with a content size, 0x40 without (no B.Indep bit), 64 KiB blocks at id 4
    flg = {n: f[4] for n, _, f, _ in C.fixture()}
    assert flg["sized_200000"] == 0x48 and flg["pieces"] == 0x40
    assert {n: nb for n, _, _, nb in C.fixture()} == {"sized_65537": 2, "sized_131073": 3, "sized_200000": 4,
                                                      "no_size_checksums": 4, "id5_300000": 2, "pieces": 30,
                                                      "pieces_raw_middle": 30}


def test_every_frame_decodes_under_liblz4():
    L = lz4f_sys.load()
    if L is None:
        pytest.skip("no system liblz4")
    z = lz4f_sys.SysLz4F(L)
    for name, x, f, nb in C.all_frames():
        assert z.decompress(f, len(x)) == (True, x), name


def test_case_set_contains_what_the_kernels_can_get_wrong():
    seen = {k: [] for k in C.KINDS}
    firsts = 0
    for name, x, f, nb in C.all_frames():
        for m in C.matches(f):
            for k in C.kinds(m):
                seen[k].append(name)
        if name == "pieces":
            firsts = len({m["k"] for m in C.matches(f) if m["first"] and m["lit"] == 0})
    for k in C.KINDS:
        assert seen[k], k
    # liblz4's own frames reach into history too, and begin blocks without literals
    assert any(n.startswith("sized_") for n in seen["history_only"])
    assert firsts >= 5, firsts
    # raw history and history over three short blocks come from a greedy frame as well as the hand-built one
    assert set(seen["raw_history"]) - {"hand", "hand_sums"} and set(seen["three_blocks_back"]) - {"hand", "hand_sums"}


def test_negative_cases_are_corrupt():
    neg = C.negatives()
    assert [n for n, _, _ in neg] == ["beyond_at_block_1", "beyond_at_block_3", "second_block_alone"]
    for name, f, cap in neg:
        assert R.parse_header(f)[0] == R.OK
        assert R.decode_frame(None, f, cap) == (R.CORRUPT, 0, None), name


def test_mutated_set_composition():
    """The counts the GPU test relies on, by the oracle alone, at exact capacity."""
    frames, caps = C.mutated()
    assert len(frames) == C.MUT_COUNT == 200
    sizes = [R.parse_header(f)[4] for _, f in C.mutation_bases()]
    assert [len(x) for x, _ in C.mutation_bases()][0] == 65536 + 3000
    assert sizes[0] == 68536 and sizes[1:] == [R.NO_SIZE] * 3
    accepted = rejected = 0
    for f, c in zip(frames, caps):
        if R.parse_header(f)[0] != R.OK:
            continue
        if R.decode_frame(None, f, c)[0] == R.OK:
            accepted += 1
        else:
            rejected += 1
    assert accepted >= 10 and rejected >= 50, (accepted, rejected)


def test_report_has_the_linked_counters():
    """fsg_lz4f_decompress_report on a hand-made header copy: counters 16 and
    17 are the new fields, and the old fields read what they read before."""
    lib = fsg.load_gpu_lib()
    ctr = list(range(100, 164))
    head = ctypes.create_string_buffer(struct.pack("<64I", *ctr), 256)
    ws = lib.fsg_lz4f_decompress_workspace_bytes(3, 1000)
    rep = fsg.Lz4fDecodeReport()
    assert lib.fsg_lz4f_decompress_report(head, 3, ws, ctypes.byref(rep)) == 0
    got = {f: int(getattr(rep, f)) for f, _ in rep._fields_}
    entries = got.pop("block_entries")
    assert entries >= 3
    assert got == {"fast_messages": 101, "fast_blocks": 102, "empty_messages": 103, "serial_linked": 104,
                   "serial_no_size": 105, "serial_rejected": 106, "serial_forced": 107, "checksummed_units": 108,
                   "inner_fallback_blocks": 109, "fast_nosize_messages": 112, "fast_nosize_blocks": 113,
                   "fast_linked_messages": 116, "fast_linked_blocks": 117}
    assert [f for f, _ in rep._fields_][-2:] == ["fast_linked_messages", "fast_linked_blocks"]


def test_option_is_known_and_off_by_default():
    saved = fsg.get_option("lz4f_linked_fast")
    try:
        import os
        if "FSG_L4F_LINKED_FAST" not in os.environ:
            assert saved == 0
        fsg.set_option("lz4f_linked_fast", 1)
        assert fsg.get_option("lz4f_linked_fast") == 1
    finally:
        fsg.set_option("lz4f_linked_fast", saved)


def test_linked_prefix_sanitized(tmp_path):
    """lz4f::linked_prefix in a stand-alone program under AddressSanitizer and
    UBSan, over every block of the case set and the values around the limit."""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("g++ not available")
    exe = tmp_path / "lz4f_linked_check"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I", str(REPO / "flare-cpp_amd" / "csrc"), str(REPO / "tests" / "cpp" / "lz4f_linked_check.cc"),
                        "-o", str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    values = [p for _, _, f, _ in C.all_frames() for p in C.block_prefixes(f)]
    values += [0, 1, 65534, 65535, 65536, (1 << 32) - 1, 1 << 32, (1 << 32) + 7, (1 << 64) - 1]
    assert max(values[:-9]) > 65535 and 0 < min(v for v in values[:-9] if v) < 100
    fin, fout = tmp_path / "p.in", tmp_path / "p.out"
    fin.write_bytes(struct.pack("<%dQ" % len(values), *values))
    r = subprocess.run([str(exe), str(fin), str(fout)], capture_output=True, text=True, timeout=300,
                       env={"ASAN_OPTIONS": "detect_leaks=0"})
    assert r.returncode == 0, r.stderr[-3000:]
    got = struct.unpack("<%dI" % len(values), fout.read_bytes())
    assert list(got) == [C.prefix(v) for v in values]
