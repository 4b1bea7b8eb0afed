"""Compression levels of the deflate writer on the CPU
(include/flare_deflate_level_gpu.h; csrc/deflate_format.h, "levels"): the host
model at levels 0 and 2 judged by Python's zlib on the family of
tests/deflate_cases.py, level 1 through the level-taking entry against the
level-less one, the stored-only bodies of level 0, the match limits from
level 2's tokens, the constructed bodies that tell the two-candidate table,
the insert rule and the lazy step from level 1's parse, the size conditions,
the model and a 64-lane emulation of the level-2 window step under
AddressSanitizer and UBSan in a stand-alone program, the new symbol and its
argument checks, and GzipCompress with GzipCompressOptions."""
import shutil
import struct
import subprocess
import zlib
from pathlib import Path

import pytest

import deflate_cases as C
import deflate_level_cases as V
import deflate_streams as D
import fsg

REPO = Path(__file__).resolve().parents[1]
FORMATS = [C.RAW, C.ZLIB, C.GZIP]


def zlib_inflate(fmt, body):
    d = zlib.decompressobj(C.WBITS[fmt])
    out = d.decompress(body)
    assert d.eof and not d.unused_data and not d.unconsumed_tail
    return out


def bodies():
    return list(C.cases()) + list(V.constructed())


@pytest.mark.parametrize("level", [V.STORED, V.BEST])
@pytest.mark.parametrize("fmt", FORMATS)
def test_family_is_read_by_zlib_and_by_the_host_inflate(fmt, level):
    import ctypes
    L = V.host()
    for name, x in bodies():
        body = V.model(fmt, level, x)
        assert zlib_inflate(fmt, body) == x, name
        out = ctypes.create_string_buffer(len(x) + 1)
        ln = ctypes.c_uint64()
        assert L.fsh_cpu_inflate(fmt, body, len(body), out, len(x), ctypes.byref(ln)) == D.OK, name
        assert ln.value == len(x) and out.raw[:len(x)] == x, name
        bound = L.fsh_cpu_deflate_bound(len(x), fmt)
        assert bound == C.bound(len(x), fmt) and len(body) <= bound, name
        n = len(body)
        st, ln, buf = V.deflate_into(fmt, level, x, bound)  # a second run: equal bytes, nothing past the length
        assert (st, ln) == (D.OK, n) and buf[:n] == body and buf[n:] == b"\xa5" * (bound - n), name
        assert V.deflate_into(fmt, level, x, n) == (D.OK, n, body), name  # exactly the length is enough
        st, ln, buf = V.deflate_into(fmt, level, x, n - 1)  # one byte short: refused, nothing written
        assert (st, ln) == (D.SLOT_TOO_SMALL, 0) and buf == b"\xa5" * (n - 1), name


def test_level_1_is_the_level_less_model_and_unknown_levels_are_refused():
    for name, x in bodies():
        for fmt in FORMATS:
            assert V.model(fmt, V.FAST, x) == C.model(fmt, x), name
        if len(x) <= C.U:
            assert V.tokens(V.FAST, x) == C.tokens(x), name
        assert V.unit_types(V.FAST, x) == C.unit_types(x), name
    for level in (3, 9, 0xFFFFFFFF):
        assert V.deflate_into(C.ZLIB, level, b"abc", 64)[:2] == (D.CORRUPT, 0)
        assert V.unit_types(level, b"abc") == (0, 0, 0)
    assert V.deflate_into(3, V.BEST, b"abc", 64)[:2] == (D.CORRUPT, 0)


def stored_blocks(raw, n):
    """Walks a raw deflate stream of stored blocks only: their lengths; the last one alone has BFINAL."""
    lens, at = [], 0
    while True:
        head, ln, nln = raw[at], int.from_bytes(raw[at + 1:at + 3], "little"), int.from_bytes(raw[at + 3:at + 5], "little")
        assert head in (0, 1) and ln ^ nln == 0xFFFF, (at, head)
        lens.append(ln)
        at += 5 + ln
        if head == 1:
            break
    assert at == len(raw) and sum(lens) == n
    return lens


def test_level_0_is_stored_units_and_exactly_the_bound():
    for name, x in bodies():
        units = max(1, -(-len(x) // C.U))
        for fmt in FORMATS:
            body = V.model(fmt, V.STORED, x)
            assert len(body) == C.bound(len(x), fmt), name
        raw = V.model(C.RAW, V.STORED, x)
        lens = stored_blocks(raw, len(x))
        assert lens == [C.U] * (units - 1) + [len(x) - C.U * (units - 1)], name
        assert V.unit_types(V.STORED, x) == (units, 0, 0), name
    import ctypes
    buf = (ctypes.c_uint32 * 16)()
    assert V.host().fsh_cpu_deflate_tokens_level(V.STORED, b"abcdabcdabcd", 12, buf, 16) == 0  # no parse at level 0


def test_match_limits_from_the_level_2_tokens():
    def matches(data):
        toks = V.tokens(V.BEST, data)
        assert sum(1 if t[0] == "lit" else t[1] for t in toks) == len(data)
        # none below the unit's first byte
        at = 0
        for t in toks:
            assert t[0] == "lit" or (4 <= t[1] <= 258 and 1 <= t[2] <= min(at, 32768)), (at, t)
            at += 1 if t[0] == "lit" else t[1]
        return [t for t in toks if t[0] == "match"]
    for r in (257, 258, 259, 260, 516, 517):
        for pre in (b"", b"xyz"):
            ms = matches(pre + b"z" * r)
            assert ms and all(4 <= m[1] <= 258 and 1 <= m[2] <= 128 for m in ms), (r, pre)
    assert max(m[1] for m in matches(b"z" * 517)) == 258
    for d in (64, 65, 32767, 32768):
        assert any(m[2] == d and m[1] >= 90 for m in matches(C.repeat_at(d))), d
    assert not any(m[2] > 128 for m in matches(C.repeat_at(32769)))  # the zeros match near by, the string does not
    for d in (1, 3, 4, 63, 64, 65, 32767, 32768, 32769):
        assert all(1 <= m[2] <= 32768 for m in matches(C.repeat_at(d)))
    for name, x in C.cases():
        if len(x) <= C.U:
            matches(x)
    assert matches(C.by_name("literals_only")) == [] and matches(C.by_name("all_256_once")) == []
    assert matches(C.by_name("one_distance")) == [("match", 10, 64)]
    # straddle: the repeat is found inside unit 2 only, and unit 2's bytes are those of its input alone
    x = C.straddle()
    raw = V.model(C.RAW, V.BEST, x)
    assert raw.endswith(V.model(C.RAW, V.BEST, x[C.U:])) and zlib_inflate(C.RAW, raw) == x
    assert any(m[2] == 200 for m in matches(x[C.U:]))


def test_two_candidates():
    x = V.two_candidates()
    assert x[V.S_AT:V.S_AT + 100] == x[V.S_AGAIN:V.S_AGAIN + 100] and x[V.T_AT:V.T_AT + 4] == x[:4]
    assert x[V.T_AT + 4] != x[4]
    assert V.token_starting_at(V.tokens(V.FAST, x), V.S_AGAIN) == ("match", 4, V.S_AGAIN - V.T_AT)
    assert V.token_starting_at(V.tokens(V.BEST, x), V.S_AGAIN) == ("match", 100, V.S_AGAIN - V.S_AT)


def test_insert_keeps_the_highest_position_of_a_window():
    x = V.insert_same_window()
    at = V.SAME_WINDOW_AT
    assert x[at:at + 12] == x[:12] and x[20:24] == x[:4] and x[24] != x[4]
    toks = V.tokens(V.BEST, x)
    assert V.token_starting_at(toks, at) == ("match", 4, at - 20)   # position 0 is no candidate
    assert V.token_starting_at(toks, 20) == ("lit", x[20])           # nor was it one inside its own window


def test_insert_drops_the_older_candidate():
    x = V.insert_three_windows()
    at = V.THREE_WINDOWS_AT
    assert x[at:at + 24] == x[:24] and x[64:68] == x[128:132] == x[:4]
    toks = V.tokens(V.BEST, x)
    assert V.token_starting_at(toks, 64) == ("match", 4, 64) and V.token_starting_at(toks, 128) == ("match", 4, 64)
    assert V.token_starting_at(toks, at) == ("match", 4, at - 128)   # 128 and 64 tie: the nearer; 0 is gone


@pytest.mark.parametrize("name", list(V.LAZY))
def test_lazy_step(name):
    at, succ = V.LAZY[name]
    x = V.constructed_by_name(name)
    fast, best = V.tokens(V.FAST, x), V.tokens(V.BEST, x)
    assert V.token_starting_at(fast, at) == ("match", 4, at)
    if name in ("lazy_lanes_0_1", "lazy_lanes_62_63"):  # deferred: a literal, then the 9-byte match
        assert at % 64 in (0, 62)
        assert V.token_starting_at(best, at) == ("lit", ord("a"))
        assert V.token_starting_at(best, at + 1) == ("match", 9, at + 1 - V.Q_AT)
    elif name == "lazy_lanes_63_64":  # the successor lies in the next window: not deferred
        assert at % 64 == 63
        assert V.token_starting_at(best, at) == ("match", 4, at) and V.token_starting_at(best, at + 1) is None
        assert best == fast
    else:  # the successor's match is 4 bytes too: not deferred
        assert succ == 4 and at % 64 < 63
        assert V.token_starting_at(best, at) == ("match", 4, at) and V.token_starting_at(best, at + 1) is None


def test_size_conditions():
    """Level 2 below 0.97 x level 1 and at most 1.01 x zlib level 1 (the
    rule's prototype: 0.951 / 0.948 and 0.979 / 0.998; bytes 26,042 and
    108,752)."""
    for n, want in ((70000, 26042), (300000, 108752)):
        x = D.text(n, 1)
        l1, l2 = len(V.model(C.ZLIB, V.FAST, x)), len(V.model(C.ZLIB, V.BEST, x))
        z1, z6 = len(zlib.compress(x, 1)), len(zlib.compress(x, 6))
        print(f"text({n}, 1): level 1 {l1}, level 2 {l2}, zlib level 1 {z1}, zlib level 6 {z6}; "
              f"{l2 / l1:.4f} x level 1, {l2 / z1:.4f} x zlib 1")
        assert l2 < 0.97 * l1, (n, l1, l2)
        assert l2 <= 1.01 * z1, (n, l2, z1)
        assert l2 == want, (n, l2)  # the model is deterministic: the rule's own figure


EMULATED = {"text_129", "text_65473", "repeat_at_63", "repeat_at_64", "repeat_at_65", "xyz_run_517"}


def test_host_model_and_level_2_lanes_sanitized(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = tmp_path / "deflate_level_check"
    host = REPO / "flare-cpp_amd" / "host"
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", str(host), str(REPO / "tests" / "cpp" / "deflate_level_check.cc"),
                        str(host / "deflate_cpu.cc"), str(host / "inflate_cpu.cc"), "-o", str(exe)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    emulated = EMULATED | {name for name, _ in V.constructed()}
    assert emulated <= {name for name, _ in bodies()}
    rec = windows = 0
    with open(tmp_path / "vectors.bin", "wb") as f:
        for name, x in bodies():
            for fmt in FORMATS:
                for level in (V.STORED, V.BEST):
                    body = V.model(fmt, level, x)
                    lanes = name in emulated and fmt == C.RAW and level == V.BEST
                    f.write(struct.pack("<5I", fmt, level, len(x), len(body), 2 if lanes else 0) + x + body)
                    rec += 1
                    if lanes:
                        units = max(1, -(-len(x) // C.U))
                        windows += sum(-(-min(C.U, len(x) - u * C.U) // 64) for u in range(units))
    r = subprocess.run([str(exe), str(tmp_path / "vectors.bin")], capture_output=True, text=True, timeout=900,
                       env={"ASAN_OPTIONS": "detect_leaks=0"})
    assert r.returncode == 0 and r.stdout.strip() == f"ok {rec} {windows}", r.stdout[-2000:] + r.stderr[-3000:]


# ---- the public header and the argument checks, no GPU

def test_new_symbol_exported_and_declared():
    inc = REPO / "include"
    assert fsg.header_symbols(inc / "flare_deflate_level_gpu.h") == ["fsg_deflate_batch_level"]
    assert fsg.header_symbols(inc / "flare_deflate_compress_gpu.h") == [
        "fsg_deflate_batch", "fsg_deflate_max_length", "fsg_deflate_report", "fsg_deflate_workspace_bytes"]
    assert fsg.header_symbols(inc / "flare_deflate_gpu.h") == [
        "fsg_adler32_batch", "fsg_crc32_batch", "fsg_inflate_batch", "fsg_inflate_lengths_batch"]
    lib = fsg.load_gpu_lib()
    assert hasattr(lib, "fsg_deflate_batch_level") and "fsg_deflate_batch_level" in fsg.header_symbols()
    assert "fsg_deflate_batch_level" in fsg._SIGS
    assert (fsg.DEFLATE_LEVEL_STORED, fsg.DEFLATE_LEVEL_FAST, fsg.DEFLATE_LEVEL_BEST) == (0, 1, 2)
    text = (inc / "flare_deflate_level_gpu.h").read_text()
    for name, value in (("STORED", 0), ("FAST", 1), ("BEST", 2)):
        assert f"#define FSG_DEFLATE_LEVEL_{name} {value}u" in text
    import inspect
    assert inspect.signature(fsg.SnappyGPU.deflate).parameters["level"].default is None


def test_invalid_arguments_rejected_without_gpu():
    lib = fsg.load_gpu_lib()
    one = 16  # any non-null, aligned value: rejected before it is looked at
    big = 1 << 40
    call = lib.fsg_deflate_batch_level
    need = lib.fsg_deflate_workspace_bytes(5, 0)
    for level in (3, 0xFFFFFFFF):  # an unknown level, whatever the other arguments
        assert call(one, one, one, 5, one, one, one, one, C.ZLIB, level, one, big, None) == -1
        assert call(None, None, None, 0, None, None, None, None, C.ZLIB, level, None, 0, None) == -1
        assert call(None, None, None, 5, None, None, None, None, 7, level, None, 0, None) == -1
    for level in V.LEVELS:
        assert call(None, None, None, 5, None, None, None, None, C.ZLIB, level, None, 0, None) == -1
        for hole in range(7):  # each NULL column
            a = [one] * 7
            a[hole] = None
            a.insert(3, 5)
            assert call(*a, C.ZLIB, level, one, big, None) == -1, (level, hole)
        for fmt in (3, 7, 0xFFFFFFFF):
            assert call(one, one, one, 5, one, one, one, one, fmt, level, one, big, None) == -1
            assert call(None, None, None, 0, None, None, None, None, fmt, level, None, 0, None) == -1
        assert call(one, one, one, 5, one, one, one, one, C.GZIP, level, one, need - 1, None) == -1  # one byte too small
        assert call(one, one, one, 5, one, one, one, one, C.GZIP, level, None, need, None) == -1     # no workspace
        assert call(one, one, one, 5, one, one, one, one, C.GZIP, level, one + 4, need, None) == -1  # misaligned
        assert call(None, None, None, 0, None, None, None, None, C.RAW, level, None, 0, None) == 0   # an empty batch


# ---- GzipCompress with GzipCompressOptions (host/gzip_compress.h)

def test_gzip_options_map_onto_the_levels(tmp_path):
    """tests/cpp/test_gzip_options.cc: compression_level 0, 1, 6 and -1 in both
    formats; Python's zlib reads every body, and the bytes are the model's for
    the mapped level (0 -> 0, 1 -> 1, 6 and -1 -> 2)."""
    subprocess.run(["make", "-C", str(REPO), "build/test_gzip_options"], check=True, capture_output=True, timeout=600)
    x = D.text(100000, 5)
    fin = tmp_path / "raw.in"
    fin.write_bytes(x)
    r = subprocess.run([str(REPO / "build" / "test_gzip_options"), str(fin), str(tmp_path)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "0 failures" in r.stdout, r.stdout + r.stderr
    for fname, fmt in (("gzip", C.GZIP), ("zlib", C.ZLIB)):
        for tag, level in (("0", V.STORED), ("1", V.FAST), ("6", V.BEST), ("m1", V.BEST)):
            body = (tmp_path / f"{fname}_{tag}.bin").read_bytes()
            assert zlib_inflate(fmt, body) == x, (fname, tag)
            assert body == V.model(fmt, level, x), (fname, tag)
