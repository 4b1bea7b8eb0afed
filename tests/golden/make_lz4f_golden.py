"""Generates tests/golden/lz4f_vectors.json from the image's system liblz4
(1.9.3, lz4frame.h: LZ4F_compressFrame, LZ4F_compressBegin / Update / flush /
End, LZ4F_decompress) -- the pin of the LZ4 frame path.

  python tests/golden/make_lz4f_golden.py

The inputs are recipes in tests/lz4f_cases.py; the file holds short rows
(lz4f_cases.load gives them names) and hex only for the foreign frames.

* compress: [frame length, frame FNV, blocks, raw blocks] of liblz4's frame
  (independent blocks, contentSize, level 0, no block checksums) per input of
  lz4f_cases.compress_inputs, without and with a content checksum.
* decode_ok: frames the compressor here never writes -- linked blocks, no
  content size, block checksums, short non-final blocks, a raw and a
  compressed block in one frame.
* decode: [source, checksum flags, byte changes, cut, liblz4's verdict, the
  frame oracle's status, its length, output FNV] of 1,500 mutated frames.
"""
import json
import random
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parent))
sys.path.insert(0, str(HERE.parents[1] / "flare-cpp_amd" / "py"))
sys.path.insert(0, str(HERE.parents[1] / "oracle"))
import lz4f_ref  # noqa: E402
from bind import Lz4Oracle  # noqa: E402
from lz4f_cases import DECODE_SOURCES, base_frame, build, compress_inputs, fnv, mutate  # noqa: E402
from lz4f_sys import LINKED, SysLz4F, load  # noqa: E402


def rows(items, per_line):
    """JSON rows, `per_line` to a line."""
    text = [json.dumps(r, separators=(",", ":")) for r in items]
    return "[\n" + ",\n".join(",".join(text[i:i + per_line]) for i in range(0, len(text), per_line)) + "\n]"


def main():
    L = load()
    if L is None:
        raise SystemExit("liblz4 with the frame API not found")
    z = SysLz4F(L)
    o = Lz4Oracle()
    compress, differs = [], []
    for spec, bid in compress_inputs():
        x = build(spec)
        blocks = lz4f_ref.blocks_of(o, x, bid)
        for checksum in (False, True):
            f = z.compress_frame(x, bid, checksum)
            ok, y = z.decompress(f, len(x))
            assert ok and y == x
            assert len(f) <= lz4f_ref.max_frame_length(len(x), bid) <= z.bound(len(x), bid)
            if not checksum and lz4f_ref.compress_frame(o, x, bid) != f:
                # both frames are valid; liblz4 chose raw or compressed otherwise than the size rule
                differs += [len(compress), len(compress) + 1]
            compress.append([len(f), fnv(f), len(blocks), sum(r for _, r in blocks)])
    base = build({"gen": "text", "seed": 21, "size": 4000})
    x = (base * 18)[:70000]
    rnd = build({"gen": "random", "seed": 22, "size": 600})
    decode_ok = []

    def foreign(name, f, want, route):
        ok, y = z.decompress(f, len(want))
        assert ok and y == want, name
        st, ln, y2 = lz4f_ref.decode_frame(o, f, len(want))
        assert st == 0 and y2 == want, name
        decode_ok.append({"name": name, "route": route, "hex": f.hex(), "out_len": len(want), "out_fnv": fnv(want)})

    foreign("linked", z.compress_frame(x, 4, mode=LINKED), x, "serial_linked")
    foreign("linked_checksums_no_size", z.compress_frame(x, 4, mode=LINKED, checksum=True, bsum=True, size=False), x,
            "serial_linked")
    foreign("no_content_size", z.compress_frame(x[:20000], 4, size=False), x[:20000], "serial_no_size")
    foreign("block_checksums", z.compress_frame(x, 4, bsum=True, checksum=True), x, "fast")
    foreign("block_checksums_id5", z.compress_frame(x + x, 5, bsum=True), x + x, "fast")
    foreign("short_blocks", z.compress_pieces([x[:3000], x[3000:5000], x[5000:7000]], size=7000), x[:7000],
            "serial_rejected")
    foreign("raw_and_compressed", z.compress_pieces([rnd, x[:3000]], size=3600), rnd + x[:3000], "serial_rejected")

    rng = random.Random(77)
    decode, only = [], []
    for i in range(1500):
        case = {"src": rng.randrange(len(DECODE_SOURCES)), "csum": i & 1, "bsum": (i >> 1) & 1}
        x = build(DECODE_SOURCES[case["src"]])
        frame = base_frame(o, case)
        assert frame == z.compress_frame(x, 4, bool(case["csum"]), bsum=bool(case["bsum"]))
        case["set"] = [[rng.randrange(min(len(frame), 24)) if rng.random() < 0.4 else rng.randrange(len(frame)),
                        rng.randrange(256)] for _ in range(rng.randint(1, 2))]
        case["cut"] = rng.randint(1, len(frame)) if rng.random() < 0.3 else None
        f = mutate(frame, case)
        ok, y = z.decompress(f, len(x))
        st, ln, y2 = lz4f_ref.decode_frame(o, f, len(x))
        assert (st, ln, y2) == lz4f_ref.decode_frame(None, f, len(x)), i
        if st == 0:
            assert ok and y == y2, i  # the one-way relation
        elif ok:
            only.append(i)
        decode.append([case["src"], case["csum"] | case["bsum"] << 1, [v for s in case["set"] for v in s],
                       -1 if case["cut"] is None else case["cut"], int(ok), st, ln, fnv(y2) if st == 0 else ""])
    assert len(only) * 100 <= len(decode)
    (HERE / "lz4f_vectors.json").write_text(
        '{"liblz4_version":%d,\n"differs_from_size_rule":%s,"liblz4_only":%s,\n"compress":%s,\n"decode_ok":%s,\n'
        '"decode":%s}\n' % (z.version, json.dumps(differs), json.dumps(only), rows(compress, 8), rows(decode_ok, 1),
                            rows(decode, 6)))
    print(len(compress), "compress rows,", len(decode_ok), "foreign frames,", len(decode), "mutated frames:",
          sum(d[4] for d in decode), "accepted by liblz4,", sum(d[5] == 0 for d in decode), "by the oracle,",
          len(only), "by liblz4 alone,", len(differs) // 2, "inputs stored otherwise than the size rule")


if __name__ == "__main__":
    main()
