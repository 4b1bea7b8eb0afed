"""Generates tests/golden/lz4f_flags_vectors.json from the image's system
liblz4 (1.9.3, LZ4F_compressFrame through tests/lz4f_sys.py): the frame of
every input of tests/lz4f_flags_cases.py at block size ids 4 and 5 for the eight
combinations of content checksum, block checksums and no content size -- one
[frame length, frame FNV] row each.

  python tests/golden/make_lz4f_flags_golden.py

Checked while generating: liblz4 reads every frame back; the flags change
nothing but the descriptor's bits, the 8 size bytes and the checksum words (the
frame oracle with the flags applied gives liblz4's bytes); the raw-middle input
has a raw block at id 4."""
import json
import struct
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parent))
sys.path.insert(0, str(HERE.parents[1] / "flare-cpp_amd" / "py"))
sys.path.insert(0, str(HERE.parents[1] / "oracle"))
import lz4f_ref as R  # noqa: E402
from bind import Lz4Oracle  # noqa: E402
from lz4f_flags_cases import BSUM, CSUM, NOSIZE, fnv, inputs, keys  # noqa: E402
from lz4f_sys import SysLz4F, load  # noqa: E402


def oracle_frame(o, x: bytes, bid: int, flags: int) -> bytes:
    """The frame oracle's frame with the flags applied by hand."""
    size = len(x) if not flags & NOSIZE else None
    out = [R.header(size, R.frame_block_id(len(x), bid), bool(flags & CSUM), bsum=bool(flags & BSUM))]
    for b, raw in R.blocks_of(o, x, bid):
        out.append(struct.pack("<I", len(b) | (R.RAW if raw else 0)) + b)
        if flags & BSUM:
            out.append(struct.pack("<I", R.xxh32(b)))
    out.append(b"\0\0\0\0")
    if flags & CSUM:
        out.append(struct.pack("<I", R.xxh32(x)))
    return b"".join(out)


def main():
    L = load()
    if L is None:
        raise SystemExit("liblz4 with the frame API not found")
    z = SysLz4F(L)
    o = Lz4Oracle()
    xs = inputs()
    assert any(raw for _, raw in R.blocks_of(o, xs[-1], 4))
    rows = []
    for i, bid, fl in keys():
        x = xs[i]
        f = z.compress_frame(x, bid, bool(fl & CSUM), bsum=bool(fl & BSUM), size=not fl & NOSIZE)
        ok, y = z.decompress(f, len(x))
        assert ok and y == x, (i, bid, fl)
        assert f == oracle_frame(o, x, bid, fl), (i, bid, fl)
        rows.append([len(f), fnv(f)])
    text = [json.dumps(r, separators=(",", ":")) for r in rows]
    body = ",\n".join(",".join(text[k:k + 8]) for k in range(0, len(text), 8))
    (HERE / "lz4f_flags_vectors.json").write_text('{"liblz4_version":%d,\n"frames":[\n%s\n]}\n' % (z.version, body))
    print(len(rows), "frames")


if __name__ == "__main__":
    main()
