"""Generates tests/golden/lz4f_linked_vectors.json from the image's system
liblz4 (1.9.3, lz4frame.h) with blockMode = LZ4F_blockLinked: the frames a
liblz4 peer sends when it leaves the preferences alone.

  python tests/golden/make_lz4f_linked_golden.py

Each entry: the frame as hex, its input as a recipe (tests/lz4f_linked_cases.
fixture_input), and liblz4's own decode result as length and FNV.
"""
import json
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parent))
sys.path.insert(0, str(HERE.parents[1] / "flare-cpp_amd" / "py"))
sys.path.insert(0, str(HERE.parents[1] / "oracle"))
import lz4f_ref  # noqa: E402
from lz4f_cases import fnv  # noqa: E402
from lz4f_linked_cases import fixture_input  # noqa: E402
from lz4f_sys import LINKED, SysLz4F, load  # noqa: E402


def main():
    L = load()
    if L is None:
        raise SystemExit("liblz4 with the frame API not found")
    z = SysLz4F(L)
    frames = []

    def add(name, spec, f):
        x = fixture_input(spec)
        ok, y = z.decompress(f, len(x))
        assert ok and y == x, name
        assert not f[4] & lz4f_ref.F_INDEP, name
        assert lz4f_ref.decode_frame(None, f, len(x)) == (0, len(x), x), name
        frames.append({"name": name, "input": spec, "hex": f.hex(), "out_len": len(y), "out_fnv": fnv(y)})

    # (every input is a text's first `period` bytes over and over: what follows the first period is long copies
    # from 4,000 to 10,000 bytes back, most of them into an earlier block, and the hex stays small)
    for n, period in ((65537, 4000), (131073, 6000), (200000, 4000)):
        spec = {"gen": "text_repeated", "seed": 60 + n % 7, "size": n, "period": period}
        add(f"sized_{n}", spec, z.compress_frame(fixture_input(spec), 4, mode=LINKED))
    spec = {"gen": "text_repeated", "seed": 64, "size": 200000, "period": 4000}
    add("no_size_checksums", spec,
        z.compress_frame(fixture_input(spec), 4, mode=LINKED, checksum=True, bsum=True, size=False))
    spec = {"gen": "text_repeated", "seed": 65, "size": 300000, "period": 4000}
    add("id5_300000", spec, z.compress_frame(fixture_input(spec), 5, mode=LINKED))
    spec = {"gen": "text_repeated", "seed": 66, "size": 90000, "period": 10000}
    x = fixture_input(spec)
    add("pieces", spec, z.compress_pieces([x[i:i + 3000] for i in range(0, 90000, 3000)], 4, mode=LINKED))
    spec = {"gen": "text_random_middle", "seed": 67, "size": 90000, "at": 45000, "piece": 3000, "period": 5000}
    x = fixture_input(spec)
    add("pieces_raw_middle", spec, z.compress_pieces([x[i:i + 3000] for i in range(0, 90000, 3000)], 4, mode=LINKED))
    text = '{"liblz4_version":%d,\n"frames":[\n%s\n]}\n' % (
        z.version, ",\n".join(json.dumps(e, separators=(",", ":")) for e in frames))
    assert len(text) < 100000, len(text)
    (HERE / "lz4f_linked_vectors.json").write_text(text)
    print(len(frames), "frames,", len(text), "bytes")


if __name__ == "__main__":
    main()
