// lz4f_flags_check.cc -- the shared frame writer (csrc/lz4_frame_format.h:
// write_header, write_block, write_end, max_frame_length with flags) through
// the host codec's CompressFrame, for every combination of the compress flags,
// as a stand-alone program to run under AddressSanitizer and UBSan:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined
//       -Iflare-cpp_amd/host tests/cpp/lz4f_flags_check.cc flare-cpp_amd/host/lz4_cpu.cc -o lz4f_flags_check
//
// Every frame is written into a heap buffer of exactly MaxFrameLength(n, id,
// flags) bytes, so a write past the bound is a sanitizer report; every length
// must be within the bound, the descriptor must carry the flags' bits, the
// frame must decode to the input, and the longest frame of each combination
// -- incompressible bytes, every block raw -- must be the bound less the
// fields the combination leaves out and the bound does not follow (8 without
// a content size, 4 without a content checksum): with a content checksum and
// a size the bound is reached exactly, with block checksums (flags 3) and
// without (flags 1), so both bounds are tight.  Prints "ok <frames>" and
// returns 0, or says what failed.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../flare-cpp_amd/csrc/lz4_frame_format.h"
#include "lz4_cpu.h"

namespace cpu = flare::lz4::cpu;

static int failures = 0;
#define CHECK(c, ...)                 \
  do {                                \
    if (!(c)) {                       \
      std::printf("FAIL %s: ", #c);   \
      std::printf(__VA_ARGS__);       \
      std::printf("\n");              \
      ++failures;                     \
    }                                 \
  } while (0)

static std::vector<uint8_t> make_input(size_t n, int kind) {
  std::vector<uint8_t> x(n);
  uint64_t s = 0x9E3779B97F4A7C15ull + n * 31 + kind;
  for (size_t i = 0; i < n; ++i) {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    const uint8_t r = static_cast<uint8_t>(s >> 56);
    // 0: incompressible; 1: a short alphabet; 2: incompressible first half, zeros after
    x[i] = kind == 0 ? r : kind == 1 ? static_cast<uint8_t>('a' + (r & 3)) : (i < n / 2 ? r : 0);
  }
  return x;
}

int main() {
  const size_t lengths[] = {0, 1, 15, 16, 17, 4095, 65535, 65536, 65537, 200000, 262144, 262145, 1100000};
  size_t frames = 0;
  for (int id = 4; id <= 7; ++id) {
    for (uint32_t flags = 0; flags < 8; ++flags) {
      for (int kind = 0; kind < 3; ++kind) {
        for (size_t n : lengths) {
          const std::vector<uint8_t> x = make_input(n, kind);
          const size_t bound = cpu::MaxFrameLength(n, id, flags);
          const size_t bs = lz4f::block_bytes(id);
          const size_t nb = (n + bs - 1) / bs;
          CHECK(bound == cpu::MaxFrameLength(n, id) + ((flags & cpu::kFrameBlockChecksums) ? 4 * nb : 0), "n %zu", n);
          uint8_t* out = new uint8_t[bound];  // exactly the bound: ASan sees a byte past it
          const size_t len = cpu::CompressFrame(x.data(), n, out, id, flags);
          ++frames;
          CHECK(len <= bound, "n %zu id %d flags %u: %zu > %zu", n, id, flags, len, bound);
          lz4f::Header h;
          CHECK(lz4f::parse_header(out, len, &h) == lz4f::kStOk, "n %zu id %d flags %u", n, id, flags);
          CHECK(!!(h.flg & lz4f::kFlgSum) == !!(flags & 1) && !!(h.flg & lz4f::kFlgBlockSum) == !!(flags & 2) &&
                    !!(h.flg & lz4f::kFlgSize) == (n && !(flags & 4)) && (h.flg & lz4f::kFlgIndep),
                "FLG %02x for n %zu flags %u", h.flg, n, flags);
          if (kind == 0 && n >= 16)  // every block raw: the longest frame there is for (n, id, flags)
            CHECK(len == bound - ((flags & 4) ? 8 : 0) - ((flags & 1) ? 0 : 4), "n %zu id %d flags %u: %zu against %zu", n, id, flags, len,
                  bound);
          std::vector<uint8_t> back(n + 1);
          uint32_t ol = 0;
          CHECK(cpu::DecompressFrame(out, len, back.data(), n, &ol) == 0 && ol == n &&
                    (n == 0 || std::memcmp(back.data(), x.data(), n) == 0),
                "round trip n %zu id %d flags %u", n, id, flags);
          if (flags == 1) {  // the bool overload is bit 0
            std::vector<uint8_t> f2(bound);
            CHECK(cpu::CompressFrame(x.data(), n, f2.data(), id, true) == len && std::memcmp(f2.data(), out, len) == 0,
                  "bool overload n %zu", n);
          }
          delete[] out;
        }
      }
    }
  }
  // a flags word with a bit above the three, a bad block size id: 0, nothing written
  const std::vector<uint8_t> x = make_input(70000, 1);
  uint8_t none[1] = {0x5A};
  CHECK(cpu::CompressFrame(x.data(), x.size(), none, 4, 8u) == 0 && cpu::CompressFrame(x.data(), x.size(), none, 4, 0x80000001u) == 0 &&
            none[0] == 0x5A,
        "undefined flag bits");
  CHECK(cpu::MaxFrameLength(10, 4, 8) == 0 && cpu::MaxFrameLength(10, 3, 2) == 0 && cpu::MaxFrameLength(10, 8, 2) == 0,
        "ids and flags");
  if (failures) return 1;
  std::printf("ok %zu\n", frames);
  return 0;
}
