// inflate_check.cc -- the host inflate model (host/inflate_cpu.cc over
// csrc/inflate_format.h) on a file of vectors, as a stand-alone program for
// AddressSanitizer and UBSan (tests/test_inflate.py builds and runs it).
// Input and output buffers are heap blocks of exactly the body's and the
// capacity's size, so a byte read or written past either is reported.
//
// File: records of  u32 format, u32 n, u32 cap, u32 status, u32 length,
// n body bytes, then `length` expected bytes when status is 0.
//
// Also checks the polynomial arithmetic the device checksum kernel relies on
// (crc_mulmod, crc_xpow8): a 64-lane emulation of its piece scheme against the
// serial CRC-32.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "../../flare-cpp_amd/csrc/inflate_format.h"
#include "inflate_cpu.h"

namespace {

uint32_t lanes_crc32(const uint8_t* p, uint32_t n) {
  const uint32_t pieces = n >> 4;
  const uint32_t step = infl::CrcXpow8<10>::v;
  uint32_t total = 0;
  for (uint32_t lane = 0; lane < 64; ++lane) {
    uint32_t s = 0, last = 0;
    for (uint32_t k = lane; k < pieces; k += 64) {
      s = infl::crc_mulmod(s, step) ^ infl::crc32_serial(0, p + 16 * (size_t)k, 16);
      last = k;
    }
    if (lane < pieces) total ^= infl::crc_mulmod(s, infl::crc_xpow8(n - 16 * (last + 1)));
  }
  if (n & 15) total ^= infl::crc32_serial(0, p + (pieces << 4), n & 15);
  return total;
}

uint32_t lanes_adler32(const uint8_t* p, uint32_t n) {
  const uint32_t M = infl::kAdlerMod, pieces = n >> 4;
  uint32_t sa = 0, sb = 0;
  for (uint32_t lane = 0; lane < 64; ++lane) {
    uint32_t a = 0, b = 0;
    for (uint32_t k = lane; k < pieces; k += 64) {
      uint32_t psum = 0, wsum = 0;
      for (uint32_t j = 0; j < 16; ++j) {
        psum += p[16 * (size_t)k + j];
        wsum += j * p[16 * (size_t)k + j];
      }
      a = (a + psum) % M;
      b = (b + ((n - 16 * k) % M) * psum + M - wsum) % M;
    }
    if (lane == 0)
      for (uint32_t i = pieces << 4; i < n; ++i) {
        a += p[i];
        b += (n - i) * p[i];
      }
    sa += a;
    sb += b;
  }
  return ((n % M + sb) % M) << 16 | (1 + sa) % M;
}

bool read32(FILE* f, uint32_t* v) { return fread(v, 4, 1, f) == 1; }

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  unsigned done = 0;
  uint32_t fmt, n, cap, want_st, want_len;
  while (read32(f, &fmt)) {
    if (!read32(f, &n) || !read32(f, &cap) || !read32(f, &want_st) || !read32(f, &want_len)) return 3;
    std::unique_ptr<uint8_t[]> body(new uint8_t[n]), out(new uint8_t[cap]);
    if (n && fread(body.get(), 1, n, f) != n) return 3;
    std::vector<uint8_t> want(want_st == 0 ? want_len : 0);
    if (!want.empty() && fread(want.data(), 1, want.size(), f) != want.size()) return 3;
    uint64_t len = ~0ull;
    const int st = fsh_cpu_inflate(fmt, body.get(), n, out.get(), cap, &len);
    if ((uint32_t)st != want_st || len != want_len || (st == 0 && want_len && memcmp(out.get(), want.data(), want_len))) {
      printf("vector %u: status %d length %llu, expected %u %u\n", done, st, (unsigned long long)len, want_st, want_len);
      return 1;
    }
    uint64_t l2 = ~0ull;
    const int st2 = fsh_cpu_inflate_length(fmt, body.get(), n, &l2);
    if (st == 0 && (st2 != 0 || l2 != len)) {
      printf("vector %u: length call %d %llu\n", done, st2, (unsigned long long)l2);
      return 1;
    }
    if (st == 0 && (lanes_crc32(out.get(), want_len) != fsh_cpu_crc32(out.get(), want_len) ||
                    lanes_adler32(out.get(), want_len) != fsh_cpu_adler32(out.get(), want_len))) {
      printf("vector %u: lane checksum scheme differs from the serial one\n", done);
      return 1;
    }
    ++done;
  }
  fclose(f);
  printf("ok %u\n", done);
  return 0;
}
