// gzip_index_check.cc -- the unit index parse (csrc/gzip_index.h through
// host/gzip_index_cpu.cc), the route model of fsg_inflate_units_batch and the
// flagged writer, as a stand-alone program to build with
// -fsanitize=address,undefined (tests/test_gzip_index.py does).
//
//   gzip_index_check vectors.bin trunc.bin
// vectors.bin: records of u32 expected route, u32 expected unit entries, u32
// length, the body.  Every body sits in a heap block of exactly its length, so
// a read past it is an error the sanitizer reports.  For each: the index, the
// route with a roomy slot, with capacity 0, and for the lengths call; the
// serial inflate with and without room.  trunc.bin: one indexed body, of which
// every truncation goes through the same calls.  Then a flagged body is
// written for a few lengths and read back.  Prints "ok <records> <cuts>".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "deflate_cpu.h"
#include "gzip_index_cpu.h"
#include "inflate_cpu.h"

namespace {

int fail(const char* what, size_t at) {
  printf("FAIL %s at %zu\n", what, at);
  return 1;
}

// All the calls on one body held in an exact heap block; the route with a roomy slot.
int run_body(const uint8_t* src, size_t n, uint32_t* units) {
  uint8_t* p = static_cast<uint8_t*>(malloc(n ? n : 1));
  if (n) memcpy(p, src, n);
  uint32_t chlen = 0, chcnt = 0;
  std::vector<uint64_t> starts(32768);
  const int st = fsh_cpu_gzip_index(p, n, &chlen, &chcnt, starts.data(), starts.size());
  if (st == FSH_GZIP_INDEX_USABLE)
    for (uint32_t k = 0; k < chcnt; ++k)
      if (starts[k] + 8 > n) abort();  // the sum rule
  fsh_cpu_gzip_index(p, n, nullptr, nullptr, nullptr, 0);
  const size_t room = 1u << 20;
  const int route = fsh_cpu_inflate_units_route(2, p, n, room, 1, units);
  uint32_t u2 = 0;
  fsh_cpu_inflate_units_route(2, p, n, 0, 1, &u2);
  const int lroute = fsh_cpu_inflate_units_route(2, p, n, 0, 0, nullptr);
  if (u2 != *units || lroute != route) abort();  // a roomy slot decides nothing the lengths call does not
  fsh_cpu_inflate_units_route(0, p, n, room, 1, nullptr);
  fsh_cpu_inflate_units_route(1, p, n, room, 1, nullptr);
  std::vector<uint8_t> out(room);
  uint64_t len = 0;
  const int verdict = fsh_cpu_inflate(2, p, n, out.data(), room, &len);
  uint64_t len0 = 0;
  fsh_cpu_inflate(2, p, n, nullptr, 0, &len0);
  (void)verdict;
  free(p);
  return route;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 3) return fail("usage", 0);
  FILE* f = fopen(argv[1], "rb");
  if (!f) return fail("open", 0);
  std::vector<uint8_t> all;
  uint8_t buf[65536];
  for (size_t k; (k = fread(buf, 1, sizeof buf, f)) > 0;) all.insert(all.end(), buf, buf + k);
  fclose(f);
  size_t at = 0, records = 0;
  while (at < all.size()) {
    uint32_t want, want_units, n;
    memcpy(&want, &all[at], 4);
    memcpy(&want_units, &all[at + 4], 4);
    memcpy(&n, &all[at + 8], 4);
    at += 12;
    uint32_t units = 99;
    const int route = run_body(all.data() + at, n, &units);
    if (route != (int)want || units != want_units) return fail("route", records);
    at += n;
    ++records;
  }
  f = fopen(argv[2], "rb");
  if (!f) return fail("open", 1);
  std::vector<uint8_t> body;
  for (size_t k; (k = fread(buf, 1, sizeof buf, f)) > 0;) body.insert(body.end(), buf, buf + k);
  fclose(f);
  size_t cuts = 0;
  for (size_t n = 0; n < body.size(); ++n, ++cuts) {
    uint32_t units = 0;
    if (run_body(body.data(), n, &units) == FSH_UNITS_ROUTE_PARALLEL) return fail("a truncation went parallel", n);
  }
  uint32_t units = 0;
  if (run_body(body.data(), body.size(), &units) != FSH_UNITS_ROUTE_PARALLEL) return fail("the whole body", 0);
  // the flagged writer at a few lengths, into exact heap blocks
  for (const size_t n : {size_t(0), size_t(1), size_t(65472), size_t(65473), size_t(200000)}) {
    std::vector<uint8_t> in(n);
    for (size_t i = 0; i < n; ++i) in[i] = (uint8_t)((i * 2654435761u) >> 27);
    for (uint32_t level = 0; level <= 2; ++level) {
      const size_t cap = fsh_cpu_deflate_bound_flags(n, 2, 1);
      uint8_t* out = static_cast<uint8_t*>(malloc(cap));
      uint64_t len = 0;
      if (fsh_cpu_deflate_flags(2, level, 1, in.data(), n, out, cap, &len) != 0 || len > cap) return fail("write", n);
      if (run_body(out, len, &units) != FSH_UNITS_ROUTE_PARALLEL || units != (n + 65471) / 65472 + (n == 0))
        return fail("own body", n);
      std::vector<uint8_t> back(n + 1);
      uint64_t blen = 0;
      if (fsh_cpu_inflate(2, out, len, back.data(), n, &blen) != 0 || blen != n || (n && memcmp(back.data(), in.data(), n)))
        return fail("read back", n);
      free(out);
    }
  }
  printf("ok %zu %zu\n", records, cuts);
  return 0;
}
