// deflate_level_check.cc -- the host deflate model at levels 0 and 2
// (host/deflate_cpu.cc over csrc/deflate_format.h, "levels") under
// AddressSanitizer and UBSan, stand-alone: built and run by
// tests/test_deflate_level.py, never loaded into Python.
//
// Input: a file of records { u32 format, level, n, want_len, flags } + n input
// bytes + want_len body bytes (what the unsanitized library gave).  Per record:
//   1. fsh_cpu_deflate_level gives exactly those bytes into a buffer of
//      exactly the bound, refuses a buffer one byte short, and
//      fsh_cpu_inflate gives the input back; at level 0 the length is the
//      bound;
//   2. (flags & 2, level 2) the window step as the device takes it, unit by
//      unit: 64 lanes each form token_at2 from the table as it stood before
//      the window, each lane's lazy decision reads its right-hand
//      neighbour's undeferred record, the chain is walked over the deferred
//      records, and every lane with 4 bytes left stores insert_word(its own
//      word, its position), the stores applied in ascending lane order.  After
//      every window the table must be the rule's by definition (per slot: the
//      old newer candidate moved up, the HIGHEST position of the window that
//      hashes to the slot below it), and the unit's tokens must be the
//      model's (fsh_cpu_deflate_tokens_level).
// Prints "ok <records> <windows emulated>".
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <vector>

#include "../../flare-cpp_amd/csrc/deflate_format.h"
#include "deflate_cpu.h"
#include "inflate_cpu.h"

namespace {

struct Reader {  // the unit in a heap block of exactly n bytes: a read past it is the sanitizer's
  const uint8_t* p;
  uint32_t n;
  uint32_t load32(uint32_t q) const {
    uint32_t v = 0;
    for (uint32_t i = 0; i < 4 && q + i < n; ++i) v |= (uint32_t)p[q + i] << (8 * i);
    return v;
  }
};

constexpr uint32_t kLanes = defl::kWindow;

// One unit at level 2 by 64 lanes.  false with a message on the first difference.
bool emulate_unit(const uint8_t* in, uint32_t n, size_t* windows) {
  std::vector<uint8_t> copy(in, in + n);
  const Reader rd{copy.data(), n};
  std::vector<uint32_t> table(defl::kTableEntries, defl::kEmptyPair), want_table = table;
  std::vector<uint32_t> tokens;
  uint32_t entry = 0;
  for (uint32_t base = 0; base < n; base += kLanes, ++*windows) {
    const uint32_t cnt = n - base < kLanes ? n - base : kLanes;
    uint32_t r[kLanes], rec[kLanes], four[kLanes], word[kLanes];
    for (uint32_t lane = 0; lane < kLanes; ++lane) {  // before the fence: reads only
      four[lane] = word[lane] = 0;
      r[lane] = lane < cnt ? defl::token_at2(rd, n, base + lane, table.data(), &four[lane], &word[lane]) : defl::kTokLit;
    }
    for (uint32_t lane = 0; lane < kLanes; ++lane)  // the neighbour's record; lane 63 reads 0
      rec[lane] = defl::defer_token(r[lane], lane + 1 < kLanes ? r[lane + 1] : 0u, lane + 1 < cnt, four[lane]);
    uint32_t cur = entry;
    while (cur < cnt) {
      tokens.push_back(rec[cur]);
      cur += defl::tok_advance(rec[cur]);
    }
    entry = cur - cnt;
    // the rule by definition, from the table before the window
    std::map<uint32_t, uint32_t> highest;
    for (uint32_t i = 0; i < cnt; ++i)
      if (n - (base + i) >= defl::kMinMatch) highest[defl::hash4(rd.load32(base + i))] = base + i;
    for (const auto& kv : highest) want_table[kv.first] = (want_table[kv.first] & 0xffffu) << 16 | kv.second;
    // after the fence: one store per lane, ascending
    for (uint32_t lane = 0; lane < cnt; ++lane)
      if (n - (base + lane) >= defl::kMinMatch)
        table[defl::hash4(four[lane])] = defl::insert_word(word[lane], base + lane);
    if (table != want_table) {
      printf("window at %u: the lanes' table is not the rule's\n", base);
      return false;
    }
  }
  std::vector<uint32_t> want(n + 1);
  const size_t k = fsh_cpu_deflate_tokens_level(2, in, n, want.data(), n + 1);
  want.resize(k);
  if (tokens != want) {
    printf("the lanes' tokens are not the model's (%zu against %zu)\n", tokens.size(), want.size());
    return false;
  }
  return true;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  size_t rec = 0, windows = 0;
  for (;; ++rec) {
    uint32_t h[5];
    if (fread(h, 4, 5, f) != 5) break;
    const uint32_t fmt = h[0], level = h[1], n = h[2], want_len = h[3], flags = h[4];
    std::vector<uint8_t> in(n), want(want_len);
    if (n && fread(in.data(), 1, n, f) != n) return 2;
    if (want_len && fread(want.data(), 1, want_len, f) != want_len) return 2;
    auto fail = [&](const char* what) {
      printf("record %zu (format %u, level %u, %u bytes): %s\n", rec, fmt, level, n, what);
      return 1;
    };
    const size_t cap = fsh_cpu_deflate_bound(n, fmt);
    std::vector<uint8_t> out(cap);
    uint64_t len = 99;
    if (fsh_cpu_deflate_level(fmt, level, in.data(), n, out.data(), cap, &len) != 0) return fail("status");
    if (len != want_len || memcmp(out.data(), want.data(), len) != 0) return fail("bytes differ from the library's");
    if (level == 0 && len != cap) return fail("a level-0 body is not as long as the bound");
    uint64_t l2 = 7;
    std::vector<uint8_t> tiny(len - 1);
    if (fsh_cpu_deflate_level(fmt, level, in.data(), n, tiny.data(), len - 1, &l2) != 3 || l2 != 0)
      return fail("small cap");
    std::vector<uint8_t> back(n);
    uint64_t blen = 0;
    if (fsh_cpu_inflate(fmt, out.data(), len, back.data(), n, &blen) != 0 || blen != n ||
        (n && memcmp(back.data(), in.data(), n) != 0))
      return fail("fsh_cpu_inflate does not return the input");
    if (!(flags & 2) || level != 2) continue;
    const uint64_t nu = n == 0 ? 1 : (n + defl::kUnit - 1) / defl::kUnit;
    for (uint64_t u = 0; u < nu; ++u) {
      const uint32_t first = (uint32_t)(u * defl::kUnit), un = n - first < defl::kUnit ? n - first : defl::kUnit;
      if (!emulate_unit(in.data() + first, un, &windows)) return fail("lanes");
    }
  }
  fclose(f);
  // an unknown level: refused, nothing written
  uint8_t one[64];
  uint64_t len = 5;
  if (fsh_cpu_deflate_level(1, 3, "abc", 3, one, sizeof one, &len) != 1 || len != 0) return 1;
  printf("ok %zu %zu\n", rec, windows);
  return 0;
}
