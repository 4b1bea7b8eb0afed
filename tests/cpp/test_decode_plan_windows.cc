// The two instances of the execution pass (exec_kernel<5>, csrc/
// decode_v4_exec5.h) as csrc/decode_v4_plan.h sizes them: the kept history of
// each over option exec_keep's whole range, and the LDS arithmetic.
// Stand-alone: includes only that header; tests/test_decode_plan_windows.py
// builds it with AddressSanitizer and UBSan and runs one part per test
// ("keep", "lds").
#include "decode_v4_plan.h"

#include <cstdio>
#include <cstring>
#include <initializer_list>

using namespace fsg;

static int g_fail = 0;
#define CHECK(cond, ...)                                   \
  do {                                                     \
    if (!(cond)) {                                         \
      ++g_fail;                                            \
      std::printf("FAIL %s:%d %s | ", __FILE__, __LINE__, #cond); \
      std::printf(__VA_ARGS__);                            \
      std::printf("\n");                                   \
    }                                                      \
  } while (0)

// What a window of `window` bytes admits as kept history: after a slide the
// write position is at most keep + 15 above the base, a group adds at most
// 1,024 bytes and an OR store writes up to 20 bytes past a 16-byte piece's
// start, all inside window + 32 bytes.
static bool keep_fits(u32 window, u32 keep) { return keep + 15 + 1023 + 20 <= window + 32; }

static void test_keep() {
  CHECK(kWindow == 3072 && kMaxKeep == 2000, "general: %u / %u", kWindow, kMaxKeep);
  CHECK(kWindowWhole == 4096 && kMaxKeepWhole == 3024, "folded: %u / %u", kWindowWhole, kMaxKeepWhole);
  CHECK(kMaxKeepWhole == ((kWindowWhole - 1024 - 48) & ~15u), "largest kept history follows the window");
  const size_t ws = decode_v4_workspace_bytes(65536, 1ull << 28);
  const DecodePlan d = decode_v4_plan(65536, ws, false, DecodeOpts{});
  CHECK(d.keep_hist == kKeep && d.keep_hist_whole == kKeepWhole, "defaults %u %u", d.keep_hist, d.keep_hist_whole);
  CHECK(kKeepWhole >= 512 && kKeepWhole <= kMaxKeepWhole && kKeepWhole % 16 == 0, "default %u", kKeepWhole);
  // every value of the option, well past both ends of its range
  for (i64 v = -64; v <= 4200; ++v) {
    DecodeOpts o;
    o.exec_keep = v;
    for (int two = 0; two < 2; ++two) {
      const DecodePlan p = decode_v4_plan(65536, ws, two != 0, o);
      const bool step = v >= 512 && v % 16 == 0;
      const u32 want = step && v <= (i64)kMaxKeep ? (u32)v : kKeep;
      const u32 want_whole = step && v <= (i64)kMaxKeepWhole ? (u32)v : kKeepWhole;
      CHECK(p.keep_hist == want, "exec_keep %lld: general %u", (long long)v, p.keep_hist);
      CHECK(p.keep_hist_whole == want_whole, "exec_keep %lld: folded %u", (long long)v, p.keep_hist_whole);
      // whatever the option, each instance's value fits its own window, is a
      // multiple of 16 and fits the 16 bits it has in the kernel's argument
      CHECK(p.keep_hist % 16 == 0 && p.keep_hist >= 512 && p.keep_hist <= kMaxKeep && keep_fits(kWindow, p.keep_hist),
            "exec_keep %lld: general %u", (long long)v, p.keep_hist);
      CHECK(p.keep_hist_whole % 16 == 0 && p.keep_hist_whole >= 512 && p.keep_hist_whole <= kMaxKeepWhole &&
                keep_fits(kWindowWhole, p.keep_hist_whole),
            "exec_keep %lld: folded %u", (long long)v, p.keep_hist_whole);
      CHECK(p.keep_hist < 65536 && p.keep_hist_whole < 65536, "exec_keep %lld", (long long)v);
    }
  }
  // a value between the two bounds sets the folded instance's alone, and
  // moves no launch geometry
  {
    DecodeOpts o;
    o.exec_keep = 2048;
    const DecodePlan p = decode_v4_plan(65536, ws, false, o);
    CHECK(p.keep_hist == kKeep && p.keep_hist_whole == 2048, "2048: %u %u", p.keep_hist, p.keep_hist_whole);
    CHECK(p.big_threshold == d.big_threshold && p.small_blocks == d.small_blocks && p.big_blocks == d.big_blocks &&
              p.small_grid == d.small_grid && p.pack_batch == d.pack_batch && p.prio == d.prio && p.fork == d.fork,
          "exec_keep changed another field");
  }
}

static void test_lds() {
  // per wave 5 KiB + 32 either way
  CHECK(exec_wave_lds_bytes(false) == 5 * 1024 + 32, "general %u", exec_wave_lds_bytes(false));
  CHECK(exec_wave_lds_bytes(true) == 5 * 1024 + 32, "folded %u", exec_wave_lds_bytes(true));
  CHECK(4 * kExecRing + kWindow + 32 == exec_wave_lds_bytes(false), "general: 32-bit ring + window");
  CHECK(2 * kExecRing + kWindowWhole + 32 == exec_wave_lds_bytes(true), "folded: 16-bit ring + window");
  CHECK(kExecRing == 512 && 2 * kExecRing == 1024 && kWindowWhole - kWindow == 2 * kExecRing,
        "the window grows by what the ring gives up");
  // a 16-bit entry holds every tag position of a body the folded instance
  // takes: big_threshold never passes kBigIndexMax
  CHECK(kBigIndexMax < 65536, "kBigIndexMax %u", kBigIndexMax);
  for (u32 n : {1u, 64u, 65u, 1000u, 65536u, 200000u})
    for (u64 T : {(u64)0, (u64)1 << 20, (u64)1 << 28, (u64)3 << 30}) {
      const DecodePlan p = decode_v4_plan(n, decode_v4_workspace_bytes(n, T), false, DecodeOpts{});
      CHECK(p.big_threshold <= kBigIndexMax, "n %u T %llu: %u", n, (unsigned long long)T, p.big_threshold);
    }
  // per block: the waves' rings and windows and the pattern, tag and mask
  // tables (variant 5 has no piece map) -- no more than the 22,160 bytes the
  // kernel took with one 3 KiB window instance, so 7 blocks still fit a CU's
  // 160 KiB
  const u32 block = kWavesPerBlock * exec_wave_lds_bytes(true) + 16 * 16 + 256 * 4 + 17 * 16;
  CHECK(block <= 22160, "block %u", block);
  CHECK(7 * 22160 <= 160 * 1024, "7 blocks per CU");
}

int main(int argc, char** argv) {
  const char* part = argc > 1 ? argv[1] : "all";
  const bool all = !std::strcmp(part, "all");
  if (all || !std::strcmp(part, "keep")) test_keep();
  if (all || !std::strcmp(part, "lds")) test_lds();
  if (g_fail) {
    std::printf("%d check(s) failed\n", g_fail);
    return 1;
  }
  std::printf("ok %s\n", part);
  return 0;
}
