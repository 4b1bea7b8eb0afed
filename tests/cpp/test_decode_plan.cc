// The launch arithmetic of the two-pass Snappy decoder (csrc/decode_v4_plan.h:
// workspace regions, thresholds, the lane walk's instance, grid sizes) on the
// CPU.  Stand-alone: includes only that header; tests/test_decode_plan.py
// builds it with AddressSanitizer and UBSan and runs one part per test
// ("table", "layout", "options").
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

// ---- the values of the parent's expressions at default options,
// ws_bytes = decode_v4_workspace_bytes(n, T)
struct Row {
  u32 n;
  u64 T, ws_bytes, cap_words, chunk_bytes, chunk_off, est_total_in;
  u32 big_threshold;
  u64 max_huge, max_recs;
  bool chunked, serial_walk;
};
static const Row kRows[] = {
    {1, 0, 3909, 192, 0, 3840, 3968, 0, 0, 0, false, true},
    {64, 262144, 38221, 8640, 512, 37632, 266240, 0, 2, 15, true, true},
    {65, 266240, 41618, 8768, 512, 40960, 270208, 16628, 2, 15, true, true},
    {65, 39000, 12759, 1664, 0, 12544, 42880, 8192, 0, 0, false, true},
    {65536, 268435456, 38082649, 8650944, 594944, 37487616, 268439552, 16384, 1025, 18335, true, true},
    {131073, 262146000, 41281438, 8716544, 644864, 40636416, 262150016, 8192, 1001, 19901, true, true},
    {131073, 314572800, 47938811, 10354880, 748800, 47189760, 314576768, 9600, 1201, 23099, true, true},
    {1000, 100000000, 12761469, 3129216, 199168, 12562176, 100004864, 49152, 382, 6128, true, false},
};

static void test_table() {
  for (const Row& r : kRows) {
    const size_t ws = decode_v4_workspace_bytes(r.n, r.T);
    CHECK(ws == r.ws_bytes, "n %u T %llu: ws_bytes %zu", r.n, (unsigned long long)r.T, ws);
    CHECK(decode_v4_bitmap_capacity_words(r.n, ws) == r.cap_words, "n %u", r.n);
    const DecodePlan p = decode_v4_plan(r.n, ws, false, DecodeOpts{});
    std::printf("n %u T %llu: ws %zu cap_words %llu chunk %llu@%llu est %llu thr %u max_huge %llu max_recs %llu "
                "chunked %d walk %d\n",
                r.n, (unsigned long long)r.T, ws, (unsigned long long)p.cap_words,
                (unsigned long long)p.chunk_bytes, (unsigned long long)p.chunk_off,
                (unsigned long long)p.est_total_in, p.big_threshold, (unsigned long long)p.max_huge,
                (unsigned long long)p.max_recs, (int)p.chunked, (int)p.walk_kind);
    CHECK(p.cap_words == r.cap_words, "n %u", r.n);
    CHECK(p.chunk_bytes == r.chunk_bytes, "n %u", r.n);
    CHECK(p.chunk_off == r.chunk_off, "n %u", r.n);
    CHECK(p.est_total_in == r.est_total_in, "n %u", r.n);
    CHECK(p.big_threshold == r.big_threshold, "n %u", r.n);
    CHECK(p.max_huge == r.max_huge, "n %u", r.n);
    CHECK(p.max_recs == r.max_recs, "n %u", r.n);
    CHECK(p.chunked == r.chunked, "n %u", r.n);
    // "serial walk": est_total_in < 16384 n selects the kIdxWavesSerial
    // instance when the walk is neither planned nor lean
    CHECK((p.est_total_in < 16384ull * r.n) == r.serial_walk, "n %u", r.n);
    CHECK((p.walk_kind == kWalkSerial) == r.serial_walk, "n %u", r.n);
    CHECK(p.walk_kind == (r.serial_walk ? kWalkSerial : kWalkStandard), "n %u", r.n);
    const u32 w = r.serial_walk ? kIdxWavesSerial : kIdxWaves;
    CHECK(p.walk.block == 64 * w && p.walk.grid == (r.n + 64 * w - 1) / (64 * w) && p.walk.lds == 0, "n %u", r.n);
    // the two-stream form walks lean whatever the sizes
    const DecodePlan p2 = decode_v4_plan(r.n, ws, true, DecodeOpts{});
    CHECK(p2.walk_kind == kWalkLean && p2.walk.lds == idx_lean_lds_bytes() && p2.walk.block == 64 * kIdxWaves,
          "n %u", r.n);
    DecodeOpts no_lean;
    no_lean.lean_walk = 0;
    CHECK(decode_v4_plan(r.n, ws, true, no_lean).walk_kind == p.walk_kind, "n %u", r.n);
  }
}

// ---- invariants over batch and workspace sizes
static const u32 kNs[] = {1, 63, 64, 65, 131072, 131073, 1u << 20};

template <class F>
static void for_each_size(F f) {
  for (u32 n : kNs)
    for (u64 T : {(u64)0, (u64)600 * n, (u64)4096 * n}) {
      const size_t full = decode_v4_workspace_bytes(n, T);
      f(n, full);
      // a workspace for a third of the input (the bitmap-fallback case)
      if (full / 3 >= decode_v4_workspace_bytes(n, 0)) f(n, full / 3);
    }
}

static void check_layout(u32 n, size_t ws, bool two) {
  const DecodePlan p = decode_v4_plan(n, ws, two, DecodeOpts{});
  // counters, the 11 lists, the bitmap, the chunk region: in that order,
  // disjoint, inside the workspace
  struct Region {
    const char* name;
    u64 off, bytes;
  };
  const u64 n4 = 4ull * n;
  const Region reg[] = {
      {"counters", 0, kWsCounterBytes},
      {"bm_base", p.bm_base_off, n4},
      {"big_list", p.big_list_off, n4},
      {"seg_list", p.seg_list_off, 2 * n4},
      {"whole_list", p.whole_list_off, n4},
      {"walk_rank", p.walk_rank_off, n4},
      {"walk_perm", p.walk_perm_off, n4},
      {"walk_hist", p.walk_hist_off, 4ull * (2 * kWalkClasses + 1)},
      {"seg_list2", p.seg_list2_off, 2 * n4},
      {"whole_list2", p.whole_list2_off, n4},
      {"bitmap", p.bitmap_off, 4 * p.cap_words},
      {"chunk region", p.chunk_off, p.chunk_bytes},
  };
  const size_t nreg = sizeof(reg) / sizeof(reg[0]);
  for (size_t i = 0; i + 1 < nreg; ++i)
    CHECK(reg[i].off + reg[i].bytes <= reg[i + 1].off, "n %u ws %zu: %s [%llu, +%llu) runs into %s at %llu", n, ws,
          reg[i].name, (unsigned long long)reg[i].off, (unsigned long long)reg[i].bytes, reg[i + 1].name,
          (unsigned long long)reg[i + 1].off);
  CHECK(p.chunk_off + p.chunk_bytes <= ws, "n %u ws %zu", n, ws);
  // 11 list slots of base_bytes each between the counters and the bitmap
  CHECK(p.bm_base_off == kWsCounterBytes && p.bitmap_off == kWsCounterBytes + kListBases * p.base_bytes &&
            p.base_bytes >= n4,
        "n %u ws %zu", n, ws);
  for (size_t i = 1; i < nreg; ++i)
    CHECK(reg[i].off % 256 == 0, "n %u ws %zu: %s at %llu", n, ws, reg[i].name, (unsigned long long)reg[i].off);
  // the chunk records
  const u64 cend = p.chunk_off + p.chunk_bytes;
  CHECK(p.first_rec_off >= p.chunk_off && p.first_rec_off + 4 * p.max_huge <= p.mstat_off, "n %u ws %zu", n, ws);
  CHECK(p.mstat_off + 4 * p.max_huge <= p.recs_off, "n %u ws %zu", n, ws);
  CHECK(p.recs_off + sizeof(ChunkRec) * p.max_recs <= cend, "n %u ws %zu", n, ws);
  CHECK(8 * p.max_huge + 32 * p.max_recs <= p.chunk_bytes, "n %u ws %zu", n, ws);
  CHECK(sizeof(ChunkRec) == 32, "record size");
  // the threshold
  CHECK((p.big_threshold == 0) == (n <= 64), "n %u ws %zu: %u", n, ws, p.big_threshold);
  if (n > 64) CHECK(p.big_threshold >= 8192 && p.big_threshold <= 49152, "n %u ws %zu: %u", n, ws, p.big_threshold);
  // every launch has at least one block
  const u32 grids[] = {p.walk.grid,      p.planned_walk.grid, p.plan_grid,       p.scatter_grid,
                       p.index_big_grid, p.small_blocks,      p.big_blocks,      p.fork_big_blocks,
                       p.small_grid,     p.chunk_list_grid,   p.chunk_rec_grid,  p.chunk_msg_grid,
                       p.fallback_grid};
  for (size_t i = 0; i < sizeof(grids) / sizeof(grids[0]); ++i) CHECK(grids[i] >= 1, "n %u ws %zu: grid %zu", n, ws, i);
  CHECK(p.walk.block >= 64 && p.planned_walk.block >= 64, "n %u", n);
  // the grids cover the batch
  CHECK((u64)p.walk.grid * p.walk.block >= n && (u64)p.planned_walk.grid * p.planned_walk.block >= n, "n %u", n);
  CHECK((u64)p.plan_grid * kPlanThreads >= n && (u64)p.scatter_grid * 256 >= n && (u64)p.fallback_grid * 64 >= n &&
            (u64)p.small_blocks * kWavesPerBlock >= n,
        "n %u", n);
  CHECK(p.big_blocks <= p.small_blocks && p.fork_big_blocks <= p.small_blocks && p.small_grid <= p.small_blocks,
        "n %u", n);
  // a persistent small-message grid strides by its own size
  CHECK(p.small_stride == (p.small_grid < p.small_blocks ? p.small_grid : 0u), "n %u", n);
}

static void test_layout() {
  for_each_size([](u32 n, size_t ws) {
    check_layout(n, ws, false);
    check_layout(n, ws, true);
  });
}

static void test_options() {
  for_each_size([](u32 n, size_t ws) {
    // fork: never in the two-stream form; else the option, or > 128K messages
    for (i64 f : {(i64)-1, (i64)0, (i64)1}) {
      DecodeOpts o;
      o.decode_fork = f;
      CHECK(!decode_v4_plan(n, ws, true, o).fork, "n %u fork %lld", n, (long long)f);
      const bool want = f >= 0 ? f != 0 : n > 131072u;
      CHECK(decode_v4_plan(n, ws, false, o).fork == want, "n %u fork %lld", n, (long long)f);
    }
    // small_batch moves the bound under which every message takes pass 1b
    for (i64 sb : {(i64)0, (i64)64, (i64)100000}) {
      DecodeOpts o;
      o.small_batch = sb;
      const DecodePlan p = decode_v4_plan(n, ws, false, o);
      CHECK((p.big_threshold == 0) == ((i64)n <= sb), "n %u small_batch %lld: %u", n, (long long)sb, p.big_threshold);
      if ((i64)n > sb) CHECK(p.big_threshold >= 8192 && p.big_threshold <= 49152, "n %u: %u", n, p.big_threshold);
    }
    // exec_keep: 512..kMaxKeep in steps of 16, anything else the default
    for (i64 k : {(i64)-1, (i64)511, (i64)520, (i64)kMaxKeep + 16}) {
      DecodeOpts o;
      o.exec_keep = k;
      CHECK(decode_v4_plan(n, ws, false, o).keep_hist == 1024, "exec_keep %lld", (long long)k);
    }
    for (i64 k : {(i64)512, (i64)768, (i64)2000}) {
      DecodeOpts o;
      o.exec_keep = k;
      CHECK(decode_v4_plan(n, ws, false, o).keep_hist == (u32)k, "exec_keep %lld", (long long)k);
    }
    // exec_pack: 1..64 bodies per batch, anything else one wave per body
    for (i64 k : {(i64)0, (i64)65, (i64)-1}) {
      DecodeOpts o;
      o.exec_pack = k;
      CHECK(decode_v4_plan(n, ws, false, o).pack_batch == 0, "exec_pack %lld", (long long)k);
    }
    CHECK(decode_v4_plan(n, ws, false, DecodeOpts{}).pack_batch == 32, "exec_pack default");
    // chunked_huge 0 turns the chunked walk off and moves nothing else
    {
      DecodeOpts o;
      o.chunked_huge = 0;
      const DecodePlan p = decode_v4_plan(n, ws, false, o), d = decode_v4_plan(n, ws, false, DecodeOpts{});
      CHECK(!p.chunked && p.max_huge == d.max_huge && p.max_recs == d.max_recs && p.recs_off == d.recs_off,
            "n %u ws %zu", n, ws);
    }
    // small_persist: 0 = a wave per message; a grid never above that
    for (i64 sp : {(i64)0, (i64)5, (i64)3584, (i64)-1, (i64)(1 << 20) + 1}) {
      DecodeOpts o;
      o.small_persist = sp;
      const DecodePlan p = decode_v4_plan(n, ws, false, o);
      const u32 eff = sp >= 0 && sp <= (1 << 20) ? (u32)sp : 3584u;
      const u32 want = eff && eff < p.small_blocks ? eff : p.small_blocks;
      CHECK(p.small_grid == want && p.small_grid >= 1, "n %u small_persist %lld: %u", n, (long long)sp, p.small_grid);
    }
  });
  // the remaining options pass through
  DecodeOpts o;
  o.split_walk = 1;
  o.split_class = 21;
  o.split_huge = 0;
  o.walk_order = 0;
  o.exec_prio = 0;
  o.exec_big_blocks = 7;
  o.exec_big_blocks_fork = 9;
  const size_t ws = decode_v4_workspace_bytes(1000, 1000000);
  const DecodePlan p = decode_v4_plan(1000, ws, false, o), d = decode_v4_plan(1000, ws, false, DecodeOpts{});
  CHECK(p.split_mode == 1 && p.split_class == 21 % kWalkClasses && !p.split_huge && !p.walk_order && p.prio == 0 &&
            p.big_blocks == 7 && p.fork_big_blocks == 9,
        "set options");
  CHECK(d.split_mode == 3 && d.split_class == 4 && d.split_huge && d.walk_order && d.prio == 1 &&
            d.big_blocks == 250 && d.fork_big_blocks == 250 && d.small_blocks == 250,
        "default options");
  // split_class: every value is a size class 0..15 (modulo 16, of the value
  // as u32), so every one names an existing walk_hist offset
  for (i64 c : {(i64)0, (i64)1, (i64)7, (i64)8, (i64)15, (i64)16, (i64)255, (i64)256, (i64)-1, (i64)1 << 40}) {
    DecodeOpts s;
    s.split_class = c;
    const u32 got = decode_v4_plan(1000, ws, false, s).split_class;
    CHECK(got == (u32)c % kWalkClasses && got < kWalkClasses, "split_class %lld: %u", (long long)c, got);
  }
  // exec_prio and the flags: any non-zero value is "on"
  for (i64 v : {(i64)-1, (i64)2, (i64)1 << 40}) {
    DecodeOpts s;
    s.exec_prio = s.split_huge = s.walk_order = s.chunked_huge = v;
    const DecodePlan sp = decode_v4_plan(1000, ws, false, s);
    CHECK(sp.prio == 1 && sp.split_huge && sp.walk_order && sp.chunked == d.chunked, "flag %lld", (long long)v);
  }
  o.exec_big_blocks = 0;  // out of range: the defaults
  o.exec_big_blocks_fork = (1 << 20) + 1;
  const size_t ws2 = decode_v4_workspace_bytes(1u << 20, 0);
  const DecodePlan q = decode_v4_plan(1u << 20, ws2, false, o);
  CHECK(q.big_blocks == 512 && q.fork_big_blocks == 1024, "out-of-range block counts");
}

int main(int argc, char** argv) {
  const char* part = argc > 1 ? argv[1] : "all";
  const bool all = !std::strcmp(part, "all");
  bool ran = false;
  if (all || !std::strcmp(part, "table")) test_table(), ran = true;
  if (all || !std::strcmp(part, "layout")) test_layout(), ran = true;
  if (all || !std::strcmp(part, "options")) test_options(), ran = true;
  if (!ran) {
    std::printf("unknown part %s\n", part);
    return 2;
  }
  std::printf("%s: %d failure(s)\n", part, g_fail);
  return g_fail ? 1 : 0;
}
