// The launch arithmetic of the Snappy encoder (csrc/encode_v3_plan.h: route,
// workspace regions, the wave encoder's threshold and geometry, the lanes
// launched, grid sizes, option range checks) on the CPU.  Stand-alone:
// includes only that header; tests/test_encode_plan.py builds it with
// AddressSanitizer and UBSan and runs one part per test ("table", "layout",
// "options").
#include "encode_v3_plan.h"

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

static EncodePlan plan_of(u32 n, u32 max_in_len, size_t ws, const EncodeOpts& o = EncodeOpts{}) {
  return encode_v3_plan(n, max_in_len, ws, true, 0, 0u, o);
}
static size_t full_ws(u32 n, u32 max_in_len) {  // fsg_compress_workspace_bytes
  return encode_tables_workspace_bytes(n, max_in_len, nullptr) + encode_plan_bytes(n, max_in_len);
}

// ---- the values of the expressions of fsg_compress_batch and
// launch_encode_v3 before they moved into encode_v3_plan, at default options
// (evaluated from a copy of those expressions at the parent commit).
// ws_bytes = fsg_compress_workspace_bytes(n, max) except in the last two rows
// (the tables alone; one byte less).  262144 x 1039848 is C5 (the
// generator's largest serialized body), 65536 x 65536 C3.
struct Row {
  u32 n, max_in_len;
  u64 ws_bytes;
  int route;
  u64 tables_bytes, plan_bytes;
  u32 slots, entries;
  int planned, can_split;
  u32 wave_min, lanes;
  u64 max_items, items_off, sizes_off, frag_base_off, big_list_off;
  u32 share;
  u64 all_bytes;
  int split_pipe;
  u32 pipe_grid, plan_grid, wave_grid, wave_block, wave_lds, wg, per_cu, waves, ht;
  int fallback;
};
static const Row kRows[] = {
    {1u, 4096u, 4194836ull, 0, 4194560ull, 276ull, 256u, 4096u, 1, 0, 15u, 256u, 1ull, 4194560ull, 4194568ull, 4194572ull, 4194576ull, 475u, 671088640ull, 0, 4u, 1u, 1u, 64u, 8192u, 1u, 18u, 1u, 4096u, 0},
    {64u, 65536u, 16779008ull, 0, 16777472ull, 1536ull, 256u, 16384u, 1, 0, 15u, 256u, 64ull, 16777472ull, 16777984ull, 16778240ull, 16778496ull, 475u, 671088640ull, 0, 4u, 1u, 64u, 64u, 32768u, 1u, 4u, 64u, 16384u, 0},
    {65u, 65536u, 16779028ull, 0, 16777472ull, 1556ull, 256u, 16384u, 1, 0, 16384u, 256u, 65ull, 16777472ull, 16777992ull, 16778252ull, 16778512ull, 475u, 671088640ull, 0, 4u, 1u, 65u, 64u, 32768u, 1u, 4u, 65u, 16384u, 0},
    {131072u, 4096u, 2150105600ull, 0, 2147483904ull, 2621696ull, 131072u, 4096u, 1, 0, 15u, 98304u, 131072ull, 2147483904ull, 2148532480ull, 2149056768ull, 2149581056ull, 475u, 671088640ull, 0, 1536u, 512u, 4608u, 64u, 8192u, 1u, 18u, 4608u, 4096u, 0},
    {131072u, 8192u, 4297589248ull, 0, 4294967552ull, 2621696ull, 131072u, 8192u, 1, 0, 15u, 98304u, 131072ull, 4294967552ull, 4296016128ull, 4296540416ull, 4297064704ull, 475u, 671088640ull, 0, 1536u, 512u, 2304u, 64u, 16384u, 1u, 9u, 2304u, 8192u, 0},
    {131072u, 8193u, 8592556544ull, 0, 8589934848ull, 2621696ull, 131072u, 16384u, 0, 0, 0u, 131072u, 0ull, 0ull, 0ull, 0ull, 0ull, 475u, 671088640ull, 0, 2048u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0},
    {65536u, 65536u, 4296278528ull, 0, 4294967552ull, 1310976ull, 65536u, 16384u, 1, 0, 16384u, 49152u, 65536ull, 4294967552ull, 4295491840ull, 4295753984ull, 4296016128ull, 475u, 671088640ull, 0, 768u, 256u, 1024u, 64u, 32768u, 1u, 4u, 1024u, 16384u, 0},
    {262144u, 1039848u, 17232298496ull, 0, 17179869440ull, 52429056ull, 262144u, 16384u, 1, 1, 16384u, 131072u, 4194304ull, 17179869440ull, 17213423872ull, 17230201088ull, 17231249664ull, 475u, 671088640ull, 1, 2048u, 1024u, 1024u, 64u, 32768u, 1u, 4u, 1024u, 16384u, 1},
    {1000u, 70000u, 67141376ull, 0, 67109120ull, 32256ull, 1024u, 16384u, 1, 1, 16384u, 768u, 2000ull, 67109120ull, 67125120ull, 67133120ull, 67137120ull, 475u, 671088640ull, 1, 12u, 4u, 1024u, 64u, 32768u, 1u, 4u, 1024u, 16384u, 1},
    {1000u, 1048576u, 67309376ull, 0, 67109120ull, 200256ull, 1024u, 16384u, 1, 1, 16384u, 768u, 16000ull, 67109120ull, 67237120ull, 67301120ull, 67305120ull, 475u, 671088640ull, 1, 12u, 4u, 1024u, 64u, 32768u, 1u, 4u, 1024u, 16384u, 1},
    {1000u, 0u, 67109120ull, 0, 67109120ull, 0ull, 1024u, 16384u, 0, 0, 0u, 1024u, 0ull, 0ull, 0ull, 0ull, 0ull, 475u, 671088640ull, 1, 16u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0},
    {300000u, 65536u, 17185869696ull, 0, 17179869440ull, 6000256ull, 262144u, 16384u, 1, 0, 16384u, 131072u, 300000ull, 17179869440ull, 17182269440ull, 17183469440ull, 17184669440ull, 475u, 671088640ull, 0, 2048u, 1172u, 1024u, 64u, 32768u, 1u, 4u, 1024u, 16384u, 0},
    {1000u, 65536u, 67109120ull, 0, 67109120ull, 20256ull, 1024u, 16384u, 0, 0, 0u, 1024u, 0ull, 0ull, 0ull, 0ull, 0ull, 475u, 671088640ull, 0, 16u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0},
    {1000u, 65536u, 67109119ull, 2, 67109120ull, 20256ull, 1024u, 16384u, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0},
};

static void test_table() {
  const size_t nrows = sizeof(kRows) / sizeof(kRows[0]);
  for (size_t i = 0; i < nrows; ++i) {
    const Row& r = kRows[i];
    const EncodePlan p = plan_of(r.n, r.max_in_len, (size_t)r.ws_bytes);
    std::printf("n %u max %u ws %llu: route %d tables %llu plan %llu slots %u x %u planned %d wave_min %u lanes %u "
                "items %llu split_pipe %d wave %u x %u lds %u (wg %u per_cu %u waves %u) fallback %d\n",
                r.n, r.max_in_len, (unsigned long long)r.ws_bytes, (int)p.route, (unsigned long long)p.tables_bytes,
                (unsigned long long)p.plan_bytes, p.slots, p.entries, (int)p.planned, p.wave_min, p.lanes,
                (unsigned long long)p.max_items, (int)p.split_pipe, p.wave.grid, p.wave.block, p.wave.lds, p.wg,
                p.per_cu, p.waves, (int)p.fallback);
    // fsg_compress_workspace_bytes stays the sum of the two sizes
    if (i + 2 < nrows) CHECK(full_ws(r.n, r.max_in_len) == r.ws_bytes, "row %zu: %zu", i, full_ws(r.n, r.max_in_len));
    CHECK((int)p.route == r.route, "row %zu", i);
    CHECK(p.tables_bytes == r.tables_bytes && p.plan_bytes == r.plan_bytes, "row %zu", i);
    CHECK(p.slots == r.slots && p.entries == r.entries, "row %zu", i);
    CHECK(p.planned == (r.planned != 0) && p.can_split == (r.can_split != 0), "row %zu", i);
    CHECK(p.wave_min == r.wave_min && p.lanes == r.lanes, "row %zu", i);
    CHECK(p.max_items == r.max_items && p.items_off == r.items_off && p.sizes_off == r.sizes_off &&
              p.frag_base_off == r.frag_base_off && p.big_list_off == r.big_list_off,
          "row %zu", i);
    CHECK(p.share_permille == r.share && p.all_bytes == r.all_bytes, "row %zu", i);
    CHECK(p.split_pipe == (r.split_pipe != 0), "row %zu", i);
    CHECK(p.pipe.grid == r.pipe_grid && (r.route != 0 || (p.pipe.block == 64 && p.pipe.lds == 0)), "row %zu", i);
    if (r.planned) CHECK(p.plan_pass.grid == r.plan_grid && p.plan_pass.block == 256, "row %zu", i);
    CHECK(p.wave.grid == r.wave_grid && p.wave.block == r.wave_block && p.wave.lds == r.wave_lds, "row %zu", i);
    CHECK(p.wg == r.wg && p.per_cu == r.per_cu && p.waves == r.waves && p.ht == r.ht, "row %zu", i);
    CHECK(p.fallback == (r.fallback != 0), "row %zu", i);
    if (r.fallback) CHECK(p.gather.grid == 1024 && p.gather.block == 256, "row %zu", i);
  }
}

// ---- invariants over batch sizes, bounds and workspace sizes
static const u32 kNs[] = {1, 63, 64, 65, 1000, 65536, 131072, 262144, 262145, 300000, 1u << 20};
static const u32 kMaxes[] = {0,     1,     14,    15,    4095,    4096,     8192,   8193,
                             16383, 16384, 65535, 65536, 65537,   70000,    1u << 20, 4u << 20};

static void check_layout(u32 n, u32 max_in_len, size_t ws) {
  const EncodePlan p = plan_of(n, max_in_len, ws);
  u32 slots = 0;
  const size_t tables = encode_tables_workspace_bytes(n, max_in_len, &slots);
  CHECK(p.tables_bytes == tables && p.slots == slots && p.plan_bytes == encode_plan_bytes(n, max_in_len),
        "n %u max %u", n, max_in_len);
  CHECK(p.route == (ws >= tables ? kEncRouteMain : kEncRouteNoWorkspace), "n %u max %u ws %zu", n, max_in_len, ws);
  if (p.route != kEncRouteMain) return;
  CHECK(p.tables_bytes == kEncCounterBytes + (u64)p.slots * p.entries * kEncEntryBytes, "n %u max %u", n, max_in_len);
  CHECK(p.slots % 256 == 0 && p.slots >= 256 && p.slots <= 262144 && (p.slots >= n || p.slots == 262144),
        "n %u: %u slots", n, p.slots);
  CHECK(p.entries >= 256 && p.entries <= kMaxHashTableSize && (p.entries & (p.entries - 1)) == 0, "max %u", max_in_len);
  // max_items inverts plan_bytes
  const u64 frags = max_in_len > kBlockSize ? ((u64)max_in_len + kBlockSize - 1) / kBlockSize : 1;
  if (p.plan_bytes) CHECK(p.plan_bytes == 12 * (n * frags) + 8ull * n + 256, "n %u max %u", n, max_in_len);
  CHECK(p.planned == (p.plan_bytes && ws >= p.tables_bytes + p.plan_bytes && (p.can_split || p.wave_min)),
        "n %u max %u ws %zu", n, max_in_len, ws);
  if (p.planned) {
    CHECK(p.max_items == n * frags && 12 * p.max_items + 8ull * n + 256 == p.plan_bytes, "n %u max %u", n, max_in_len);
    // counters, tables, items, sizes, frag_base, big_list: in that order,
    // disjoint, 4-byte aligned, inside the workspace
    struct Region {
      const char* name;
      u64 off, bytes;
    };
    const Region reg[] = {
        {"counters", 0, kEncCounterBytes},
        {"tables", kEncCounterBytes, (u64)p.slots * p.entries * kEncEntryBytes},
        {"items", p.items_off, 8 * p.max_items},
        {"sizes", p.sizes_off, 4 * p.max_items},
        {"frag_base", p.frag_base_off, 4ull * n},
        {"big_list", p.big_list_off, 4ull * n},
    };
    const size_t nreg = sizeof(reg) / sizeof(reg[0]);
    for (size_t i = 0; i < nreg; ++i) {
      CHECK(reg[i].off % 4 == 0, "n %u max %u: %s at %llu", n, max_in_len, reg[i].name, (unsigned long long)reg[i].off);
      const u64 next = i + 1 < nreg ? reg[i + 1].off : (u64)ws;
      CHECK(reg[i].off + reg[i].bytes <= next, "n %u max %u ws %zu: %s [%llu, +%llu) runs past %llu", n, max_in_len, ws,
            reg[i].name, (unsigned long long)reg[i].off, (unsigned long long)reg[i].bytes, (unsigned long long)next);
    }
    CHECK(p.items_off == p.tables_bytes, "n %u max %u", n, max_in_len);
    CHECK(p.plan_pass.block == 256 && p.plan_pass.grid >= 1 && (u64)p.plan_pass.grid * 256 >= n, "n %u", n);
  } else {
    CHECK(p.wave_min == 0 && !p.fallback, "n %u max %u ws %zu", n, max_in_len, ws);
  }
  // the lanes
  CHECK(p.lanes >= 64 && p.lanes <= p.slots && p.lanes % 64 == 0, "n %u max %u: %u lanes", n, max_in_len, p.lanes);
  CHECK(p.pipe.grid >= 1 && p.pipe.grid * 64 == p.lanes && p.pipe.block == 64 && p.pipe.lds == 0, "n %u", n);
  CHECK(p.split_pipe == (max_in_len > kBlockSize || max_in_len == 0), "max %u", max_in_len);
  CHECK(p.can_split == (max_in_len > kBlockSize), "max %u", max_in_len);
  CHECK(p.fallback == (p.planned && p.can_split), "n %u max %u", n, max_in_len);
  if (p.fallback) CHECK(p.gather.grid >= 1 && p.gather.block == 256, "n %u", n);
  // the wave encoder
  if (p.wave_min) {
    CHECK(p.wave_min <= max_in_len && (p.wave_min == kInputMarginBytes || p.wave_min >= kWaveMinBound), "n %u max %u: %u",
          n, max_in_len, p.wave_min);
    CHECK(p.wg >= 1 && p.wg <= kWaveEncMaxWaves && p.wave.block == 64 * p.wg, "n %u max %u", n, max_in_len);
    CHECK(p.ht == table_size_for(max_in_len > kBlockSize ? kBlockSize : max_in_len), "max %u", max_in_len);
    CHECK(p.wave.lds == p.wg * p.ht * 2 && p.wave.lds <= kCuLds, "n %u max %u: %u", n, max_in_len, p.wave.lds);
    CHECK(p.per_cu >= 1 && p.per_cu <= 32 && p.waves >= 1 && p.waves <= kEncCus * p.per_cu, "n %u max %u", n, max_in_len);
    CHECK(p.waves <= n * frags, "n %u max %u: %u waves", n, max_in_len, p.waves);
    CHECK(p.wave.grid >= 1 && (u64)p.wave.grid * p.wg >= p.waves && (u64)(p.wave.grid - 1) * p.wg < p.waves,
          "n %u max %u", n, max_in_len);
  } else {
    CHECK(p.wave.grid == 0 && p.waves == 0, "n %u max %u", n, max_in_len);
  }
}

static void test_layout() {
  for (u32 n : kNs)
    for (u32 max_in_len : kMaxes) {
      const size_t tables = encode_tables_workspace_bytes(n, max_in_len, nullptr);
      const size_t full = full_ws(n, max_in_len);
      CHECK(full >= tables, "n %u max %u", n, max_in_len);
      check_layout(n, max_in_len, full);
      check_layout(n, max_in_len, full + 4096);
      if (full > tables) check_layout(n, max_in_len, full - 1);  // no room for the plan region
      check_layout(n, max_in_len, tables);
      check_layout(n, max_in_len, tables - 1);  // the other route
    }
  CHECK(sizeof(LaunchDim) == 12, "LaunchDim");
}

static void test_options() {
  const u32 n = 2000, big = 65536;
  const size_t ws = full_ws(n, big);
  // ---- encode_wave_min: below 0 the default; non-zero below 4096 raised to
  // it; all-on-wave: kInputMarginBytes; above the bound, or no plan pass: 0
  struct WaveMin {
    i64 opt;
    u32 n, max_in_len, want;
  };
  const WaveMin wm[] = {
      {-1, n, big, 16384},      {0, n, big, 0},          {1, n, big, 4096},      {4095, n, big, 4096},
      {4096, n, big, 4096},     {4097, n, big, 4097},    {65536, n, big, 65536}, {65537, n, big, 0},
      {-1, n, 16384, 16384},    {-1, n, 16383, 0},       {1, n, 8193, 4096},     {1, n, 8192, kInputMarginBytes},
      {-1, n, 8192, kInputMarginBytes}, {0, n, 8192, 0}, {-1, 64, big, kInputMarginBytes}, {0, 64, big, 0},
      {-1, 65, big, 16384},     {-1, 64, 15, kInputMarginBytes}, {-1, 64, 14, 0}, {-1, n, 0, 0},
      {-1, n, 70000, 16384},    {0, n, 70000, 0},        {1ll << 32, n, big, 0},  // (u32) of the value
  };
  for (const WaveMin& w : wm) {
    EncodeOpts o;
    o.encode_wave_min = w.opt;
    const EncodePlan p = plan_of(w.n, w.max_in_len, full_ws(w.n, w.max_in_len), o);
    CHECK(p.wave_min == w.want, "wave_min %lld n %u max %u: %u", (long long)w.opt, w.n, w.max_in_len, p.wave_min);
    // the plan pass runs for the wave encoder or for split messages
    CHECK(p.planned == (w.want != 0 || w.max_in_len > kBlockSize), "wave_min %lld n %u max %u", (long long)w.opt, w.n,
          w.max_in_len);
    // and without the plan region nothing is listed
    const EncodePlan q = plan_of(w.n, w.max_in_len, encode_tables_workspace_bytes(w.n, w.max_in_len, nullptr), o);
    CHECK(q.route == kEncRouteMain && !q.planned && q.wave_min == 0 && !q.fallback,
          "wave_min %lld n %u max %u", (long long)w.opt, w.n, w.max_in_len);
  }
  // ---- max_in_len 0: whole 64 KiB tables, no plan region, the split instance
  {
    const EncodePlan p = plan_of(n, 0, full_ws(n, 0));
    CHECK(p.entries == kMaxHashTableSize && p.plan_bytes == 0 && !p.planned && p.split_pipe && !p.can_split && !p.fallback,
          "max_in_len 0");
    CHECK(!plan_of(n, 65536, ws).split_pipe && plan_of(n, 65537, full_ws(n, 65537)).split_pipe, "flat up to 64 KiB");
    CHECK(!plan_of(n, 1, full_ws(n, 1)).split_pipe, "flat");
  }
  // ---- encode_lanes: a cap rounded up to 64, only below the table slots;
  // any non-zero value turns the 3/4 rule off; tables sized for the slots
  {
    const EncodePlan d = plan_of(n, big, ws);
    CHECK(d.slots == 2048 && d.lanes == 1536 && d.wave_min, "3/4 of 2000, rounded up to 256: %u", d.lanes);
    struct Lanes {
      i64 opt;
      u32 want;
    };
    const Lanes ls[] = {{1, 64},      {64, 64},     {65, 128},           {1536, 1536},         {2047, 2048},
                        {2048, 2048}, {5000, 2048}, {-1, 2048},          {(1ll << 32) + 5, 64},  // (unsigned) of the value
                        {1ll << 32, 2048}};  // caps nothing, and is not 0: no 3/4 rule
    for (const Lanes& l : ls) {
      EncodeOpts o;
      o.encode_lanes = l.opt;
      const EncodePlan p = plan_of(n, big, ws, o);
      CHECK(p.lanes == l.want && p.pipe.grid == l.want / 64, "encode_lanes %lld: %u", (long long)l.opt, p.lanes);
      CHECK(p.slots == d.slots && p.tables_bytes == d.tables_bytes && p.items_off == d.items_off, "encode_lanes %lld",
            (long long)l.opt);
    }
    // the 3/4 rule: only beside the wave encoder, only above 64 messages
    EncodeOpts lanes_only;
    lanes_only.encode_wave_min = 0;
    CHECK(plan_of(n, big, ws, lanes_only).lanes == 2048, "no wave encoder: every slot");
    CHECK(plan_of(n, big, encode_tables_workspace_bytes(n, big, nullptr)).lanes == 2048, "no plan region: every slot");
    CHECK(plan_of(64, big, full_ws(64, big)).lanes == 256 && plan_of(65, big, full_ws(65, big)).lanes == 256, "small");
    CHECK(plan_of(1025, big, full_ws(1025, big)).lanes == 768 && plan_of(1025, big, full_ws(1025, big)).slots == 1280,
          "3/4 of 1025 is 768, a multiple of 256");
    CHECK(plan_of(1026, big, full_ws(1026, big)).lanes == 1024, "3/4 of 1026 is 769, rounded up to 256");
    CHECK(plan_of(1u << 20, big, full_ws(1u << 20, big)).lanes == 131072, "at most 131,072");
  }
  // ---- encode_wave_wg: 1..5, otherwise 1; at most the waves
  {
    struct Wg {
      i64 opt;
      u32 wg, per_cu, waves, grid;
    };
    // 32 KiB tables: four one-wave workgroups per CU, or one of five waves
    const Wg ws5[] = {{0, 1, 4, 1024, 1024}, {1, 1, 4, 1024, 1024}, {2, 2, 4, 1024, 512}, {3, 3, 3, 768, 256},
                      {4, 4, 4, 1024, 256},  {5, 5, 5, 1280, 256},  {6, 1, 4, 1024, 1024}, {-1, 1, 4, 1024, 1024}};
    for (const Wg& w : ws5) {
      EncodeOpts o;
      o.encode_wave_wg = w.opt;
      const EncodePlan p = plan_of(n, big, ws, o);
      CHECK(p.wg == w.wg && p.per_cu == w.per_cu && p.waves == w.waves && p.wave.grid == w.grid &&
                p.wave.block == 64 * w.wg && p.wave.lds == w.wg * 32768 && p.wave.lds <= kCuLds,
            "encode_wave_wg %lld: wg %u per_cu %u waves %u grid %u", (long long)w.opt, p.wg, p.per_cu, p.waves,
            p.wave.grid);
    }
    EncodeOpts o;
    o.encode_wave_wg = 5;
    const EncodePlan two = plan_of(2, big, full_ws(2, big), o);  // two units: two waves, one workgroup of two
    CHECK(two.waves == 2 && two.wg == 2 && two.wave.grid == 1 && two.wave.block == 128 && two.wave.lds == 65536, "wg > waves");
    // together with encode_wave_per_cu 1: 256 waves in workgroups of five
    o.encode_wave_per_cu = 1;
    const EncodePlan p = plan_of(n, big, ws, o);
    CHECK(p.wg == 5 && p.per_cu == 1 && p.waves == 256 && p.wave.grid == 52 && p.wave.block == 320, "wg 5 per_cu 1");
  }
  // ---- encode_wave_per_cu: in (0, per_cu), otherwise what the LDS holds (at most 32)
  {
    struct PerCu {
      i64 opt;
      u32 max_in_len, per_cu;
    };
    const PerCu pcs[] = {{0, big, 4},  {1, big, 1},   {3, big, 3},   {4, big, 4},   {33, big, 4},  {-1, big, 4},
                         {0, 4096, 18}, {17, 4096, 17}, {33, 4096, 18}, {0, 200, 32}, {31, 200, 31}, {33, 200, 32}};
    for (const PerCu& c : pcs) {
      EncodeOpts o;
      o.encode_wave_per_cu = c.opt;
      const u32 nn = 131072;
      const EncodePlan p = plan_of(nn, c.max_in_len, full_ws(nn, c.max_in_len), o);
      CHECK(p.wave_min && p.per_cu == c.per_cu && p.waves == 256 * c.per_cu && p.wave.grid == p.waves,
            "encode_wave_per_cu %lld max %u: %u", (long long)c.opt, c.max_in_len, p.per_cu);
    }
    // at most one wave per unit
    CHECK(plan_of(8, 4096, full_ws(8, 4096)).waves == 8 && plan_of(8, 4096, full_ws(8, 4096)).wave.grid == 8, "8 units");
    CHECK(plan_of(8, 70000, full_ws(8, 70000)).waves == 16, "8 bodies of two fragments");
  }
  // ---- share in 0..1000 (otherwise 475), MiB in [0, 2^24) (otherwise 640)
  for (i64 s : {(i64)-1, (i64)0, (i64)1, (i64)475, (i64)1000, (i64)1001, (i64)1 << 40}) {
    EncodeOpts o;
    o.encode_wave_share = s;
    CHECK(plan_of(n, big, ws, o).share_permille == (s >= 0 && s <= 1000 ? (u32)s : 475u), "share %lld", (long long)s);
  }
  for (i64 mb : {(i64)-1, (i64)0, (i64)1, (i64)640, (i64)(1 << 24) - 1, (i64)1 << 24, (i64)1 << 40}) {
    EncodeOpts o;
    o.encode_wave_all_mb = mb;
    CHECK(plan_of(n, big, ws, o).all_bytes == (mb >= 0 && mb < (1 << 24) ? (u64)mb : 640ull) << 20, "all_mb %lld",
          (long long)mb);
  }
  // ---- the route: a forced variant 1, else the workspace; the report's
  // "has a workspace" is ws_bytes != 0, the batch call's a pointer
  {
    const size_t tables = encode_tables_workspace_bytes(n, big, nullptr);
    const EncodeOpts o;
    CHECK(encode_v3_plan(n, big, ws, true, 0, 0, o).route == kEncRouteMain, "main");
    CHECK(encode_v3_plan(n, big, tables, true, 0, 0, o).route == kEncRouteMain, "tables alone");
    CHECK(encode_v3_plan(n, big, tables - 1, true, 0, 0, o).route == kEncRouteNoWorkspace, "too small");
    CHECK(encode_v3_plan(n, big, 0, false, 0, 0, o).route == kEncRouteNoWorkspace, "none");
    CHECK(encode_v3_plan(n, big, ws, false, 0, 0, o).route == kEncRouteNoWorkspace, "no pointer");
    CHECK(encode_v3_plan(n, big, ws, true, 1, 0, o).route == kEncRouteForced, "forced");
    CHECK(encode_v3_plan(n, big, 0, false, 1, 0, o).route == kEncRouteForced, "forced, no workspace");
    CHECK(encode_v3_plan(n, big, ws, true, 3, 0, o).route == kEncRouteMain, "variant 3 is the main route");
    const EncodePlan off = encode_v3_plan(n, big, tables - 1, true, 0, 4096, o);
    CHECK(!off.planned && !off.wave_min && off.lanes == 0 && off.tables_bytes == tables && off.slots == 2048,
          "only the sizes off the main route");
    CHECK(encode_v3_plan(n, big, ws, true, 0, 4096, o).region_cap == 4096 && plan_of(n, big, ws).region_cap == 0,
          "region cap passes through");
    CHECK(encode_v3_plan(0, big, full_ws(0, big), true, 0, 0, o).route == kEncRouteMain, "an empty batch");
  }
  // wave_quota_of with the plan's parameters: all units under the bound, else the share
  {
    const EncodePlan p = plan_of(n, big, ws);
    CHECK(wave_quota_of(1000, p.all_bytes, p.share_permille, p.all_bytes) == 1000, "all");
    CHECK(wave_quota_of(1000, p.all_bytes + 1, p.share_permille, p.all_bytes) == 475, "share");
    CHECK(wave_quota_of(3, p.all_bytes + 1, p.share_permille, p.all_bytes) == 2, "rounded up");
  }
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
