// encode_v3_plan.h -- Snappy encode (snappy_encode_v3.hip, snappy_encode_wave.hip):
// the workspace layout and everything one fsg_compress_batch call decides
// before its first launch, as plain host arithmetic.  fsg_compress_report
// reads the same struct.  No HIP include: tests/cpp/test_encode_plan.cc
// checks it on the CPU.  The format constants and wave_quota_of are also what
// the kernels see (snappy_device.h includes this header; ENC_HD is
// __host__ __device__ there).  DESIGN.md section 4, "Encode".
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "decode_v4_plan.h"  // the integer typedefs, LaunchDim

#if defined(__HIPCC__)
#define ENC_HD __host__ __device__ inline
#else
#define ENC_HD inline
#endif

namespace fsg {

// ---- format constants (the reference's vendored Snappy 1.1.3)
constexpr u32 kBlockLog = 16;                    // snappy.h:201
constexpr u32 kBlockSize = 1u << kBlockLog;      // snappy.h:202
constexpr u32 kMaxHashTableBits = 14;            // snappy.h:204
constexpr u32 kMaxHashTableSize = 1u << kMaxHashTableBits;  // snappy.h:205
constexpr u32 kInputMarginBytes = 15;            // snappy.cc:346

// WorkingMemory::GetHashTable sizing, snappy.cc:247-271.
ENC_HD u32 table_size_for(u32 frag_len) {
  u32 ht = 256;
  while (ht < kMaxHashTableSize && ht < frag_len) ht <<= 1;
  return ht;
}

// ---- encode work units (encode_plan_kernel's long list)
constexpr u32 kWaveEncMaxWaves = 5;      // waves per encode_wave_kernel workgroup (at most)

// Units [0, quota) of the long list go to the wave encoder, the rest to the
// lane encoder.  All of them when their bytes fit what the wave encoder does
// in about the time one lane needs for a 64 KiB fragment at full load (the
// lane path's floor: a lane taking a long unit late sets the batch's tail;
// measured on MI355X: one lane ~40 ms per 64 KiB fragment); otherwise the
// wave encoder's share of a bandwidth-bound batch (0.5 since round 5: the
// wave encoder alone does C3 in ~165 ms, the lanes in ~135 ms, and a sweep
// of 280 / 400 / 500 / 600 permille measured 97-101 / 94 / 87 / 101 ms).
// Both kernels compute it from the plan pass's counters.
// (wave_quota_of: the formula on plain values, which the path report
// evaluates on the host from a copy of the counters.)
ENC_HD __attribute__((always_inline)) u32 wave_quota_of(u32 n_long, u64 bytes, u32 share_permille, u64 all_bytes) {
  if (bytes <= all_bytes) return n_long;
  const u64 q = ((u64)n_long * share_permille + 999) / 1000;
  return q < n_long ? (u32)q : n_long;
}

// ---- the lane encoder's tables
// Table entries carry a 16-bit fingerprint of the 4 bytes at the stored
// position (high half; the position is the low half).  A probe whose
// fingerprint differs from its candidate's cannot match, so it skips the
// candidate load: about half of the probes fail, and their candidate lines
// were a quarter of the fetched bytes.  A fingerprint hit is confirmed by
// the loaded bytes as before, so the parse is unchanged (FSG_V3_FP=0: the
// reference's u16 position-only entries).
#ifndef FSG_V3_FP
#define FSG_V3_FP 1
#endif
constexpr u32 kEncEntryBytes = FSG_V3_FP ? 4 : 2;  // sizeof(tent), snappy_encode_v3.hip

// Plan region: present when a message may be split (max_in_len > 64 KiB) or
// may be long enough for the wave encoder (>= kWaveMinBound).  (max_in_len
// 0 = unknown: no plan, every message encoded whole by one lane.)
constexpr u32 kWaveMinBound = 4096;  // smallest wave_min the plan region is sized for
constexpr u32 kSmallBatchEnc = 64;   // batches of at most this many messages: every message on the wave encoder
// Batches of short bodies only (at most this many bytes each): every message
// on the wave encoder too.  Their tables are small (8 KiB for 4 KiB bodies),
// so many waves fit per CU, and nothing else in the batch needs the LDS:
// 131,072 x 4 KiB text 19.1 -> 8.6 ms, 65,536 x 8 KiB 18.5 -> 11.4 ms
// against the lanes.
#ifndef FSG_ENC_ALL_WAVE_MAX
#define FSG_ENC_ALL_WAVE_MAX 8192
#endif
constexpr u32 kAllWaveMax = FSG_ENC_ALL_WAVE_MAX;
inline bool all_on_wave(u32 n_msgs, u32 max_in_len) {
  return max_in_len >= kInputMarginBytes && (n_msgs <= kSmallBatchEnc || max_in_len <= kAllWaveMax);
}

// ---- the chip, as the launch sees it
constexpr u32 kEncCus = 256;
// LDS is allocated per workgroup in 1,280-byte granules out of 163,840 per CU
// (profiles/r5/wenc/lds_resident_probe.txt: one-wave workgroups of
// 31,744 B fit five per CU, of 32,256 B four), so five 32 KiB tables fit
// only as one five-wave workgroup.
constexpr u32 kCuLds = 160u * 1024u, kLdsGranule = 1280u;
// enough lanes to fill the chip several times over: 256 CUs x 16 waves x 64
constexpr u32 kEncMaxSlots = 262144u;
// Lanes in flight beside the wave encoder (decided once it is known
// to run): 3/4 of the messages, at most 131,072.  The lanes' waves share
// the SIMDs with the wave encoder's waves, whose serial chains set the
// batch's time, and fewer lanes keep their tables and recent input
// cache-resident, each encoding more messages.  Measured (A/B, one box): C5
// 27.0 -> 18.8 ms (131,072 of 262,144; 98,304: 20.8, 196,608: 22.4), C3
// 92.3 -> 85.4 ms (49,152 of 65,536; 32,768: 85.3).  Option encode_lanes
// (a cap) replaces this rule.
constexpr u32 kLanesBesideMax = 131072u;
constexpr u32 kLanesBesideNum = 3, kLanesBesideDen = 4;

// ---- workspace layout (bytes from the start):
//   [0, 256)  counters (u32 ctr[], zeroed by the launch's one fill), at the
//             kEncCtr* slots below
//   then the lanes' tables: slots x entries x kEncEntryBytes
//     (entries per WorkingMemory::GetHashTable, snappy.cc:247-271, for the
//     largest fragment of the batch)
//   then the plan region, when present (encode_plan_bytes):
//     items[2 x max_items] (message, fragment or kWholeUnit) |
//     sizes[max_items] | frag_base[n] (a message's first unit) |
//     big_list[n] (the split messages) | 256 spare bytes
constexpr u32 kEncCtrLaneNext = 0;      // the lanes' work counter
constexpr u32 kEncCtrUnits = 1;         // units listed by encode_plan_kernel
constexpr u32 kEncCtrSplit = 2;         // split messages
constexpr u32 kEncCtrFallbackNext = 4;  // the fallback pass's work counter
constexpr u32 kEncCtrWaveNext = 5;      // the wave encoder's work counter
constexpr u32 kEncCtrUnitBytes = 6;     // u64 (slots 6-7): bytes of the listed units
// Path report (fsg_compress_report): the split messages handed to the
// whole-message fallback pass, counted where they are marked.
constexpr u32 kEncCtrFallback = 8;
constexpr u32 kEncCounterBytes = 256;
// the counters are distinct u32 slots inside the 256-byte header
constexpr u32 kEncCtrSlots[] = {kEncCtrLaneNext, kEncCtrUnits, kEncCtrSplit, kEncCtrFallbackNext, kEncCtrWaveNext,
                                kEncCtrUnitBytes, kEncCtrUnitBytes + 1, kEncCtrFallback};
constexpr bool enc_ctr_slots_ok() {
  for (u32 i = 0; i < sizeof(kEncCtrSlots) / sizeof(kEncCtrSlots[0]); ++i) {
    if (4 * kEncCtrSlots[i] + 4 > kEncCounterBytes) return false;
    for (u32 j = 0; j < i; ++j)
      if (kEncCtrSlots[i] == kEncCtrSlots[j]) return false;
  }
  return kEncCtrUnitBytes % 2 == 0;  // one aligned 64-bit atomic
}
static_assert(enc_ctr_slots_ok(), "encode counters overlap or leave the header");

// Per-lane hash tables for the lane-per-message encoder: [counter: 256 B]
// [tables: slots x entries x sizeof(tent)] (tent = u32 with FSG_V3_FP, the
// default: position + fingerprint, twice the u16 footprint), entries per WorkingMemory::GetHashTable
// (snappy.cc:247-271) for the largest fragment of the batch.
inline size_t encode_tables_workspace_bytes(u32 n_msgs, u32 max_in_len, u32* slots_out) {
  u32 cap = max_in_len == 0 || max_in_len > kBlockSize ? kBlockSize : max_in_len;
  const u32 entries = table_size_for(cap);
  u32 slots = n_msgs < kEncMaxSlots ? n_msgs : kEncMaxSlots;
  slots = (slots + 255) / 256 * 256;
  if (slots == 0) slots = 256;
  if (slots_out) *slots_out = slots;
  return kEncCounterBytes + (size_t)slots * entries * kEncEntryBytes;
}

// Plan region: units (2 x u32 each: message, fragment or kWholeUnit), per-unit
// sizes, per-message first unit, split-message list.
inline size_t encode_plan_bytes(u32 n_msgs, u32 max_in_len) {
  if (max_in_len < kWaveMinBound && !all_on_wave(n_msgs, max_in_len)) return 0;
  u64 per_msg = ((u64)max_in_len + kBlockSize - 1) >> kBlockLog;
  if (per_msg < 1) per_msg = 1;
  const u64 max_items = (u64)n_msgs * per_msg;
  return (size_t)(max_items * 12 + (u64)n_msgs * 8 + 256);
}

// The encode options (csrc/options.h, indices 14-19) as one call sees them:
// read_encode_opts (snappy_encode_v3.hip) fills this once from opt().  The
// initialisers are the option table's defaults (capi.hip checks that they
// agree).
struct EncodeOpts {
  i64 encode_wave_min = 16384;
  i64 encode_wave_share = 475;
  i64 encode_wave_all_mb = 640;
  i64 encode_lanes = 0;
  i64 encode_wave_per_cu = 0;
  i64 encode_wave_wg = 1;
};

// fsg_compress_batch's routes (the values of FSG_PATH_MAIN, _NO_WORKSPACE and
// _FORCED, include/flare_snappy_gpu.h; capi.hip checks that they agree).
// Main = the lane-per-message encoder with global-memory tables (v3: batched
// speculative probes), when the workspace holds them; otherwise the
// wave-per-message LDS-table encoder (v1).
enum EncodeRoute : int { kEncRouteMain = 0, kEncRouteNoWorkspace = 2, kEncRouteForced = 3 };

// What one fsg_compress_batch call computes before its first launch.  Offsets
// are bytes from the workspace's start.  Everything after `entries` is set on
// the main route only.
struct EncodePlan {
  EncodeRoute route;
  // ---- workspace
  u64 tables_bytes;  // counters + tables: what the main route needs
  u64 plan_bytes;    // the plan region (0: none for this batch)
  u32 slots;         // tables in the workspace
  u32 entries;       //   entries of each
  u64 max_items;     // units the plan region holds
  u64 items_off, sizes_off, frag_base_off, big_list_off;  // valid when planned
  // ---- decisions
  bool planned;     // encode_plan_kernel runs, the encoders read its list
  bool can_split;   // a message may have several fragments
  bool split_pipe;  // encode_pipe_kernel with the split batches' probe counts
  bool fallback;    // encode_gather_kernel and the fallback pass run
  u32 wave_min;     // units of at least this many bytes are listed for the wave encoder (0: it does not run)
  u32 lanes;        // lanes launched (<= slots, a multiple of 64)
  u32 share_permille;  // wave_quota_of's parameters
  u64 all_bytes;
  u32 region_cap;   // test knob, passed through (split_region, snappy_device.h)
  // ---- launches
  LaunchDim plan_pass;  // encode_plan_kernel
  LaunchDim pipe;       // encode_pipe_kernel, both passes
  LaunchDim wave;       // encode_wave_kernel (wave_min != 0)
  LaunchDim gather;     // encode_gather_kernel
  u32 wg, per_cu, waves, ht;  // the wave encoder: waves per workgroup and per CU, waves in all, table entries
};

// have_ws: the caller has a workspace of ws_bytes (the batch call: the
// pointer is not null; the report: ws_bytes != 0).  forced_variant: the
// encode variant of fsg_select_kernels (0 automatic).
inline EncodePlan encode_v3_plan(u32 n_msgs, u32 max_in_len, size_t ws_bytes, bool have_ws, int forced_variant,
                                 u32 region_cap, const EncodeOpts& o) {
  EncodePlan p{};
  p.tables_bytes = encode_tables_workspace_bytes(n_msgs, max_in_len, &p.slots);
  p.plan_bytes = encode_plan_bytes(n_msgs, max_in_len);
  const u32 cap = max_in_len == 0 || max_in_len > kBlockSize ? kBlockSize : max_in_len;
  p.entries = table_size_for(cap);
  p.route = forced_variant == 1 ? kEncRouteForced
            : have_ws && ws_bytes >= p.tables_bytes ? kEncRouteMain
                                                    : kEncRouteNoWorkspace;
  if (p.route != kEncRouteMain) return p;
  p.region_cap = region_cap;
  p.can_split = max_in_len > kBlockSize;
  // Messages of at least wave_min bytes (and every fragment of a message over
  // 64 KiB) form the long list, whose units the wave encoder (hash table in
  // LDS, one wave per fragment) and the lane encoder share (wave_quota); the
  // shorter messages go to the lane encoder.  Option encode_wave_min
  // (FSG_ENCODE_WAVE_MIN; 0 = lane encoder only).  Measured on MI355X (A/B, one box): C3
  // compress 108.0 -> 98.4 ms, C5 54.9 -> 39.1 ms.
  u32 wave_min = o.encode_wave_min >= 0 ? (u32)o.encode_wave_min : 16384u;
  if (wave_min && wave_min < kWaveMinBound) wave_min = kWaveMinBound;
  // A batch of at most one wave of messages (the host runtime's one-caller
  // batches: the wave encoder's latency for one message is a fraction of one
  // lane's, 4 KiB text ~0.2 ms against 1.1 ms in the C1 echo trace), or of
  // short bodies only (kAllWaveMax): every message on the wave encoder
  if (wave_min && all_on_wave(n_msgs, max_in_len)) wave_min = kInputMarginBytes;
  if (max_in_len < wave_min) wave_min = 0;  // nothing long enough (or no bound known)
  p.planned = p.plan_bytes && ws_bytes >= p.tables_bytes + p.plan_bytes && (p.can_split || wave_min);
  p.wave_min = p.planned ? wave_min : 0u;
  if (p.planned) {
    p.max_items = (p.plan_bytes - 256 - (u64)n_msgs * 8) / 12;
    p.items_off = p.tables_bytes;
    p.sizes_off = p.items_off + 8 * p.max_items;
    p.frag_base_off = p.sizes_off + 4 * p.max_items;
    p.big_list_off = p.frag_base_off + 4ull * n_msgs;
  }
  p.plan_pass = LaunchDim{(n_msgs + 255) / 256, 256u, 0u};
  // Lanes in flight: option encode_lanes caps them (the tables stay sized for
  // `slots`); otherwise the rule beside the wave encoder (kLanesBesideMax),
  // once the wave encoder is known to run.
  p.lanes = p.slots;
  const unsigned lanes_cap = (unsigned)o.encode_lanes;
  if (lanes_cap && lanes_cap < p.lanes) p.lanes = (lanes_cap + 63) / 64 * 64;
  if (p.wave_min && n_msgs > 64 && o.encode_lanes == 0) {
    u32 beside = (u32)(((u64)n_msgs * kLanesBesideNum / kLanesBesideDen + 255) / 256 * 256);
    if (beside > kLanesBesideMax) beside = kLanesBesideMax;
    if (beside < p.lanes) p.lanes = beside;
  }
  p.pipe = LaunchDim{p.lanes / 64, 64u, 0u};
  // (options encode_wave_share / encode_wave_all_mb: the tests force the lane
  // share with encode_wave_all_mb 0).  The wave encoder's share of the long
  // units' bytes above the all-on-wave bound, in permille: C3, A/B on one box
  // (profiles/r6/enc/ab_c3_share_sweep*.log), 400 86.3-86.9 ms, 425 80.8-81.0,
  // 450 80.4-80.6, 475 80.2-80.3, 500 82.4-82.6, 550 89.6-90.1.
  const i64 share_opt = o.encode_wave_share, all_opt = o.encode_wave_all_mb;
  p.share_permille = share_opt >= 0 && share_opt <= 1000 ? (u32)share_opt : 475u;
  p.all_bytes = (all_opt >= 0 && all_opt < (1 << 24) ? (u64)all_opt : 640ull) << 20;
  p.split_pipe = max_in_len > kBlockSize || max_in_len == 0;
  // The wave encoder's share of the long units (hash table in LDS, one wave
  // per fragment: snappy_encode_wave.hip) runs on a side stream beside the
  // lanes, one wave per table's worth of LDS.
  if (p.wave_min) {
    const u32 wcap = max_in_len > kBlockSize ? kBlockSize : max_in_len;
    const u32 ht = table_size_for(wcap), lds = ht * 2;
    // Workgroups of wg waves, one table each in the workgroup's LDS (kCuLds,
    // kLdsGranule).
    // Waves per workgroup (option encode_wave_wg, 1..5; default 1).  Five
    // 32 KiB tables fit per CU only as one five-wave workgroup, which takes
    // the CU's whole LDS: C3 with every unit on the wave encoder 159 -> 132
    // ms, but beside the lanes (whose 80-byte LDS windows then find no room)
    // C3 gained <= 1% and C5 lost 12% with the lanes' windows moved to
    // registers, and batches of short bodies alone lost 33-60% (DESIGN.md
    // section 5, round 6).
    const i64 wg_opt = o.encode_wave_wg;
    u32 wg = wg_opt >= 1 && wg_opt <= (i64)kWaveEncMaxWaves ? (u32)wg_opt : 1u;
    while (wg > 1 && wg * lds > kCuLds) --wg;
    const u32 alloc = (wg * lds + kLdsGranule - 1) / kLdsGranule * kLdsGranule;
    u32 per_cu = (kCuLds / alloc) * wg;
    if (per_cu > 32) per_cu = 32;  // waves per CU
    const i64 pc_opt = o.encode_wave_per_cu;
    if (pc_opt > 0 && (u64)pc_opt < per_cu) per_cu = (u32)pc_opt;
    u32 waves = kEncCus * (per_cu ? per_cu : 1u);
    // A batch has at most n_msgs x fragments units; the waves past them find
    // no unit but are still dispatched (one 4 KiB body: 5,120 waves of 8 KiB
    // tables, ~60 us in front of the lanes' launch).
    {
      const u64 units = (u64)n_msgs * (((u64)max_in_len + kBlockSize - 1) >> kBlockLog);
      if (units && units < waves) waves = (u32)units;
    }
    if (wg > waves) wg = waves;
    p.wg = wg;
    p.per_cu = per_cu;
    p.waves = waves;
    p.ht = ht;
    p.wave = LaunchDim{(waves + wg - 1) / wg, 64 * wg, wg * lds};
  }
  p.fallback = p.planned && p.can_split;
  p.gather = LaunchDim{1024u, 256u, 0u};
  return p;
}

}  // namespace fsg
