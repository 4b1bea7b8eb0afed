// decode_v4_plan.h -- two-pass Snappy decode (snappy_decode_v4.hip and the
// decode_v4_*.h of its passes): the
// workspace layout and everything launch_decode_v4 decides before its first
// launch, as plain host arithmetic.  No HIP include: tests/cpp/
// test_decode_plan.cc checks it on the CPU.  DESIGN.md section 4, "Decode".
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace fsg {

typedef uint8_t u8;  // (as snappy_device.h)
typedef uint32_t u32;
typedef uint64_t u64;
typedef int64_t i64;

// ---- pass 1 geometry
// Waves per pass-1 workgroup.  One: most resident waves for large batches
// (CM 15.1 ms vs 17.9 with four).  Four (82 KB of LDS: one workgroup per CU,
// one wave per SIMD) pins the placement and makes the pass insensitive to the
// launches before it (launch-order effect); C3 the same
// either way (7.81 vs 7.84 ms).
#ifndef FSG_IDX_WAVES
#define FSG_IDX_WAVES 1
#endif
constexpr u32 kIdxWaves = FSG_IDX_WAVES;
static_assert(kIdxWaves == 1 || kIdxWaves == 2 || kIdxWaves == 4, "tag table init");
// The one-stream lane walk of batches of short bodies (mean compressed size
// < 16 KiB, e.g. C2) runs four waves per workgroup so its bitmap allocation
// takes one device-scope atomic per workgroup instead of one per wave: C2
// 0.1354 -> 0.1276 ms; with long walks (C3) the one-wave blocks stay ahead
// (6.02 vs 6.06 ms).
#ifndef FSG_IDX_WAVES_SERIAL
#define FSG_IDX_WAVES_SERIAL 4
#endif
constexpr u32 kIdxWavesSerial = FSG_IDX_WAVES_SERIAL;
static_assert(kIdxWavesSerial == 1 || kIdxWavesSerial == 2 || kIdxWavesSerial == 4, "tag table init");
// Size classes of the planned lane walk (see index_plan_kernel,
// decode_v4_index.h).
constexpr u32 kWalkClasses = 16;
constexpr u32 kPlanThreads = 1024;

// ---- pass 1b (index_big_message, decode_v4_index_big.h) geometry
constexpr u32 kBigIndexMin = 8 * 1024;       // large: compressed size above
constexpr u32 kBigIndexMax = 48 * 1024;      // clamp(4 x the batch mean, min, max)
#ifndef FSG_HUGE_KB
#define FSG_HUGE_KB 256
#endif
constexpr u32 kHugeIndexBytes = FSG_HUGE_KB * 1024;  // large ones handed out first (forked: chunked walk)
// chunked pass 1b (chunk_*_kernel, decode_v4_chunked.h)
constexpr u32 kChunkBytes = 32 * 1024;  // a multiple of 512: chunks own whole bitmap words
struct ChunkRec {
  u32 m, k, exit, bad, len, base, flags, nchunks;
};

// ---- pass 2 geometry
constexpr u32 kWavesPerBlock = 4;
// bm_base[m] with this bit set: the message is one literal starting at the
// low bits (set by pass 1; bitmap bases stay below 2^31 words)
constexpr u32 kSingleLiteral = 0x80000000u;
// A/B knobs of the execution pass
// The software-pipelined execution pass (exec6_message; A/B variant).
// Window and kept history: 3 KiB / 1 KiB at 7 waves per SIMD (C3 6.35 ->
// 6.20 ms against 4 KiB / 2 KiB at 6 waves, A/B on one box; 4 KiB / 1 KiB
// at 6 waves 6.33, a 256-entry tag ring 7.04).
#ifndef FSG_WINDOW
#define FSG_WINDOW 3072
#define FSG_KEEP 1024
#endif
constexpr u32 kWindow = FSG_WINDOW;  // LDS output window per wave
constexpr u32 kKeep = FSG_KEEP;      // history kept when the window slides
// After a slide op - sbase <= keep + 15; a group adds <= 16 * kMaxPieces
// (decode_v4_exec_common.h) bytes and an OR store writes up to 20 bytes past
// a piece's start, all of which must stay inside the window's kWindow + 32
// bytes.
constexpr u32 kMaxKeep = (kWindow - 16 * 64 - 48) & ~15u;
static_assert(kKeep <= kMaxKeep, "kept history leaves room for one group");
// exec_kernel<5>'s folded instance (whole bodies of at most big_threshold
// compressed bytes, one wave each; decode_v4_exec5.h): its tag positions fit
// 16 bits (big_threshold <= kBigIndexMax), so its ring takes half the bytes of
// the general instance's and its window the KiB that frees -- the same LDS
// per wave.  Kept history (C3, A/B on one box, DESIGN.md section 5,
// "Execution pass: folded instance"): 1,024 5.635 ms, 1,536 5.585, 2,048
// 5.579, 3,024 (the largest) 5.636; the parent's 3 KiB window 5.759.
constexpr u32 kExecRing = 512;  // tag positions per wave (= kTagRing, decode_v4_exec_common.h)
static_assert(kBigIndexMax < 65536, "the folded instance's ring entries are 16 bits");
constexpr u32 kWindowWhole = kWindow + 2 * kExecRing;
#ifndef FSG_KEEP_WHOLE
#define FSG_KEEP_WHOLE 2048
#endif
constexpr u32 kKeepWhole = FSG_KEEP_WHOLE;
constexpr u32 kMaxKeepWhole = (kWindowWhole - 16 * 64 - 48) & ~15u;
static_assert(kKeepWhole <= kMaxKeepWhole && kKeepWhole % 16 == 0, "kept history leaves room for one group");
// LDS per wave of exec_kernel and exec_packed_kernel: ring, window and the 32
// bytes an OR store may write past it -- either instance.
constexpr u32 exec_wave_lds_bytes(bool whole) {
  return (whole ? 2 * kExecRing + kWindowWhole : 4 * kExecRing + kWindow) + 32;
}
static_assert(exec_wave_lds_bytes(true) == exec_wave_lds_bytes(false), "one LDS carve-up per wave");
// Path report: the packed pass counts the bodies it hands to pass 3 in the
// workspace header, at these u32 slots after its batch counter (kWsPackNext).
constexpr u32 kPackCtrWide = 3, kPackCtrGuard = 4;

// Workspace layout (bytes from the start; every counter a u32, zeroed by the
// launch's one fill together with the lists):
//   [0, 256)  counters, at the kWs* offsets below
//   then kListBases arrays of base_bytes = round_up(4 n, 256) bytes each:
//     0 bm_base[n] | 1 big_list[n] | 2-3 seg_list[n] (u64) | 4 whole_list[n] |
//     5 walk_rank[n] | 6 walk_perm[n] | 7 walk_hist (16 classes + count) |
//     8-9 seg_list2[n] (u64) | 10 whole_list2[n]
//   then the tag-start bitmap words.
// Set 0 = every large message (one stream) or the non-huge ones (forked);
// set 1 = the huge ones (forked, second side stream).
constexpr u32 kWsBmCounter = 0;        // bitmap bump allocator
constexpr u32 kWsSet1BigNext = 16;     // set 1: pass-1b work counter
constexpr u32 kWsSet1SegCount = 32;    // set 1: segment count
constexpr u32 kWsSet1WholeCount = 48;  // set 1: whole-message count
constexpr u32 kWsBigCount = 64;        // large-message count (huge count at +32: big_count + 8)
constexpr u32 kWsHugeCount = kWsBigCount + 32;
constexpr u32 kWsSet0BigNext = 128;
constexpr u32 kWsSet0SegCount = 160;
constexpr u32 kWsSet0ExecNext = 192;   // pass-2 queue head
constexpr u32 kWsSet0WholeCount = 224;
constexpr u32 kWsSet1ExecNext = 240;
constexpr u32 kWsChunkCount = 80;      // chunked pass 1b: records listed
constexpr u32 kWsChunkSpecNext = 84;   //   work counters of its passes
constexpr u32 kWsChunkFixNext = 88;
constexpr u32 kWsChunkCheckNext = 92;
constexpr u32 kWsChunkFinalNext = 100;
constexpr u32 kWsPackNext = 104;      // packed execution: batch counter
// path report (fsg_decompress_report): pass 3's message count, then its
// causes -- bitmap overflow (counted by pass 3), the packed pass's 32-bit
// offset check and its iteration guard (counted where the packed pass marks)
constexpr u32 kWsFallbackCount = 108;
constexpr u32 kWsFallbackBitmap = 112;
constexpr u32 kWsFallbackWide = kWsPackNext + 4 * kPackCtrWide;
constexpr u32 kWsFallbackGuard = kWsPackNext + 4 * kPackCtrGuard;
static_assert(kWsFallbackBitmap == kWsFallbackCount + 4, "fallback_kernel counts at fb_count[0..1]");
constexpr u32 kWsCounterBytes = 256;
// the counters are distinct u32 slots inside the 256-byte header
constexpr u32 kWsOffsets[] = {kWsBmCounter, kWsSet1BigNext, kWsSet1SegCount, kWsSet1WholeCount, kWsBigCount,
                              kWsHugeCount, kWsSet0BigNext, kWsSet0SegCount, kWsSet0ExecNext, kWsSet0WholeCount,
                              kWsSet1ExecNext, kWsChunkCount, kWsChunkSpecNext, kWsChunkFixNext,
                              kWsChunkCheckNext, kWsChunkFinalNext, kWsPackNext, kWsFallbackCount,
                              kWsFallbackBitmap, kWsFallbackWide, kWsFallbackGuard};
constexpr bool ws_offsets_ok() {
  for (u32 i = 0; i < sizeof(kWsOffsets) / sizeof(kWsOffsets[0]); ++i) {
    if (kWsOffsets[i] % 4 || kWsOffsets[i] + 4 > kWsCounterBytes) return false;
    for (u32 j = 0; j < i; ++j)
      if (kWsOffsets[i] < kWsOffsets[j] + 4 && kWsOffsets[j] < kWsOffsets[i] + 4) return false;
  }
  return true;
}
static_assert(ws_offsets_ok(), "workspace counters overlap or leave the header");
constexpr u64 kListBases = 11;  // u32 arrays of n entries before the bitmap
// The chunked pass 1b's records live at the workspace's end: 1/64 of it
// (>= 40 bytes per 20 KiB of input: one 32-byte record per 32 KiB chunk plus
// two words per huge message).
constexpr u64 kChunkRegionDiv = 64;
inline size_t decode_v4_workspace_bytes(u32 n_msgs, u64 total_in_bytes) {
  const u64 base_bytes = (4ull * n_msgs + 255) & ~255ull;
  const u64 words = total_in_bytes / 32 + 4ull * n_msgs + 64;
  const u64 base = 256 + kListBases * base_bytes + 4 * words;
  return (size_t)(base + base / (kChunkRegionDiv - 1) + 512);
}

// The tag-start bitmap's capacity in words: what the fixed part and the chunk
// records (at the end, 256-byte aligned whatever ws_bytes: the passes load
// them with scalar loads, which ignore the low address bits) leave.  Shared by
// the launch and the path report.  ws_bytes >= decode_v4_workspace_bytes(n, 0).
inline u64 decode_v4_bitmap_capacity_words(u32 n_msgs, size_t ws_bytes) {
  const u64 base_bytes = (4ull * n_msgs + 255) & ~255ull;
  const u64 chunk_bytes = (ws_bytes / kChunkRegionDiv) & ~255ull;
  const u64 chunk_off = (ws_bytes - chunk_bytes) & ~255ull;
  u64 cap_words = (chunk_off - 256 - kListBases * base_bytes) / 4;
  if (cap_words >= kSingleLiteral) cap_words = kSingleLiteral - 1;  // bases < 2^31 words
  return cap_words;
}

// Dynamic LDS of the lean lane walk: per wave an 8-chunk input ring (+5
// dwords) and 2 bit groups, [dword][lane] (64 lanes); the 256-entry tag table.
constexpr size_t idx_lean_lds_bytes() { return 4 * (kIdxWaves * (8 * 4 + 5 + 8) * 64 + 256); }

// The decode options (csrc/options.h, the first 14) as one call sees them:
// the launch fills this once from opt().  The initialisers are the option
// table's defaults (capi.hip checks that they agree).
struct DecodeOpts {
  i64 decode_fork = -1;
  i64 split_walk = 3;
  i64 split_class = 4;
  i64 exec_keep = -1;
  i64 chunked_huge = 1;
  i64 small_persist = 3584;
  i64 small_batch = 64;
  i64 split_huge = 1;
  i64 walk_order = 1;
  i64 lean_walk = 1;
  i64 exec_big_blocks = 512;
  i64 exec_prio = 1;
  i64 exec_big_blocks_fork = 1024;
  i64 exec_pack = 32;
};

// One launch geometry: <<<grid, block, lds>>>.
struct LaunchDim {
  u32 grid, block, lds;
};
// The index_kernel instance of the lane walk.
enum WalkKind : int {
  kWalkPlanned,   // index_kernel<true>: after index_plan_kernel (forked path)
  kWalkLean,      // index_kernel<false, true>: the two-stream form
  kWalkSerial,    // index_kernel<false, false, kIdxWavesSerial>: batches of short bodies
  kWalkStandard,  // index_kernel<false>
};

// What launch_decode_v4 computes before its first launch.  Offsets are bytes
// from the workspace's start.
struct DecodePlan {
  // ---- workspace regions (the layout above)
  u64 base_bytes;  // one list
  u64 bm_base_off, big_list_off, seg_list_off, whole_list_off, walk_rank_off, walk_perm_off, walk_hist_off,
      seg_list2_off, whole_list2_off;
  u64 bitmap_off;  // = the bytes the launch's fill zeroes (counters and lists)
  u64 cap_words;   // bitmap capacity
  // chunk records (chunked pass 1b) at the end, the bitmap before them
  u64 chunk_off, chunk_bytes;
  u64 first_rec_off, mstat_off, recs_off;  // u32[max_huge], u32[max_huge], ChunkRec[max_recs]
  u64 max_huge, max_recs;
  bool chunked;  // the huge messages' pass 1b runs chunked
  // ---- thresholds
  u64 est_total_in;   // the batch's compressed bytes, estimated from the workspace
  u32 big_threshold;  // compressed size above which a message takes pass 1b
  // ---- options, range-checked
  bool split_huge, walk_order, fork;
  u32 split_mode, split_class, prio, keep_hist, keep_hist_whole, pack_batch;
  // ---- launches
  WalkKind walk_kind;      // the lane walk without a plan pass (one stream, two-stream form)
  LaunchDim walk;          //   its launch
  LaunchDim planned_walk;  // index_kernel<true> (forked path)
  u32 plan_grid;           // index_plan_kernel, kPlanThreads threads
  u32 scatter_grid;        // walk_scatter_kernel, 256 threads
  u32 index_big_grid;      // index_big_kernel, 256 threads
  u32 small_blocks;        // exec blocks at one wave per message
  u32 big_blocks;          // one-stream exec launch: large-message blocks (grid: big_blocks + small_blocks)
  u32 fork_big_blocks;     // forked path: the large-message exec launches
  u32 small_grid;          // forked path: the small-message exec and packed launches
  u32 small_stride;        //   their persistent stride in blocks (0: one wave per message)
  u32 chunk_list_grid, chunk_rec_grid, chunk_msg_grid;  // chunk_list / spec, check / fixup, final
  u32 fallback_grid;       // fallback_kernel, 64 threads
};

// two_stream: pass 1 runs on a stream of its own (fsg_decompress_batch_2s
// with the per-device event set).  ws_bytes >= decode_v4_workspace_bytes(n_msgs, 0).
inline DecodePlan decode_v4_plan(u32 n_msgs, size_t ws_bytes, bool two_stream, const DecodeOpts& o) {
  DecodePlan p{};
  // planned lane walk in size-class order (FSG_WALK_ORDER=0 disables)
  p.split_huge = o.split_huge != 0;  // 0: one side stream
  p.walk_order = o.walk_order != 0;
  // Two-stream form: the lean lane walk (FSG_LEAN_WALK=0: the standard one).
  // Measured (C3, stream of two alternating batches, one box): lean 6.13 ms
  // per batch, standard 6.57, serial 6.15; an execution pass made persistent
  // at 5 or 6 blocks per CU to leave wave slots for the walk: 6.38 / 7.25
  // (the dispatcher does not spread a persistent grid evenly); the execution
  // pass held to six blocks per CU by padding its LDS, with a two-wave lean
  // walk in the space left: 6.32 vs serial 6.11 (the walk's instructions
  // compete with an execution pass already at the issue limit).
  const bool lean_walk = o.lean_walk != 0;
  const u64 base_bytes = (4ull * n_msgs + 255) & ~255ull;
  p.base_bytes = base_bytes;
  p.bm_base_off = 256;
  p.big_list_off = 256 + base_bytes;
  p.seg_list_off = 256 + 2 * base_bytes;
  p.whole_list_off = 256 + 4 * base_bytes;
  // the planned lane walk's order: ranks, the permutation, class counts and
  // offsets (+ the walk count)
  p.walk_rank_off = 256 + 5 * base_bytes;
  p.walk_perm_off = 256 + 6 * base_bytes;
  p.walk_hist_off = 256 + 7 * base_bytes;
  // the huge messages' pass-2 work lists (forked path, second side stream)
  p.seg_list2_off = 256 + 8 * base_bytes;
  p.whole_list2_off = 256 + 10 * base_bytes;
  p.bitmap_off = 256 + kListBases * base_bytes;
  // chunk records (chunked pass 1b) at the end, the bitmap before them
  // (decode_v4_bitmap_capacity_words)
  const u64 chunk_bytes = (ws_bytes / kChunkRegionDiv) & ~255ull;
  const u64 chunk_off = (ws_bytes - chunk_bytes) & ~255ull;
  p.chunk_bytes = chunk_bytes;
  p.chunk_off = chunk_off;
  const u64 cap_words = decode_v4_bitmap_capacity_words(n_msgs, ws_bytes);
  p.cap_words = cap_words;
  // Large-message threshold: 4x the batch's mean compressed size (estimated
  // from the workspace, which callers size from the packed input), clamped
  // to [8, 48] KiB.  The lane pass's time is its longest message; uniform
  // batches (C2, C3) send nothing to the wave pass.
  const u64 est_total_in = cap_words > 4ull * n_msgs + 64 ? (cap_words - 4ull * n_msgs - 64) * 32 : 0;
  p.est_total_in = est_total_in;
  u64 thr = 4 * est_total_in / n_msgs;
  thr = thr < kBigIndexMin ? kBigIndexMin : (thr > kBigIndexMax ? kBigIndexMax : thr);
  // A batch of at most one wave of messages (the host runtime's one-caller
  // batches): the lane walk would be one lane per message, its latency the
  // longest message's tag chain (~160 us for a 4 KiB text body), where pass
  // 1b walks each message with a whole wave (a few us).  Every message goes
  // to pass 1b (option small_batch sets the bound; 0 disables).
  if ((i64)n_msgs <= o.small_batch) thr = 0;
  p.big_threshold = (u32)thr;
  const u32 idx_blocks = (n_msgs + 64 * kIdxWaves - 1) / (64 * kIdxWaves);
  // Order of the forked path's small-message execution.  The split point:
  // bodies of size class >= split_class (compressed size < 2^(16 -
  // split_class) bytes; option split_class) vs the larger ones.
  // Option split_walk (A/B): 0 the execution in message order
  // after one walk; 1 the walk and execution split on two streams (above);
  // 2 one walk, then the execution in walk order (size classes, largest
  // first); 3 (default) one walk, then the smaller bodies' execution, then
  // the larger ones'.  CM, A/B on one box, two rounds, with the chunked
  // huge-body walk: 0 6.74 / 6.72, 1 (unchunked) 7.54 / 7.45 -- the third
  // stream shares a hardware queue with the huge bodies' stream and waits
  // behind it --, 2 6.55 / 6.45, 3 6.45 / 6.44 ms.  In message order a
  // wave's run of bodies mixes sizes and the launch waits for the waves that
  // drew the larger ones (execution 4.66 ms; in walk order 3.91).
  p.split_mode = (u32)o.split_walk;
  p.split_class = (u32)o.split_class % kWalkClasses;
  p.planned_walk = LaunchDim{idx_blocks, 64 * kIdxWaves, 0u};
  if (two_stream && lean_walk) {
    p.walk_kind = kWalkLean;
    p.walk = LaunchDim{idx_blocks, 64 * kIdxWaves, (u32)idx_lean_lds_bytes()};
  } else if (est_total_in < 16384ull * n_msgs) {
    p.walk_kind = kWalkSerial;
    p.walk = LaunchDim{(n_msgs + 64 * kIdxWavesSerial - 1) / (64 * kIdxWavesSerial), 64 * kIdxWavesSerial, 0u};
  } else {
    p.walk_kind = kWalkStandard;
    p.walk = LaunchDim{idx_blocks, 64 * kIdxWaves, 0u};
  }
  // Pass 1b and the large-message exec blocks run on a side stream, after a
  // plan pass (headers, bitmap bases, the large-message list) and beside the
  // lane walk and the one-wave-per-message exec launch: pass 1b is bound by
  // the serial window walk of the few largest bodies and leaves most CUs
  // idle, which the small messages' passes fill.  Both streams join before
  // the fallback pass.
  // Only for batches of > 128K messages (the mixed-size ones): a fork and
  // join cost ~10 us (C2 0.159 -> 0.169 ms), and uniform batches send nothing
  // to pass 1b (CM 14.4 -> 12.1 ms).  Option decode_fork 0/1 forces (A/B).
  const u32 small_blocks = (n_msgs + kWavesPerBlock - 1) / kWavesPerBlock;
  p.small_blocks = small_blocks;
  // A/B knob; at least one block: the large-message lists are only drained there
  const i64 big_opt = o.exec_big_blocks;
  const u32 big_blocks_opt = big_opt >= 1 && big_opt <= (1 << 20) ? (u32)big_opt : 512u;
  p.prio = o.exec_prio != 0 ? 1u : 0u;  // A/B knob: 0 disables the priority raise
  // history kept when an exec window slides (option exec_keep: the tests
  // shrink it to exercise the slide's flush rule; 512..kMaxKeep bytes, a
  // multiple of 16; anything else is the default).
  // Per instance of exec_kernel<5>: keep_hist the general one (and variant 4,
  // the packed pass), keep_hist_whole the folded one, whose wider window
  // admits up to kMaxKeepWhole: a value above kMaxKeep sets it alone.
  p.keep_hist = kKeep;
  p.keep_hist_whole = kKeepWhole;
  {
    const i64 v = o.exec_keep;
    if (v >= 512 && v <= (i64)kMaxKeep && v % 16 == 0) p.keep_hist = (u32)v;
    if (v >= 512 && v <= (i64)kMaxKeepWhole && v % 16 == 0) p.keep_hist_whole = (u32)v;
  }
  const i64 fork_opt = o.decode_fork;
  p.fork = !two_stream && (fork_opt >= 0 ? fork_opt != 0 : n_msgs > 131072u);
  p.big_blocks = small_blocks < big_blocks_opt ? small_blocks : big_blocks_opt;
  // pass 1b: large messages, one wave each (an empty list costs one short
  // launch)
  {
    const u32 q = (n_msgs + 3) / 4;
    p.index_big_grid = q < 1024u ? q : 1024u;
  }
  // The forked path's large-message launches: CM 9.9 -> 8.85 ms with 1,792
  // blocks against 512 when they ran alone after the lane walk; 1,024 since
  // the small bodies' execution (walk order, 3,584 blocks) runs beside them:
  // CM 6.32-6.37 -> 6.20-6.25 ms for the two grid sizes together (A/B on one
  // box, four rounds).
  const i64 bbf_opt = o.exec_big_blocks_fork;  // A/B knob, separate from the one-stream launch's
  const u32 big_blocks_fork_opt = bbf_opt >= 1 && bbf_opt <= (1 << 20) ? (u32)bbf_opt : 1024u;
  // the large-message blocks only (exit after one atomic when the lists
  // are empty)
  p.fork_big_blocks = small_blocks < big_blocks_fork_opt ? small_blocks : big_blocks_fork_opt;
  // The huge messages' pass 1b, chunked (chunk_*_kernel): when the record
  // region holds a batch of this workspace's size (option chunked_huge 0:
  // one wave per message).  On by default since the small bodies' execution runs
  // in walk order (FSG_SPLIT_WALK 3): CM 6.77-6.81 -> 6.44 ms, where the
  // chunked walk alone had measured slower (the huge bodies were then off
  // the critical path).
  const bool chunked_opt = o.chunked_huge != 0;  // (the tests run both forms)
  // record region: 8 B per possible huge message (its first record, its
  // chain verdict), then the chunk records -- sized for the batch's bound on
  // huge messages (est_total_in / kHugeIndexBytes), the records after them
  const u64 max_huge_need = est_total_in / kHugeIndexBytes + 1;
  const u64 max_huge = 8 * max_huge_need < chunk_bytes ? max_huge_need : chunk_bytes / 320;
  const u64 max_recs = max_huge ? (chunk_bytes - 8 * max_huge) / sizeof(ChunkRec) : 0;
  p.max_huge = max_huge;
  p.max_recs = max_recs;
  p.first_rec_off = chunk_off;
  p.mstat_off = chunk_off + 4 * max_huge;
  p.recs_off = chunk_off + 8 * max_huge;
  p.chunked = chunked_opt && max_huge >= est_total_in / kHugeIndexBytes + 1 &&
              max_recs >= est_total_in / kChunkBytes + est_total_in / kHugeIndexBytes + 2;
  {
    const u32 lb = (u32)((max_huge + 255) / 256);
    p.chunk_list_grid = lb ? lb : 1u;
    p.chunk_rec_grid = (u32)(max_recs / 4 + 1 < 1024 ? max_recs / 4 + 1 : 1024);
    p.chunk_msg_grid = (u32)(max_huge / 4 + 1 < 256 ? max_huge / 4 + 1 : 256);
  }
  // The forked path's small-message launches: a grid of small_persist blocks,
  // each wave looping over messages; CM 7.31 -> 7.02 ms against one wave per
  // message (A/B on one box, two passes; 1,024 blocks: 7.11, 3,584: 7.03);
  // 3,584 (two rounds of blocks at 7 waves per SIMD) since the execution
  // runs in walk order (see exec_big_blocks_fork).  Option small_persist
  // (blocks: the tests shrink it; 0 = one wave per message).
  const i64 sp_opt = o.small_persist;
  const u32 small_persist = sp_opt >= 0 && sp_opt <= (1 << 20) ? (u32)sp_opt : 3584u;
  p.small_grid = small_persist && small_persist < small_blocks ? small_persist : small_blocks;
  p.small_stride = p.small_grid < small_blocks ? p.small_grid : 0u;
  // The short bodies of walk part 2 packed several to a wave (exec5_packed,
  // decode_v4_packed.h):
  // option exec_pack = bodies per batch (1..64, default 32; 0 = one wave per
  // body, the small-message grid above).  Grid: the small-message grid's
  // size.  Measured on CM (A/B on one box):
  // 5.85-5.92 ms against 6.11-6.19 with one wave per body, once literals of
  // 65..896 bytes ran inside the group (6.60-6.63 while each was a
  // wave-wide copy with a window restart).
  const i64 pack_opt = o.exec_pack;
  p.pack_batch = pack_opt >= 1 && pack_opt <= 64 ? (u32)pack_opt : 0u;
  p.plan_grid = (n_msgs + kPlanThreads - 1) / kPlanThreads;
  p.scatter_grid = (n_msgs + 255) / 256;
  p.fallback_grid = (n_msgs + 63) / 64;
  return p;
}

}  // namespace fsg
