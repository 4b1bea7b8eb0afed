// lz4_plan.h -- the LZ4 block codec (lz4_decode2.hip, lz4_encode_wave.hip,
// lz4.hip): the workspace layouts and everything a launch decides before its
// first kernel, as plain host arithmetic.  The path reports read the same
// structs.  No HIP include: tests/cpp/test_lz4_plan.cc checks it on the CPU.
// DESIGN.md section 4, "LZ4" and "LZ4 compress: the wave encoder".
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "decode_v4_plan.h"  // the integer typedefs

namespace fsg {

// The LZ4 options (csrc/options.h, kOptLz4BigMin .. kOptLz4fLinkedFast) as one
// call sees them: read_lz4_opts (capi.hip) fills this once from opt().  The
// initialisers are the option table's defaults (capi.hip checks that they
// agree).
struct Lz4Opts {
  i64 lz4_big_min = -1;
  i64 lz4_encode_wave_min = -1;
  i64 lz4_encode_wave_per_cu = 0;
  i64 lz4f_force_serial = 0;
  i64 lz4f_block_wave_min = -1;
  i64 lz4f_nosize_fast = 0;
  i64 lz4f_length_wave_min = -1;
  i64 lz4f_linked_fast = 0;
};

// ================================================================ decode
// Workspace of the two-pass decoder: [0, 256) counters (0 bitmap words
// allocated, 1 large blocks listed, 2 large blocks taken) | bm_base[n] |
// hdr[n] | big_list[n] | bitmap words (round_up(ceil(block / 32), 4) per
// message <= total / 32 + 4 n).  Counter 3: the messages the one-pass lane
// kernel finished as this launch's fallback (path report,
// fsg_lz4_decompress_report).
constexpr u64 kL4Head = 256;
constexpr u32 kL4CtrFallback = 3;
constexpr u32 kL4Waves = 4;      // execution pass: waves per block
constexpr u32 kL4BigGrid = 256;  // the large blocks' wave walk: with no listed block each wave reads the count and leaves
inline u64 l4_list_bytes(u32 n) { return ((u64)n * 4 + 255) & ~(u64)255; }  // a u32 per message, 256-aligned (both directions)
// the part in front of the bitmap
inline u64 lz4_decode_fixed_bytes(u32 n_msgs) { return kL4Head + 3 * l4_list_bytes(n_msgs); }
// bitmap words for `entries` blocks of total_in_bytes in all
inline u64 lz4_decode_bitmap_words(u64 entries, u64 total_in_bytes) { return total_in_bytes / 32 + 4 * entries + 4; }
inline size_t lz4_decode_workspace_bytes(u32 n_msgs, u64 total_in_bytes) {
  return lz4_decode_fixed_bytes(n_msgs) + 4 * lz4_decode_bitmap_words(n_msgs, total_in_bytes);
}
// Bitmap capacity in words (whole 16-byte groups) of a workspace of at least
// lz4_decode_fixed_bytes(n_msgs) bytes.
inline u64 lz4_decode_bitmap_capacity_words(u32 n_msgs, size_t ws_bytes) {
  return (ws_bytes - lz4_decode_fixed_bytes(n_msgs)) / 16 * 4;
}
// blocks above this many bytes take the wave walk.  A batch of at most
// kL4SmallBatch messages has the chip to itself: a wave per block is quicker
// than one lane per block from a few KiB on (option lz4_big_min overrides,
// -1 = this rule; the tests lower it)
constexpr u32 kL4BigMin = 65536;
constexpr u32 kL4SmallBatch = 256;
constexpr u32 kL4BigMinSmall = 2048;

// What launch_lz4_decode2 computes before its first launch.  Offsets are bytes
// from the workspace's start.
struct Lz4DecodePlan {
  bool valid;     // the workspace holds the fixed part (otherwise hipErrorInvalidValue)
  bool two_pass;  // and the two-pass minimum, lz4_decode_workspace_bytes(n, 0): the
                  // route of fsg_lz4_decompress_batch_ws (below it, the one-pass kernel)
  u64 bm_base, hdr, big_list, bitmap;
  u64 cap_words;  // bitmap words the workspace holds
  u32 big_min;
  u32 index_grid, index_big_grid, exec_grid, chain_grid;  // blocks (chain_grid 0: no launch)
};
// n_chains: the chains of a linked frame's blocks (launch.h, Lz4Chains; 0 for the block calls)
inline Lz4DecodePlan lz4_decode_plan(u32 n_msgs, size_t ws_bytes, u32 n_chains, const Lz4Opts& o) {
  Lz4DecodePlan p{};
  const u64 fixed = lz4_decode_fixed_bytes(n_msgs);
  p.valid = ws_bytes >= fixed;
  p.two_pass = ws_bytes >= lz4_decode_workspace_bytes(n_msgs, 0);
  if (!p.valid) return p;
  p.bm_base = kL4Head;
  p.hdr = p.bm_base + l4_list_bytes(n_msgs);
  p.big_list = p.hdr + l4_list_bytes(n_msgs);
  p.bitmap = fixed;
  p.cap_words = lz4_decode_bitmap_capacity_words(n_msgs, ws_bytes);
  p.big_min = o.lz4_big_min >= 0 && o.lz4_big_min <= 0xffffffffll
                  ? (u32)o.lz4_big_min
                  : (n_msgs <= kL4SmallBatch ? kL4BigMinSmall : kL4BigMin);
  p.index_grid = (n_msgs + 63) / 64;
  p.index_big_grid = kL4BigGrid;
  p.exec_grid = (n_msgs + kL4Waves - 1) / kL4Waves;
  p.chain_grid = (n_chains + kL4Waves - 1) / kL4Waves;
  return p;
}

// ================================================================ encode
// Workspace of the routed call: [0, 256) header | list[n] | the lanes' tables,
// 16 KiB per message.  A workspace of the earlier size, the tables alone:
// the lanes only, as before the wave encoder.
constexpr u64 kLz4WaveNone = 1ull << 32;  // wave_min: no body goes to the wave encoder
constexpr u32 kLz4EncHead = 256;
constexpr u32 kLz4EncTableBytes = 16384;  // 8,192 x u16 or 4,096 x u32
constexpr u32 kLz4EncCus = 256, kLz4EncCuLds = 160 * 1024;
// one-wave workgroups of 16 KiB: nine fit beside the CU's other allocations
constexpr u32 kLz4EncWavesPerCu = kLz4EncCuLds / kLz4EncTableBytes - 1;
inline size_t lz4_compress_tables_bytes(u32 n_msgs) { return (size_t)n_msgs * kLz4EncTableBytes; }
inline size_t lz4_compress_workspace_bytes(u32 n_msgs) {
  return kLz4EncHead + l4_list_bytes(n_msgs) + lz4_compress_tables_bytes(n_msgs);
}

// The wave threshold from option lz4_encode_wave_min (or lz4f_block_wave_min,
// for a frame's blocks): < 0 automatic, >= 0xFFFFFFFF none.
// Automatic, from the size matrix measured on MI355X (DESIGN.md section 4,
// profiles/lz4wenc/): in batches of up to 256 bodies the wave encoder was
// faster in every row, down to the smallest size measured (8 KiB); at 65,536
// bodies (C3) the lanes were twice as fast.  Nothing between was measured, so
// batches over 256 bodies stay on the lanes.
constexpr u32 kLz4WaveBatchMax = 256;
constexpr u64 kLz4WaveMinSmallBatch = 8192;
inline u64 lz4_encode_wave_min(i64 option, u32 n_msgs) {
  if (option < 0) return n_msgs <= kLz4WaveBatchMax ? kLz4WaveMinSmallBatch : kLz4WaveNone;
  return option >= 0xFFFFFFFFll ? kLz4WaveNone : (u64)option;
}

// What launch_lz4_encode computes before its first launch.
struct Lz4EncodePlan {
  bool valid;      // the workspace holds the tables (fsg_lz4_compress_batch: otherwise an invalid argument)
  int route;       // 0 = list + lanes + waves (lz4_compress_workspace_bytes), 1 = the lanes alone on the tables
  u64 wave_min;    // bodies of at least this many bytes take the wave encoder (kLz4WaveNone: none; route 1: none)
  u64 zero_bytes;  // what the launch zeroes
  u64 list_off, tables_off;
  u32 list_grid;   // lz4_encode_list_kernel, blocks of 256
  u32 wave_grid;   // resident waves: an upper bound (LDS: 16 KiB a wave); waves past the list leave at once
};
inline Lz4EncodePlan lz4_encode_plan(u32 n_msgs, size_t ws_bytes, const Lz4Opts& o) {
  Lz4EncodePlan p{};
  p.valid = ws_bytes >= lz4_compress_tables_bytes(n_msgs);
  p.route = ws_bytes >= lz4_compress_workspace_bytes(n_msgs) ? 0 : 1;
  if (p.route != 0) {
    p.wave_min = kLz4WaveNone;
    p.zero_bytes = lz4_compress_tables_bytes(n_msgs);
    return p;
  }
  p.wave_min = lz4_encode_wave_min(o.lz4_encode_wave_min, n_msgs);
  p.zero_bytes = lz4_compress_workspace_bytes(n_msgs);
  p.list_off = kLz4EncHead;
  p.tables_off = p.list_off + l4_list_bytes(n_msgs);
  p.list_grid = (n_msgs + 255) / 256;
  const i64 pc = o.lz4_encode_wave_per_cu;
  const u32 per_cu = pc > 0 && pc < (i64)kLz4EncWavesPerCu ? (u32)pc : kLz4EncWavesPerCu;
  const u32 waves = kLz4EncCus * per_cu;
  p.wave_grid = n_msgs < waves ? n_msgs : waves;
  return p;
}

}  // namespace fsg
