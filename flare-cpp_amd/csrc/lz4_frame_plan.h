// lz4_frame_plan.h -- LZ4 frames (lz4_frame_encode.hip,
// lz4_frame_decode.hip): the workspace layouts and
// everything a launch decides before its first kernel, the plans of the inner
// block launches included, as plain host arithmetic.  The path reports read
// the same structs.  No HIP include: tests/cpp/test_lz4_plan.cc checks it on
// the CPU.  DESIGN.md section 4, "LZ4 frames".
#pragma once

#include "lz4_frame_format.h"  // block_bytes; LZ4F_HD
#include "lz4_plan.h"

namespace fsg {

constexpr u64 kLz4fHead = 256;  // the workspace header: counters (kFc*, kFd* of lz4_frame_encode.hip, lz4_frame_decode.hip)

LZ4F_HD u64 round_up(u64 v, u64 a) { return (v + a - 1) / a * a; }

// staging slot of a block of L input bytes in the compressor: the body bound
// of the block codec (fsg_lz4_max_compressed_length), 16-byte aligned, and 64
// spare bytes
LZ4F_HD u64 enc_slot(u64 L) { return round_up(5 + L + L / 255 + 16, 16) + 64; }
// and of a stored block of sz bytes in the decompressor: varint32 + bytes
LZ4F_HD u64 dec_slot(u64 sz) { return round_up(5 + sz, 16) + 16; }

// ---- columns: four u32 per message (route, first, nb, xxh), each 256-aligned;
// per block entry three u64 and six u32 columns, packed in Lz4fBlockColOff's order
inline u64 lz4f_list_bytes(u64 n) { return round_up(n * 4, 256); }
constexpr u64 kLz4fMsgCols = 4;
constexpr u64 kLz4fBlockColBytes = 3 * 8 + 6 * 4;
inline u64 lz4f_block_cols_bytes(u64 nb) { return round_up(nb * kLz4fBlockColBytes, 256); }
struct Lz4fBlockColOff {  // bytes from the block columns' start
  u64 in_off, out_off, src_off, in_len, out_cap, out_len, status, src_len, flags;
};
inline Lz4fBlockColOff lz4f_block_col_off(u64 nb) {
  return Lz4fBlockColOff{0, 8 * nb, 16 * nb, 24 * nb, 28 * nb, 32 * nb, 36 * nb, 40 * nb, 44 * nb};
}

// A workspace for `total` input bytes: header | message columns | block
// columns | [compress: a 64-byte slot per entry] | the block codec's workspace
// | staging.
struct Lz4fLayout {
  u32 nb_cap;
  u64 stage_cap;
  u64 off_msg, off_blk, off_dummy, off_inner, inner_bytes, off_stage, total;
};
constexpr u64 kLz4fMaxBlocks = 1ull << 30;

inline bool lz4f_enc_layout(u32 n_msgs, u64 total, u32 id, Lz4fLayout* p) {
  const u64 bs = lz4f::block_bytes(id);
  const u64 nb = (u64)n_msgs + total / bs;
  if (nb > kLz4fMaxBlocks) return false;
  p->nb_cap = (u32)nb;
  p->stage_cap = total + total / 255 + nb * (enc_slot(0) + 16);
  p->off_msg = kLz4fHead;
  p->off_blk = p->off_msg + kLz4fMsgCols * lz4f_list_bytes(n_msgs);
  p->off_dummy = p->off_blk + lz4f_block_cols_bytes(nb);
  p->off_inner = p->off_dummy + round_up(64 * nb, 256);
  p->inner_bytes = lz4_compress_workspace_bytes((u32)nb);  // the inner route is always 0
  p->off_stage = round_up(p->off_inner + p->inner_bytes, 256);
  p->total = p->off_stage + round_up(p->stage_cap, 256);
  return true;
}

// a full compressed block of the smallest size, 64 KiB, has at least 257
// bytes (a length byte adds at most 255), so a frame the fast route takes has
// at most one block per 256 input bytes and one more
inline bool lz4f_dec_layout(u32 n_msgs, u64 total, Lz4fLayout* p) {
  const u64 nb = (u64)n_msgs + total / 256;
  if (nb > kLz4fMaxBlocks) return false;
  p->nb_cap = (u32)nb;
  p->stage_cap = total + 32 * nb;
  p->off_msg = kLz4fHead;
  p->off_blk = p->off_msg + kLz4fMsgCols * lz4f_list_bytes(n_msgs);
  p->off_dummy = p->off_blk + lz4f_block_cols_bytes(nb);
  p->off_inner = p->off_dummy;
  // the block decoder's workspace: its fixed part for every entry, and a
  // bitmap for `total` block bytes with 16 bytes of rounding for a block per
  // message and per 4 KiB (64 KiB blocks that shrank 16 times).  Blocks past
  // that go to the block decoder's one-pass kernel: slower, the same bytes.
  p->inner_bytes = lz4_decode_fixed_bytes((u32)nb) + 4 * lz4_decode_bitmap_words((u64)n_msgs + total / 4096, total);
  p->off_stage = round_up(p->off_inner + p->inner_bytes, 256);
  p->total = p->off_stage + round_up(p->stage_cap, 256);
  return true;
}

// the largest `total` whose workspace fits ws_bytes (the calls get no input
// size: the workspace says what it was sized for); false below total = 0
template <typename F>
bool lz4f_layout_for(size_t ws_bytes, Lz4fLayout* p, F make) {
  if (!make(0, p) || p->total > ws_bytes) return false;
  u64 lo = 0, hi = 1ull << 46;  // make(lo) fits
  while (lo + 1 < hi) {
    const u64 mid = lo + (hi - lo) / 2;
    Lz4fLayout q;
    if (make(mid, &q) && q.total <= ws_bytes) lo = mid;
    else hi = mid;
  }
  return make(lo, p);
}

inline size_t lz4f_compress_workspace_bytes(u32 n_msgs, u64 total_in_bytes, u32 id) {
  Lz4fLayout p;
  return lz4f_enc_layout(n_msgs, total_in_bytes, id, &p) ? (size_t)p.total : 0;
}
inline size_t lz4f_decompress_workspace_bytes(u32 n_msgs, u64 total_in_bytes) {
  Lz4fLayout p;
  return lz4f_dec_layout(n_msgs, total_in_bytes, &p) ? (size_t)p.total : 0;
}

// The wave threshold of the length pass from option lz4f_length_wave_min.
// Automatic: 2 KiB whatever the batch.  Measured on MI355X (DESIGN.md section
// 5, "LZ4 frames without a content size", the lane-against-wave table): the
// wave won at every point, from 1.14x (4,096 blocks of 4 KiB, 2.7 KB stored)
// to 10.7x (64 blocks of 4 MiB); the smallest stored size in the table is
// 2.7 KB and nothing below it was measured, so blocks of at most 2 KiB stay
// with the lanes.  (The first build took the block decoder's rule, 2 KiB up
// to 256 block entries and 64 KiB above; the table did not bear out the 64
// KiB.)
inline u32 lz4f_length_wave_min(i64 option) {
  if (option < 0) return 2048u;
  return option >= 0xFFFFFFFFll ? 0xFFFFFFFFu : (u32)option;
}

// What launch_lz4f_encode computes before its first launch (valid: the block
// size id is one of the format's and the workspace holds total = 0).
struct Lz4fEncodePlan {
  bool valid;
  Lz4fLayout w;
  u32 prefill_grid, plan_grid, assemble_grid;  // blocks of 256, 64 and 64 threads
  // the block encoders on the block columns: option lz4f_block_wave_min by the
  // rule of lz4_encode_wave_min, whose automatic form sees the block entries
  // as its batch; option lz4_encode_wave_per_cu as in the block call
  Lz4EncodePlan inner;
};
inline Lz4fEncodePlan lz4f_encode_plan(u32 n_msgs, size_t ws_bytes, u32 id, const Lz4Opts& o) {
  Lz4fEncodePlan p{};
  p.valid = id >= lz4f::kMinBlockId && id <= lz4f::kMaxBlockId &&
            lz4f_layout_for(ws_bytes, &p.w, [&](u64 t, Lz4fLayout* q) { return lz4f_enc_layout(n_msgs, t, id, q); });
  if (!p.valid) return p;
  p.prefill_grid = (p.w.nb_cap + 255) / 256;
  p.plan_grid = (n_msgs + 63) / 64;
  p.assemble_grid = n_msgs;
  Lz4Opts inner = o;
  inner.lz4_encode_wave_min = o.lz4f_block_wave_min;
  p.inner = lz4_encode_plan(p.w.nb_cap, p.w.inner_bytes, inner);
  return p;
}

// What launch_lz4f_decode and launch_lz4f_decoded_lengths compute before
// their first launch (valid: the workspace holds total = 0).
struct Lz4fDecodePlan {
  bool valid;
  Lz4fLayout w;
  bool force_serial, nosize_fast, linked_fast;  // options lz4f_force_serial, lz4f_nosize_fast, lz4f_linked_fast
  u32 length_wave_min;
  u32 msg_grid;          // the kernels with a lane per message (index, finish, length index): blocks of 64
  u32 length_lane_grid;  // length pass: a lane per entry, at most 4,096 blocks of 64
  u32 length_wave_grid;  // and the listed large blocks (with none listed each wave reads the count and leaves)
  u32 place_grid;        // a wave per message, four to a block
  u32 stage_grid;        // a wave per entry, four to a block, at most 8,192 blocks
  u32 verdict_grid;      // a lane per entry, blocks of 64
  // the block decoder on the block columns, a chain per message with option
  // lz4f_linked_fast; option lz4_big_min as in the block call
  Lz4DecodePlan inner;
};
inline Lz4fDecodePlan lz4f_decode_plan(u32 n_msgs, size_t ws_bytes, const Lz4Opts& o) {
  Lz4fDecodePlan p{};
  p.valid = lz4f_layout_for(ws_bytes, &p.w, [&](u64 t, Lz4fLayout* q) { return lz4f_dec_layout(n_msgs, t, q); });
  if (!p.valid) return p;
  p.force_serial = o.lz4f_force_serial != 0;
  p.nosize_fast = o.lz4f_nosize_fast != 0;
  p.linked_fast = o.lz4f_linked_fast != 0;
  p.length_wave_min = lz4f_length_wave_min(o.lz4f_length_wave_min);
  const u32 nb = p.w.nb_cap;
  p.msg_grid = (n_msgs + 63) / 64;
  p.length_lane_grid = (nb + 63) / 64 < 4096 ? (nb + 63) / 64 : 4096;
  p.length_wave_grid = 256;
  p.place_grid = (n_msgs + 3) / 4;
  p.stage_grid = (nb + 3) / 4 < 8192 ? (nb + 3) / 4 : 8192;
  p.verdict_grid = (nb + 63) / 64;
  p.inner = lz4_decode_plan(nb, p.w.inner_bytes, p.linked_fast ? n_msgs : 0, o);
  return p;
}

}  // namespace fsg
