// lz4_frame_cols.h -- what the two sides of the LZ4 frame codec
// (lz4_frame_encode.hip, lz4_frame_decode.hip) share on the device: the block
// and message columns of a workspace (offsets and sizes: lz4_frame_plan.h) and
// three wave helpers.
#pragma once

#include "lz4_frame_plan.h"
#include "snappy_device.h"
#include "wave_util.h"

namespace fsg {
namespace {

__device__ __forceinline__ u32 wave_scan(u32 v) { return wave_incl_scan(v); }

// adds `pred` lanes to a counter: one atomic for the wave's active lanes
__device__ __forceinline__ void count_lanes(u32* ctr, bool pred) {
  const u64 b = __ballot(pred);
  const u64 act = __ballot(true);
  if (b && __lane_id() == (u32)__builtin_ctzll(act)) atomicAdd(ctr, (u32)__builtin_popcountll(b));
}

// n bytes from s to d by one wave, exactly: single bytes up to d's 16-byte
// boundary, 16 bytes per lane, single bytes at the end
__device__ __forceinline__ void wave_copy(u8* d, const u8* s, u32 n, u32 lane) {
  u32 head = (16u - (u32)(reinterpret_cast<uintptr_t>(d) & 15)) & 15;
  if (head > n) head = n;
  if (lane < head) d[lane] = s[lane];
  const u32 body = (n - head) & ~15u;
  for (u32 i = 16 * lane; i < body; i += 1024) copy16(d + head + i, s + head + i);
  const u32 done = head + body;
  if (done + lane < n) d[done + lane] = s[done + lane];
}

struct BlockCols {
  u64* in_off;   // compress: into d_in; decompress: staged body, into the workspace
  u64* out_off;  // compress: staging slot, into the workspace; decompress: into d_out
  u64* src_off;  // decompress: the stored block's bytes, into d_in
  u32* in_len;
  u32* out_cap;
  u32* out_len;
  i32* status;
  u32* src_len;  // decompress: stored size
  u32* flags;
};

struct MsgCols {
  u32* route;
  u32* first;
  u32* nb;
  u32* xxh;
};

// ---- the columns in a workspace
inline MsgCols msg_cols(u8* w, u32 n_msgs) {
  MsgCols mc;
  const u64 lb = lz4f_list_bytes(n_msgs);
  mc.route = reinterpret_cast<u32*>(w);
  mc.first = reinterpret_cast<u32*>(w + lb);
  mc.nb = reinterpret_cast<u32*>(w + 2 * lb);
  mc.xxh = reinterpret_cast<u32*>(w + 3 * lb);
  return mc;
}
inline BlockCols block_cols(u8* w, u64 nb) {
  const Lz4fBlockColOff o = lz4f_block_col_off(nb);
  BlockCols c;
  c.in_off = reinterpret_cast<u64*>(w + o.in_off);
  c.out_off = reinterpret_cast<u64*>(w + o.out_off);
  c.src_off = reinterpret_cast<u64*>(w + o.src_off);
  c.in_len = reinterpret_cast<u32*>(w + o.in_len);
  c.out_cap = reinterpret_cast<u32*>(w + o.out_cap);
  c.out_len = reinterpret_cast<u32*>(w + o.out_len);
  c.status = reinterpret_cast<i32*>(w + o.status);
  c.src_len = reinterpret_cast<u32*>(w + o.src_len);
  c.flags = reinterpret_cast<u32*>(w + o.flags);
  return c;
}

}  // namespace
}  // namespace fsg
