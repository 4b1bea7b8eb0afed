// lz4_frame_decode.hip -- LZ4 frame bodies (LZ4 Frame Format 1.6.x) on the
// batch layout of the block codec, the decompress side and the lengths call:
// include/flare_lz4_gpu.h, "LZ4 frames".
//
// The block decoder this library already has (lz4_decode2.hip) runs a frame's
// blocks as if they were messages, on the plan the frame's plan holds for it
// and with one more argument for the linked frames below; the kernels here
// only take frames apart and judge the result.  Workspace layout, capacities,
// thresholds and grid sizes: lz4_frame_plan.h.  A frame's structure is read by
// the one walk of lz4_frame_format.h (tests/cpp/test_lz4f_walk.cc).
//
// Decompress: index (a lane per message: descriptor, route, the walk over the
// block size words, block columns) -> stage (a wave per block: varint32 +
// block bytes into the workspace, a raw block straight to its place) ->
// launch_lz4_decode2 on the block columns -> the checksum kernel on the listed
// blocks that carry a checksum -> verdict (a lane per block: status, length)
// -> the checksum kernel on the output of every pending frame with a content
// checksum -> finish (a lane per message: status; and the serial decoder,
// lz4_frame_format.h, for linked blocks, frames without a content size and
// every frame the fast route did not accept).
// With option lz4f_nosize_fast, frames with independent blocks and no content
// size go block-parallel too: index lists their blocks with the length unknown,
// length (a lane per small block, a wave per large one: lz4_frame_length.h)
// finds every block's decoded length, place (a wave per message: prefix sum of
// the lengths) gives the blocks their places in the slot; stage, the block
// decoder, verdict and finish go on as for the sized frames.
// fsg_lz4f_decoded_lengths_batch is index, length and the sum alone.
// With option lz4f_linked_fast, frames with linked blocks are listed the same
// two ways, each entry with its prefix -- the bytes the frame produced before
// the block, at most 65,535 -- and marked chained: the block decoder indexes
// all of them side by side and one wave per frame executes the frame's blocks
// in order (lz4_decode2.hip, lz4_exec_chain_kernel).  Finish accepts such a
// frame only when its chain ran to the end.
#include "launch.h"
#include "lz4_frame_cols.h"
#include "lz4_frame_format.h"
#include "lz4_frame_length.h"
#include "lz4f_xxh.h"

namespace fsg {

namespace {

// ---- workspace header (the first 256 bytes; u32 indices)
constexpr u32 kFdBlocks = 0;    // block entries asked for
constexpr u32 kFdFastMsgs = 1, kFdFastBlocks = 2, kFdEmpty = 3;
constexpr u32 kFdLinked = 4, kFdNoSize = 5, kFdRejected = 6, kFdForced = 7;
constexpr u32 kFdSums = 8, kFdInner = 9;
constexpr u32 kFdStage = 10;    // u64
constexpr u32 kFdNsMsgs = 12, kFdNsBlocks = 13;  // answered by the fast route without a content size
constexpr u32 kFdBig = 14;      // length pass: blocks listed for the wave walk
constexpr u32 kFdBigNext = 15;  // and the next of them to take
constexpr u32 kFdLkMsgs = 16, kFdLkBlocks = 17;  // answered by the fast route for linked blocks
// listed block entries with a checksum, pending frames with a content
// checksum: 0 lets the checksum kernels leave at once
constexpr u32 kFdSumBlocks = 18, kFdSumMsgs = 19;

// msg_route values
constexpr u32 kRouteDone = 0, kRouteFast = 1, kRouteLinked = 2, kRouteNoSize = 3, kRouteRejected = 4,
              kRouteForced = 5;
constexpr u32 kRouteNoSizeFast = 6;  // fast route without a content size (pending until finish accepts it)
// linked blocks, pending: with a content size, without one (bit 0); the chain
// wave that executed all of a frame's blocks adds kRouteChainDone
constexpr u32 kRouteLinkedFast = 8, kRouteLinkedNsFast = 9, kRouteChainDone = 2;
constexpr u32 kRouteLinkedOk = kRouteLinkedFast + kRouteChainDone, kRouteLinkedNsOk = kRouteLinkedNsFast + kRouteChainDone;
// block flags
constexpr u32 kBlkRaw = 1, kBlkSum = 2, kBlkFailed = 4, kBlkListed = 8;
constexpr u32 kBlkUnknown = 16;  // decoded length unknown: the length pass finds it
constexpr u32 kBlkChained = 32;  // a linked frame's block: executed by its frame's wave
constexpr u32 kBlkMaxShift = 8;  // with kBlkUnknown: log2 of the frame's block maximum, from this bit up
// a chained block's prefix, from this bit up (written by index, or by place
// once the length pass, which reads f >> kBlkMaxShift, is over)
constexpr u32 kBlkPrefixShift = 16;

// (the staging slot of a block, dec_slot: lz4_frame_plan.h)

__global__ __launch_bounds__(64) void lz4f_sizes_kernel(const u8* __restrict__ in, const u64* __restrict__ in_off,
                                                      const u32* __restrict__ in_len, u32 n_msgs, u64* sizes,
                                                      i32* status) {
  const u32 m = blockIdx.x * 64 + threadIdx.x;
  if (m >= n_msgs) return;
  lz4f::Header h;
  const i32 st = lz4f::parse_header(in + in_off[m], in_len[m], &h);
  sizes[m] = h.size;
  status[m] = st;
}

// The claim of a frame check_blocks accepted: nb entries from *base and, with
// `stage`, `need` staging bytes from *sb and the counts the checksum kernels
// leave by.  false: no room in the workspace; else the message's columns.
__device__ inline bool claim_blocks(u32* hdr, MsgCols mc, u32 m, const lz4f::Header& h, u32 nb, u32 xxh, u32 route,
                                    u32 nb_cap, bool stage, u64 need, u64 stage_cap, u32* base, u64* sb) {
  *base = atomicAdd(&hdr[kFdBlocks], nb);
  *sb = stage ? atomicAdd(reinterpret_cast<unsigned long long*>(hdr + kFdStage), (unsigned long long)need) : 0;
  if ((u64)*base + nb > nb_cap || (stage && *sb + need > stage_cap)) return false;
  if (stage && (h.flg & lz4f::kFlgBlockSum)) atomicAdd(&hdr[kFdSumBlocks], nb);
  if (stage && (h.flg & lz4f::kFlgSum)) atomicAdd(&hdr[kFdSumMsgs], 1u);
  mc.xxh[m] = xxh;
  mc.first[m] = *base;
  mc.nb[m] = nb;
  mc.route[m] = route;
  return true;
}

// The listing pass over the nb blocks check_blocks accepted (nothing is tested
// again), entries from `base` on: where the stored bytes are, the flags, a
// staging slot from `at` on for a compressed block (at = 0: none, the lengths
// call).  A sized frame's entries get places and lengths, a chained one its
// prefix.  Without a content size the flags say "length unknown" with the
// block maximum; in_len, out_off and out_cap stay 0 -- an empty body for the
// block decoder -- until the place kernel knows the lengths.
__device__ inline void list_blocks(const u8* ib, u64 n, const lz4f::Header& h, u64 io, u64 oo, u32 nb, u32 base,
                                   u64 at, bool chain, BlockCols c) {
  const bool sized = h.size != lz4f::kNoSize;
  const u64 bs = h.block_max;
  const u32 common = kBlkListed | ((h.flg & lz4f::kFlgBlockSum) ? kBlkSum : 0) | (chain ? kBlkChained : 0) |
                     (sized ? 0 : kBlkUnknown | ((u32)(31 - __builtin_clz(h.block_max)) << kBlkMaxShift));
  lz4f::BlockWalk w = lz4f::begin_blocks(ib, n, h);
  lz4f::Block b, next;
  lz4f::next_block<false>(&w, &next);
  for (u32 k = 0; k < nb; ++k) {
    b = next;  // (the next word loads under this block's stores; after the last block it is the end mark, dropped)
    lz4f::next_block<false>(&w, &next);
    const u32 e = base + k;
    const u32 exp = sized ? (u32)(h.size - k * bs < bs ? h.size - k * bs : bs) : 0;
    u32 f = common | (b.raw ? kBlkRaw : 0);
    c.src_off[e] = io + b.at;
    c.src_len[e] = b.size;
    if (sized) {
      c.out_off[e] = oo + k * bs;
      c.out_cap[e] = exp;
      if (chain) f |= lz4f::linked_prefix(k * bs) << kBlkPrefixShift;
    }
    c.flags[e] = f;
    if (!b.raw && at) {
      c.in_off[e] = at;
      if (sized) c.in_len[e] = (u32)varint32_len(exp) + b.size;
      at += dec_slot(b.size);
    }
  }
}

// One lane per message: descriptor, route, and for the fast routes the walk
// over the block size words (two passes: validate, then list).
__global__ __launch_bounds__(64) void lz4f_index_kernel(const u8* __restrict__ in, const u64* __restrict__ in_off,
                                                      const u32* __restrict__ in_len, u32 n_msgs,
                                                      const u64* __restrict__ out_off, const u32* __restrict__ out_cap,
                                                      u32* __restrict__ out_len, i32* __restrict__ status, u32* hdr,
                                                      MsgCols mc, BlockCols c, u32 nb_cap, u64 stage_off,
                                                      u64 stage_cap, u32 force_serial, u32 nosize_fast,
                                                      u32 linked_fast) {
  const u32 m = blockIdx.x * 64 + threadIdx.x;
  if (m >= n_msgs) return;
  const u8* ib = in + in_off[m];
  const u64 n = in_len[m];
  lz4f::Header h;
  mc.route[m] = kRouteDone;
  if (lz4f::parse_header(ib, n, &h) != lz4f::kStOk) {
    out_len[m] = 0;
    status[m] = kBadHeader;
    return;
  }
  const u64 cap = out_cap[m];
  const bool sized = h.size != lz4f::kNoSize;
  // linked blocks on the fast route: with a content size, or with both options
  const bool linked = !(h.flg & lz4f::kFlgIndep);
  const bool chain = linked && linked_fast && !force_serial && (sized || nosize_fast);
  if (chain && sized && h.size > cap) {  // (the serial decoder answers from the descriptor)
    mc.route[m] = kRouteRejected;
    return;
  }
  if (sized && h.size > cap) {
    out_len[m] = h.size > 0xFFFFFFFFull ? 0xFFFFFFFFu : (u32)h.size;
    status[m] = kSlotTooSmall;
    return;
  }
  // a frame with no blocks is finished here
  if (n - h.len >= 4 && lz4f::rd32(ib + h.len) == 0) {
    u32 ol, sums = 0;
    status[m] = lz4f::decode_frame(ib, n, nullptr, cap, &ol, &sums);
    out_len[m] = ol;
    atomicAdd(&hdr[kFdEmpty], 1u);
    if (sums) atomicAdd(&hdr[kFdSums], sums);
    return;
  }
  if (force_serial) {
    mc.route[m] = kRouteForced;
    return;
  }
  if (linked && !chain) {
    mc.route[m] = kRouteLinked;
    return;
  }
  if (!sized && !nosize_fast) {
    mc.route[m] = kRouteNoSize;
    return;
  }
  // the fast routes.  Sized: every block but the last is full.  No content
  // size: the blocks' lengths are unknown until the length pass.
  mc.route[m] = kRouteRejected;
  u32 nb, xxh, base;
  u64 need = 0, sb;  // (staging bytes for the compressed blocks)
  const auto each = [&need](const lz4f::Block& b) { need += b.raw ? 0 : dec_slot(b.size); };
  if (!lz4f::check_blocks(ib, n, h, lz4f::BlockRules{false, sized}, each, &nb, &xxh)) return;
  const u32 route = sized ? (chain ? kRouteLinkedFast : kRouteFast) : (chain ? kRouteLinkedNsFast : kRouteNoSizeFast);
  if (!claim_blocks(hdr, mc, m, h, nb, xxh, route, nb_cap, true, need, stage_cap, &base, &sb)) return;
  list_blocks(ib, n, h, in_off[m], out_off[m], nb, base, stage_off + sb, chain, c);
}

// ---- the length pass (frames without a content size)
// One lane per claimed entry whose length is unknown: a raw block decodes to
// its stored size, a compressed block of at most wave_min bytes to what
// block_length says; a larger one is listed for lz4f_length_wave_kernel.  The
// length goes to out_len and the list to status: both columns are idle until
// the block decoder runs.
__global__ __launch_bounds__(64) void lz4f_length_lane_kernel(const u8* __restrict__ in, u32* hdr, BlockCols c,
                                                            u32 nb_cap, u32 wave_min) {
  const u32 claimed = hdr[kFdBlocks] < nb_cap ? hdr[kFdBlocks] : nb_cap;
  u32* const big = reinterpret_cast<u32*>(c.status);
  for (u32 e = blockIdx.x * 64 + threadIdx.x; e < claimed; e += gridDim.x * 64) {
    const u32 f = c.flags[e];
    if (!(f & kBlkUnknown)) continue;
    const u32 sz = c.src_len[e];
    if (f & kBlkRaw) {
      c.out_len[e] = sz;
    } else if (sz > wave_min) {
      big[atomicAdd(&hdr[kFdBig], 1u)] = e;  // each entry at most once: fewer than nb_cap
    } else {
      u64 len = 0;
      if (lz4f::block_length(in + c.src_off[e], sz, 1ull << (f >> kBlkMaxShift), &len)) c.out_len[e] = (u32)len;
      else c.flags[e] = f | kBlkFailed;
    }
  }
}

// One wave per listed block, taken from a counter: whichever wave is free
// takes the next, so a frame's adjacent large blocks spread over the chip.
__global__ __launch_bounds__(kLenWaves * 64) void lz4f_length_wave_kernel(const u8* __restrict__ in, u32* hdr,
                                                                        BlockCols c) {
  __shared__ u32 ring_s[kLenWaves][kLenRing / 4];
  const u32 wv = (u32)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const u32 lane = threadIdx.x & 63;
  const u32 count = hdr[kFdBig];
  const u32* const big = reinterpret_cast<const u32*>(c.status);
  for (;;) {  // lane 0 adds 1; its result is the index
    const u32 got = atomicAdd(&hdr[kFdBigNext], lane == 0 ? 1u : 0u);
    const u32 idx = (u32)__builtin_amdgcn_readfirstlane((int)got);
    if (idx >= count) break;
    const u32 e = (u32)__builtin_amdgcn_readfirstlane((int)big[idx]);
    const u32 f = (u32)__builtin_amdgcn_readfirstlane((int)c.flags[e]);
    const u32 sz = (u32)__builtin_amdgcn_readfirstlane((int)c.src_len[e]);
    u32 len = 0;
    const bool ok = lz4f_wave_block_length(in + c.src_off[e], sz, 1u << (f >> kBlkMaxShift), ring_s[wv], lane, &len);
    if (lane == 0) {
      if (ok) c.out_len[e] = len;
      else c.flags[e] = f | kBlkFailed;
    }
  }
}

// One wave per message on the pending route: the blocks' places from an
// exclusive sum over their lengths, 64 at a time.  A frame with a block that
// has no length, or longer than its slot, leaves the route: its entries are
// unlisted, so that stage and the block decoder write nothing for it, and the
// serial decoder gives its verdict.  lengths != nullptr
// (fsg_lz4f_decoded_lengths_batch): the sum and its status are the answer.
__global__ __launch_bounds__(256) void lz4f_place_kernel(u32 n_msgs, const u64* __restrict__ out_off,
                                                       const u32* __restrict__ out_cap, MsgCols mc, BlockCols c,
                                                       u64* lengths, i32* status) {
  const u32 m = blockIdx.x * 4 + (threadIdx.x >> 6);
  const u32 lane = threadIdx.x & 63;
  if (m >= n_msgs || (mc.route[m] != kRouteNoSizeFast && mc.route[m] != kRouteLinkedNsFast)) return;
  const u32 first = mc.first[m], nb = mc.nb[m];
  u64 total = 0;
  bool bad = false;
  for (u32 k0 = 0; k0 < nb; k0 += 64) {
    const bool valid = k0 + lane < nb;
    const u32 e = first + k0 + lane;
    const bool failed = valid && (c.flags[e] & kBlkFailed);
    const u32 len = valid && !failed ? c.out_len[e] : 0u;
    bad = bad || __ballot(failed) != 0;
    total += __shfl(wave_scan(len), 63, 64);
  }
  if (lengths) {
    if (lane == 0) {
      lengths[m] = bad ? 0 : total;
      status[m] = bad ? kCorrupt : kOk;
      mc.route[m] = kRouteDone;
    }
    return;
  }
  if (bad || total > out_cap[m]) {
    for (u32 k = lane; k < nb; k += 64) c.flags[first + k] = 0;
    if (lane == 0) mc.route[m] = kRouteRejected;
    return;
  }
  u64 at = out_off[m];
  for (u32 k0 = 0; k0 < nb; k0 += 64) {
    const bool valid = k0 + lane < nb;
    const u32 e = first + k0 + lane;
    const u32 len = valid ? c.out_len[e] : 0u;
    const u32 incl = wave_scan(len);
    if (valid) {
      c.out_off[e] = at + (incl - len);
      c.out_cap[e] = len;
      // (flags without kBlkChained have no bits from kBlkPrefixShift up once the length pass is over)
      if (c.flags[e] & kBlkChained)
        c.flags[e] = (c.flags[e] & ((1u << kBlkPrefixShift) - 1)) |
                     (lz4f::linked_prefix(at + (incl - len) - out_off[m]) << kBlkPrefixShift);
      if (!(c.flags[e] & kBlkRaw)) c.in_len[e] = (u32)varint32_len(len) + c.src_len[e];
    }
    at += __shfl(incl, 63, 64);
  }
}

// fsg_lz4f_decoded_lengths_batch, one lane per message: the stated content
// size, or the frame's blocks listed for the length pass (linked or not:
// lengths do not depend on linking).  A frame whose entries do not fit is
// walked here, by the host codec's own function.
__global__ __launch_bounds__(64) void lz4f_length_index_kernel(const u8* __restrict__ in,
                                                             const u64* __restrict__ in_off,
                                                             const u32* __restrict__ in_len, u32 n_msgs,
                                                             u64* __restrict__ lengths, i32* __restrict__ status,
                                                             u32* hdr, MsgCols mc, BlockCols c, u32 nb_cap) {
  const u32 m = blockIdx.x * 64 + threadIdx.x;
  if (m >= n_msgs) return;
  const u8* ib = in + in_off[m];
  const u64 n = in_len[m];
  lz4f::Header h;
  mc.route[m] = kRouteDone;
  lengths[m] = 0;
  if (lz4f::parse_header(ib, n, &h) != lz4f::kStOk) {
    status[m] = kBadHeader;
    return;
  }
  status[m] = kOk;
  if (h.size != lz4f::kNoSize) {
    lengths[m] = h.size;
    return;
  }
  u32 nb, xxh, base;
  u64 sb;
  if (!lz4f::check_blocks(ib, n, h, lz4f::BlockRules{true, false}, [](const lz4f::Block&) {}, &nb, &xxh)) {
    status[m] = kCorrupt;
    return;
  }
  if (nb == 0) return;
  if (claim_blocks(hdr, mc, m, h, nb, xxh, kRouteNoSizeFast, nb_cap, false, 0, 0, &base, &sb)) {
    list_blocks(ib, n, h, in_off[m], 0, nb, base, 0, false, c);
    return;
  }
  u64 total;
  if (lz4f::blocks_decoded_length(ib, n, h, &total)) lengths[m] = total;
  else status[m] = kCorrupt;
}

// One wave per listed block: a compressed block becomes a body of the block
// decoder in the staging area, a raw block goes to its place in the slot.
__global__ __launch_bounds__(256) void lz4f_stage_kernel(const u8* __restrict__ in, u8* out, u8* ws, BlockCols c,
                                                       u32 nb_cap) {
  const u32 lane = threadIdx.x & 63;
  const u32 waves = gridDim.x * 4;
  for (u32 e = blockIdx.x * 4 + (threadIdx.x >> 6); e < nb_cap; e += waves) {
    const u32 f = c.flags[e];
    if (!(f & kBlkListed)) continue;
    const u8* src = in + c.src_off[e];
    const u32 sz = c.src_len[e];
    if (f & kBlkRaw) {
      wave_copy(out + c.out_off[e], src, sz, lane);
      continue;
    }
    u8* d = ws + c.in_off[e];
    u32 v = c.out_cap[e];
    const u32 hl = (u32)varint32_len(v);
    if (lane == 0) {
      u8* p = d;
      while (v >= 0x80) {
        *p++ = (u8)(v | 0x80);
        v >>= 7;
      }
      *p = (u8)v;
    }
    wave_copy(d + hl, src, sz, lane);
  }
}

// ---- units of the checksum kernel (lz4f_xxh.h) on this side
// every listed entry with a block checksum, over the stored bytes; a word
// that differs from the stated one marks the entry failed
struct BlockSumUnits {
  const u8* in;
  const u32* hdr;
  BlockCols c;
  __device__ bool any() const { return hdr[kFdSumBlocks] != 0; }
  __device__ bool get(u32 e, const u8** p, u64* n, u32* sd) const {
    const u32 f = c.flags[e];
    if (!(f & kBlkListed) || !(f & kBlkSum)) return false;
    *p = in + c.src_off[e];
    *n = c.src_len[e];
    *sd = 0;
    return true;
  }
  __device__ void put(u32 e, u32 h) const {
    if (h != lz4f::rd32(in + c.src_off[e] + c.src_len[e])) c.flags[e] |= kBlkFailed;
  }
};

// every frame pending on a fast route whose descriptor (valid: index parsed
// it) flags a content checksum, over the bytes in its slot: the content size,
// or where the last block ends.  xxh[m] held the stated word; computed ^
// stated stays there, 0 when they agree.
struct ContentUnits {
  const u8* in;
  const u64* in_off;
  const u8* out;
  const u64* out_off;
  const u32* hdr;
  MsgCols mc;
  BlockCols c;
  __device__ bool any() const { return hdr[kFdSumMsgs] != 0; }
  __device__ bool get(u32 m, const u8** p, u64* n, u32* sd) const {
    const u32 route = mc.route[m];
    const bool sized = route == kRouteFast || route == kRouteLinkedOk;
    if (!sized && route != kRouteNoSizeFast && route != kRouteLinkedNsOk) return false;
    const u8* ib = in + in_off[m];
    if (!(ib[4] & lz4f::kFlgSum)) return false;
    if (sized) {
      *n = (u64)lz4f::rd32(ib + 6) | (u64)lz4f::rd32(ib + 10) << 32;
    } else {
      const u32 last = mc.first[m] + mc.nb[m] - 1;
      *n = c.out_off[last] + c.out_cap[last] - out_off[m];
    }
    *p = out + out_off[m];
    *sd = 0;
    return true;
  }
  __device__ void put(u32 m, u32 h) const { mc.xxh[m] ^= h; }
};

// One lane per block entry: what the checksum kernel and the block decoder
// said.
__global__ __launch_bounds__(64) void lz4f_verdict_kernel(BlockCols c, u32 nb_cap, u32* hdr) {
  const u32 e = blockIdx.x * 64 + threadIdx.x;
  if (e >= nb_cap) return;
  const u32 f = c.flags[e];
  const bool listed = f & kBlkListed;
  bool fail = false;
  if (listed && !(f & kBlkRaw)) fail = c.status[e] != kOk || c.out_len[e] != c.out_cap[e];
  if (fail) c.flags[e] = f | kBlkFailed;
  count_lanes(&hdr[kFdSums], listed && (f & kBlkSum));
}

// One lane per message: the fast route's answer (only ever FSG_OK), and the
// serial decoder for everything else.
__global__ __launch_bounds__(64) void lz4f_finish_kernel(const u8* __restrict__ in, const u64* __restrict__ in_off,
                                                       const u32* __restrict__ in_len, u32 n_msgs, u8* out,
                                                       const u64* __restrict__ out_off,
                                                       const u32* __restrict__ out_cap, u32* __restrict__ out_len,
                                                       i32* __restrict__ status, u32* hdr, MsgCols mc, BlockCols c,
                                                       const u32* inner_fallback) {
  const u32 m = blockIdx.x * 64 + threadIdx.x;
  if (m == 0 && inner_fallback) hdr[kFdInner] = *inner_fallback;
  if (m >= n_msgs) return;
  u32 route = mc.route[m];
  if (route == kRouteDone) return;
  const u8* ib = in + in_off[m];
  u8* ob = out + out_off[m];
  u32 blocks = 0, ns_blocks = 0, sums = 0;
  // a linked frame whose chain did not run to its end: the serial decoder
  if (route == kRouteLinkedFast || route == kRouteLinkedNsFast) route = kRouteRejected;
  const bool lk = route == kRouteLinkedOk || route == kRouteLinkedNsOk;
  const bool sized = route == kRouteFast || route == kRouteLinkedOk;
  if (sized || route == kRouteNoSizeFast || route == kRouteLinkedNsOk) {
    const u32 first = mc.first[m], nb = mc.nb[m], last = first + nb - 1;
    bool ok = true;
    for (u32 k = 0; k < nb && ok; ++k) ok = !(c.flags[first + k] & kBlkFailed);
    lz4f::Header h;
    lz4f::parse_header(ib, in_len[m], &h);
    if (ok && (h.flg & lz4f::kFlgSum)) {
      ok = mc.xxh[m] == 0;  // (the checksum kernel left computed ^ stated)
      sums = 1;
    }
    if (ok) {
      // without a content size the blocks lie end to end from the slot's
      // start: decoded exactly the lengths the walk found
      out_len[m] = sized ? (u32)h.size : (u32)(c.out_off[last] + c.out_cap[last] - out_off[m]);
      status[m] = kOk;
      (sized ? blocks : ns_blocks) = nb;
    } else {
      route = kRouteRejected;
    }
  }
  if (route != kRouteFast && route != kRouteNoSizeFast && !(lk && route != kRouteRejected)) {
    u32 ol, s = 0;
    status[m] = lz4f::decode_frame(ib, in_len[m], ob, out_cap[m], &ol, &s);
    out_len[m] = ol;
    sums += s;
  }
  count_lanes(&hdr[kFdFastMsgs], route == kRouteFast);
  count_lanes(&hdr[kFdLinked], route == kRouteLinked);
  count_lanes(&hdr[kFdNoSize], route == kRouteNoSize);
  count_lanes(&hdr[kFdRejected], route == kRouteRejected);
  count_lanes(&hdr[kFdForced], route == kRouteForced);
  if (lk && route != kRouteRejected) {  // (no frame is on this route unless the option is set)
    atomicAdd(&hdr[kFdLkMsgs], 1u);
    atomicAdd(&hdr[kFdLkBlocks], blocks + ns_blocks);
    blocks = ns_blocks = 0;
  }
  if (blocks) atomicAdd(&hdr[kFdFastBlocks], blocks);
  if (sums) atomicAdd(&hdr[kFdSums], sums);
  if (ns_blocks) {  // (no frame is on this route unless the option is set)
    atomicAdd(&hdr[kFdNsMsgs], 1u);
    atomicAdd(&hdr[kFdNsBlocks], ns_blocks);
  }
}

// the length pass on the claimed entries: lanes, then the listed large blocks
hipError_t launch_length_pass(const u8* in, u32* hdr, const BlockCols& c, const Lz4fDecodePlan& plan,
                              hipStream_t stream) {
  lz4f_length_lane_kernel<<<plan.length_lane_grid, 64, 0, stream>>>(in, hdr, c, plan.w.nb_cap, plan.length_wave_min);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  lz4f_length_wave_kernel<<<plan.length_wave_grid, kLenWaves * 64, 0, stream>>>(in, hdr, c);
  return hipGetLastError();
}

}  // namespace

void lz4f_decode_header_counts(const void* header, Lz4fDecodeHeaderCounts* c) {
  u32 ctr[kFdLkBlocks + 1];
  __builtin_memcpy(ctr, header, sizeof(ctr));
  c->fast_linked_messages = ctr[kFdLkMsgs];
  c->fast_linked_blocks = ctr[kFdLkBlocks];
  c->fast_nosize_messages = ctr[kFdNsMsgs];
  c->fast_nosize_blocks = ctr[kFdNsBlocks];
  c->fast_messages = ctr[kFdFastMsgs];
  c->fast_blocks = ctr[kFdFastBlocks];
  c->empty_messages = ctr[kFdEmpty];
  c->serial_linked = ctr[kFdLinked];
  c->serial_no_size = ctr[kFdNoSize];
  c->serial_rejected = ctr[kFdRejected];
  c->serial_forced = ctr[kFdForced];
  c->checksummed_units = ctr[kFdSums];
  c->inner_fallback = ctr[kFdInner];
}

hipError_t launch_lz4f_content_sizes(const u8* in, const u64* in_off, const u32* in_len, u32 n_msgs, u64* sizes,
                                     i32* status, hipStream_t stream) {
  if (n_msgs == 0) return hipSuccess;
  lz4f_sizes_kernel<<<(n_msgs + 63) / 64, 64, 0, stream>>>(in, in_off, in_len, n_msgs, sizes, status);
  return hipGetLastError();
}

// every size and decision of the two launches below from lz4f_decode_plan (lz4_frame_plan.h)
hipError_t launch_lz4f_decoded_lengths(const u8* in, const u64* in_off, const u32* in_len, u32 n_msgs, u64* lengths,
                                       i32* status, void* ws, hipStream_t stream, const Lz4fDecodePlan& plan) {
  if (n_msgs == 0) return hipSuccess;
  if (!plan.valid) return hipErrorInvalidValue;
  const Lz4fLayout& p = plan.w;
  u8* const w = static_cast<u8*>(ws);
  u32* const hdr = reinterpret_cast<u32*>(w);
  const MsgCols mc = msg_cols(w + p.off_msg, n_msgs);
  const BlockCols c = block_cols(w + p.off_blk, p.nb_cap);
  hipError_t e = hipMemsetAsync(w, 0, p.off_dummy, stream);
  if (e != hipSuccess) return e;
  lz4f_length_index_kernel<<<plan.msg_grid, 64, 0, stream>>>(in, in_off, in_len, n_msgs, lengths, status, hdr, mc, c,
                                                            p.nb_cap);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if ((e = launch_length_pass(in, hdr, c, plan, stream)) != hipSuccess) return e;
  lz4f_place_kernel<<<plan.place_grid, 256, 0, stream>>>(n_msgs, nullptr, nullptr, mc, c, lengths, status);
  return hipGetLastError();
}

hipError_t launch_lz4f_decode(const u8* in, const u64* in_off, const u32* in_len, u32 n_msgs, u8* out,
                              const u64* out_off, const u32* out_cap, u32* out_len, i32* status, void* ws,
                              hipStream_t stream, const Lz4fDecodePlan& plan) {
  if (n_msgs == 0) return hipSuccess;
  if (!plan.valid) return hipErrorInvalidValue;
  const Lz4fLayout& p = plan.w;
  u8* const w = static_cast<u8*>(ws);
  u32* const hdr = reinterpret_cast<u32*>(w);
  const MsgCols mc = msg_cols(w + p.off_msg, n_msgs);
  const BlockCols c = block_cols(w + p.off_blk, p.nb_cap);
  // header, message and block columns: an entry nobody lists stays an empty
  // body, which the block decoder answers without touching the output
  hipError_t e = hipMemsetAsync(w, 0, p.off_dummy, stream);
  if (e != hipSuccess) return e;
  lz4f_index_kernel<<<plan.msg_grid, 64, 0, stream>>>(in, in_off, in_len, n_msgs, out_off, out_cap, out_len, status, hdr,
                                                     mc, c, p.nb_cap, p.off_stage, p.stage_cap,
                                                     plan.force_serial ? 1u : 0u, plan.nosize_fast ? 1u : 0u,
                                                     plan.linked_fast ? 1u : 0u);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  const u32* inner_fallback = nullptr;
  if (!plan.force_serial && plan.nosize_fast) {
    if ((e = launch_length_pass(in, hdr, c, plan, stream)) != hipSuccess) return e;
    lz4f_place_kernel<<<plan.place_grid, 256, 0, stream>>>(n_msgs, out_off, out_cap, mc, c, nullptr, nullptr);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  if (!plan.force_serial) {
    lz4f_stage_kernel<<<plan.stage_grid, 256, 0, stream>>>(in, out, w, c, p.nb_cap);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    // option lz4f_linked_fast: the flags column carries the prefixes, the
    // route column the chains' results; without it, the launch of before
    const Lz4Chains chains{c.flags,  kBlkPrefixShift, kBlkChained,      kBlkRaw,          n_msgs, mc.first,
                           mc.nb,    mc.route,        kRouteLinkedFast, 1u,               kRouteChainDone};
    e = launch_lz4_decode2(w, c.in_off, c.in_len, p.nb_cap, out, c.out_off, c.out_cap, c.out_len, c.status,
                           w + p.off_inner, stream, nullptr, plan.inner, plan.linked_fast ? &chains : nullptr);
    if (e != hipSuccess) return e;
    // the checksum kernel: block checksums of the listed entries, then (the
    // chains' results and the blocks' places are known) the content checksums
    // of the pending frames; each leaves at once when index counted none
    if ((e = launch_xxh_quads(BlockSumUnits{in, hdr, c}, p.nb_cap, stream)) != hipSuccess) return e;
    lz4f_verdict_kernel<<<plan.verdict_grid, 64, 0, stream>>>(c, p.nb_cap, hdr);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = launch_xxh_quads(ContentUnits{in, in_off, out, out_off, hdr, mc, c}, n_msgs, stream)) != hipSuccess)
      return e;
    inner_fallback = reinterpret_cast<const u32*>(w + p.off_inner) + kL4CtrFallback;  // the block decoder's counter
  }
  lz4f_finish_kernel<<<plan.msg_grid, 64, 0, stream>>>(in, in_off, in_len, n_msgs, out, out_off, out_cap, out_len,
                                                      status, hdr, mc, c, inner_fallback);
  return hipGetLastError();
}

}  // namespace fsg
