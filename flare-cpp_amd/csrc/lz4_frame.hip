// lz4_frame.hip -- LZ4 frame bodies (LZ4 Frame Format 1.6.x, what
// LZ4F_compressFrame and the lz4 command write) on the batch layout of the
// block codec: include/flare_lz4_gpu.h, "LZ4 frames".
//
// A frame with independent blocks is a list of small LZ4 blocks, so the block
// codecs this library already has (lz4.hip, lz4_encode_wave.hip,
// lz4_decode2.hip) run a frame's blocks as if they were messages; the kernels
// here only cut messages into blocks and put frames together (compress), or
// take frames apart and judge the result (decompress).  Those launches are
// called as they are, on the plans the frame's plan holds for them;
// launch_lz4_decode2 alone takes one more argument, for the linked frames
// below.  Workspace layouts, capacities, thresholds and grid sizes:
// lz4_frame_plan.h (tests/cpp/test_lz4_plan.cc).
//
// Compress: plan (a lane per message: its blocks' columns, staging slots from
// two counters) -> launch_lz4_encode on the block columns -> XXH32 of the
// inputs when a content checksum is asked for, and of every block's bytes as
// stored when block checksums are (the checksum kernel, lz4f_xxh.h: a quad of
// lanes per unit) -> assemble (a wave per message: prefix sum of the stored
// sizes, size words, block copies, block checksums, descriptor, end mark).
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
#include "lz4_frame_format.h"
#include "lz4_frame_length.h"
#include "lz4f_xxh.h"
#include "snappy_device.h"

namespace fsg {

namespace {

// ---- workspace header (the first 256 bytes; u32 indices)
// compress
constexpr u32 kFcBlocks = 0;    // blocks asked for (past the capacity when a message did not fit)
constexpr u32 kFcRaw = 1;       // blocks stored raw
constexpr u32 kFcOverflow = 2;  // messages whose blocks did not fit the workspace
constexpr u32 kFcListed = 3;    // blocks of the messages that fitted
constexpr u32 kFcStage = 4;     // u64: staging bytes asked for
// decompress
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

constexpr u32 kNoFit = 0xFFFFFFFFu;

// (the staging slots of a block, enc_slot and dec_slot: lz4_frame_plan.h)

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

// ================================================================ compress

// every block entry: an empty input and a 64-byte slot of its own, so that
// the entries past the batch's blocks encode to nothing anybody reads
__global__ __launch_bounds__(256) void lz4f_prefill_kernel(BlockCols c, u32 nb_cap, u64 dummy_off) {
  const u32 e = blockIdx.x * 256 + threadIdx.x;
  if (e >= nb_cap) return;
  c.in_off[e] = 0;
  c.in_len[e] = 0;
  c.out_off[e] = dummy_off + 64ull * e;
}

__global__ __launch_bounds__(64) void lz4f_plan_kernel(const u64* __restrict__ in_off, const u32* __restrict__ in_len,
                                                     u32 n_msgs, u32 bs, u32* hdr, MsgCols mc, BlockCols c, u32 nb_cap,
                                                     u64 stage_off, u64 stage_cap) {
  const u32 m = blockIdx.x * 64 + threadIdx.x;
  if (m >= n_msgs) return;
  const u32 n = in_len[m];
  const u32 nb = (u32)(((u64)n + bs - 1) / bs);
  mc.nb[m] = nb;
  mc.first[m] = 0;
  if (nb == 0) return;
  const u32 last = n - (nb - 1) * bs;
  const u64 need = (u64)(nb - 1) * enc_slot(bs) + enc_slot(last);
  const u32 base = atomicAdd(&hdr[kFcBlocks], nb);
  u64 sb = atomicAdd(reinterpret_cast<unsigned long long*>(hdr + kFcStage), (unsigned long long)need);
  if ((u64)base + nb > nb_cap || sb + need > stage_cap) {
    mc.first[m] = kNoFit;
    atomicAdd(&hdr[kFcOverflow], 1u);
    return;
  }
  mc.first[m] = base;
  atomicAdd(&hdr[kFcListed], nb);
  const u64 io = in_off[m];
  for (u32 k = 0; k < nb; ++k) {
    const u32 L = k + 1 < nb ? bs : last;
    c.in_off[base + k] = io + (u64)k * bs;
    c.in_len[base + k] = L;
    c.out_off[base + k] = stage_off + sb;
    sb += enc_slot(L);
  }
}

// ---- units of the checksum kernel (lz4f_xxh.h)
// each body of a batch: the content checksum of compress, fsg_lz4f_xxh32_batch
struct BodyUnits {
  const u8* in;
  const u64* in_off;
  const u32* in_len;
  u32 seed;
  u32* xxh;
  __device__ bool any() const { return true; }
  __device__ bool get(u32 m, const u8** p, u64* n, u32* sd) const {
    *p = in + in_off[m];
    *n = in_len[m];
    *sd = seed;
    return true;
  }
  __device__ void put(u32 m, u32 h) const { xxh[m] = h; }
};

// compress, block checksums: every block entry that holds a block (the
// prefilled rest is empty), over the bytes as stored -- the choice of
// lz4f_assemble_kernel; the word goes to src_len, idle on this side
struct StoredUnits {
  const u8* in;
  const u8* ws;
  BlockCols c;
  __device__ bool any() const { return true; }
  __device__ bool get(u32 e, const u8** p, u64* n, u32* sd) const {
    const u32 L = c.in_len[e];
    if (L == 0) return false;
    const u32 hl = (u32)varint32_len(L);
    const u32 csize = c.out_len[e] - hl;
    const bool raw = csize >= L;
    *p = raw ? in + c.in_off[e] : ws + c.out_off[e] + hl;
    *n = raw ? L : csize;
    *sd = 0;
    return true;
  }
  __device__ void put(u32 e, u32 h) const { c.src_len[e] = h; }
};

// One wave per message: the frame from the staged blocks.
__global__ __launch_bounds__(64) void lz4f_assemble_kernel(const u8* __restrict__ in, const u32* __restrict__ in_len,
                                                         u8* out, const u64* __restrict__ out_off,
                                                         u32* __restrict__ out_len, i32* __restrict__ status, u32 id,
                                                         u32 flags, u32* hdr, MsgCols mc, BlockCols c,
                                                         const u8* ws) {
  const u32 m = blockIdx.x;
  const u32 lane = threadIdx.x;
  const u32 n = in_len[m];
  const u32 first = mc.first[m], nb = mc.nb[m];
  if (first == kNoFit || lz4f::max_frame_length(n, id, flags) > 0xFFFFFFFFull) {
    if (lane == 0) {
      out_len[m] = 0;
      status[m] = kCorrupt;
    }
    return;
  }
  u8* const ob = out + out_off[m];
  if (lane == 0) lz4f::write_header(ob, n, id, flags);
  const u32 bsum = (flags & lz4f::kOptBlockSums) ? 4 : 0;
  u64 pos = n && !(flags & lz4f::kOptNoSize) ? 15 : 7;
  u32 raws = 0;
  for (u32 k0 = 0; k0 < nb; k0 += 64) {
    const u32 k = k0 + lane;
    const bool valid = k < nb;
    u32 L = 0, stored = 0, hl = 0;
    bool raw = false;
    u64 src = 0;
    if (valid) {
      const u32 e = first + k;
      L = c.in_len[e];
      hl = (u32)varint32_len(L);
      const u32 csize = c.out_len[e] - hl;
      raw = csize >= L;
      stored = raw ? L : csize;
      src = raw ? c.in_off[e] : c.out_off[e] + hl;
    }
    const u32 sz = valid ? 4 + stored + bsum : 0;
    const u32 incl = wave_scan(sz);
    const u64 at = pos + (incl - sz);
    if (valid) {
      lz4f::wr32(ob + at, raw ? (L | lz4f::kRawBit) : stored);
      if (bsum) lz4f::wr32(ob + at + 4 + stored, c.src_len[first + k]);
    }
    raws += (u32)__builtin_popcountll(__ballot(valid && raw));
    const u32 cnt = nb - k0 < 64 ? nb - k0 : 64;
    for (u32 j = 0; j < cnt; ++j) {
      const u64 s = __shfl(src, j, 64), a = __shfl(at, j, 64);
      const u32 len = __shfl(stored, j, 64);
      const bool r = __shfl((int)raw, j, 64);
      wave_copy(ob + a + 4, (r ? in : ws) + s, len, lane);
    }
    pos += __shfl(incl, 63, 64);
  }
  if (lane == 0) {
    lz4f::wr32(ob + pos, 0);
    pos += 4;
    if (flags & lz4f::kOptContentSum) {
      lz4f::wr32(ob + pos, mc.xxh[m]);
      pos += 4;
    }
    out_len[m] = (u32)pos;
    status[m] = kOk;
    if (raws) atomicAdd(&hdr[kFcRaw], raws);
  }
}

// ================================================================ decompress

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

// The block structure of a frame without a content size, from the size words
// alone: every size at most the block maximum (and not 0, unless zero_raw
// allows an empty raw block, which the serial decoder accepts) and inside the
// input with its block checksum, the end mark, the content checksum when
// flagged, nothing after the frame.  *nb blocks, *need staging bytes for the
// compressed ones, *xxh the stated content checksum.
__device__ inline bool walk_blocks(const u8* ib, u64 n, const lz4f::Header& h, bool zero_raw, u32* nb, u64* need,
                                   u32* xxh) {
  const u32 bsum = (h.flg & lz4f::kFlgBlockSum) ? 4 : 0;
  u64 ip = h.len, nd = 0;
  u32 k = 0;
  for (;; ++k) {
    if (n - ip < 4) return false;
    const u32 word = lz4f::rd32(ib + ip);
    ip += 4;
    if (word == 0) break;
    const u32 sz = word & ~lz4f::kRawBit;
    if ((sz == 0 && !zero_raw) || sz > h.block_max || n - ip < (u64)sz + bsum) return false;
    if (!(word & lz4f::kRawBit)) {
      if (sz == 0) return false;  // a compressed block has a token
      nd += dec_slot(sz);
    }
    ip += sz + bsum;
  }
  *xxh = 0;
  if (h.flg & lz4f::kFlgSum) {
    if (n - ip < 4) return false;
    *xxh = lz4f::rd32(ib + ip);
    ip += 4;
  }
  if (ip != n) return false;
  *nb = k;
  *need = nd;
  return true;
}

// The entries [base, base + nb) of a frame walk_blocks accepted: where the
// stored bytes are, the flags with "length unknown", a staging slot from `at`
// on for a compressed block (at = 0: none, the lengths call).  in_len,
// out_off and out_cap stay 0 -- an empty body for the block decoder -- until
// the place kernel knows the lengths.
__device__ inline void list_unknown(const u8* ib, const lz4f::Header& h, u64 io, u32 nb, u32 base, u64 at,
                                    BlockCols c, u32 more_flags = 0) {
  const u32 bsum = (h.flg & lz4f::kFlgBlockSum) ? 4 : 0;
  const u32 common = kBlkListed | kBlkUnknown | more_flags | (bsum ? kBlkSum : 0) |
                     ((u32)(31 - __builtin_clz(h.block_max)) << kBlkMaxShift);
  u64 ip = h.len;
  for (u32 k = 0; k < nb; ++k) {
    const u32 e = base + k;
    const u32 word = lz4f::rd32(ib + ip);
    const u32 sz = word & ~lz4f::kRawBit;
    const bool raw = word & lz4f::kRawBit;
    ip += 4;
    c.src_off[e] = io + ip;
    c.src_len[e] = sz;
    c.flags[e] = common | (raw ? kBlkRaw : 0);
    if (!raw && at) {
      c.in_off[e] = at;
      at += dec_slot(sz);
    }
    ip += sz + bsum;
  }
}

// One lane per message: descriptor, route, and for the fast route the walk
// over the block size words (two walks: sizes, then columns).
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
  // linked blocks on the fast route: with a content size, or with both options
  const bool linked = !(h.flg & lz4f::kFlgIndep);
  const bool chain = linked && linked_fast && !force_serial && (h.size != lz4f::kNoSize || nosize_fast);
  if (chain && h.size != lz4f::kNoSize && h.size > cap) {  // (the serial decoder answers from the descriptor)
    mc.route[m] = kRouteRejected;
    return;
  }
  if (h.size != lz4f::kNoSize && h.size > cap) {
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
  if (h.size == lz4f::kNoSize) {
    if (!nosize_fast) {
      mc.route[m] = kRouteNoSize;
      return;
    }
    // no content size: the blocks' lengths are unknown until the length pass
    mc.route[m] = kRouteRejected;
    u32 nb, xxh;
    u64 need;
    if (!walk_blocks(ib, n, h, false, &nb, &need, &xxh)) return;
    const u32 base = atomicAdd(&hdr[kFdBlocks], nb);
    const u64 sb = atomicAdd(reinterpret_cast<unsigned long long*>(hdr + kFdStage), (unsigned long long)need);
    if ((u64)base + nb > nb_cap || sb + need > stage_cap) return;
    list_unknown(ib, h, in_off[m], nb, base, stage_off + sb, c, chain ? kBlkChained : 0);
    if (h.flg & lz4f::kFlgBlockSum) atomicAdd(&hdr[kFdSumBlocks], nb);
    if (h.flg & lz4f::kFlgSum) atomicAdd(&hdr[kFdSumMsgs], 1u);
    mc.xxh[m] = xxh;
    mc.first[m] = base;
    mc.nb[m] = nb;
    mc.route[m] = chain ? kRouteLinkedNsFast : kRouteNoSizeFast;
    return;
  }
  // fast route: every block but the last is full
  mc.route[m] = kRouteRejected;
  const u32 bs = h.block_max;
  const u32 bsum = (h.flg & lz4f::kFlgBlockSum) ? 4 : 0;
  const u32 nb = (u32)((h.size + bs - 1) / bs);
  u64 ip = h.len, need = 0;
  for (u32 k = 0; k < nb; ++k) {
    if (n - ip < 4) return;
    const u32 word = lz4f::rd32(ib + ip);
    const u32 sz = word & ~lz4f::kRawBit;
    ip += 4;
    if (sz == 0 || sz > bs || n - ip < (u64)sz + bsum) return;
    const u64 exp = h.size - (u64)k * bs < bs ? h.size - (u64)k * bs : bs;
    if (word & lz4f::kRawBit) {
      if (sz != exp) return;
    } else {
      need += dec_slot(sz);
    }
    ip += sz + bsum;
  }
  if (n - ip < 4 || lz4f::rd32(ib + ip) != 0) return;
  ip += 4;
  if (h.flg & lz4f::kFlgSum) {
    if (n - ip < 4) return;
    mc.xxh[m] = lz4f::rd32(ib + ip);
    ip += 4;
  }
  if (ip != n) return;
  const u32 base = atomicAdd(&hdr[kFdBlocks], nb);
  u64 sb = atomicAdd(reinterpret_cast<unsigned long long*>(hdr + kFdStage), (unsigned long long)need);
  if ((u64)base + nb > nb_cap || sb + need > stage_cap) return;
  const u64 io = in_off[m], oo = out_off[m];
  ip = h.len;
  for (u32 k = 0; k < nb; ++k) {
    const u32 e = base + k;
    const u32 word = lz4f::rd32(ib + ip);
    const u32 sz = word & ~lz4f::kRawBit;
    const bool raw = word & lz4f::kRawBit;
    ip += 4;
    const u32 exp = (u32)(h.size - (u64)k * bs < bs ? h.size - (u64)k * bs : bs);
    c.src_off[e] = io + ip;
    c.src_len[e] = sz;
    c.out_off[e] = oo + (u64)k * bs;
    c.out_cap[e] = exp;
    c.flags[e] = kBlkListed | (raw ? kBlkRaw : 0) | (bsum ? kBlkSum : 0) |
                 (chain ? kBlkChained | (lz4f::linked_prefix((u64)k * bs) << kBlkPrefixShift) : 0);
    if (!raw) {
      c.in_off[e] = stage_off + sb;
      c.in_len[e] = (u32)varint32_len(exp) + sz;
      sb += dec_slot(sz);
    }
    ip += sz + bsum;
  }
  if (bsum) atomicAdd(&hdr[kFdSumBlocks], nb);
  if (h.flg & lz4f::kFlgSum) atomicAdd(&hdr[kFdSumMsgs], 1u);
  mc.first[m] = base;
  mc.nb[m] = nb;
  mc.route[m] = chain ? kRouteLinkedFast : kRouteFast;
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
// walked here.
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
  u32 nb, xxh;
  u64 need;
  if (!walk_blocks(ib, n, h, true, &nb, &need, &xxh)) {
    status[m] = kCorrupt;
    return;
  }
  if (nb == 0) return;
  const u32 base = atomicAdd(&hdr[kFdBlocks], nb);
  if ((u64)base + nb <= nb_cap) {
    list_unknown(ib, h, in_off[m], nb, base, 0, c);
    mc.first[m] = base;
    mc.nb[m] = nb;
    mc.route[m] = kRouteNoSizeFast;
    return;
  }
  const u32 bsum = (h.flg & lz4f::kFlgBlockSum) ? 4 : 0;
  u64 ip = h.len, total = 0;
  for (u32 k = 0; k < nb; ++k) {
    const u32 word = lz4f::rd32(ib + ip);
    const u32 sz = word & ~lz4f::kRawBit;
    ip += 4;
    u64 len = sz;
    if (!(word & lz4f::kRawBit) && !lz4f::block_length(ib + ip, sz, h.block_max, &len)) {
      status[m] = kCorrupt;
      return;
    }
    total += len;
    ip += sz + bsum;
  }
  lengths[m] = total;
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
  if (route == kRouteFast || route == kRouteLinkedOk) {
    const u32 first = mc.first[m], nb = mc.nb[m];
    bool ok = true;
    for (u32 k = 0; k < nb && ok; ++k) ok = !(c.flags[first + k] & kBlkFailed);
    lz4f::Header h;
    lz4f::parse_header(ib, in_len[m], &h);
    if (ok && (h.flg & lz4f::kFlgSum)) {
      ok = mc.xxh[m] == 0;  // (the checksum kernel left computed ^ stated)
      sums = 1;
    }
    if (ok) {
      out_len[m] = (u32)h.size;
      status[m] = kOk;
      blocks = nb;
    } else {
      route = kRouteRejected;
    }
  } else if (route == kRouteNoSizeFast || route == kRouteLinkedNsOk) {
    // the blocks lie end to end from the slot's start: decoded exactly the
    // lengths the walk found, and the checksum over them
    const u32 first = mc.first[m], nb = mc.nb[m], last = first + nb - 1;
    bool ok = true;
    for (u32 k = 0; k < nb && ok; ++k) ok = !(c.flags[first + k] & kBlkFailed);
    const u32 total = (u32)(c.out_off[last] + c.out_cap[last] - out_off[m]);
    lz4f::Header h;
    lz4f::parse_header(ib, in_len[m], &h);
    if (ok && (h.flg & lz4f::kFlgSum)) {
      ok = mc.xxh[m] == 0;
      sums = 1;
    }
    if (ok) {
      out_len[m] = total;
      status[m] = kOk;
      ns_blocks = nb;
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

// ---- the columns in a workspace (offsets and sizes: lz4_frame_plan.h)
MsgCols msg_cols(u8* w, u32 n_msgs) {
  MsgCols mc;
  const u64 lb = lz4f_list_bytes(n_msgs);
  mc.route = reinterpret_cast<u32*>(w);
  mc.first = reinterpret_cast<u32*>(w + lb);
  mc.nb = reinterpret_cast<u32*>(w + 2 * lb);
  mc.xxh = reinterpret_cast<u32*>(w + 3 * lb);
  return mc;
}
BlockCols block_cols(u8* w, u64 nb) {
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

void lz4f_encode_header_counts(const void* header, Lz4fEncodeHeaderCounts* c) {
  u32 ctr[8];
  __builtin_memcpy(ctr, header, sizeof(ctr));
  c->blocks = ctr[kFcListed];
  c->raw_blocks = ctr[kFcRaw];
  c->overflow_messages = ctr[kFcOverflow];
}
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

// every size and decision from lz4f_encode_plan (lz4_frame_plan.h)
hipError_t launch_lz4f_encode(const u8* in, const u64* in_off, const u32* in_len, u32 n_msgs, u8* out,
                              const u64* out_off, u32* out_len, i32* status, u32 id, u32 flags, void* ws,
                              hipStream_t stream, const Lz4fEncodePlan& plan) {
  if (n_msgs == 0) return hipSuccess;
  if (!plan.valid) return hipErrorInvalidValue;
  const Lz4fLayout& p = plan.w;
  u8* const w = static_cast<u8*>(ws);
  u32* const hdr = reinterpret_cast<u32*>(w);
  const MsgCols mc = msg_cols(w + p.off_msg, n_msgs);
  const BlockCols c = block_cols(w + p.off_blk, p.nb_cap);
  const u32 bs = lz4f::block_bytes(id);
  hipError_t e = hipMemsetAsync(w, 0, kLz4fHead, stream);
  if (e != hipSuccess) return e;
  lz4f_prefill_kernel<<<plan.prefill_grid, 256, 0, stream>>>(c, p.nb_cap, p.off_dummy);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  lz4f_plan_kernel<<<plan.plan_grid, 64, 0, stream>>>(in_off, in_len, n_msgs, bs, hdr, mc, c, p.nb_cap, p.off_stage,
                                                     p.stage_cap);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  // the block encoders on the block columns, with their own routing
  e = launch_lz4_encode(in, c.in_off, c.in_len, p.nb_cap, w, c.out_off, c.out_len, c.status, w + p.off_inner, stream,
                        plan.inner);
  if (e != hipSuccess) return e;
  // the checksum kernel: the messages, and the entries' bytes as stored
  if (flags & lz4f::kOptContentSum) {
    if ((e = launch_xxh_quads(BodyUnits{in, in_off, in_len, 0u, mc.xxh}, n_msgs, stream)) != hipSuccess) return e;
  }
  if (flags & lz4f::kOptBlockSums) {
    if ((e = launch_xxh_quads(StoredUnits{in, w, c}, p.nb_cap, stream)) != hipSuccess) return e;
  }
  lz4f_assemble_kernel<<<plan.assemble_grid, 64, 0, stream>>>(in, in_len, out, out_off, out_len, status, id, flags, hdr,
                                                             mc, c, w);
  return hipGetLastError();
}

hipError_t launch_lz4f_xxh32(const u8* in, const u64* in_off, const u32* in_len, u32 n_msgs, u32 seed, u32* xxh,
                             hipStream_t stream) {
  return launch_xxh_quads(BodyUnits{in, in_off, in_len, seed, xxh}, n_msgs, stream);
}

hipError_t launch_lz4f_content_sizes(const u8* in, const u64* in_off, const u32* in_len, u32 n_msgs, u64* sizes,
                                     i32* status, hipStream_t stream) {
  if (n_msgs == 0) return hipSuccess;
  lz4f_sizes_kernel<<<(n_msgs + 63) / 64, 64, 0, stream>>>(in, in_off, in_len, n_msgs, sizes, status);
  return hipGetLastError();
}

namespace {
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
