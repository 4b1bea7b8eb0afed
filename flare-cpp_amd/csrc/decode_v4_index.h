// decode_v4_index.h -- pass 1 of the two-pass Snappy decoder
// (snappy_decode_v4.hip): the lane walk, one LANE per message.  It checks a
// message's header and tags without touching output and leaves its status
// and its tag-start bitmap.  The launch uses index_kernel (the walk) and, for
// batches whose large messages go to side streams, index_plan_kernel,
// walk_offsets_kernel and walk_scatter_kernel (the size-ordered walk);
// index_prologue's bitmap test is repeated by fallback_kernel.
#pragma once

#include "decode_v4_plan.h"
#include "snappy_pieces.h"
#include "wave_util.h"

namespace fsg {

namespace {

// ---- pass 1 geometry (per-lane LDS ring of input chunks, as v3)
// tags per iteration of the lane walk: 32 for single-stream batches (C3
// 7.37 -> 7.33 ms), 24 for the planned large-batch walk (CM +1.8% at 32)
constexpr int kIdxTagsOne = 32, kIdxTagsPlanned = 24;
constexpr u32 kRingChunks = 16;              // 16-byte chunks per lane (256 B)
constexpr u32 kAhead = 7;                    // chunks prefetched per iteration
// (kIdxWaves, kIdxWavesSerial -- waves per pass-1 workgroup --, the size
// thresholds kBigIndexMin/Max and kHugeIndexBytes, kWavesPerBlock and
// kSingleLiteral: decode_v4_plan.h, with the launch arithmetic that uses them)

// what a lane without input prefetches
__device__ u32x4 g_dummy_chunk[1];

// ---- the walk's tag rule (the role of char_table, snappy.cc:516-549): per
// tag byte c the advance (tag byte + extra bytes + a short literal's bytes,
// <= kMaxAdv) and the output length (<= kMaxLen).  The four long literal tags
// (0xF0, 0xF4, 0xF8, 0xFC) have advance and length 0, which is also their
// flag: the unrolled walk stays on such a tag and the long-literal path after
// it takes the length from the ring.  Every other advance is non-zero.
constexpr u32 kMaxAdv = 65, kMaxLen = 64;
struct TagRule {
  u32 adv, len;
};
__host__ __device__ constexpr TagRule tag_rule(u32 c) {
  const u32 type = c & 3, l0 = (c >> 2) + 1;
  if (type == 0) return l0 > 60 ? TagRule{0, 0} : TagRule{1 + l0, l0};
  if (type == 1) return TagRule{2, 4 + ((c >> 2) & 7)};
  return TagRule{type == 2 ? 3u : 5u, l0};
}
// The walk does not look the advance up: it computes it, already shifted to
// the position field of its accumulator (bit kPosShift), from a "pick" byte
// -- c itself for a literal, (advance - 2) * 4 for a copy, taken by one bit
// field extract at 8 * type out of c | kAdvPick -- as (pick << 4) + (2 << 6).
// Long literals and lanes past their limit do not advance (tag_stay).
constexpr u32 kPosShift = 6;
constexpr u32 kAdvPick = 0x0c040000u;  // bytes 1-3: (advance - 2) * 4 of copy types 1-3
// byte (c & 3) of w
__host__ __device__ constexpr u32 type_byte(u32 w, u32 c) {
#if defined(__HIP_DEVICE_COMPILE__)
  // (v_bfe_u32 takes the low 5 bits of its offset; written out, the compiler
  // makes four instructions of the line below)
  if (!__builtin_is_constant_evaluated()) return __builtin_amdgcn_ubfe(w, c << 3, 8);
#endif
  return (w >> ((c << 3) & 31u)) & 0xffu;
}
__host__ __device__ constexpr u32 tag_pick(u32 c) { return type_byte(c | kAdvPick, c); }
__host__ __device__ constexpr bool tag_stay(u32 c, u32 thr = 1) { return ((c & 0xf3u) ^ 0xf0u) < thr; }
__host__ __device__ constexpr u32 tag_advance(u32 c) {
  return tag_stay(c) ? 0u : (tag_pick(c) << (kPosShift - 2)) + (2u << kPosShift);
}
constexpr bool tag_advance_is_rule() {
  for (u32 c = 0; c < 256; ++c)
    if (tag_advance(c) != tag_rule(c).adv << kPosShift || tag_rule(c).adv > kMaxAdv || tag_rule(c).len > kMaxLen) return false;
  return true;
}
static_assert(tag_advance_is_rule(), "the computed advance differs from the tag rule");

}  // namespace

// ===========================================================================
// Pass 1: index + validate.  One lane per message.
// Bump allocation of `total` (this wave's sum) from *counter with one atomic
// per workgroup: every thread of the block calls it; blk is LDS scratch of
// (waves + 1) words.  Returns the wave's base.  A device-scope atomic on one
// address is serialised across the chip: one per wave cost the 1M-message
// plan pass ~0.25 ms.
__device__ __forceinline__ u32 block_bump(u32 total, u32* counter, u32* blk) {
  const u32 wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
  if ((threadIdx.x & 63) == 0) blk[wv] = total;
  __syncthreads();
  if (threadIdx.x == 0) {
    u32 t = 0;
    for (u32 w = 0; w < nw; ++w) {
      const u32 x = blk[w];
      blk[w] = t;
      t += x;
    }
    blk[nw] = t ? atomicAdd(counter, t) : 0u;
  }
  __syncthreads();
  const u32 r = blk[nw] + blk[wv];
  __syncthreads();
  return r;
}

// ===========================================================================
// Per-lane start of pass 1 (one message per lane, the whole wave calling):
// header (ReadUncompressedLength / Parse32WithLimit), slot check, the
// message's bitmap words (bump-allocated per wave), and the large-message
// list.  Returns the status (< 0: the lane walk follows) and sets the
// header length, expected length and bitmap base.
__device__ __forceinline__ i32 index_prologue(
    const u8* ib, u32 n_in, bool valid_msg, u32 m, u32 lane, u32 n_msgs, u32 flags,
    const u32* __restrict__ out_cap, u32* __restrict__ out_len, u32* __restrict__ bm_counter,
    u32* __restrict__ bm_base_out, u32* __restrict__ bitmap, u64 bm_capacity_words,
    u32* __restrict__ big_count, u32* __restrict__ big_list, u32 big_threshold, u32* ip,
    u32* expected, u32* bm_base_ret, u32* blk = nullptr) {
  const bool strict = flags & 2u;
  const bool validate = flags & 1u;
  i32 status = kOk;  // < 0: parsing
  if (valid_msg) {
    u32 ulen = 0;
    const int h = parse_varint_header(ib, n_in, strict, &ulen);
    if (h == 0) {
      status = kBadHeader;
      out_len[m] = 0;
    } else {
      out_len[m] = ulen;
      *expected = ulen;
      *ip = (u32)h;
      status = (!validate && ulen > out_cap[m]) ? kSlotTooSmall : -1;
    }
  }

  // ---- bitmap allocation: round_up(ceil(n_in / 32), 4) words, bump-allocated
  // per wave (order is irrelevant; bases stay 16-byte aligned)
  u32 bm_base = 0;
  if (bitmap) {
    const u32 words = status < 0 ? (((n_in + 31) >> 5) + 3) & ~3u : 0u;
    const u32 incl = wave_incl_scan(words);
    const u32 total = readlane(incl, 63);
    u32 base0 = 0;
    if (blk) {
      base0 = block_bump(total, bm_counter, blk);
    } else {
      if (lane == 0 && total) base0 = atomicAdd(bm_counter, total);
      base0 = readlane(base0, 0);
    }
    bm_base = base0 + incl - words;
    if (status < 0 && (u64)bm_base + words > bm_capacity_words) status = kNeedFallback;
    if (valid_msg) bm_base_out[m] = bm_base;
  }
  *bm_base_ret = bm_base;

  // ---- large messages go to index_big_message (a whole wave per message);
  // one lane would walk them serially for tens of milliseconds
  if (big_list) {
    // the largest ones (> kHugeIndexBytes) are listed from the end of the
    // list so both large-message passes hand them out first
    const bool big = status < 0 && n_in > big_threshold;
    const bool huge = big && n_in > kHugeIndexBytes;
    const u64 bb = __ballot(big && !huge), bh = __ballot(huge);
    const u64 below = (1ull << lane) - 1;
    if (bb) {
      u32 base1 = 0;
      if (lane == 0) base1 = atomicAdd(big_count, (u32)__builtin_popcountll(bb));
      base1 = readlane(base1, 0);
      if (big && !huge) big_list[base1 + (u32)__builtin_popcountll(bb & below)] = m;
    }
    if (bh) {
      u32 base2 = 0;
      if (lane == 0) base2 = atomicAdd(big_count + 8, (u32)__builtin_popcountll(bh));
      base2 = readlane(base2, 0);
      if (huge) big_list[n_msgs - 1 - (base2 + (u32)__builtin_popcountll(bh & below))] = m;
    }
    if (big) status = kNeedBigIndex;
  }
  return status;
}

// Size classes of the planned lane walk (kWalkClasses of them, see
// index_plan_kernel).
__device__ __forceinline__ u32 walk_class(u32 n_in) {
  const u32 lg = 31u - (u32)__builtin_clz(n_in | 1u);
  return kWalkClasses - 1 - (lg < kWalkClasses - 1 ? lg : kWalkClasses - 1);
}

// Pass 1 plan (batches whose large messages are indexed on a side stream):
// the prologue alone, so pass 1b can start on the listed large messages while
// the lane walk (index_kernel<true>) runs; lanes left for the walk get
// kNeedLaneWalk.  (kPlanThreads per block.)
__global__ __launch_bounds__(kPlanThreads) void index_plan_kernel(
    const u8* __restrict__ in, const u64* __restrict__ in_off,
    const u32* __restrict__ in_len, u32 n_msgs, const u32* __restrict__ out_cap,
    u32* __restrict__ out_len, i32* __restrict__ status_out, u32 flags,
    u32* __restrict__ bm_counter, u32* __restrict__ bm_base_out,
    u32* __restrict__ bitmap, u64 bm_capacity_words, u32* __restrict__ big_count,
    u32* __restrict__ big_list, u32 big_threshold, u32* __restrict__ walk_rank,
    u32* __restrict__ walk_hist) {
  __shared__ u32 blk[kPlanThreads / 64 + 1];
  __shared__ u32 hist[kWalkClasses], hbase[kWalkClasses];
  const u32 lane = threadIdx.x & 63;
  const u32 m = blockIdx.x * kPlanThreads + threadIdx.x;
  const bool valid_msg = m < n_msgs;
  const u8* ib = valid_msg ? in + in_off[m] : in;
  const u32 n_in = valid_msg ? in_len[m] : 0u;
  u32 ip = 0, expected = 0, bm_base = 0;
  if (threadIdx.x < kWalkClasses) hist[threadIdx.x] = 0;
  __syncthreads();
  const i32 st = index_prologue(ib, n_in, valid_msg, m, lane, n_msgs, flags, out_cap, out_len,
                                bm_counter, bm_base_out, bitmap, bm_capacity_words, big_count,
                                big_list, big_threshold, &ip, &expected, &bm_base, blk);
  if (valid_msg) status_out[m] = st < 0 ? kNeedLaneWalk : st;
  if (!walk_rank) return;
  // Size classes for the lane walk (a wave's walk lasts as long as its
  // longest message): class = 15 - floor(log2(compressed size)), so the
  // largest come first; rank within the class from a per-class counter.
  const bool walk = valid_msg && st < 0;
  const u32 cls = walk_class(n_in);
  u32 mine = 0, below_mask_cnt = 0;
#pragma unroll
  for (u32 c = 0; c < kWalkClasses; ++c) {
    const u64 b = __ballot(walk && cls == c);
    const u32 cnt = (u32)__builtin_popcountll(b);
    if (lane == c) mine = cnt;
    if (cls == c) below_mask_cnt = (u32)__builtin_popcountll(b & ((1ull << lane) - 1));
  }
  // per-class ranks: this wave's base inside the block (LDS atomics), then
  // one global atomic per class per block
  u32 base = 0;
  if (lane < kWalkClasses && mine) base = atomicAdd(&hist[lane], mine);
  __syncthreads();
  if (threadIdx.x < kWalkClasses) {
    const u32 h = hist[threadIdx.x];
    hbase[threadIdx.x] = h ? atomicAdd(&walk_hist[threadIdx.x], h) : 0u;
  }
  __syncthreads();
  base = (u32)__shfl((int)base, (int)(cls & (kWalkClasses - 1)), 64);
  if (walk) walk_rank[m] = hbase[cls & (kWalkClasses - 1)] + base + below_mask_cnt;
}

// Class offsets of the size-ordered lane walk (one block): exclusive prefix
// of the per-class counts, and the number of messages to walk.
__global__ __launch_bounds__(64) void walk_offsets_kernel(u32* __restrict__ walk_hist) {
  const u32 lane = threadIdx.x;
  const u32 v = lane < kWalkClasses ? walk_hist[lane] : 0u;
  const u32 inc = wave_incl_scan(v);
  if (lane < kWalkClasses) walk_hist[kWalkClasses + lane] = inc - v;
  if (lane == 63) walk_hist[2 * kWalkClasses] = inc;
}

// Lane-walk order: perm[offset(class) + rank] = m for every message to walk.
__global__ __launch_bounds__(256) void walk_scatter_kernel(
    const u32* __restrict__ in_len, u32 n_msgs, const i32* __restrict__ status,
    const u32* __restrict__ walk_rank, const u32* __restrict__ walk_hist, u32* __restrict__ perm) {
  const u32 m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= n_msgs || status[m] != kNeedLaneWalk) return;
  perm[walk_hist[kWalkClasses + walk_class(in_len[m])] + walk_rank[m]] = m;
}

// kPlanned: index_plan_kernel ran first (statuses, bitmap bases and the
// large-message list are in place; only kNeedLaneWalk messages are walked).
template <bool kPlanned, bool kLean = false, u32 kW = kIdxWaves>
__global__ __launch_bounds__(64 * kW)
__attribute__((amdgpu_waves_per_eu(kLean ? 6 : 1))) void index_kernel(
    const u8* __restrict__ in, const u64* __restrict__ in_off,
    const u32* __restrict__ in_len, u32 n_msgs, const u32* __restrict__ out_cap,
    u32* __restrict__ out_len, i32* __restrict__ status_out, u32 flags,
    u32* __restrict__ bm_counter, u32* __restrict__ bm_base_out,
    u32* __restrict__ bitmap, u64 bm_capacity_words, u32* __restrict__ big_count,
    u32* __restrict__ big_list, u32 big_threshold, const u32* __restrict__ walk_perm,
    const u32* __restrict__ walk_hist, u32 walk_part = 0, u32 split_class = 0) {
  // Lean geometry (the two-stream form, whose walk runs beside the previous
  // batch's execution pass in the CU resources that pass leaves free: <= 80
  // VGPRs, 12.3 KB of LDS): an 8-chunk input ring, 16 tags per iteration, 4
  // chunks prefetched, 2 bit groups (an iteration's tags lie within the 128
  // bytes the ring holds, so within 2 groups of 128 input bytes).
  constexpr int kIdxTags = kLean ? 16 : (kPlanned ? kIdxTagsPlanned : kIdxTagsOne);
  constexpr u32 kRC = kLean ? 8 : kRingChunks, kRD = kRC * 4, kAH = kLean ? 4 : kAhead;
  // Bit groups (4 words each) per lane.  The one-stream walk (C2, C3) stores
  // its groups four at a time (kSuper: 64 bytes of bitmap, 512 input bytes,
  // as four back-to-back 16-byte stores of one lane), so the L2 merges them
  // into whole lines: stored one at a time, ~18 us apart, a lane's groups
  // left the XCD's L2 between stores and every 16-byte store cost a line
  // write (0.90 GB written for C3's 0.27 GB bitmap).  Its ring
  // then holds 8 groups: the groups since the last stored super-group (<= 3)
  // plus the <= 3 an iteration spans.
  constexpr bool kSuper = !kPlanned && !kLean;
  constexpr u32 kBG = kLean ? 2 : (kSuper ? 8 : 4), kBW = 4 * kBG;
  // per wave, [dword][lane]; dwords kRD + 1 .. kRD + 4 absorb unused
  // prefetches (dword kRD is not used)
  // The lean form takes its LDS dynamically (idx_lean_lds_bytes(), given at
  // launch): with a compile-time size the compiler sizes the VGPR allocation
  // for the occupancy that LDS alone would allow (97 registers reserved for
  // 52 used), too many to fit beside the execution pass's waves.
  extern __shared__ u32 idx_dyn_lds[];
  __shared__ u32 ring_s[kLean ? 1 : kW][kLean ? 1 : (kRD + 5) * kWave];
  __shared__ u8 lentab_s[kLean ? 1 : 256];
  __shared__ u32 bmr_s[kLean ? 1 : kW][kLean ? 1 : kBW * kWave];
  const u32 wv = (u32)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  u32* const ring = kLean ? idx_dyn_lds + wv * (kRD + 5) * kWave : ring_s[wv];
  // (lean: the first 256 bytes of the 256 words idx_lean_lds_bytes() keeps between the rings)
  u8* const lentab = kLean ? reinterpret_cast<u8*>(idx_dyn_lds + kW * (kRD + 5) * kWave) : lentab_s;
  u32* const bmr = kLean ? idx_dyn_lds + kW * (kRD + 5) * kWave + 256 + wv * kBW * kWave : bmr_s[wv];

  const u32 lane = threadIdx.x & 63;
  // The unrolled walk addresses both rings from the workgroup's first wave, so
  // the array's LDS address folds into the instruction and the wave's share
  // into one per-lane term: ring byte P of this lane is
  // ring_b0[(dword << 8) + ((P & 3) | ring_lane)], bit word w is
  // bmr_w0[(w << 6) + bmr_lane].
  constexpr u32 kRDlog = kLean ? 5 : 6, kBWlog = kLean ? 3 : (kSuper ? 5 : 4);
  static_assert(kRD == 1u << kRDlog && kBW == 1u << kBWlog, "ring sizes are powers of two");
  const u8* const ring_b0 = reinterpret_cast<const u8*>(kLean ? idx_dyn_lds : &ring_s[0][0]);
  u32* const bmr_w0 = kLean ? idx_dyn_lds + kW * (kRD + 5) * kWave + 256 : &bmr_s[0][0];
  const u32 ring_lane = (wv * (kRD + 5) * kWave + lane) * 4, bmr_lane = wv * kBW * kWave + lane;
  // The walk's accumulator holds the ring position at bit kPosShift = 6
  // (tag_advance gives the advance there), so that the position field,
  // masked, IS the ring address of its dword ([dword][lane]: byte P of a lane
  // is at (P >> 2) * 256 + lane * 4 + (P & 3), and ((P << 6) & 0x3f00) is the
  // first term).  It starts an iteration at the low 8 bits of the ring
  // position and advances by at most kMaxDist (the clamp of the limit) plus
  // one tag: it stays inside bits 6-15, the half the limit compare looks at.
  // The iteration's output length is summed in a register of its own.
  constexpr u32 kMaxDist = 255;
  static_assert(255 + kMaxDist + kMaxAdv < (1u << (16 - kPosShift)), "position field of the accumulator overflows");
  static_assert(kIdxTags * kMaxLen <= 0xffffu, "an iteration's length sum overflows");
  // Length table: tag_rule(c).len per tag byte, read when the byte arrives
  // and added in the shadow of the next byte's read (off the tag-to-tag
  // chain).
#pragma unroll
  for (u32 q = 0; q < 4 / kW; ++q) {
    const u32 c = threadIdx.x * (4 / kW) + q;
    lentab[c] = (u8)tag_rule(c).len;
  }
  __syncthreads();
  // planned with a walk order: lane g walks message walk_perm[g], the
  // messages grouped by size class so a wave's lanes finish together
  const u32 gid = blockIdx.x * blockDim.x + threadIdx.x;
  // (walk_part 1 / 2: only the walk order's positions below / from the
  // first one of class split_class -- the larger / the smaller bodies)
  const bool ordered = kPlanned && walk_perm;
  const u32 n_walk = ordered ? walk_hist[2 * kWalkClasses] : n_msgs;
  // (split_class bits 8-15, when set: the first class another pass takes --
  // positions from its first one are not walked here; no pass sets it now)
  const u32 tcls = split_class >> 8;
  const u32 split = walk_part ? walk_hist[kWalkClasses + (split_class & 0xffu)] : 0u;
  const u32 t_hi = tcls ? walk_hist[kWalkClasses + tcls] : n_walk;
  const u32 w_lo = walk_part == 2 ? split : 0u, w_hi = walk_part == 1 ? split : t_hi;
  const bool valid_msg = ordered ? gid < w_hi - w_lo : gid < n_walk;
  const u32 m = ordered ? (valid_msg ? walk_perm[w_lo + gid] : 0u) : gid;

  const u8* ib = valid_msg ? in + in_off[m] : in;
  const u32 n_in = valid_msg ? in_len[m] : 0u;
  u32 expected = 0, ip = 0, bm_base = 0;
  i32 status = kOk;
  if (!kPlanned) {
    __shared__ u32 blk_s[kW + 1];
    status = index_prologue(ib, n_in, valid_msg, m, lane, n_msgs, flags, out_cap, out_len,
                            bm_counter, bm_base_out, bitmap, bm_capacity_words, big_count, big_list,
                            big_threshold, &ip, &expected, &bm_base, kW > 1 ? blk_s : nullptr);
  } else if (valid_msg && status_out[m] == kNeedLaneWalk) {
    u32 ulen = 0;
    ip = (u32)parse_varint_header(ib, n_in, flags & 2u, &ulen);  // valid: checked by the plan
    expected = ulen;
    bm_base = bitmap ? bm_base_out[m] : 0u;
    status = -1;
  }
  const bool walked = status < 0;  // (planned: the other lanes' statuses stand)
  // Planned without a walk order (option walk_order 0) the lanes cover every
  // message, also those the plan gave a final status or listed for pass 1b:
  // such a lane keeps kOk and bitmap base 0 here and has its input length, so
  // with a bitmap pointer it would store ceil(n_in / 128) zero groups over
  // the words of whichever messages were allocated first.  No pointer for it.
  u32* bm = bitmap && (!kPlanned || walked) ? bitmap + bm_base : nullptr;

  const u32 ibal = (u32)(reinterpret_cast<uintptr_t>(ib) & 15);
  const u8* abase = ib - ibal;
  const u32 last_chunk = n_in ? (ibal + n_in - 1) >> 4 : 0u;

  u32 wend = 0, iend = 0;
  auto ring_write = [&](u32 k, u32x4 v, bool live) {
    const u32 d = live ? (k & (kRC - 1)) * 4 : kRD + 1;
#pragma unroll
    for (int i = 0; i < 4; ++i) ring[(d + i) * kWave + lane] = v[i];
  };
  // Single-literal message (random bodies: the encoder emits one literal when
  // it finds no match): its first tag is a literal whose bytes end the input.
  // Decided here from the first chunks, once per message; pass 2 copies such
  // a message without walking the bitmap (bm_base = kSingleLiteral | source).
  u32 single_src = 0;
  if (status < 0) {
    u32x4 c0[4];
#pragma unroll
    for (u32 c = 0; c < 4; ++c) {
      const u32 k = c <= last_chunk ? c : last_chunk;
      c0[c] = *reinterpret_cast<const u32x4*>(abase + 16 * k);
    }
#pragma unroll
    for (u32 c = 0; c < 4; ++c) ring_write(c, c0[c], c <= last_chunk);
    wend = iend = (last_chunk + 1 < 4) ? last_chunk + 1 : 4;
    // tag byte at ip (header <= 5 bytes) and its <= 4 length bytes lie in the
    // first 32 bytes of the aligned chunks (ibal + 9 < 32)
    const u32 P = ip + ibal;
    const u32 w[8] = {c0[0][0], c0[0][1], c0[0][2], c0[0][3], c0[1][0], c0[1][1], c0[1][2], c0[1][3]};
    const u32 d = P >> 2;
    const u32 w0 = mux8(w, d), w1 = mux8(w, d + 1), w2 = d + 2 < 8 ? mux8(w, d + 2) : 0u;
    const u32 t0 = alignbyte(w1, w0, P & 3);
    const u32 ext = alignbyte(alignbyte(w2, w1, P & 3), t0, 1);
    const u32 c = t0 & 0xffu;
    const u32 l0 = (c >> 2) + 1;
    const u32 nbl = l0 > 60 ? l0 - 60 : 0u;
    const u32 val = ext & (0xffffffffu >> ((32 - 8 * nbl) & 31));
    const u32 len = nbl ? val + 1u : l0;
    const u64 end = (u64)ip + 1 + nbl + len;
    if ((c & 3) == 0 && end == n_in && ip < n_in && len == expected) single_src = ip + 1 + nbl;
  }

  u32 op = 0;
  // Tag-start bits go to a per-lane LDS ring of 4 groups of 128 input bytes
  // (group g in slot g & 3, [word][lane]) by a fire-and-forget ds_or; a group
  // is stored to the bitmap (if it holds bits) once the walk has left it.  One
  // iteration covers at most 3 groups (the input ring spans 256 bytes, and a
  // long literal that leaves it ends the lane's iteration).
#pragma unroll
  for (u32 q = 0; q < kBW; ++q) bmr[q * kWave + lane] = 0;
  u32 fg = 0;  // lowest group that may still hold unstored bits

  u32x4 g[kAH];
#pragma unroll
  for (u32 c = 0; c < kAH; ++c) g[c] = u32x4{0, 0, 0, 0};
  u32 gk_w = 0, gn_w = 0;

  __builtin_amdgcn_s_waitcnt(0);
  bool more = __any(status < 0);
  while (more) {
    // ---------- parse up to kIdxTags tags from the ring
    // a tag at ip is parsed this iteration iff ip < lim: still parsing, before
    // the end of input, and its 5 bytes are in the ring
    u32 lim = 0;
    if (status < 0) {
      const u32 ring_end = 16 * wend >= 4 + ibal ? 16 * wend - 4 - ibal : 0u;
      lim = (wend > last_chunk || ring_end > n_in) ? n_in : ring_end;
    }
    // The unrolled walk keeps the ring position in bits 6-15 of one
    // accumulator (the low 8 bits of ip + ibal at the iteration's start, plus
    // the advance since; the static_asserts above bound it) and the output
    // length of the iteration so far in another register.  A tag costs one
    // byte read of the ring on the tag-to-tag chain; the advance is computed
    // from the byte (tag_advance), the length read from the table beside the
    // chain; the walk never looks at a copy's offset bytes.
    // The 16-bit compare `pos < lim_pos` is `ip < lim`.  The limit's distance
    // is clamped to kMaxDist: the ring holds no more than 256 bytes from the
    // start, and a tag the clamp cuts off waits for the next iteration.
    const u32 op_it = op;
    const u32 pos_it = (ip + ibal) & 255u;
    const u32 ip_base = ip - pos_it;  // ip = ip_base + position field (mod 2^32)
    const u32 dist = lim > ip ? lim - ip : 0u;
    const u16 lim_pos = (u16)((pos_it + (dist < kMaxDist ? dist : kMaxDist)) << kPosShift);
    auto tag_read = [&](u32 a) -> u32 {
      return ring_b0[(a & ((kRD - 1) << 8)) + (__builtin_amdgcn_ubfe(a, kPosShift, 2) | ring_lane)];
    };
    // Software-pipelined: tag j+1's ring read is issued before tag j's ds_or
    // and length add, so the LDS latency overlaps them.  The read after the
    // last tag shows the long-literal path what the lane stands on.
    u32 acc = pos_it << kPosShift, len_it = 0;
    u32 c = tag_read(acc);
    // What a step knows before its byte arrives is prepared while the read
    // is in flight: the limit compare (a lane past its limit stays, by the
    // threshold of tag_stay) and the position plus the advance's constant 2.
    bool look = (u16)acc < lim_pos;
    u32 thr = look ? 1u : 0x100u, acc2 = acc + (2u << kPosShift);
    // (the empty statements and the scheduling barrier pin that order, which
    // the compiler's scheduler does not keep: everything above such a
    // statement is issued before the wait for c)
    asm volatile("" : "+v"(c), "+v"(thr), "+v"(acc2));
#pragma unroll
    for (int j = 0; j < kIdxTags; ++j) {
      // The walk advances over every tag below lim whether or not it will
      // pass the iteration's checks, so they stay off the dependency chain.
      // A long literal does not advance: the lane stays on it, looks at it
      // again in every remaining slot and ORs the same bit again.
      const u32 len_rd = lentab[c];
      const bool stay = tag_stay(c, thr);
      u32 acc_next = stay ? acc : (tag_pick(c) << (kPosShift - 2)) + acc2;
      // (opaque: knowing that a staying lane reads the byte it has, the
      // compiler turns the select into a branch around the read)
      asm volatile("" : "+v"(acc_next));
      const u32 c_next = tag_read(acc_next);
      __builtin_amdgcn_sched_barrier(0);
      // ---- in the shadow of that read: the tag's bit, its length, and the
      // next step's preparation
      u32 len = len_rd;
      asm volatile("" : "+v"(len), "+v"(acc_next));
      const u32 at = ip_base + __builtin_amdgcn_ubfe(acc, kPosShift, 16 - kPosShift);
      atomicOr(&bmr_w0[(__builtin_amdgcn_ubfe(at, 5, kBWlog) << 6) + bmr_lane], look ? 1u << (at & 31) : 0u);
      len_it += stay ? 0u : len;
      acc = acc_next;
      c = c_next;
      look = (u16)acc < lim_pos;
      thr = look ? 1u : 0x100u;
      acc2 = acc + (2u << kPosShift);
      asm volatile("" : "+v"(c), "+v"(thr), "+v"(acc2), "+v"(len_it) : : "memory");
    }
    ip = ip_base + __builtin_amdgcn_ubfe(acc, kPosShift, 16 - kPosShift);
    op = op_it + len_it;

    // ---------- long literals (tags 0xF0/0xF4/0xF8/0xFC), off the unrolled
    // walk: a wave-uniform branch for the lanes that stand on one below lim.
    // A lane stays here while its next tag is a long literal too, so a body
    // of long literals does not take one iteration per tag; a literal that
    // leaves the ring (ip >= lim) ends the lane's iteration.
    // Bounds are checked once per iteration (below): a tag whose bytes run
    // past the input leaves ip > n_in (no u32 wrap while the length is
    // <= n_in, since ip <= n_in < 2^31), after which the lane looks at
    // nothing more (ip >= lim); a larger length (a huge or wrapping 4-byte
    // one, which could bring ip back below lim) stops the lane and shows in
    // ll_bad.  The bit and length of such a tag land only in state that a
    // corrupt message never stores, and ring indices are masked.
    bool ll_bad = false;
    bool ll = ip < lim && (c & 0xf3u) == 0xf0u;
    while (__any(ll)) {
      const u32 P = ip + ibal;
      const u32 dw = (P >> 2) & (kRD - 1);
      const u32 lo = ring[dw * kWave + lane];
      const u32 hi = ring[((dw + 1) & (kRD - 1)) * kWave + lane];
      const u32 bsh = P & 3;
      const u32 t0 = alignbyte(hi, lo, bsh);              // bytes ip..ip+3
      const u32 ext = alignbyte(hi >> (8 * bsh), t0, 1);  // bytes ip+1..ip+4
      const u32 cc = t0 & 0xffu;
      ll = ll && (cc & 0xf3u) == 0xf0u;
      if (ll) {
        // the length's nb = 1..4 bytes follow the tag byte; uint32 wrap
        // (0xffffffff + 1 == 0) as the reference's uint32 sum
        const u32 nb = (cc >> 2) - 59u;
        const u32 lpart = (ext & (0xffffffffu >> (32 - 8 * nb))) + 1u;
        atomicOr(&bmr[((ip >> 5) & (kBW - 1)) * kWave + lane], 1u << (ip & 31));
        ll_bad = lpart > n_in;
        ip += 1 + nb + lpart;
        op += lpart;
        ll = !ll_bad && ip < lim;
      }
    }
    if (status < 0 && (ip > n_in || ll_bad)) status = kCorrupt;
    // writer space (:1166, :1400), checked once per iteration: op only grows,
    // and one iteration cannot wrap it (accepted literals fit the input)
    if (status < 0 && (op > expected || op < op_it)) status = kCorrupt;
    // end of input between tags (RefillTag eof): the result, snappy.cc:858-868
    if (status < 0 && ip == n_in) status = op == expected ? kOk : kCorrupt;

    // ---------- store the bit groups the walk has left
    // The bitmap is not zeroed by the launch: every group of a message the
    // execution pass will read is stored here, zero groups included (a
    // single-literal message's bitmap is never read), and the groups a long
    // literal jumps over are stored as zeros; at the end the walk's
    // remaining groups up to the allocation (ceil(n_in / 128)).
    if (bm && !single_src) {
      const u32 ngroups = (((n_in + 31) >> 5) + 3) >> 2;
      const u32 cur0 = status < 0 ? ip >> 7 : (status == kOk ? ngroups : 0u);
      // super-group stores: while walking, only the whole super-groups below
      // the current one; once the walk is over, everything up to the end
      const u32 cur = kSuper && status < 0 ? cur0 & ~3u : cur0;
      if constexpr (kSuper) {
        // fg is a multiple of 4 until the walk ends: the super-group at fg
        // is one half of the 8-slot ring; past fg + 4 only after a long
        // literal (or at the end)
        auto super_store = [&](u32 g0) {
          const u32 sl = (g0 & 4u) * 4;
          u32x4 v[4];
#pragma unroll
          for (u32 q = 0; q < 16; ++q) v[q >> 2][q & 3] = bmr[(sl + q) * kWave + lane];
#pragma unroll
          for (u32 k = 0; k < 4; ++k)
            if (g0 + k < cur) *reinterpret_cast<u32x4*>(bm + 4 * (g0 + k)) = v[k];
#pragma unroll
          for (u32 q = 0; q < 16; ++q) bmr[(sl + q) * kWave + lane] = 0;
        };
        if (cur > fg) {
          super_store(fg);
          if (cur > fg + 4) {
            super_store(fg + 4);
            for (u32 gi = fg + 8; gi < cur; ++gi) *reinterpret_cast<u32x4*>(bm + 4 * gi) = u32x4{0, 0, 0, 0};
          }
          fg = cur;
        }
      } else {
#pragma unroll
        for (u32 k = 0; k < kBG; ++k) {
          const u32 gi = fg + k;
          if (gi < cur) {
            const u32 sl = (gi & (kBG - 1)) * 4;
            u32x4 v;
#pragma unroll
            for (u32 q = 0; q < 4; ++q) v[q] = bmr[(sl + q) * kWave + lane];
            *reinterpret_cast<u32x4*>(bm + 4 * gi) = v;
#pragma unroll
            for (u32 q = 0; q < 4; ++q) bmr[(sl + q) * kWave + lane] = 0;
          }
        }
        for (u32 gi = fg + kBG; gi < cur; ++gi) *reinterpret_cast<u32x4*>(bm + 4 * gi) = u32x4{0, 0, 0, 0};
        fg = cur > fg ? cur : fg;
      }
    }

    // ---------- land the chunks loaded last iteration
#pragma unroll
    for (u32 c = 0; c < kAH; ++c) ring_write(gk_w + c, g[c], c < gn_w);
    wend = gn_w ? gk_w + gn_w : wend;

    // ---------- prefetch from the parse position
    {
      const u32 P = ip + ibal;
      const u32 pc = P >> 4;
      const u32 base = pc >= iend ? pc : iend;  // a long literal jumped past the ring: restart
      u32 cnt = 0;
#pragma unroll
      for (u32 c = 0; c < kAH; ++c) {
        const u32 k = base + c;
        const bool ok = status < 0 && k <= last_chunk && k <= pc + (kRC - 1);
        cnt += ok ? 1u : 0u;
        const u32 kk = k <= last_chunk ? k : last_chunk;
        g[c] = *reinterpret_cast<const u32x4*>(n_in ? abase + 16 * kk
                                                    : reinterpret_cast<const u8*>(g_dummy_chunk));
      }
      iend = cnt ? base + cnt : iend;
      gk_w = base;
      gn_w = cnt;
    }
    more = __any(status < 0);
  }
  const bool mine = valid_msg && (!kPlanned || walked);
  if (mine) status_out[m] = status;
  if (mine && bitmap && status == kOk && single_src) bm_base_out[m] = kSingleLiteral | single_src;
}

}  // namespace fsg
