// snappy_decode_v4.hip -- two-pass Snappy decode for gfx950: a lane-per-message
// index pass, then a wave-per-message execution pass.
//
// Why two passes.  The lane-per-message decoders (v1-v3) give a 65,536 x
// 64 KiB batch exactly one wave per SIMD, and every piece load/store of a wave
// instruction touches 64 unrelated cache lines.  The only serial part of Snappy
// decode is finding the tag boundaries (each tag's length is in its first
// bytes); everything else -- output offsets (a prefix sum), literal bytes and
// most copy sources -- is data-parallel.  So:
//
//   pass 1, index_kernel (one LANE per message): the reference's tag walk
//     (SnappyDecompressor::DecompressAllTags, flare/io/snappy/snappy.cc:716-787,
//     with the writer checks of :1141-1227 / :1331-1481) without touching
//     output.  It produces the per-message status (pass 2 adds the copy-offset
//     check, :1200/:1410/:1466, where every tag's output position is already
//     known) and a tag-start bitmap over the compressed bytes (bit p = a tag
//     starts at compressed offset p), 1/8 of the input size.  Pure VALU + LDS
//     ring reads; each lane reads its own input once.  Large messages are
//     listed instead and walked by a wave each (pass 1b), the huge ones of a
//     forked batch in chunks.
//
//   pass 2, exec_kernel (one WAVE per message, only status-OK messages):
//     walks the bitmap and takes up to 64 tags per group, one TAG per lane.
//     A lane decodes its tag through a table in LDS (the tag's bytes, and
//     with them a short literal's, were prefetched a group ahead), the tags'
//     output lengths are prefix-summed, and each lane executes its own tag as
//     <= 4 chunks of 16 bytes in an LDS output window: round A writes every
//     chunk whose source is in registers or global memory (literals, copies
//     from before the window), rounds B run the other copies' chunks in
//     dependency order -- a chunk runs once every byte it reads precedes the
//     first unfinished chunk of the group.  Completed 16-byte blocks of the
//     window are flushed to the slot 1 KiB per wave instruction, so the
//     loads/stores coalesce, and 4 waves per workgroup / 7 per SIMD hide the
//     latency.  Literals longer than 64 bytes are copied by the whole wave.
//     This is variant 5, the default.  Variant 4, the A/B variant behind
//     FSG_DECODE_KERNEL=4, cuts the group's tags into <= 16-byte pieces, one
//     PIECE per lane, and runs the pieces in the same rounds.  The short
//     bodies of a forked batch go through the packed pass instead: several
//     bodies per wave, their tags in one stream of groups.
//
// Rounds rely on the in-order processing of one wave's vector memory
// instructions: a round's loads are issued after the previous round's stores
// (same wave), so they observe them, exactly as v3's batches do.
//
// A message whose bitmap does not fit the workspace gets status kNeedFallback
// in pass 1 and is decoded serially by one lane in pass 3 (fallback_kernel).
//
// One translation unit; each pass's device code is a header of its own,
// included below in the order the code object keeps (see exec_kernel_variant):
//   decode_v4_index.h        pass 1: the lane walk and its plan kernels
//   decode_v4_index_big.h    pass 1b: the wave walk of large messages
//   decode_v4_chunked.h      pass 1b, chunked: the huge messages
//   decode_v4_exec_common.h  the tag ring's geometry, phase stamps
//   decode_v4_exec4.h        pass 2, variant 4 (exec_message)
//   decode_v4_exec5.h        pass 2, variant 5 (exec5_message)
//   decode_v4_packed.h       the packed execution pass (exec5_packed)
// Here: the kernels that bind those to the LDS layout (exec_kernel<V>,
// exec_packed_kernel), pass 3, and the launch (its arithmetic:
// decode_v4_plan.h).
#include "options.h"
#include "snappy_lane_decode.h"
#include "snappy_pieces.h"
#include "wave_util.h"

#include <mutex>
#include <type_traits>

#include "decode_v4_plan.h"
#include "launch.h"
#include "launch_util.h"

// (in this order: definitions are emitted in it)
#include "decode_v4_index.h"
#include "decode_v4_index_big.h"
#include "decode_v4_chunked.h"
#include "decode_v4_exec4.h"
#include "decode_v4_exec5.h"
#include "decode_v4_packed.h"

namespace fsg {

static_assert(kWave == 64, "idx_lean_lds_bytes (decode_v4_plan.h) counts 64 lanes per wave");

// 7 waves per SIMD by default (FSG_EXEC_WAVES; 72 VGPRs, 22.2 KB of LDS per
// block with the 3 KiB window: C3 6.35 -> 6.20 ms against 6 waves with a
// 4 KiB window, A/B on one box; 8 waves spill and were slower).
// The v4 variant (exec_kernel<4>) shares the setting and was not re-measured
// at 7.  Variant 5's folded instance (wave-per-message bodies) has a 4 KiB
// window in the same LDS, its ring entries being 16 bits: C3 5.76 -> 5.58 ms,
// DESIGN.md §5 "Execution pass: folded instance".
// The first kBigBlocks blocks take the large messages listed by pass 1 from a
// device counter (blocks dispatch in order, so the longest messages start
// first); every other block runs the wave-per-message mapping and skips them.
// (A fully persistent grid was measured slower on uniform batches.)
#ifndef FSG_EXEC_WAVES
#define FSG_EXEC_WAVES 7
#endif
template <int V>
__global__ __launch_bounds__(kWavesPerBlock * 64) __attribute__((amdgpu_waves_per_eu(FSG_EXEC_WAVES, FSG_EXEC_WAVES))) void exec_kernel(
    const u8* __restrict__ in, const u64* __restrict__ in_off,
    const u32* __restrict__ in_len, u32 n_msgs, u8* out,
    const u64* __restrict__ out_off, const u32* __restrict__ out_len,
    i32* __restrict__ status, const u32* __restrict__ bm_base,
    u32* __restrict__ bitmap, const u32* __restrict__ seg_list,
    const u32* __restrict__ seg_count, const u32* __restrict__ whole_list,
    const u32* __restrict__ whole_count, u32* __restrict__ exec_next, u32 big_blocks,
    u32 big_threshold, u32 prio, u32 keep_hist, u32 small_stride, const u32* __restrict__ walk_perm = nullptr,
    const u32* __restrict__ walk_hist = nullptr, u32 walk_part = 0, u32 split_class = 0) {
  // per wave: the tag ring, then the output window
  __shared__ __attribute__((aligned(16))) u8 wl_s[kWavesPerBlock][4 * kTagRing + kWindow + 32];
  __shared__ __attribute__((aligned(16))) u8 pmap_s[kWavesPerBlock][V == 5 ? 1 : kMaxPieces];
  __shared__ u32x4 sel_tab[16];
  __shared__ u32 tagtab[V == 5 ? 256 : 1];
  __shared__ u32x4 mask_tab[17];
  static_assert(kWavesPerBlock * 64 == 256, "one tag table entry per thread");

  if (threadIdx.x < 64) init_pattern_table(sel_tab, threadIdx.x);
  if constexpr (V == 5) tagtab[threadIdx.x] = exec_tag_entry(threadIdx.x);
  init_mask_table(mask_tab, threadIdx.x);
  __syncthreads();
  // wave index made visibly uniform: the message's sizes, pointers and the
  // walk state (head, tail, op, window base) then live in SGPRs and branches
  // on them are scalar
  const u32 wv = (u32)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const u32 lane = threadIdx.x & 63;
  u8* wl = wl_s[wv];
  u8* pmap = pmap_s[wv];
  // One message (or segment) with the pass-2 variant V.  Variant 5 has two
  // instances of exec5_message, one call site each: the folded one
  // (whole = true_type: a whole body of at most big_threshold bytes; 16-bit
  // ring, kWindowWhole window) and the general one.  keep_hist carries the
  // kept history of both: the general instance's in bits 0-15, the folded
  // one's in bits 16-31.
  auto run = [&](auto whole, u32 m, i32 st, u32 ip0, u32 op0, u32 op1) {
    constexpr bool kWhole = decltype(whole)::value;
    if constexpr (V == 5 && kWhole)
      exec5_message<true, u16, kWindowWhole>(m, in, in_off, in_len, out, out_off, out_len, status, bm_base, bitmap,
                                             reinterpret_cast<u16*>(wl), tagtab, wl + 2 * kTagRing, sel_tab,
                                             mask_tab, lane, st, 0u, 0u, 0u, prio != 0, keep_hist >> 16);
    else if constexpr (V == 5)
      exec5_message<false, u32, kWindow>(m, in, in_off, in_len, out, out_off, out_len, status, bm_base, bitmap,
                                         reinterpret_cast<u32*>(wl), tagtab, wl + 4 * kTagRing, sel_tab, mask_tab,
                                         lane, st, ip0, op0, op1, prio != 0, keep_hist & 0xffffu);
    else
      exec_message(m, in, in_off, in_len, out, out_off, out_len, status, bm_base, bitmap,
                   reinterpret_cast<u32*>(wl), pmap, wl + 4 * kTagRing, sel_tab, mask_tab, lane, st, ip0, op0, op1,
                   prio != 0, keep_hist & 0xffffu);
  };

  if (blockIdx.x >= big_blocks) {
    // one message per wave; or, with small_stride (blocks), every
    // small_stride-th group of kWavesPerBlock messages: a wave runs many
    // small messages, paying its launch and the block's table set-up once
    // (the forked path's batches of mostly small bodies)
    const u32 m0 = (blockIdx.x - big_blocks) * kWavesPerBlock + wv;
    const u32 step = small_stride ? small_stride * kWavesPerBlock : 0xffffffffu;
    // message numbers [0, n_msgs); or, in walk order (forked path), positions
    // [lo, hi) of walk_perm -- part 1 / 2 the larger / smaller bodies, 3 all
    // of them
    u32 lo = 0, n = n_msgs;
    if (walk_perm) {
      const u32 n_walk = walk_hist[2 * kWalkClasses];
      // (split_class bits 8-15: the first class another pass takes, whose
      // positions on are not executed here; no pass sets it now)
      const u32 tcls = split_class >> 8;
      const u32 split = walk_hist[kWalkClasses + (split_class & 0xffu)];
      const u32 t_hi = tcls ? walk_hist[kWalkClasses + tcls] : n_walk;
      lo = walk_part == 2 ? split : 0u;
      n = (walk_part == 1 ? split : t_hi) - lo;
    }
    for (u32 i = m0; i < n; i = i + step < i ? 0xffffffffu : i + step) {
      const u32 m = walk_perm ? walk_perm[lo + i] : i;
      // (the walk order lists no large message: pass 1 sent those to pass 1b)
      if (in_len[m] <= big_threshold) run(std::true_type{}, m, status[m], 0u, 0u, out_len[m]);
    }
    return;
  }
  // large messages, listed by pass 1b: whole ones first (the longest start
  // first), then 64 KiB segments of the others
  const u32 n_whole = *whole_count;
  const u32 n_seg_raw = *seg_count;
  const u32 n_seg = n_seg_raw < n_msgs ? n_seg_raw : n_msgs;
  const u32 total = n_whole + n_seg;
  if (total == 0) return;
  const u64* segs = reinterpret_cast<const u64*>(seg_list);
  for (;;) {  // all-lane atomic: lane 0 adds 1, lane 0's result is the index
    const u32 got = atomicAdd(exec_next, lane == 0 ? 1u : 0u);
    const u32 idx = (u32)__builtin_amdgcn_readfirstlane((int)got);
    if (idx >= total) break;
    // the message and its range: input from ip0, output [op0, op1)
    u32 m, ip0 = 0, op0 = 0, op1;
    if (idx < n_whole) {
      m = whole_list[idx];
      op1 = out_len[m];
    } else {
      const u64 e = segs[idx - n_whole];
      m = (u32)e;
      if (m == 0xffffffffu) continue;  // a hole (the message runs whole)
      const u32 k = (u32)(e >> 32) & 0x7fffffffu;
      op0 = k << 16;
      op1 = (e >> 63) ? out_len[m] : op0 + 65536u;
      // segment k > 0 starts at the input offset pass 1b left in its slot
      if (k) __builtin_memcpy(&ip0, out + out_off[m] + op0, 4);
    }
    run(std::false_type{}, m, status[m], ip0, op0, op1);
  }
}

// The packed execution pass (exec5_packed) over walk part 2 (the bodies of
// size class >= split_class): batches of `batch` consecutive walk positions
// from a work counter.
#ifndef FSG_PACK_WAVES
#define FSG_PACK_WAVES 6
#endif
__global__ __launch_bounds__(kWavesPerBlock * 64) __attribute__((amdgpu_waves_per_eu(FSG_PACK_WAVES, FSG_PACK_WAVES))) void exec_packed_kernel(
    const u8* __restrict__ in, const u64* __restrict__ in_off, const u32* __restrict__ in_len, u8* out,
    const u64* __restrict__ out_off, const u32* __restrict__ out_len, i32* __restrict__ status,
    const u32* __restrict__ bm_base, const u32* __restrict__ bitmap, const u32* __restrict__ walk_perm,
    const u32* __restrict__ walk_hist, u32 split_class, u32* __restrict__ batch_next, u32 batch, u32 keep_hist) {
  __shared__ __attribute__((aligned(16))) u8 wl_s[kWavesPerBlock][4 * kTagRing + kWindow + 32];
  __shared__ u32x4 sel_tab[16];
  __shared__ u32 tagtab[256];
  __shared__ u32x4 mask_tab[17];
  static_assert(kWavesPerBlock * 64 == 256, "one tag table entry per thread");
  if (threadIdx.x < 64) init_pattern_table(sel_tab, threadIdx.x);
  tagtab[threadIdx.x] = exec_tag_entry(threadIdx.x);
  init_mask_table(mask_tab, threadIdx.x);
  __syncthreads();
  const u32 wv = (u32)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const u32 lane = threadIdx.x & 63;
  u32* ring = reinterpret_cast<u32*>(wl_s[wv]);
  u8* sb = wl_s[wv] + 4 * kTagRing;
  const u32 n_walk = walk_hist[2 * kWalkClasses];
  const u32 tcls = split_class >> 8;
  const u32 lo = walk_hist[kWalkClasses + (split_class & 0xffu)];
  const u32 hi = tcls ? walk_hist[kWalkClasses + tcls] : n_walk;
  const u32 n = hi > lo ? hi - lo : 0u;
  for (;;) {
    const u32 got = atomicAdd(batch_next, lane == 0 ? 1u : 0u);
    const u32 bi = (u32)__builtin_amdgcn_readfirstlane((int)got);
    if ((u64)bi * batch >= n) break;
    const u32 first = bi * batch;
    const u32 cnt = n - first < batch ? n - first : batch;
    exec5_packed(in, in_off, in_len, out, out_off, out_len, status, bm_base, bitmap, walk_perm, lo + first, cnt,
                 ring, tagtab, sb, sel_tab, mask_tab, lane, keep_hist, batch_next);
  }
}

#ifdef FSG_STAMPS
extern "C" int fsg_debug_stamps(unsigned long long* out, int reset) {
  hipError_t e = hipMemcpyFromSymbol(out, HIP_SYMBOL(g_stamps), sizeof(g_stamps));
  if (reset) {
    unsigned long long z[24] = {};
    (void)hipMemcpyToSymbol(HIP_SYMBOL(g_stamps), z, sizeof(z));
  }
  return e == hipSuccess ? 0 : -1;
}
#endif

// Pass 3: the messages whose bitmap did not fit the workspace (status
// kNeedFallback, header and slot already checked by pass 1), one lane each,
// with the reference's serial tag loop.  A lean grid-sized launch: no LDS, a
// status load per lane.  (Measured: a grid-sized launch here keeps the next
// call's passes at full speed on C3, a one-block launch or none does not --
// DESIGN.md section 5; the former v3 fallback launch cost 14 us more on C2.)
__global__ __launch_bounds__(64) void fallback_kernel(
    const u8* __restrict__ in, const u64* __restrict__ in_off, const u32* __restrict__ in_len,
    u32 n_msgs, u8* out, const u64* __restrict__ out_off, const u32* __restrict__ out_len,
    i32* __restrict__ status, u32 flags, const u32* __restrict__ bm_base, u64 bm_capacity_words,
    u32* __restrict__ fb_count) {
  const u32 m = blockIdx.x * 64 + threadIdx.x;
  const bool mine = m < n_msgs && status[m] == kNeedFallback;
  // path report: the messages decoded here, and those of them that pass 1
  // sent (index_prologue's bitmap test, repeated); the packed pass counts its
  // own.  One ballot per wave, atomics only from a wave that has work.
  const u64 fb = __ballot(mine);
  if (!fb) return;
  const u32 n_in = mine ? in_len[m] : 0u;
  const u32 bmb = mine ? bm_base[m] : 0u;
  const u32 words = (((n_in + 31) >> 5) + 3) & ~3u;
  const u64 fb_bm = __ballot(mine && !(bmb & kSingleLiteral) && (u64)bmb + words > bm_capacity_words);
  if (threadIdx.x == 0) {
    atomicAdd(fb_count, (u32)__builtin_popcountll(fb));
    if (fb_bm) atomicAdd(fb_count + 1, (u32)__builtin_popcountll(fb_bm));
  }
  if (!mine) return;
  const u8* ib = in + in_off[m];
  u32 ulen = 0;
  const int h = parse_varint_header(ib, n_in, flags & 2u, &ulen);
  status[m] = decode_one(ib + h, ib + n_in, out + out_off[m], out_len[m], true);
}

void decode_v4_header_counts(const void* header, DecodeHeaderCounts* c) {
  u32 ctr[kWsCounterBytes / 4];
  __builtin_memcpy(ctr, header, sizeof(ctr));
  auto at = [&ctr](u32 off) { return ctr[off / 4]; };
  c->bitmap_words = at(kWsBmCounter);
  c->large = at(kWsBigCount);
  c->huge = at(kWsHugeCount);
  c->fallback = at(kWsFallbackCount);
  c->fallback_bitmap = at(kWsFallbackBitmap);
  c->fallback_wide = at(kWsFallbackWide);
  c->fallback_guard = at(kWsFallbackGuard);
}

namespace {

// Per-device side stream and fork/join events for launch_decode_v4 (created
// on first use; the mutex orders each call's record/wait pairs when several
// host threads decode at once).  nullptr when they cannot be created: the
// passes then run in one stream.
struct SideStream {
  hipStream_t stream = nullptr;
  hipStream_t stream2 = nullptr;  // the huge messages' pass 1b + execution (nullptr: not created)
  hipEvent_t join2 = nullptr;
  hipStream_t stream3 = nullptr;  // the larger small bodies' walk + execution (split walk)
  hipEvent_t join3 = nullptr;
  hipEvent_t fork = nullptr, join = nullptr;
  hipEvent_t pass1 = nullptr;  // two-stream calls: pass 1 done (fsg_decompress_batch_2s)
  std::mutex mu;
};
bool create_side_stream(SideStream* s) {
  if (hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking) != hipSuccess ||
      hipEventCreateWithFlags(&s->fork, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&s->join, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&s->pass1, hipEventDisableTiming) != hipSuccess)
    return false;
  // optional second side stream (the huge messages of a forked batch)
  if (hipStreamCreateWithFlags(&s->stream2, hipStreamNonBlocking) != hipSuccess ||
      hipEventCreateWithFlags(&s->join2, hipEventDisableTiming) != hipSuccess)
    s->stream2 = nullptr;
  if (hipStreamCreateWithFlags(&s->stream3, hipStreamNonBlocking) != hipSuccess ||
      hipEventCreateWithFlags(&s->join3, hipEventDisableTiming) != hipSuccess)
    s->stream3 = nullptr;
  return true;
}
SideStream* side_stream() { return per_device<SideStream>(create_side_stream); }

// pass 1b's large messages land in pass 2's work lists.  set 0: every large
// message (one stream) or the non-huge ones (forked); set 1: the huge ones
// (forked, second side stream), with their own counters and lists.
struct BigSet {
  u32 *big_next, *seg_count, *whole_count, *exec_next;
  u64* seg_list;
  u32* whole_list;
};

// pass 2: one tag per lane (5) or <= 16-byte pieces per lane (4)
using ExecKernel = decltype(&exec_kernel<5>);
// (Defined ahead of the other launch functions: the compiler emits template
// instances in the order of their first use, and the measurements in
// DESIGN.md section 5 were taken with exec_kernel<4>, <5> ahead of the
// index_kernel instances in the code object.)
ExecKernel exec_kernel_variant(int v) { return v == 4 ? &exec_kernel<4> : &exec_kernel<5>; }
// exec_kernel's keep_hist argument: the general instance's kept history in
// bits 0-15, the folded instance's in bits 16-31
u32 exec_keep_arg(const DecodePlan& p) { return p.keep_hist | (p.keep_hist_whole << 16); }

// One call's arrays: the caller's, and the workspace regions at the plan's
// offsets.
struct DecodeBufs {
  const u8* in;
  const u64* in_off;
  const u32* in_len;
  u32 n_msgs;
  u8* out;
  const u64* out_off;
  const u32* out_cap;
  u32* out_len;
  i32* status;
  u32 flags;
  ExecKernel ek;
  u8* w;  // the workspace (counters at the kWs* offsets)
  u32 *counter, *big_count, *bm_base, *big_list;
  // the planned lane walk's order: ranks, the permutation, class counts and
  // offsets (+ the walk count)
  u32 *walk_rank, *walk_perm, *walk_hist;
  u32* bitmap;
  BigSet set0, set1;
  // chunked pass 1b's record region
  u32 *first_rec, *mstat;
  ChunkRec* recs;
  u32* ctr(u32 off) const { return reinterpret_cast<u32*>(w + off); }
};

void workspace_pointers(const DecodePlan& p, void* ws, DecodeBufs* b) {
  u8* w = static_cast<u8*>(ws);
  auto words = [w](u64 off) { return reinterpret_cast<u32*>(w + off); };
  b->w = w;
  b->counter = words(kWsBmCounter);
  b->big_count = words(kWsBigCount);
  b->bm_base = words(p.bm_base_off);
  b->big_list = words(p.big_list_off);
  b->walk_rank = words(p.walk_rank_off);
  b->walk_perm = words(p.walk_perm_off);
  b->walk_hist = words(p.walk_hist_off);
  b->bitmap = words(p.bitmap_off);
  b->set0 = BigSet{words(kWsSet0BigNext), words(kWsSet0SegCount), words(kWsSet0WholeCount), words(kWsSet0ExecNext),
                   reinterpret_cast<u64*>(w + p.seg_list_off), words(p.whole_list_off)};
  b->set1 = BigSet{words(kWsSet1BigNext), words(kWsSet1SegCount), words(kWsSet1WholeCount), words(kWsSet1ExecNext),
                   reinterpret_cast<u64*>(w + p.seg_list2_off), words(p.whole_list2_off)};
  b->first_rec = words(p.first_rec_off);
  b->mstat = words(p.mstat_off);
  b->recs = reinterpret_cast<ChunkRec*>(w + p.recs_off);
}

// The lane walk: planned (after index_plan_kernel; part 1 / 2: one side of
// the split walk) or the plan's one-stream instance.
hipError_t launch_index(const DecodePlan& p, const DecodeBufs& b, bool planned, hipStream_t st, u32 part = 0) {
  const LaunchDim& d = planned ? p.planned_walk : p.walk;
  if (planned)
    index_kernel<true><<<d.grid, d.block, d.lds, st>>>(
        b.in, b.in_off, b.in_len, b.n_msgs, b.out_cap, b.out_len, b.status, b.flags, b.counter, b.bm_base, b.bitmap,
        p.cap_words, b.big_count, b.big_list, p.big_threshold, p.walk_order ? b.walk_perm : nullptr, b.walk_hist,
        part, p.split_class);
  else if (p.walk_kind == kWalkLean)
    index_kernel<false, true><<<d.grid, d.block, d.lds, st>>>(
        b.in, b.in_off, b.in_len, b.n_msgs, b.out_cap, b.out_len, b.status, b.flags, b.counter, b.bm_base, b.bitmap,
        p.cap_words, b.big_count, b.big_list, p.big_threshold, nullptr, nullptr);
  else if (p.walk_kind == kWalkSerial)
    index_kernel<false, false, kIdxWavesSerial><<<d.grid, d.block, d.lds, st>>>(
        b.in, b.in_off, b.in_len, b.n_msgs, b.out_cap, b.out_len, b.status, b.flags, b.counter, b.bm_base, b.bitmap,
        p.cap_words, b.big_count, b.big_list, p.big_threshold, nullptr, nullptr);
  else
    index_kernel<false><<<d.grid, d.block, d.lds, st>>>(
        b.in, b.in_off, b.in_len, b.n_msgs, b.out_cap, b.out_len, b.status, b.flags, b.counter, b.bm_base, b.bitmap,
        p.cap_words, b.big_count, b.big_list, p.big_threshold, nullptr, nullptr);
  return hipGetLastError();
}

// pass 1b: large messages, one wave each (an empty list costs one short
// launch); they land in set s of pass 2's work lists.
hipError_t launch_index_big(const DecodePlan& p, const DecodeBufs& b, hipStream_t st, const BigSet& s, u32 mode) {
  index_big_kernel<<<p.index_big_grid, 256, 0, st>>>(
      b.in, b.in_off, b.in_len, b.out_len, b.flags, b.status, b.bm_base, b.bitmap, b.big_count, b.big_list,
      s.big_next, b.n_msgs, b.out, b.out_off, s.seg_list, s.seg_count, s.whole_list, s.whole_count, mode);
  return hipGetLastError();
}

// The forked path's large-message exec launch: the large-message blocks only
// (exit after one atomic when the lists are empty).
hipError_t launch_big_exec(const DecodePlan& p, const DecodeBufs& b, hipStream_t st, const BigSet& s) {
  b.ek<<<p.fork_big_blocks, kWavesPerBlock * 64, 0, st>>>(
      b.in, b.in_off, b.in_len, b.n_msgs, b.out, b.out_off, b.out_len, b.status, b.bm_base, b.bitmap,
      reinterpret_cast<const u32*>(s.seg_list), s.seg_count, s.whole_list, s.whole_count, s.exec_next,
      p.fork_big_blocks, p.big_threshold, 0u, exec_keep_arg(p), 0u, nullptr, nullptr, 0u, 0u);
  return hipGetLastError();
}

hipError_t launch_big(const DecodePlan& p, const DecodeBufs& b, hipStream_t st, const BigSet& s, u32 mode) {
  const hipError_t e = launch_index_big(p, b, st, s, mode);
  if (e != hipSuccess) return e;
  return launch_big_exec(p, b, st, s);
}

// The huge messages' pass 1b, chunked (chunk_*_kernel; DecodePlan::chunked),
// then their execution.
hipError_t launch_big_chunked(const DecodePlan& p, const DecodeBufs& b, hipStream_t st, const BigSet& s) {
  u32* const cctr = b.ctr(kWsChunkCount);
  chunk_list_kernel<<<p.chunk_list_grid, 256, 0, st>>>(b.in, b.in_off, b.in_len, b.big_count, b.big_list, b.n_msgs,
                                                       b.flags, cctr, b.recs, b.first_rec, (u32)p.max_recs);
  chunk_spec_kernel<<<p.chunk_rec_grid, 256, 0, st>>>(b.in, b.in_off, b.in_len, b.flags, b.bm_base, b.bitmap, cctr,
                                                      b.recs, b.ctr(kWsChunkSpecNext), (u32)p.max_recs);
  chunk_fixup_kernel<<<p.chunk_msg_grid, 256, 0, st>>>(b.in, b.in_off, b.in_len, b.out_len, b.bm_base, b.bitmap,
                                                       b.big_count, b.recs, b.first_rec, b.mstat,
                                                       b.ctr(kWsChunkFixNext));
  chunk_check_kernel<<<p.chunk_rec_grid, 256, 0, st>>>(b.in, b.in_off, b.in_len, b.out_len, b.bm_base, b.bitmap, cctr,
                                                       b.recs, b.out, b.out_off, b.ctr(kWsChunkCheckNext),
                                                       (u32)p.max_recs);
  chunk_final_kernel<<<p.chunk_msg_grid, 256, 0, st>>>(b.in, b.in_off, b.in_len, b.flags, b.bm_base, b.bitmap, b.out,
                                                       b.out_off, b.big_list, b.out_len, b.status, b.big_count,
                                                       b.recs, b.first_rec, b.mstat, b.n_msgs, s.seg_list,
                                                       s.seg_count, s.whole_list, s.whole_count,
                                                       b.ctr(kWsChunkFinalNext));
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  return launch_big_exec(p, b, st, s);
}

// The forked path's small-message launch: one wave per message, or a grid of
// small_grid blocks whose waves loop; large ones are skipped (big_blocks = 0:
// no block takes the large-message role).  part 1 / 2: the messages of that
// part of the split walk, in walk order; 3: all of them in walk order.
hipError_t launch_small(const DecodePlan& p, const DecodeBufs& b, hipStream_t st, u32 part) {
  b.ek<<<p.small_grid, kWavesPerBlock * 64, 0, st>>>(
      b.in, b.in_off, b.in_len, b.n_msgs, b.out, b.out_off, b.out_len, b.status, b.bm_base, b.bitmap,
      reinterpret_cast<const u32*>(b.set0.seg_list), b.set0.seg_count, b.set0.whole_list, b.set0.whole_count,
      b.set0.exec_next, 0u, p.big_threshold, 0u, exec_keep_arg(p), p.small_stride, part ? b.walk_perm : nullptr,
      part ? b.walk_hist : nullptr, part, p.split_class);
  return hipGetLastError();
}

// The short bodies of walk part 2 packed several to a wave (exec5_packed).
hipError_t launch_packed(const DecodePlan& p, const DecodeBufs& b, hipStream_t st) {
  exec_packed_kernel<<<p.small_grid, kWavesPerBlock * 64, 0, st>>>(
      b.in, b.in_off, b.in_len, b.out, b.out_off, b.out_len, b.status, b.bm_base, b.bitmap, b.walk_perm, b.walk_hist,
      p.split_class, b.ctr(kWsPackNext), p.pack_batch, p.keep_hist);
  return hipGetLastError();
}

// The forked path: the plan pass lists the large messages; pass 1b starts on
// them (side streams) while the lane walk and the small messages' execution
// run on `stream`; all streams join on `stream`.
hipError_t launch_forked(const DecodePlan& p, const DecodeBufs& b, SideStream* side, hipStream_t stream) {
  hipError_t e;
  index_plan_kernel<<<p.plan_grid, kPlanThreads, 0, stream>>>(
      b.in, b.in_off, b.in_len, b.n_msgs, b.out_cap, b.out_len, b.status, b.flags, b.counter, b.bm_base, b.bitmap,
      p.cap_words, b.big_count, b.big_list, p.big_threshold, p.walk_order ? b.walk_rank : nullptr, b.walk_hist);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if (p.walk_order) {
    walk_offsets_kernel<<<1, 64, 0, stream>>>(b.walk_hist);
    walk_scatter_kernel<<<p.scatter_grid, 256, 0, stream>>>(b.in_len, b.n_msgs, b.status, b.walk_rank, b.walk_hist,
                                                            b.walk_perm);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  // The huge messages (> kHugeIndexBytes compressed) are walked and
  // executed on a second side stream, so the other large messages'
  // execution starts when their own (shorter) walks end instead of after
  // the longest walk: CM 7.6 -> see DESIGN.md section 5.
  std::lock_guard<std::mutex> lk(side->mu);
  if ((e = hipEventRecord(side->fork, stream)) != hipSuccess) return e;
  if ((e = hipStreamWaitEvent(side->stream, side->fork, 0)) != hipSuccess) return e;
  const bool split = p.split_huge && side->stream2;
  if (split) {
    if ((e = hipStreamWaitEvent(side->stream2, side->fork, 0)) != hipSuccess) return e;
    if ((e = p.chunked ? launch_big_chunked(p, b, side->stream2, b.set1)
                       : launch_big(p, b, side->stream2, b.set1, 1u)) != hipSuccess)
      return e;
    if ((e = hipEventRecord(side->join2, side->stream2)) != hipSuccess) return e;
  }
  if ((e = launch_big(p, b, side->stream, b.set0, split ? 2u : 0u)) != hipSuccess) return e;
  if ((e = hipEventRecord(side->join, side->stream)) != hipSuccess) return e;
  const bool three = p.split_mode == 1 && p.walk_order && side->stream3;
  if (three) {
    // the larger small bodies: walk and execution on the third stream
    if ((e = hipStreamWaitEvent(side->stream3, side->fork, 0)) != hipSuccess) return e;
    if ((e = launch_index(p, b, true, side->stream3, 1u)) != hipSuccess) return e;
    if ((e = launch_small(p, b, side->stream3, 1u)) != hipSuccess) return e;
    if ((e = hipEventRecord(side->join3, side->stream3)) != hipSuccess) return e;
    if ((e = launch_index(p, b, true, stream, 2u)) != hipSuccess) return e;
    if ((e = launch_small(p, b, stream, 2u)) != hipSuccess) return e;
    if ((e = hipStreamWaitEvent(stream, side->join3, 0)) != hipSuccess) return e;
  } else {
    if ((e = launch_index(p, b, true, stream)) != hipSuccess) return e;
    if (p.walk_order && p.split_mode == 2) {
      if ((e = launch_small(p, b, stream, 3u)) != hipSuccess) return e;
    } else if (p.walk_order && p.split_mode == 3) {
      if ((e = p.pack_batch ? launch_packed(p, b, stream) : launch_small(p, b, stream, 2u)) != hipSuccess) return e;
      if ((e = launch_small(p, b, stream, 1u)) != hipSuccess) return e;
    } else {
      if ((e = launch_small(p, b, stream, 0u)) != hipSuccess) return e;
    }
  }
  if ((e = hipStreamWaitEvent(stream, side->join, 0)) != hipSuccess) return e;
  if (split && (e = hipStreamWaitEvent(stream, side->join2, 0)) != hipSuccess) return e;
  return hipSuccess;
}

// This call's options (csrc/options.h, set with fsg_set_option; never the
// environment here).
DecodeOpts read_decode_opts() {
  DecodeOpts o;
  o.decode_fork = opt(kOptDecodeFork);
  o.split_walk = opt(kOptSplitWalk);
  o.split_class = opt(kOptSplitClass);
  o.exec_keep = opt(kOptExecKeep);
  o.chunked_huge = opt(kOptChunkedHuge);
  o.small_persist = opt(kOptSmallPersist);
  o.small_batch = opt(kOptSmallBatch);
  o.split_huge = opt(kOptSplitHuge);
  o.walk_order = opt(kOptWalkOrder);
  o.lean_walk = opt(kOptLeanWalk);
  o.exec_big_blocks = opt(kOptExecBigBlocks);
  o.exec_prio = opt(kOptExecPrio);
  o.exec_big_blocks_fork = opt(kOptExecBigBlocksFork);
  o.exec_pack = opt(kOptExecPack);
  return o;
}

}  // namespace

hipError_t launch_decode_v4(const u8* in, const u64* in_off, const u32* in_len,
                            u32 n_msgs, u8* out, const u64* out_off,
                            const u32* out_cap, u32* out_len, i32* status,
                            u32 flags, void* ws, size_t ws_bytes, hipStream_t stream,
                            int exec_variant, hipStream_t pass1_stream) {
  if (n_msgs == 0) return hipSuccess;
  // Two-stream form: pass 1 (fill, lane walk, pass 1b) on pass1_stream, pass 2
  // (exec, fallback) on `stream` behind an event, so a caller's next batch
  // (its own workspace and outputs) can walk while this one executes.
  SideStream* two = nullptr;
  if (pass1_stream && pass1_stream != stream) {
    two = side_stream();
    if (!two) {
      // No per-device event set: order `stream` behind whatever the caller
      // queued on pass1_stream with a temporary event and run every pass on
      // `stream` (as capi.hip's single-pass path does).
      const hipError_t e0 = order_after(stream, pass1_stream);
      if (e0 != hipSuccess) return e0;
    }
  }
  // the fixed part, the chunk-record region and a bitmap of at least the
  // per-message minimum (decode_v4_workspace_bytes with no input): below it
  // the plan's region arithmetic would underflow
  if (ws_bytes < decode_v4_workspace_bytes(n_msgs, 0)) return hipErrorInvalidValue;

  // ---- plan, and the pointers at its offsets
  const DecodePlan p = decode_v4_plan(n_msgs, ws_bytes, two != nullptr, read_decode_opts());
  DecodeBufs b{in, in_off, in_len, n_msgs, out, out_off, out_cap, out_len, status, flags,
               exec_kernel_variant(exec_variant)};
  workspace_pointers(p, ws, &b);

  // ---- fill
  hipStream_t const s1 = two ? pass1_stream : stream;  // every pass-1 launch goes there
  // zero the counters and the bitmap (pass 1 writes only groups holding
  // tags) with one fill from the counters to the end of the bitmap: the
  // lists between them are 20 B per message (A/B: C2 0.159 -> 0.157 ms, C3
  // and CM neutral; a zeroing kernel in place of the runtime fill makes the
  // next index pass place its one-wave workgroups unevenly: C3 +0.27 ms)
  // counters and lists only: the passes that write the bitmap store every
  // word the execution pass reads (C3: an 80 us fill of 267 MB saved)
  hipError_t e = hipMemsetAsync(b.w, 0, p.bitmap_off, s1);
  if (e != hipSuccess) return e;

  // ---- streams
  SideStream* side = p.fork ? side_stream() : nullptr;
  if (side) {
    if ((e = launch_forked(p, b, side, stream)) != hipSuccess) return e;
  } else {
    // one stream: pass 1, pass 1b, then one exec launch whose first blocks
    // take the large messages (dispatched first) and the rest one message
    // per wave
    if ((e = launch_index(p, b, false, s1)) != hipSuccess) return e;
    if ((e = launch_index_big(p, b, s1, b.set0, 0u)) != hipSuccess) return e;
    if (two) {
      std::lock_guard<std::mutex> lk(two->mu);
      if ((e = hipEventRecord(two->pass1, s1)) != hipSuccess) return e;
      if ((e = hipStreamWaitEvent(stream, two->pass1, 0)) != hipSuccess) return e;
    }
    b.ek<<<p.big_blocks + p.small_blocks, kWavesPerBlock * 64, 0, stream>>>(
        in, in_off, in_len, n_msgs, out, out_off, out_len, status, b.bm_base, b.bitmap,
        reinterpret_cast<const u32*>(b.set0.seg_list), b.set0.seg_count, b.set0.whole_list, b.set0.whole_count,
        b.set0.exec_next, p.big_blocks, p.big_threshold, p.prio, exec_keep_arg(p), 0u, nullptr, nullptr, 0u, 0u);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  fallback_kernel<<<p.fallback_grid, 64, 0, stream>>>(in, in_off, in_len, n_msgs, out, out_off, out_len, status,
                                                      flags, b.bm_base, p.cap_words, b.ctr(kWsFallbackCount));
  return hipGetLastError();
}

}  // namespace fsg
