// decode_v4_index_big.h -- pass 1b of the two-pass Snappy decoder
// (snappy_decode_v4.hip): the wave walk, one WAVE per large message listed by
// pass 1.  The launch uses index_big_kernel; the chunked walk
// (decode_v4_chunked.h) calls index_big_message for a message whose chunk
// records did not fit, and shares the stage geometry.
#pragma once

#include "decode_v4_plan.h"
#include "snappy_pieces.h"
#include "wave_util.h"

namespace fsg {

// ---- pass 1b geometry (the LDS stage of a walking wave)
constexpr u32 kBigStageChunks = 5 * 64;      // 16-byte chunks staged per wave
constexpr u32 kBigStageBytes = 16 * kBigStageChunks;

// ===========================================================================
// Pass 1b: index + validate one LARGE message per wave (compressed size >
// the launch's big_threshold, listed by pass 1).  One lane walking 100K+ tags serially
// is the tail of a mixed batch; here the walk advances a 64-byte window
// [wb, wb+64) at a time: every lane decodes the tag that WOULD start at
// wb + lane (length, advance, offset, local validity -- the same branch-free
// decode and checks as pass 1), the real tag starts in the window (the chain
// from the current position) are found by pointer doubling over the lanes'
// successor pointers (5 rounds of shuffles), their output positions by a
// prefix sum, and the position-dependent checks run on all of them at once.
// Input is staged into LDS 5 KiB at a time.
// ===========================================================================
// Indexes message m (listed by pass 1) with the calling wave: writes its
// bitmap bits and returns its final status.  `st` is the wave's LDS stage
// (kBigStageBytes + 16 bytes).
__device__ __forceinline__ i32 index_big_message(
    u32 m, const u8* __restrict__ in, const u64* __restrict__ in_off,
    const u32* __restrict__ in_len, const u32* __restrict__ out_len, bool strict,
    const u32* __restrict__ bm_base, u32* __restrict__ bitmap, u32* st, u32 lane, u8* ob,
    bool& seg) {
  const u8* ib = in + in_off[m];
  const u32 n_in = in_len[m];
  const u32 expected = out_len[m];
  u32 ulen = 0;
  u32 ip = (u32)parse_varint_header(ib, n_in, strict, &ulen);  // pass 1 accepted it
  u32 op = 0;
  i32 status = -1;
  u32* bm = bitmap + bm_base[m];
  {  // the launch does not zero the bitmap: this message's words first
    const u32 words = (((n_in + 31) >> 5) + 3) & ~3u;
    for (u32 wd = 4 * lane; wd < words; wd += 256) *reinterpret_cast<u32x4*>(bm + wd) = u32x4{0, 0, 0, 0};
  }
  const u32 ibal = (u32)(reinterpret_cast<uintptr_t>(ib) & 15);
  const u8* abase = ib - ibal;
  const u32 last_chunk = (ibal + n_in - 1) >> 4;
  int spos = -1;  // message position of stage byte 0 (-1: nothing staged)
  u32 send = 0;   // positions [spos, send) are valid in the stage

  // Two 64-byte windows per step, A = [wb, wb + 64) and B = [wb + 64,
  // wb + 128), each lane decoding one candidate tag in each: the pointer
  // doubling does not depend on where the chain enters a window, so both
  // windows' doublings run interleaved (one latency chain of shuffles per
  // 128 bytes instead of per 64), and B's chain is read at A's exit.
  while (status < 0) {
    if (ip >= n_in) {  // end of input between tags (snappy.cc:858-868)
      status = (ip == n_in && op == expected) ? kOk : kCorrupt;
      break;
    }
    const u32 wb = ip & ~31u;
    // ---------- stage input covering [wb, wb + 128 + 8)
    if (spos < 0 || wb < (u32)spos || wb + 136 > send) {
      const u32 c0 = (wb + ibal) >> 4;
      u32x4 x[kBigStageChunks / 64];
#pragma unroll
      for (u32 r = 0; r < kBigStageChunks / 64; ++r) {
        u32 k = c0 + r * 64 + lane;
        k = k <= last_chunk ? k : last_chunk;
        x[r] = *reinterpret_cast<const u32x4*>(abase + 16 * k);
      }
      wave_lds_fence();  // previous window's stage reads are done
#pragma unroll
      for (u32 r = 0; r < kBigStageChunks / 64; ++r)
        *reinterpret_cast<u32x4*>(st + 4 * (r * 64 + lane)) = x[r];
      wave_lds_fence();
      spos = (int)(16 * c0) - (int)ibal;
      send = (u32)spos + kBigStageBytes - 8;
    }
    // ---------- every lane decodes the tag that would start at wb + lane
    // (A) and at wb + 64 + lane (B): length, offset, next position, local
    // validity (tag and literal bytes present), successor lane in the window
    struct Cand {
      u32 len, coff, nxt, J;
      bool lit, bad_local;
    };
    auto decode = [&](u32 p) {
      const u32 s = p - (u32)spos;
      const u32 dw = s >> 2, bsh = s & 3;
      const u32 lo = st[dw], hi = st[dw + 1];
      const u32 t0 = alignbyte(hi, lo, bsh);
      const u32 b4 = (hi >> (8 * bsh)) & 0xffu;
      const u32 c = t0 & 0xffu;
      const u32 type = c & 3;
      Cand d;
      d.lit = type == 0;
      const u32 l0 = (c >> 2) + 1;
      const bool longlit = d.lit & (l0 >= 61);
      const u32 nb = d.lit ? (longlit ? l0 - 60 : 0u) : (1u << (type - 1));
      const u32 ext = (b4 << 24) | (t0 >> 8);
      const u32 val = nb >= 4 ? ext : ext & ((1u << (8 * nb)) - 1u);
      d.len = d.lit ? (longlit ? val + 1u : l0) : (type == 1 ? 4 + ((c >> 2) & 7) : l0);
      d.coff = type == 1 ? (((c >> 5) << 8) | val) : val;
      const u32 avail = n_in - p - 1;
      d.bad_local = (p >= n_in) | (avail < nb) | (d.lit & (avail - nb < d.len));
      const u32 adv = 1 + nb + (d.lit ? d.len : 0u);
      d.nxt = p + adv;
      d.J = (d.bad_local || adv >= 64 - lane || d.nxt >= n_in) ? 64u : lane + adv;
      return d;
    };
    const u32 pA = wb + lane, pB = wb + 64 + lane;
    const Cand A = decode(pA), B = decode(pB);
    // ---------- pointer doubling in both windows (see the one-window form)
    u64 MA = 1ull << lane, MB = 1ull << lane;
    u32 JA = A.J, JB = B.J;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      const u32 sA = JA < 64 ? JA : lane, sB = JB < 64 ? JB : lane;
      const u64 MAj = ((u64)(u32)__shfl((int)(u32)(MA >> 32), (int)sA, 64) << 32) |
                      (u32)__shfl((int)(u32)MA, (int)sA, 64);
      const u64 MBj = ((u64)(u32)__shfl((int)(u32)(MB >> 32), (int)sB, 64) << 32) |
                      (u32)__shfl((int)(u32)MB, (int)sB, 64);
      const u32 JAj = (u32)__shfl((int)JA, (int)sA, 64);
      const u32 JBj = (u32)__shfl((int)JB, (int)sB, 64);
      if (JA < 64) {
        MA |= MAj;
        JA = JAj;
      }
      if (JB < 64) {
        MB |= MBj;
        JB = JBj;
      }
    }
    const u32 firstA = ip - wb;
    const u64 SA = ((u64)readlane((u32)(MA >> 32), firstA) << 32) | readlane((u32)MA, firstA);
    const u32 lastA = 63u - (u32)__builtin_clzll(SA);
    const u32 ipA = readlane(A.nxt, lastA);  // where the chain leaves A
    // B is entered when A's last tag is good and ends inside B
    const bool enterB = ipA >= wb + 64 && ipA < wb + 128 && ipA < n_in;
    const u32 firstB = enterB ? ipA - wb - 64 : 0u;
    const u64 SB = enterB ? ((u64)readlane((u32)(MB >> 32), firstB) << 32) | readlane((u32)MB, firstB) : 0ull;
    const bool inA = (SA >> lane) & 1ull, inB = (SB >> lane) & 1ull;
    // output positions: A's chain from op, then B's
    const u32 lvA = inA ? A.len : 0u;
    const u32 incA = dpp_incl_scan(lvA);
    const u32 t_opA = op + incA - lvA;
    const u32 opA = op + readlane(incA, 63);
    const u32 lvB = inB ? B.len : 0u;
    const u32 incB = dpp_incl_scan(lvB);
    const u32 t_opB = opA + incB - lvB;
    // writer space and copy offset checks (:761, :1166, :1200, :1410, :1466)
    const bool badA = inA && (A.bad_local || expected - t_opA < A.len || (!A.lit && A.coff - 1u >= t_opA));
    const bool badB = inB && (B.bad_local || expected - t_opB < B.len || (!B.lit && B.coff - 1u >= t_opB));
    if (__any(badA || badB)) {
      status = kCorrupt;
      break;
    }
    // 64 KiB output segments (see the one-window form)
    if (seg) {
      const bool spanA = inA && A.len > 0 && ((t_opA ^ (t_opA + A.len - 1)) >> 16) != 0;
      const bool spanB = inB && B.len > 0 && ((t_opB ^ (t_opB + B.len - 1)) >> 16) != 0;
      const bool xA = inA && !A.lit && t_opA - A.coff < (t_opA & ~0xffffu);
      const bool xB = inB && !B.lit && t_opB - B.coff < (t_opB & ~0xffffu);
      if (__any(spanA || spanB || xA || xB)) seg = false;
      if (seg && inA && t_opA != 0 && (t_opA & 0xffffu) == 0 && t_opA + 4 <= expected)
        __builtin_memcpy(ob + t_opA, &pA, 4);
      if (seg && inB && t_opB != 0 && (t_opB & 0xffffu) == 0 && t_opB + 4 <= expected)
        __builtin_memcpy(ob + t_opB, &pB, 4);
    }
    if (SB) {
      const u32 lastB = 63u - (u32)__builtin_clzll(SB);
      ip = readlane(B.nxt, lastB);
      op = opA + readlane(incB, 63);
    } else {
      ip = ipA;
      op = opA;
    }
    const u64 Sw = lane < 2 ? SA : SB;
    const u32 wbits = (lane & 1) == 0 ? (u32)Sw : (u32)(Sw >> 32);
    if (lane < 4 && wbits) bm[(wb >> 5) + lane] = wbits;
  }
  return status;
}

// Pass 1b launch: one wave per listed large message (taken from a counter,
// huge ones first).  Each finished message goes to pass 2's work lists: its
// 64 KiB segments (seg_list: m | k << 32 | last << 63) when the stream
// allows them, else the whole message (whole_list).
__global__ __launch_bounds__(4 * 64) void index_big_kernel(
    const u8* __restrict__ in, const u64* __restrict__ in_off,
    const u32* __restrict__ in_len, const u32* __restrict__ out_len, u32 flags,
    i32* __restrict__ status_out, const u32* __restrict__ bm_base,
    u32* __restrict__ bitmap, const u32* __restrict__ big_count,
    const u32* __restrict__ big_list, u32* __restrict__ big_next, u32 n_msgs, u8* out,
    const u64* __restrict__ out_off, u64* __restrict__ seg_list, u32* __restrict__ seg_count,
    u32* __restrict__ whole_list, u32* __restrict__ whole_count, u32 mode) {
  __shared__ u32 stage_s[4][kBigStageBytes / 4 + 4];
  const u32 wv = (u32)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const u32 lane = threadIdx.x & 63;
  const bool strict = flags & 2u;
  // mode 0: every listed message, the huge ones (> kHugeIndexBytes) first;
  // 1: the huge ones only; 2: the others only (the forked path walks the two
  // sets on two streams, so the others' execution starts without waiting for
  // the longest walks)
  const u32 n_huge = mode == 2 ? 0u : big_count[8];
  const u32 count = (mode == 1 ? 0u : big_count[0]) + n_huge;
  if (count == 0) return;  // uniform batches: no atomics on the shared counter
  for (;;) {  // all-lane atomic: lane 0 adds 1, lane 0's result is the index
    const u32 got = atomicAdd(big_next, lane == 0 ? 1u : 0u);
    const u32 idx = (u32)__builtin_amdgcn_readfirstlane((int)got);
    if (idx >= count) break;
    const u32 m = idx < n_huge ? big_list[n_msgs - 1 - idx] : big_list[idx - n_huge];
    bool seg = true;
    const i32 st = index_big_message(m, in, in_off, in_len, out_len, strict, bm_base, bitmap,
                                     stage_s[wv], lane, out + out_off[m], seg);
    if (lane == 0) status_out[m] = st;
    if (st != kOk) continue;
    const u32 expected = out_len[m];
    u32 nseg = 0;  // > 1: run as segments
    if (seg && expected > 65536u) {
      nseg = (expected + 65535u) >> 16;
      if (expected - ((nseg - 1) << 16) < 4) --nseg;  // the tail joins the previous segment
    }
    bool whole = nseg < 2;
    if (!whole) {
      u32 b = 0;
      if (lane == 0) b = atomicAdd(seg_count, nseg);
      b = readlane(b, 0);
      for (u32 k = lane; k < nseg; k += 64) {
        const u64 e = b + k < n_msgs
            ? ((u64)m | ((u64)k << 32) | ((u64)(k == nseg - 1) << 63))
            : 0xffffffffull;  // past the list: dropped, the message runs whole
        if (b + k < n_msgs) seg_list[b + k] = e;
      }
      if (b + nseg > n_msgs) {
        // partly listed: the listed entries become holes
        for (u32 k = lane; b + k < n_msgs && k < nseg; k += 64) seg_list[b + k] = 0xffffffffull;
        whole = true;
      }
    }
    if (whole) {
      u32 b = 0;
      if (lane == 0) b = atomicAdd(whole_count, 1u);
      b = readlane(b, 0);
      if (lane == 0) whole_list[b] = m;
    }
  }
}

}  // namespace fsg
