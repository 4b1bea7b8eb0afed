// decode_v4_exec4.h -- pass 2 of the two-pass Snappy decoder
// (snappy_decode_v4.hip), variant 4: one WAVE per message, one <= 16-byte
// PIECE per lane.  The A/B variant; variant 5 (decode_v4_exec5.h) is the
// default.  exec_kernel<4> calls exec_message per message or 64 KiB segment.
#pragma once

#include "decode_v4_exec_common.h"
#include "decode_v4_plan.h"
#include "snappy_pieces.h"
#include "wave_util.h"

namespace fsg {

// ===========================================================================
// Pass 2: execute.  One wave per status-OK message.
//
// Output is assembled in a per-wave LDS window `sb` (kWindow bytes) holding
// output positions [sbase, sbase + kWindow); sbase is kept congruent to the
// slot's address modulo 16 so window offsets and global addresses share
// 16-byte alignment.  Per group of <= 64 pieces:
//   round A   literal pieces (input bytes) and far copies (source before the
//             window, already stored) load from global memory -- one round
//             trip, all independent -- and land in the window;
//   rounds B  near copies (source inside the window) resolve in LDS in
//             dependency rounds, OR-ing their bytes into the zeroed window
//             ahead of the write front (five aligned ds_or_b32 per piece);
//   flush     completed 16-byte blocks go to global memory, 1 KiB per wave
//             instruction.
// The window slides (keeping >= 2 KiB of history) when a group would overrun
// it.  Literals longer than 64 bytes bypass it: the wave copies them
// global-to-global, 1 KiB per instruction.
// ===========================================================================
// (The window constants kWindow, kKeep and kMaxKeep: decode_v4_plan.h, which
// range-checks option exec_keep against them.)

// One message, executed by the calling wave (see the pass-2 comment above).
__device__ __forceinline__ void exec_message(
    u32 m, const u8* __restrict__ in, const u64* __restrict__ in_off,
    const u32* __restrict__ in_len, u8* out, const u64* __restrict__ out_off,
    const u32* __restrict__ out_len, i32* __restrict__ status, const u32* __restrict__ bm_base,
    const u32* __restrict__ bitmap, u32* ring, u8* pmap, u8* sb, const u32x4* sel_tab,
    const u32x4* mtab, u32 lane, i32 st, u32 ip0, u32 op0, u32 op1, bool prio, u32 keep_hist) {
  // One message (ip0 = op0 = 0, op1 = its length), or one segment of a large
  // one: output [op0, op1) from the tags starting at input offset ip0, whose
  // copies stay inside the segment (checked by the index walk).
  // every per-message scalar is loaded up front (one round trip, not a chain)
  const u32 bmb = bm_base[m];
  const u32 n_in = in_len[m];
  const u32 expected = out_len[m];
  const u8* ib = in + in_off[m];
  u8* ob = out + out_off[m];
  if (st != kOk) return;
  const u32 ibal = (u32)(reinterpret_cast<uintptr_t>(ib) & 15);
  const u32 obal = (u32)(reinterpret_cast<uintptr_t>(ob) & 15);
  // the message's input as a buffer: tag and literal loads need no clamping
  const __amdgpu_buffer_rsrc_t irsrc = msg_rsrc(ib - ibal, ibal + n_in);
  // the message's slot as a buffer: far copies load through it past L1
  const __amdgpu_buffer_rsrc_t orsrc =
      __builtin_amdgcn_make_buffer_rsrc(ob - obal, (short)0, (int)(expected + obal), 0x00020000);

  if ((bmb & kSingleLiteral) && op1 == expected && op0 == 0) {
    // one literal (checked by pass 1): a straight copy, 4 KiB per step with
    // all loads first
    const u32 S = bmb & ~kSingleLiteral;
    for (u32 k0 = 0; k0 < expected; k0 += 4096) {
      u32x4 x[4];
#pragma unroll
      for (u32 r = 0; r < 4; ++r) {
        const u32 k = k0 + 1024 * r + lane * 16;
        x[r] = k < expected ? rsrc_load16(irsrc, S + k + ibal) : u32x4{0, 0, 0, 0};
      }
#pragma unroll
      for (u32 r = 0; r < 4; ++r) {
        const u32 k = k0 + 1024 * r + lane * 16;
        if (k < expected) store_exact(ob + k, x[r], expected - k < 16 ? expected - k : 16u);
      }
    }
    return;
  }
  const u32* bm = bitmap + bmb;
  const u32 nwords = (n_in + 31) >> 5;

#ifdef FSG_STAMPS
  u64 st_[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  u64 t_last_ = __builtin_amdgcn_s_memtime();
#endif
  u32 head = 0, tail = 0, scan = ip0 >> 5, op = op0;
  int sbase = (int)((op0 + obal) & ~15u) - (int)obal;  // output position of sb[0]
  u32 flushed = op0;  // output [op0, flushed) is in global memory
  // window bytes from the write front up to zero_end are zero, so rounds B
  // can OR their pieces in (or_store)
  auto zero_from = [&](u32 from) {  // 1 KiB of zeros at a 16-aligned offset
    const u32 i = from + 16 * lane;
    if (i < kWindow + 32) *reinterpret_cast<u32x4*>(sb + i) = u32x4{0, 0, 0, 0};
  };
  zero_from(0);
  u32 zero_end = 1024;
  wave_lds_fence();
  // next fill, prefetched: lane l holds word scan + l / 4 and takes its byte l % 4
  auto fill_word = [&](u32 sc) -> u32 {
    const u32 wi = sc + (lane >> 2);
    return (lane < 4 * kFillWords && wi < nwords) ? bm[wi] : 0u;
  };
  u32 bmw = fill_word(scan);
  u32 pf_head = 0xffffffffu, pf_cnt = 0;  // tag bytes prefetched for ring [pf_head, +pf_cnt)
  u32x2 tv = u32x2{0, 0};

  // Store window bytes [flushed, fe) to the slot: one 16-byte block per lane,
  // whole aligned blocks with one store, partial edge blocks exactly.
  auto flush_to = [&](u32 fe) {
    if (fe <= flushed) return;
    const int b0 = (int)(((flushed + obal) & ~15u)) - (int)obal;  // block start <= flushed
    for (int blk = b0 + 16 * (int)lane; blk < (int)fe; blk += 1024) {
      const u32 lo = blk < (int)flushed ? flushed : (u32)blk;
      const u32 hi = blk + 16 < (int)fe ? (u32)(blk + 16) : fe;
      if (hi - lo == 16) {
        const u32x4 v = *reinterpret_cast<const u32x4*>(sb + (blk - sbase));
        __builtin_memcpy(ob + blk, &v, 16);
      } else {
        store_exact(ob + lo, lds_read16(sb + ((int)lo - sbase)), hi - lo);
      }
    }
    flushed = fe;
  };

  for (;;) {
    // ---------- refill the tag ring from the bitmap (keeps >= 64 tags ahead)
    if (tail - head < 2 * kMaxPieces && scan < nwords) {
      if (prio) __builtin_amdgcn_s_setprio(1);  // the fill's bitmap load: same rule (C3 -1.5%)
      u32 bits = (bmw >> (8 * (lane & 3))) & 0xffu;  // 8 bits per lane
      const u32 bitbase = (scan + (lane >> 2)) * 32 + 8 * (lane & 3);
      // a segment's walk starts at ip0: earlier tag starts are not its own
      if (bitbase < ip0) bits &= bitbase + 8 <= ip0 ? 0u : (0xffu << (ip0 - bitbase)) & 0xffu;
      const u32 cnt = __builtin_popcount(bits);
      const u32 incl = dpp_incl_scan(cnt);
      u32 slot = tail + incl - cnt;
      while (bits) {
        ring[slot & (kTagRing - 1)] = bitbase + __builtin_ctz(bits);
        ++slot;
        bits &= bits - 1;
      }
      tail += readlane(incl, 63);
      scan += kFillWords;
      bmw = fill_word(scan);
      wave_lds_fence();
      STAMP(0);
      continue;
    }
    const u32 avail = tail - head;
    if (avail == 0 || op >= op1) break;
    const u32 take0 = avail < 64 ? avail : 64u;
    const bool valid = lane < take0;
    const u32 pos = valid ? ring[(head + lane) & (kTagRing - 1)] : 0u;
    if (pf_head != head || pf_cnt < take0)
      tv = valid ? rsrc_tag5(irsrc, pos + ibal) : u32x2{0, 0};

    // ---------- decode one tag per lane (checked by pass 1)
    // A wave on its way to the group's global loads (round A; and the bitmap
    // load of a fill) runs at raised priority until it has issued them, so the
    // SIMD's issue slots go to the waves that will put memory requests in
    // flight (A/B on one box: C3 7.53 -> 7.37 ms, C2 neutral; CM +2%, so
    // only for the single-stream batches: `prio`; lowering it only for
    // rounds B instead measured the same).
    if (prio) __builtin_amdgcn_s_setprio(1);
    const u32 t0 = tv[0], t1 = tv[1];
    const u32 c = t0 & 0xffu;
    const u32 type = c & 3;
    const bool is_lit = type == 0;
    const u32 l0 = (c >> 2) + 1;
    const bool longlit = is_lit && l0 >= 61;
    const u32 nbl = longlit ? l0 - 60 : 0u;
    const u32 ext = (t0 >> 8) | (t1 << 24);
    const u32 msk = nbl >= 4 ? 0xffffffffu : ((1u << (8 * nbl)) - 1u);
    const u32 litlen = longlit ? (ext & msk) + 1u : l0;
    const u32 nb = is_lit ? nbl : (type == 1 ? 1u : (type == 2 ? 2u : 4u));
    const u32 clen = type == 1 ? 4 + ((c >> 2) & 7) : l0;
    const u32 coff = type == 1 ? (((c >> 5) << 8) | ((t0 >> 8) & 0xffu))
                               : (type == 2 ? ((t0 >> 8) & 0xffffu) : ext);
    const u32 len = is_lit ? litlen : clen;
    const u32 lsrc = pos + 1 + nb;

    const u64 bigm = __ballot(valid && is_lit && len > 64);
    STAMP(1);
    if (bigm & 1ull) {
      // ---------- long literal: written straight to the slot by the whole
      // wave; the window restarts behind it
      const u32 L = readlane(len, 0), S = readlane(lsrc, 0);
      if ((u64)op + L > op1) {  // writer overrun
        if (lane == 0) status[m] = kCorrupt;
        return;
      }
      flush_to(op);
      // 4 KiB per step: all loads first, so their latencies overlap
      for (u32 k0 = 0; k0 < L; k0 += 4096) {
        u32x4 x[4];
#pragma unroll
        for (u32 r = 0; r < 4; ++r) {
          const u32 k = k0 + 1024 * r + lane * 16;
          x[r] = k < L ? rsrc_load16(irsrc, S + k + ibal) : u32x4{0, 0, 0, 0};
        }
#pragma unroll
        for (u32 r = 0; r < 4; ++r) {
          const u32 k = k0 + 1024 * r + lane * 16;
          if (k < L) store_exact(ob + op + k, x[r], L - k < 16 ? L - k : 16u);
        }
      }
      op += L;
      flushed = op;
      // The window restarts one block before the block holding op, so that
      // >= 16 flushed bytes precede it (a copy reading before the window
      // then reads only stored bytes); its head comes from the literal's tail.
      sbase = (int)((op + obal) & ~15u) - (int)obal - 16;
      zero_from(0);
      zero_end = 1024;
      wave_lds_fence();
      if (lane < 2) {
        const u32 lo = (u32)sbase + 16 * lane;
        if (lo < op) {
          const u32 cnt = op - lo < 16 ? op - lo : 16u;
          store_exact(sb + 16 * lane, rsrc_load16(irsrc, S + L - (op - lo) + ibal), cnt);
        }
      }
      wave_lds_fence();
      head += 1;
      pf_head = 0xffffffffu;
      // the literal's bytes hold no tag starts: resume the bitmap scan at the
      // word of the next tag instead of scanning the zero words in between
      if (head == tail) {
        const u32 nw = (S + L) >> 5;
        if (nw > scan) {
          scan = nw;
          bmw = fill_word(scan);
        }
      }
      STAMP(7);
      continue;
    }
    const u32 take = bigm ? (u32)__builtin_ctzll(bigm) : take0;
    const bool v = lane < take;

    // ---------- pieces: <= 16 bytes each, one per lane
    const bool pat = !is_lit && coff < 16;
    const u32 step = pat ? pat_step(coff) : 16u;
    const u32 pc = v ? (pat ? pattern_pieces(len, step) : (len + 15) >> 4) : 0u;
    const u32 lv = v ? len : 0u;
    const u32 incl = dpp_incl_scan(pc | (lv << 16));
    const u32 incl_pc = incl & 0xffffu, excl_pc = incl_pc - pc;
    const u32 t_op = op + (incl >> 16) - lv;
    const bool fits = v && incl_pc <= kMaxPieces && t_op < op1;
    const u32 k_tags = (u32)__builtin_popcountll(__ballot(fits));
    const u32 tot_pc = readlane(incl_pc, k_tags - 1);
    const u32 tot_len = readlane(incl >> 16, k_tags - 1);
    // copy offset 0 or past the bytes produced so far: the reference's
    // writer check (snappy.cc:1200, :1410, :1466); the message is corrupt
    // and the writer's space check (:1166, :1400) against the header length
    if (__any(fits && ((u64)t_op + len > op1 || (!is_lit && (coff == 0 || coff > t_op - op0))))) {
      if (lane == 0) status[m] = kCorrupt;
      return;
    }

    STAMP(2);
    // ---------- slide the window if this group would overrun it
    if (op + tot_len - sbase > kWindow) {
      const int nsb = (int)(((op - keep_hist + obal) & ~15u)) - (int)obal;
      // a far piece (source below the new base) may read up to 15 bytes at
      // and above the base, so those must be stored too
      if ((int)flushed < nsb + 16) flush_to((u32)((int)((op + obal) & ~15u) - (int)obal));
      // From this group on, far loads read bytes below the new base + 16:
      // stored by this flush or by earlier groups' flushes, which may still
      // be in flight (no waited load was issued after the last of them, the
      // ordering argument of DESIGN.md §4).  Wait until they are
      // acknowledged by L2, where the far loads (sc1) are served.  Once per
      // slide (~every 3 KiB of output).
      wait_all_memory();
      const u32 shift = (u32)(nsb - sbase), keep = (u32)((int)op - nsb);
      for (u32 k = 0; k < keep; k += 1024) {
        const u32 i = k + 16 * lane;
        u32x4 x = u32x4{0, 0, 0, 0};
        if (i < keep) x = *reinterpret_cast<const u32x4*>(sb + shift + i);
        wave_lds_fence();
        if (i < keep) *reinterpret_cast<u32x4*>(sb + i) = x;
        wave_lds_fence();
      }
      sbase = nsb;
      zero_end = (keep + 15) & ~15u;  // the copied blocks end in zeros past op
    }
    // ---------- prefetch the next group's tag bytes (lands during this group; issued after a
    // slide's store wait, which then waits only for older operations)
    {
      const u32 nh = head + k_tags;
      const u32 na = tail - nh;
      const u32 ncnt = na < 64 ? na : 64u;
      if (lane < ncnt) {
        const u32 npos = ring[(nh + lane) & (kTagRing - 1)];
        tv = rsrc_tag5(irsrc, npos + ibal);
      }
      pf_head = nh;
      pf_cnt = ncnt;
    }

    while (op + tot_len + 20 - sbase > zero_end) {  // the group's OR stores land in zeros
      zero_from(zero_end);
      zero_end += 1024;
    }
    wave_lds_fence();

    if (fits)
      for (u32 p = 0; p < pc; ++p) pmap[excl_pc + p] = (u8)lane;
    wave_lds_fence();
    const bool has = lane < tot_pc;
    const u32 t = has ? pmap[lane] : 0u;
    const u32 kind = is_lit ? 0u : (pat ? 2u : 1u);
    const u32 A = t_op;
    const u32 B = len | (excl_pc << 8) | (kind << 16) | ((pat ? coff : 0u) << 20);
    const u32 C = is_lit ? lsrc : t_op - coff;
    const u32 At = __shfl(A, t, 64), Bt = __shfl(B, t, 64), Ct = __shfl(C, t, 64);
    const u32 lenT = Bt & 0xffu, exT = (Bt >> 8) & 0xffu, kT = (Bt >> 16) & 3u, offT = Bt >> 20;
    const u32 stepT = kT == 2 ? pat_step(offT) : 16u;
    const u32 qs = (lane - exT) * stepT;
    const u32 dst = At + qs;
    const u32 n = lenT - qs < stepT ? lenT - qs : stepT;
    const u32 src = kT == 2 ? Ct : Ct + qs;
    const u32 need_end = kT == 0 ? 0u : (kT == 2 ? At : src + n);
    u8* const wdst = sb + ((int)dst - sbase);

    STAMP(3);
    // ---------- round A: literal pieces and far copies, from global memory
    const bool global_src = has && (kT == 0 || (int)src < sbase);
    u32x4 xa = u32x4{0, 0, 0, 0};
    if (global_src)
      xa = kT == 0 ? rsrc_load16(irsrc, src + ibal) : far_load(orsrc, src + obal);
    if (prio) __builtin_amdgcn_s_setprio(0);
    // the previous group's completed blocks are flushed while these loads are
    // in flight (far sources lie before the window: flushed long ago)
    {
      const int fe = (int)((op + obal) & ~15u) - (int)obal;
      // once a wave instruction's worth (1 KiB) is complete: every lane
      // stores a full block.  A slide first flushes what it would drop, so
      // far sources (below the window base) are always in global memory.
      if (fe >= (int)flushed + 1024) flush_to((u32)fe);
    }
    if (global_src) {
      if (kT == 2) xa = expand_pattern(xa, offT, sel_tab);
      store_exact(wdst, xa, n);  // (or_store here measured 4% slower)
    }
    wave_lds_fence();

    STAMP(4);
    // ---------- rounds B: near copies, in LDS, in dependency order.  The
    // pending set lives in a scalar mask: per round one find-first, one
    // readlane and one ballot (C3 7.95 -> 7.87 ms against a per-lane done
    // flag re-balloted each round).  The pattern expansion keeps its branch:
    // running it for every piece measured 2.8% slower.
    u64 pend = __ballot(has && !global_src);
    while (pend) {
      const u32 wm = readlane(dst, (u32)__builtin_ctzll(pend));
      const bool ready = ((pend >> lane) & 1ull) && need_end <= wm;
      if (ready) {
        u32x4 x = lds_read16(sb + ((int)src - sbase));
        if (kT == 2) x = expand_pattern(x, offT, sel_tab);
        or_store(sb, (u32)((int)dst - sbase), x, n, mtab);
      }
      wave_lds_fence();
      pend &= ~__ballot(ready);
    }
    op += tot_len;
    head += k_tags;

    STAMP(5);
  }
  if (op != op1) {  // the stream ended early (snappy.cc:858-868)
    if (lane == 0) status[m] = kCorrupt;
    return;
  }
  flush_to(op1);
#ifdef FSG_STAMPS
  if (lane == 0)
    for (int k = 0; k < 8; ++k) atomicAdd(&g_stamps[k], (unsigned long long)st_[k]);
#endif
}

}  // namespace fsg
