// decode_v4_exec5.h -- pass 2 of the two-pass Snappy decoder
// (snappy_decode_v4.hip), variant 5, the default: one WAVE per message, one
// TAG per lane.  exec_kernel<5> calls exec5_message per message or 64 KiB
// segment; exec_tag_entry fills the tag table of exec_kernel<5> and
// exec_packed_kernel.
#pragma once

#include "decode_v4_exec_common.h"
#include "decode_v4_plan.h"
#include "snappy_pieces.h"
#include "wave_util.h"

namespace fsg {

// ===========================================================================
// Pass 2, v5 (default): one TAG per lane.
//
// Same walk as v4 (tag ring from the bitmap, LDS output window, far copies
// from the slot, flush, slide, long literals), with the per-group work cut
// down to what a tag needs:
//   - the next group's tag bytes are prefetched as 20 bytes per lane (one
//     16-byte and one 4-byte buffer load at the dword below the tag: no
//     clamping, bytes past the message read 0), so a short literal's bytes
//     (<= 16 of them follow the tag byte) are already in registers -- a
//     literal tag needs no load of its own;
//   - the tag is decoded through a 256-entry table in LDS (char_table,
//     snappy.cc:516-549);
//   - no piece map: a lane executes its own tag as <= 4 chunks of 16 bytes.
//     Round A writes every chunk whose source is in registers or global
//     memory (literals, far copies); rounds B run the near chunks in
//     dependency order (a chunk runs once its source ends at or below the
//     first unfinished chunk of the group).  A copy with offset < 16 that
//     overlaps itself writes pat_step(off)-byte chunks of its expanded
//     pattern; each later chunk copies the previous one.
// ===========================================================================
namespace {
constexpr u32 kGroupBytes = 1024;  // output bytes per group (as v4: 64 pieces x 16)
static_assert(kExecRing == kTagRing, "decode_v4_plan.h sizes the folded instance's window from the ring");

// Per tag byte c: bits 0-4 the right shift of 0xffffffff that masks the nb
// extra bytes ((32 - 8 nb) & 31), bit 5 long literal (length = extra + 1),
// bit 6 literal, bits 8-14 length (short literal, copies), bits 16-18 nb,
// bits 20-30 COPY_1's offset bits 8-10 (snappy.cc:744-781).
__device__ __forceinline__ u32 exec_tag_entry(u32 c) {
  const u32 type = c & 3, l0 = (c >> 2) + 1;
  u32 nb, len, lit = 0, ll = 0, hi = 0;
  if (type == 0) {
    lit = 1;
    nb = l0 > 60 ? l0 - 60 : 0;
    ll = nb ? 1 : 0;
    len = nb ? 0 : l0;
  } else if (type == 1) {
    nb = 1;
    len = 4 + ((c >> 2) & 7);
    hi = (c >> 5) << 8;
  } else {
    nb = type == 2 ? 2 : 4;
    len = l0;
  }
  return ((32 - 8 * nb) & 31) | (ll << 5) | (lit << 6) | (len << 8) | (nb << 16) | (hi << 20);
}
}  // namespace

// Two instances (exec_kernel<5>):
//   - folded, <true, u16, kWindowWhole>: a whole body of at most big_threshold
//     compressed bytes (every wave-per-message block).  The range it decodes
//     is the whole message, so ip0 = 0, op0 = 0 and op1 = out_len[m] are
//     constants (the arguments are ignored) and the range tests fold away; a
//     tag position is below kBigIndexMax < 2^16, so the ring holds 16-bit
//     entries, and the KiB that frees goes to the window;
//   - general, <false, u32, kWindow>: the listed large messages, whole or one
//     64 KiB segment [op0, op1) of the output starting at input offset ip0.
// Per wave both use 4 kTagRing + kWindow + 32 bytes of LDS: the ring
// (sizeof(RingT) kTagRing bytes), then the window (kWin + 32).
template <bool kWhole, typename RingT, u32 kWin>
__device__ __forceinline__ void exec5_message(
    u32 m, const u8* __restrict__ in, const u64* __restrict__ in_off,
    const u32* __restrict__ in_len, u8* out, const u64* __restrict__ out_off,
    const u32* __restrict__ out_len, i32* __restrict__ status, const u32* __restrict__ bm_base,
    const u32* __restrict__ bitmap, RingT* ring, const u32* tagtab, u8* sb, const u32x4* sel_tab,
    const u32x4* mtab, u32 lane, i32 st, u32 ip0_, u32 op0_, u32 op1_, bool prio, u32 keep_hist) {
  static_assert(sizeof(RingT) == 4 || (kWhole && sizeof(RingT) == 2 && kBigIndexMax < 65536),
                "16-bit ring entries: tag positions of a body of at most big_threshold bytes");
  static_assert(sizeof(RingT) * kTagRing + kWin == 4 * kTagRing + kWindow && kWin % 16 == 0,
                "ring + window fill the wave's LDS");
  const u32 bmb = bm_base[m];
  const u32 n_in = in_len[m];
  const u32 expected = out_len[m];
  const u32 ip0 = kWhole ? 0u : ip0_, op0 = kWhole ? 0u : op0_, op1 = kWhole ? expected : op1_;
  const u8* ib = in + in_off[m];
  u8* ob = out + out_off[m];
  if (st != kOk) return;
  const u32 ibal = (u32)(reinterpret_cast<uintptr_t>(ib) & 15);
  const u32 obal = (u32)(reinterpret_cast<uintptr_t>(ob) & 15);
  const __amdgpu_buffer_rsrc_t irsrc = msg_rsrc(ib - ibal, ibal + n_in);
  // the slot as a buffer: far copies load through it past L1 (see far_load)
  const __amdgpu_buffer_rsrc_t orsrc =
      __builtin_amdgcn_make_buffer_rsrc(ob - obal, (short)0, (int)(expected + obal), 0x00020000);

  if ((bmb & kSingleLiteral) && op1 == expected && op0 == 0) {
    const u32 S = bmb & ~kSingleLiteral;
    for (u32 k0 = 0; k0 < expected; k0 += 4096) {
      Raw16 x[4];
#pragma unroll
      for (u32 r = 0; r < 4; ++r) x[r] = raw_load16(irsrc, S + k0 + 1024 * r + lane * 16 + ibal);
#pragma unroll
      for (u32 r = 0; r < 4; ++r) {
        const u32 k = k0 + 1024 * r + lane * 16;
        if (k < expected) store_exact(ob + k, shifted16(x[r]), expected - k < 16 ? expected - k : 16u);
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
  u32 flushed = op0;                                    // output [op0, flushed) is in global memory
  auto zero_from = [&](u32 from) {  // 1 KiB of zeros at a 16-aligned offset
    const u32 i = from + 16 * lane;
    if (i < kWin + 32) *reinterpret_cast<u32x4*>(sb + i) = u32x4{0, 0, 0, 0};
  };
  zero_from(0);
  u32 zero_end = 1024;
  wave_lds_fence();
  auto fill_word = [&](u32 sc) -> u32 {
    const u32 wi = sc + (lane >> 2);
    return (lane < 4 * kFillWords && wi < nwords) ? bm[wi] : 0u;
  };
  u32 bmw = fill_word(scan);
  // the next group's tag bytes: 20 bytes from the dword below the tag
  u32 pf_head = 0xffffffffu, pf_cnt = 0;
  u32 pf_pos = 0;  // the ring positions the prefetch used
  u32x4 pd = u32x4{0, 0, 0, 0};
  u32 pd4 = 0;
  auto prefetch = [&](u32 p) {
    const u32 a = (p + ibal) & ~3u;
    pd = __builtin_amdgcn_raw_buffer_load_b128(irsrc, a, 0, 0);
    pd4 = __builtin_amdgcn_raw_buffer_load_b32(irsrc, a + 16, 0, 0);
  };

  auto flush_to = [&](u32 fe) {
    if (fe <= flushed) return;
    const int b0 = (int)(((flushed + obal) & ~15u)) - (int)obal;
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
    // ---------- refill the tag ring from the bitmap (as v4)
    if (tail - head < 2 * kMaxPieces && scan < nwords) {
      if (prio) __builtin_amdgcn_s_setprio(1);
      u32 bits = (bmw >> (8 * (lane & 3))) & 0xffu;
      const u32 bitbase = (scan + (lane >> 2)) * 32 + 8 * (lane & 3);
      if (bitbase < ip0) bits &= bitbase + 8 <= ip0 ? 0u : (0xffu << (ip0 - bitbase)) & 0xffu;
      const u32 cnt = __builtin_popcount(bits);
      const u32 incl = dpp_incl_scan(cnt);
      u32 slot = tail + incl - cnt;
      while (bits) {
        ring[slot & (kTagRing - 1)] = (RingT)(bitbase + __builtin_ctz(bits));
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
    // every lane reads the ring and prefetches: a lane past the valid tags
    // reads a stale position, whose buffer loads return message bytes or 0
    const u32 pos = ring[(head + lane) & (kTagRing - 1)];
    if (pf_head != head || pf_cnt < take0) prefetch(pos);
    if (prio) __builtin_amdgcn_s_setprio(1);

    // ---------- decode one tag per lane (checked by pass 1)
    const u32 s = (pos + ibal) & 3u;
    const u32 c = __builtin_amdgcn_alignbyte(pd[1], pd[0], s) & 0xffu;
    const u32 e = tagtab[c];
    // bytes pos+1 .. pos+16 (a short literal's bytes; a copy's offset bytes)
    const bool q = s == 3;
    const u32 w0 = q ? pd[1] : pd[0], w1 = q ? pd[2] : pd[1], w2 = q ? pd[3] : pd[2];
    const u32 w3 = q ? pd4 : pd[3];
    const u32 b = (s + 1) & 3u;
    const u32x4 xr = u32x4{__builtin_amdgcn_alignbyte(w1, w0, b), __builtin_amdgcn_alignbyte(w2, w1, b),
                           __builtin_amdgcn_alignbyte(w3, w2, b), __builtin_amdgcn_alignbyte(pd4, w3, b)};
    const u32 val = xr[0] & (0xffffffffu >> (e & 31u));
    const bool is_lit = e & 64u;
    const u32 len = (e & 32u) ? val + 1u : (e >> 8) & 0x7fu;
    const u32 off = val + (e >> 20);
    const u32 nb = (e >> 16) & 7u;
    const u32 lsrc = pos + 1 + nb;

    const u64 bigm = __ballot(valid && is_lit && len > 64);
    STAMP(1);
    if (bigm & 1ull) {
      // ---------- long literal: written straight to the slot by the whole
      // wave; the window restarts behind it (as v4)
      const u32 L = readlane(len, 0), S = readlane(lsrc, 0);
      if ((u64)op + L > op1) {
        if (lane == 0) status[m] = kCorrupt;
        return;
      }
      flush_to(op);
      for (u32 k0 = 0; k0 < L; k0 += 4096) {
        Raw16 x[4];
#pragma unroll
        for (u32 r = 0; r < 4; ++r) x[r] = raw_load16(irsrc, S + k0 + 1024 * r + lane * 16 + ibal);
#pragma unroll
        for (u32 r = 0; r < 4; ++r) {
          const u32 k = k0 + 1024 * r + lane * 16;
          if (k < L) store_exact(ob + op + k, shifted16(x[r]), L - k < 16 ? L - k : 16u);
        }
      }
      op += L;
      flushed = op;
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

    // ---------- output positions: <= kGroupBytes per group
    const u32 lv = v ? len : 0u;
    const u32 incl = dpp_incl_scan(lv);
    const u32 t_op = op + incl - lv;
    const bool fits = v && incl <= kGroupBytes && t_op < op1;
    const u32 k_tags = (u32)__builtin_popcountll(__ballot(fits));
    const u32 tot_len = readlane(incl, k_tags - 1);
    // the writer's checks (snappy.cc:1166, :1200, :1400, :1410, :1466)
    if (__any(fits && (len > op1 - t_op || (!is_lit && (off == 0 || off > t_op - op0))))) {
      if (lane == 0) status[m] = kCorrupt;
      return;
    }

    // ---------- slide the window if this group would overrun it (as v4)
    if (op + tot_len - sbase > kWin) {
      const int nsb = (int)(((op - keep_hist + obal) & ~15u)) - (int)obal;
      if ((int)flushed < nsb + 16) flush_to((u32)((int)((op + obal) & ~15u) - (int)obal));
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
      zero_end = (keep + 15) & ~15u;
    }
    // ---------- prefetch the next group's tag bytes; zero the window ahead
    auto prefetch_next_and_zero = [&]() {
      {
        const u32 nh = head + k_tags;
        const u32 na = tail - nh;
        const u32 ncnt = na < 64 ? na : 64u;
        pf_pos = ring[(nh + lane) & (kTagRing - 1)];
        prefetch(pf_pos);
        pf_head = nh;
        pf_cnt = ncnt;
      }
      while (op + tot_len + 20 - sbase > zero_end) {
        zero_from(zero_end);
        zero_end += 1024;
      }
      wave_lds_fence();
    };

    STAMP(2);
    // ---------- chunks: a literal's all come in round A (registers for
    // chunk 0 of a short literal, else the input); a copy's leading chunks
    // whose 16-byte source starts below the window base come from the slot
    // (far: stored at least one group ago); the rest run in rounds B
    const u32 src = is_lit ? lsrc : t_op - off;
    const u32 nch = (len + 15) >> 4;
    const bool pat = !is_lit && off < 16 && off < len;
    // leading chunks done in round A: all of a literal's; a copy's whose
    // 16-byte source starts below the window base (far: from the slot), then
    // those whose source ends at or below the group's first output byte op
    // (near-ready: final window bytes, read from LDS) -- none for a pattern.
    // A near-ready chunk would run in the first round B anyway; in round A it
    // is one OR store among the group's, not a read-modify-write of its own.
    const u32 below = (u32)(sbase - (int)src);  // > 0 as int: far
    const u32 kfar = (int)below > 0 ? ((below - 1) >> 4) + 1 : 0u;
    // chunk k's source ends at src + min(16 (k + 1), len): <= op for the
    // first (op - src) / 16 chunks, or all of them when src + len <= op
    const u32 kready = src + len <= op ? nch : (src < op ? (op - src) >> 4 : 0u);
    const u32 klead = kfar > kready ? kfar : kready;
    const u32 kc = pat ? 0u : (klead < nch ? klead : nch);
    const u32 kf = fits ? (is_lit ? nch : kc) : 0u;
    const bool reg0 = is_lit && nb == 0;
    // Loads only here: the data is first used after the flush below, so all
    // of a lane's chunk loads are in flight together.  A literal chunk is a
    // 16- and a 4-byte load at the dword below it, shifted later by sh; a far
    // chunk one unaligned 16-byte load (shift 0).
    const u32 sh = is_lit ? (src + ibal) & 3u : 0u;
    auto gload = [&](u32 k, u32x4& d, u32& d4) {
      if (is_lit) {
        const u32 a = (src + 16 * k + ibal) & ~3u;
        d = __builtin_amdgcn_raw_buffer_load_b128(irsrc, a, 0, 0);
        d4 = __builtin_amdgcn_raw_buffer_load_b32(irsrc, a + 16, 0, 0);
      } else if (k >= kfar) {  // near-ready: final bytes below op in the window
        d = lds_read16(sb + ((int)(src + 16 * k) - sbase));
      } else {
        d = far_load(orsrc, src + 16 * k + obal);
      }
    };
    u32x4 a0 = xr, a1 = u32x4{0, 0, 0, 0};
    u32 a0e = 0, a1e = 0;
    if (kf > 0 && !reg0) gload(0, a0, a0e);
    const u64 m1 = __ballot(kf > 1);
    if (m1 && kf > 1) gload(1, a1, a1e);
    // (the round-A loads go out before the next group's ring read and tag
    // prefetch and the window zeroing: their latency is the group's longest
    // wait; the near-ready LDS reads above read bytes below op, which the
    // zeroing (from zero_end >= op) does not touch)
    prefetch_next_and_zero();
    if (prio) __builtin_amdgcn_s_setprio(0);
    STAMP(3);
    {  // the previous groups' completed blocks, while the loads are in flight
      const int fe = (int)((op + obal) & ~15u) - (int)obal;
      if (fe >= (int)flushed + 1024) flush_to((u32)fe);
    }
    STAMP(4);
    const u32 wa = (u32)((int)t_op - sbase);
    if (kf > 0) or_store(sb, wa, shift16(a0, a0e, reg0 ? 0u : sh), len < 16 ? len : 16u, mtab);
    if (m1) {
      if (kf > 1) or_store(sb, wa + 16, shift16(a1, a1e, sh), len - 16 < 16 ? len - 16 : 16u, mtab);
      // chunks 2-3 (literals and far copies of 33..64 bytes: rare) reuse the
      // registers, one more round trip
      if (__ballot(kf > 2)) {
        if (kf > 2) gload(2, a0, a0e);
        if (kf > 3) gload(3, a1, a1e);
        if (kf > 2) or_store(sb, wa + 32, shift16(a0, a0e, sh), len - 32 < 16 ? len - 32 : 16u, mtab);
        if (kf > 3) or_store(sb, wa + 48, shift16(a1, a1e, sh), len - 48, mtab);
      }
    }
    wave_lds_fence();

    STAMP(5);
    // ---------- rounds B: near chunks, in LDS, in dependency order.  Per
    // lane: the current chunk's window offsets (cw destination, sw source),
    // its length n and the end of the bytes it needs, ne (~0: lane done).
    // A chunk runs once ne <= the first unfinished chunk's destination; it is
    // written read-modify-write: 16 window bytes are read and written back
    // with the chunk's n bytes merged in (v_bfi with the n-byte mask), so the
    // write is exact whatever n.  Within one write instruction overlapping
    // lanes land highest-lane-last (tools/probes/lds_overlap_probe.hip), and
    // a lane's 16-byte span only reaches later chunks, whose bytes it writes
    // back unchanged unless their own (higher) lane writes them.
    u32 rem = (fits && kf < nch) ? len - 16 * kf : 0u;
    u32 cw = (u32)((int)t_op - sbase) + 16 * kf;
    u32 sw = (u32)((int)src - sbase) + 16 * kf;
    const u32 stp = pat ? pat_step(off) : 16u;
    u32 n = rem < stp ? rem : stp;
    bool pf = pat;
    u32 ne = rem ? (pf ? cw : sw + n) : 0xffffffffu;
    u64 pend = __ballot(rem > 0);
    // Most groups (~90% on text) hold no pattern copy: their rounds run a
    // loop with no per-lane pattern state (the general loop below costs ~6
    // more instructions per round).
    if (!__ballot(pat && rem > 0)) {
      while (pend) {
        const u32 W = readlane(cw, (u32)__builtin_ctzll(pend));
        if (ne <= W) {
          const u32x4 x = lds_read16(sb + sw);
          const u32x4 o = lds_read16(sb + cw);
          const u32x4 y = merge16(x, o, mtab[n]);
          __builtin_memcpy(sb + cw, &y, 16);
          rem -= n;
          cw += n;
          sw += n;
          n = rem < 16u ? rem : 16u;
          ne = rem ? sw + n : 0xffffffffu;
        }
        wave_lds_fence();
        pend = __ballot(rem > 0);
      }
    }
    while (pend) {
      const u32 W = readlane(cw, (u32)__builtin_ctzll(pend));
      if (ne <= W) {
        u32x4 x = lds_read16(sb + sw);
        if (pf) x = expand_pattern(x, off, sel_tab);
        const u32x4 o = lds_read16(sb + cw);
        const u32x4 y = merge16(x, o, mtab[n]);
        __builtin_memcpy(sb + cw, &y, 16);
        rem -= n;
        cw += n;
        sw = pat ? cw - stp : sw + n;
        pf = false;
        n = rem < stp ? rem : stp;
        ne = rem ? sw + n : 0xffffffffu;
      }
      wave_lds_fence();
      pend = __ballot(rem > 0);
    }
    op += tot_len;
    head += k_tags;
    STAMP(6);
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
