// inflate_walk.h -- the deflate block loop of one wave, shared by the decode
// kernels: inflate.hip (a wave per body) and inflate_units.hip (a wave per
// unit of an indexed gzip body).  The two phases, the ordering of the slot
// reads and the count-only mode are described at the top of inflate.hip; they
// hold per walk, so per unit where a body is walked by units.
#pragma once

#include "inflate_format.h"
#include "launch.h"
#include "wave_util.h"

namespace fsg {
namespace {

using infl::e_bits;
using infl::e_op;
using infl::e_val;

// LDS decode tables: the dynamic block's, then the fixed code's
constexpr u32 kTabLit = 0, kTabDist = infl::kEnoughLens, kTabFixLit = kTabDist + infl::kEnoughDists,
              kTabFixDist = kTabFixLit + 512, kTabEntries = kTabFixDist + 32;
// Bodies above this are FSG_CORRUPT: byte positions are 32 bits wide and run
// up to one group's bits past the input's end.
constexpr u32 kMaxBody = 0xFFFF0000u;

__device__ __forceinline__ u32 uniform(u32 v) { return (u32)__builtin_amdgcn_readfirstlane((int)v); }

// Wave-uniform 64-bit bit buffer over a body.  Input words come through the
// body's buffer descriptor (wave_util.h msg_rsrc: dwords past the body read 0
// and touch no memory) and the bytes at and past n are masked to 0.
struct WaveReader {
  __amdgpu_buffer_rsrc_t rs;
  u32 base;  // the body's first byte in the descriptor
  u32 n;
  u32 pos;   // next byte to load
  u64 hold;
  u32 nbits;
  __device__ __forceinline__ void need() {
    if (nbits < 32) {
      const u32 P = base + pos, s = P & 3u;
      const u32x2 d = __builtin_amdgcn_raw_buffer_load_b64(rs, P & ~3u, 0, 0);
      u32 w = __builtin_amdgcn_alignbyte(d[1], d[0], s);
      const u32 keep = pos < n ? n - pos : 0u;
      if (keep < 4) w &= (1u << (8 * keep)) - 1u;
      hold |= (u64)uniform(w) << nbits;
      nbits += 32;
      pos += 4;
    }
  }
  __device__ __forceinline__ void restart(u32 at) {
    pos = at;
    hold = 0;
    nbits = 0;
  }
  __device__ __forceinline__ u32 peek(u32 k) const { return (u32)hold & ((1u << k) - 1u); }
  __device__ __forceinline__ void drop(u32 k) {
    hold >>= k;
    nbits -= k;
  }
  __device__ __forceinline__ u32 bits(u32 k) {
    const u32 v = peek(k);
    drop(k);
    return v;
  }
  __device__ __forceinline__ u64 consumed() const { return 8ull * pos - nbits; }
};

__device__ __forceinline__ u32 lookup(WaveReader& r, const u32* tab, u32 root) {
  u32 e = uniform(tab[r.peek(root)]);
  if (e_op(e) & infl::kOpLink) {
    r.drop(e_bits(e));
    e = uniform(tab[e_val(e) + r.peek(e_op(e) & 15u)]);
  }
  r.drop(e_bits(e));
  return e;
}

constexpr u32 kRecLiteral = 0x80000000u;  // | the byte; a copy: length | distance << 9

// The execute phase of one group: cnt records (lane k: rec, len; the other
// lanes 0, 0) whose first output byte is slot position g < cap.
__device__ __forceinline__ void execute_group(u32 lane, u32 rec, u32 len, u32 g, u32 cap,
                                              __amdgpu_buffer_rsrc_t slot, u32* s_start, u32* s_rec) {
  const u32 incl = dpp_incl_scan(len);
  const u32 total = readlane(incl, 63);
  s_start[lane] = incl - len;  // lanes past the last record: total, above every position
  s_rec[lane] = rec;
  wave_lds_fence();
  wait_all_memory();  // the earlier groups' stores, before this group's loads
  for (u32 j = lane; j < total; j += 64) {
    const u32 at = g + j;
    if (at >= cap || at < g) break;  // count-only from the capacity on
    u32 p = j, val;
    for (;;) {  // every round moves to an earlier record: 64 rounds at most
      u32 r = 0;
#pragma unroll
      for (u32 step = 32; step; step >>= 1)
        if (s_start[r + step] <= p) r += step;
      const u32 rc = s_rec[r], first = s_start[r];
      if (rc & kRecLiteral) {
        val = rc & 0xffu;
        break;
      }
      const u32 dist = (rc >> 9) & 0xffffu, i = p - first;
      const u32 back = dist - (i < dist ? i : i % dist);  // 1 .. dist bytes below the record
      if (back > first) {  // below the group: g + first >= dist was checked when the record was decoded
        val = __builtin_amdgcn_raw_buffer_load_b8(slot, g + first - back, 0, 16);
        break;
      }
      p = first - back;
    }
    __builtin_amdgcn_raw_buffer_store_b8((u8)val, slot, at, 0, 0);
  }
  wave_lds_fence();
}

// The block loop of the body p[0 .. n) from byte `at`; false: corrupt.  The
// walk's first output byte is dst[0] (distances count from there), cap the
// room at dst, outpos the bytes declared so far.  The decode tables and the
// execute phase's records are LDS arrays of this function: one walk at a time
// per workgroup, which is one wave.
//   Whole stream, or the last unit of an indexed body (nonlast false): blocks
//   until BFINAL, whose last bit must lie in byte n_end - 1.
//   kUnits and nonlast: a unit in front of the last (gzip_index.h).  It ends
//   clean after the block whose last bit is bit 8 * n_end - 1, with exactly
//   chlen bytes declared and no BFINAL met; a block that passes n_end, BFINAL,
//   more than chlen bytes, fewer at the stop, a distance below dst[0] and
//   every corrupt block are `false`.
template <bool kStore, bool kUnits>
__device__ __forceinline__ bool inflate_walk(u32 lane, const u8* p, u32 n, u32 at, u32 n_end, bool nonlast, u32 chlen,
                                             u8* dst, u32 cap, u64& outpos) {
  __shared__ u32 s_tab[kTabEntries];
  __shared__ u8 s_lens[infl::kLensArray];
  __shared__ u16 s_work[infl::kLensArray];
  __shared__ infl::TableScratch s_scr;
  __shared__ u32 s_start[64], s_rec[64];
  const u32 bal = (u32)(reinterpret_cast<uintptr_t>(p) & 15u);
  WaveReader r;
  r.rs = msg_rsrc(p - bal, bal + n);
  r.base = bal;
  r.n = n;
  r.restart(at);
  const __amdgpu_buffer_rsrc_t slot =
      __builtin_amdgcn_make_buffer_rsrc(dst, (short)0, (int)cap, 0x00020000);
  bool have_fixed = false;
  u32 last;
  // A unit in front of the last, after each block: 0 go on, 1 clean, 2 not clean.
  auto unit_end = [&](u32 last) -> u32 {
    if (last || outpos > chlen) return 2u;
    if (r.consumed() == 8ull * n_end) return outpos == chlen ? 1u : 2u;
    return 0u;
  };
  // Termination: every block takes at least 3 bits, every symbol at least
  // one, every stored block lies inside the input, and the bit position is
  // compared with the stream's end after every group of at most 64 symbols
  // (48 bits each at most), so it stays below 8 * (n + 400) and each loop
  // below ends; a body's time is bounded by its length and the bytes it
  // declares (258 per symbol at most).
  do {
    r.need();
    last = r.bits(1);
    const u32 type = r.bits(2);
    if (type == 3) return false;
    if (type == 0) {  // stored: cooperative 16-byte copies
      r.drop(r.nbits & 7u);
      r.need();
      const u32 len = r.bits(16), nlen = r.bits(16);
      if ((len ^ 0xffffu) != nlen) return false;
      const u64 start = r.consumed() >> 3;
      if (start + len > n_end) return false;
      if (kStore && outpos < cap) {
        const u32 room = cap - (u32)outpos, ne = len < room ? len : room;
        const u8* s = p + start;
        u8* d = dst + outpos;
        for (u32 c = lane; c < (ne >> 4); c += 64) copy16(d + 16 * c, s + 16 * c);
        for (u32 t = (ne & ~15u) + lane; t < ne; t += 64) d[t] = s[t];
      }
      outpos += len;
      r.restart((u32)start + len);
      if constexpr (kUnits) {
        if (nonlast) {
          const u32 v = unit_end(last);
          if (v) return v == 1;
        }
      }
      continue;
    }
    u32 lit, dist, lroot = infl::kLenRoot, droot = infl::kDistRoot;
    if (type == 1) {  // fixed: built on first use, kept for the body
      lit = kTabFixLit;
      dist = kTabFixDist;
      if (!have_fixed) {
        for (u32 k = lane; k < infl::kFixedLens + infl::kFixedDists; k += 64) s_lens[k] = (u8)infl::fixed_length(k);
        wave_lds_fence();
        infl::build_table(infl::kLens, s_lens, infl::kFixedLens, s_tab + lit, 512, &lroot, s_work, &s_scr, lane, 64);
        infl::build_table(infl::kDists, s_lens + infl::kFixedLens, infl::kFixedDists, s_tab + dist, 32, &droot,
                          s_work, &s_scr, lane, 64);
        have_fixed = true;
      }
      lroot = 9;
      droot = 5;
    } else {
      lit = kTabLit;
      dist = kTabDist;
      u32 nl, nd;
      if (!infl::read_dynamic_header(r, s_lens, &nl, &nd, s_tab + dist, s_work, &s_scr, lane, 64)) return false;
      if (infl::build_table(infl::kLens, s_lens, nl, s_tab + lit, infl::kEnoughLens, &lroot, s_work, &s_scr, lane,
                            64) != infl::kTableOk)
        return false;
      if (infl::build_table(infl::kDists, s_lens + nl, nd, s_tab + dist, infl::kEnoughDists, &droot, s_work, &s_scr,
                            lane, 64) != infl::kTableOk)
        return false;
    }
    lroot = uniform(lroot);
    droot = uniform(droot);
    bool eob = false;
    while (!eob) {
      // ---- symbol phase
      const u64 gstart = outpos;
      u32 cnt = 0, rec = 0, len = 0;
      while (cnt < 64) {
        r.need();
        u32 e = lookup(r, s_tab + lit, lroot);
        u32 op = e_op(e), rc, ln;
        if (op == infl::kOpLit) {
          rc = kRecLiteral | e_val(e);
          ln = 1;
        } else {
          if (op == infl::kOpEnd) {
            eob = true;
            break;
          }
          if (!(op & infl::kOpBase)) return false;  // a symbol with no code
          ln = e_val(e) + r.bits(op & 15u);
          r.need();
          e = lookup(r, s_tab + dist, droot);
          op = e_op(e);
          if (!(op & infl::kOpBase)) return false;
          const u32 distance = e_val(e) + r.bits(op & 15u);
          if (distance > outpos) return false;  // before the body's first byte
          rc = ln | distance << 9;
        }
        if (lane == cnt) {
          rec = rc;
          len = ln;
        }
        outpos += ln;
        ++cnt;
      }
      if (r.consumed() > 8ull * n_end) return false;
      if constexpr (kUnits) {
        if (nonlast && outpos > chlen) return false;  // the stores stay inside cap either way
      }
      // ---- execute phase
      if (kStore && cnt && gstart < cap) execute_group(lane, rec, len, (u32)gstart, cap, slot, s_start, s_rec);
    }
    if constexpr (kUnits) {
      if (nonlast) {
        const u32 v = unit_end(last);
        if (v) return v == 1;
      }
    }
  } while (!last);
  const u64 used = r.consumed();
  return used <= 8ull * n_end && (used + 7) / 8 == n_end;  // not cut short, no bytes after the stream
}

}  // namespace
}  // namespace fsg
