// deflate_unit.h -- the unit kernel of the batched deflate compress
// (deflate.hip has the launches and says what the phases do), a template over
// the level (deflate_format.h, "levels").  Level 1 is instantiated in
// deflate.hip and levels 0 and 2 in deflate_level.hip: in a translation unit
// of its own the level-1 kernel compiles to the code it had before there
// were levels (with a caller per level in one file the compiler stops
// inlining build_dynamic_header, which costs that kernel a scratch slot).
#pragma once

#include <type_traits>

#include "deflate_format.h"
#include "launch.h"
#include "wave_util.h"

// Diagnostic builds (make deflate_phases, tools/deflate_bench.py): the unit
// kernel stops after phase 1 or 2 and every unit reports an empty output, so
// the call's time is that of the phases left in.  Never the product library.
#ifndef FSG_DEFLATE_PHASES
#define FSG_DEFLATE_PHASES 3
#endif

namespace fsg {

namespace {

constexpr u32 kTokCap = defl::kUnit + 64;     // tokens of a unit: a literal per byte and the end token
constexpr u32 kUnitWords = 10;                // a unit's entry
constexpr u32 kGranulesFull = (defl::kUnit + 5 + 15) / 16 + 1;
constexpr u32 kBroken = 3;                    // a unit whose writer and size formula disagreed (never seen)
// a unit's entry
enum : u32 { kUBody, kUFirst, kULen, kULast, kUStageLo, kUStageHi, kUOutLen, kUType, kUPosLo, kUPosHi };
// header words (the first 256 bytes of the workspace)
enum : u32 { kHdrUnits = 1, kHdrNext = 2, kHdrStored = 3, kHdrFixed = 4, kHdrDynamic = 5, kHdrOverflow = 6 };
// bit window: the longest block header, or a carry of up to 127 bits, 64 tokens and the tail
constexpr u32 kWinBits = 5120, kWinWords = kWinBits / 32 + 4;
static_assert(defl::kMaxHeaderBits + 64 <= kWinBits && 128 + 64 * 48 + 48 <= kWinBits, "window");

__device__ __forceinline__ u32 rfl(u32 v) { return (u32)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ u64 rfl64(u64 v) { return (u64)rfl((u32)(v >> 32)) << 32 | rfl((u32)v); }
// Lane + 1's value (lane 63: 0): a DPP row shift inside each row of 16, the
// rows' first lanes read for the last lane of the row before.
__device__ __forceinline__ u32 next_lane(u32 v, u32 lane) {
  u32 r = (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x101, 0xf, 0xf, true);  // row_shl:1
  const u32 a = readlane(v, 16), b = readlane(v, 32), c = readlane(v, 48);
  r = lane == 15 ? a : r;
  r = lane == 31 ? b : r;
  r = lane == 47 ? c : r;
  return r;
}
__device__ __forceinline__ u32 granules(u32 len) { return (len + 5 + 15) / 16 + 1; }

// ---- the unit kernel
struct DeviceReader {
  __amdgpu_buffer_rsrc_t rs;
  u32 bal;
  // bytes q .. q+3 of the unit; dwords past the unit's last read 0
  __device__ __forceinline__ u32 load32(u32 q) const {
    const u32 P = bal + q;
    const u32x2 d = __builtin_amdgcn_raw_buffer_load_b64(rs, P & ~3u, 0, 0);
    return __builtin_amdgcn_alignbyte(d[1], d[0], P & 3u);
  }
};

struct Emit {
  u32* win;
  u8* stage;
  u32 cap;     // 16-byte blocks the staging slot holds
  u32 blocks;  // 16-byte blocks stored so far
  u32 bits;    // bits in the window
  // Stores the window's whole 16-byte blocks (all of it when `all`) and
  // moves the rest to its front.
  __device__ __forceinline__ void flush(u32 lane, bool all) {
    wave_lds_fence();
    const u32 nb = all ? (bits + 127) >> 7 : bits >> 7;
    for (u32 k = lane; k < nb && blocks + k < cap; k += 64) {
      const u32x4 v{win[4 * k], win[4 * k + 1], win[4 * k + 2], win[4 * k + 3]};
      __builtin_memcpy(stage + (size_t)(blocks + k) * 16, &v, 16);
    }
    const u32 carry = lane < 4 ? win[4 * nb + lane] : 0u;
    wave_lds_fence();
    for (u32 w = lane; w < 4 * nb + 4; w += 64) win[w] = 0;
    wave_lds_fence();
    if (lane < 4 && !all) win[lane] = carry;
    wave_lds_fence();
    blocks += nb;
    bits = all ? 0u : bits & 127u;
  }
};

// One instantiation per level (deflate_format.h, "levels").  Level 1's
// position table is u16 (16 KiB), level 2's u32 (32 KiB, two candidates a
// word), level 0 has none.
template <u32 kLevel>
__global__ __launch_bounds__(64) void deflate_unit_kernel(const u8* __restrict__ in, const u64* __restrict__ in_off,
                                                          u32* hdr, u32* units, u32* tokens, u8* stage_base) {
  using TableWord = std::conditional_t<kLevel == defl::kLevelBest, u32, u16>;
  __shared__ TableWord s_table[kLevel == defl::kLevelStored ? 1 : defl::kTableEntries];
  __shared__ defl::Build s_b;
  __shared__ u32 s_win[kWinWords];
  __shared__ u32 s_pass;
  const u32 lane = threadIdx.x;
  u32* const tok = tokens + (size_t)blockIdx.x * kTokCap;
  const __amdgpu_buffer_rsrc_t tok_rs = __builtin_amdgcn_make_buffer_rsrc(tok, (short)0, (int)(kTokCap * 4), 0x00020000);
  const u32 total = rfl(hdr[kHdrUnits]);
  for (;;) {
    // every lane takes part in the fetch (lz4_encode_wave.hip says why)
    const u32 ui = rfl(atomicAdd(&hdr[kHdrNext], lane == 0 ? 1u : 0u));
    if (ui >= total) break;
    u32* const e = units + (size_t)ui * kUnitWords;
    const u32 body = rfl(e[kUBody]), first = rfl(e[kUFirst]), n = rfl(e[kULen]);
    const bool last = rfl(e[kULast]) != 0;
    u8* const stage = stage_base + ((u64)rfl(e[kUStageHi]) << 32 | rfl(e[kUStageLo])) * 16;
    const u8* const src = in + rfl64(in_off[body]) + first;

    if constexpr (kLevel == defl::kLevelStored) {
      // ---- level 0: no parse, no code build; the stored branch of phase 3
      // (written out here as well: with the copy in a helper that both
      // places call, the level-1 kernel is no longer the code it was)
      if (FSG_DEFLATE_PHASES < 3) {
        if (lane == 0) {
          e[kUOutLen] = 0;
          e[kUType] = defl::kStored;
        }
        continue;
      }
      if (lane == 0) {
        u8 h[5];
        defl::write_stored_head(n, last, h);
        for (u32 k = 0; k < 5; ++k) stage[k] = h[k];
      }
      for (u32 k = lane; k < n; k += 64) stage[5 + k] = src[k];
      if (lane == 0) {
        e[kUOutLen] = n + 5;
        e[kUType] = defl::kStored;
        atomicAdd(&hdr[kHdrStored], 1u);
      }
      continue;
    }
    // ---- phase 1: the window parse
    {
      u32* t32 = reinterpret_cast<u32*>(s_table);
      for (u32 k = lane; k < sizeof(s_table) / 4; k += 64) t32[k] = defl::kEmptyPair;
      u32* b32 = reinterpret_cast<u32*>(&s_b);
      for (u32 k = lane; k < sizeof(defl::Build) / 4; k += 64) b32[k] = 0;
    }
    wave_lds_fence();
    DeviceReader rd;
    rd.bal = (u32)(reinterpret_cast<uintptr_t>(src) & 15u);
    rd.rs = msg_rsrc(src - rd.bal, rd.bal + n);
    u32 ntok = 0, entry = 0;
    for (u32 base = 0; base < n; base += defl::kWindow) {
      const u32 cnt = n - base < defl::kWindow ? n - base : defl::kWindow;
      const u32 p = base + lane;
      const bool active = lane < cnt;
      u32 rec, four = 0, word = 0;
      if constexpr (kLevel == defl::kLevelBest) {
        // both candidates from one word; the lazy step reads the right-hand
        // neighbour's undeferred token (row_shl:1 inside a row of 16, the
        // row's last lane by readlane) for all lanes before the chain walk
        const u32 r = active ? defl::token_at2(rd, n, p, s_table, &four, &word) : defl::kTokLit;
        rec = defl::defer_token(r, next_lane(r, lane), lane + 1 < cnt, four);
      } else {
        rec = active ? defl::token_at(rd, n, p, s_table) : defl::kTokLit;
      }
      const u32 succ = lane + defl::tok_advance(rec);
      u64 chain = 0;
      u32 cur = entry;
      while (cur < cnt) {  // wave-uniform: at most one step per token of the window
        chain |= 1ull << cur;
        cur = readlane(succ, cur);
      }
      entry = cur - cnt;
      if ((chain >> lane) & 1) {
        const u32 at = ntok + (u32)__builtin_popcountll(chain & ((1ull << lane) - 1));
        __builtin_amdgcn_raw_buffer_store_b32(rec, tok_rs, at * 4, 0, 0);
        defl::count_token(&s_b, rec);
      }
      ntok += (u32)__builtin_popcountll(chain);
      wave_lds_fence();  // the window's candidates were read before its positions go in
      // one store: where two lanes hash alike the highest lane lands last
      // (tools/probes/lds_overlap_probe.hip), which is the highest position
      if constexpr (kLevel == defl::kLevelBest) {
        // every lane of a slot forms its word from the same `word`, read with the candidates before the fence
        if (active && n - p >= defl::kMinMatch) s_table[defl::hash4(four)] = defl::insert_word(word, p);
      } else {
        if (active && n - p >= defl::kMinMatch) s_table[defl::hash4(rd.load32(p))] = (u16)p;
      }
      wave_lds_fence();
    }
    if (lane == 0) {
      __builtin_amdgcn_raw_buffer_store_b32(defl::kTokEnd, tok_rs, ntok * 4, 0, 0);
      defl::count_token(&s_b, defl::kTokEnd);
    }
    ++ntok;
    wave_lds_fence();

    if (FSG_DEFLATE_PHASES < 2) {
      if (lane == 0) {
        e[kUOutLen] = 0;
        e[kUType] = defl::kFixed;
      }
      continue;
    }
    // ---- phase 2: code lengths, the three sizes, the choice
    defl::build_lengths(s_b.hist, defl::kLitSyms, 15, s_b.len, &s_b, lane, 64);
    defl::build_lengths(s_b.hist + defl::kDistBase, defl::kDistSyms, 15, s_b.len + defl::kDistBase, &s_b, lane, 64);
    const u32 header = rfl(defl::build_dynamic_header(&s_b, lane, 64));
    u32 dyn, fix;
    defl::symbol_bits(&s_b, lane, 64, &dyn, &fix);
    dyn = readlane(dpp_incl_scan(dyn), 63);
    fix = readlane(dpp_incl_scan(fix), 63);
    const defl::Choice c = defl::choose_block(n, last, dyn + header, fix);
    u32 type = c.type;

    if (FSG_DEFLATE_PHASES < 3) {
      if (lane == 0) {
        e[kUOutLen] = 0;
        e[kUType] = type;
      }
      continue;
    }
    // ---- phase 3: emit into the staging slot
    if (type == defl::kStored) {
      if (lane == 0) {
        u8 h[5];
        defl::write_stored_head(n, last, h);
        for (u32 k = 0; k < 5; ++k) stage[k] = h[k];
      }
      for (u32 k = lane; k < n; k += 64) stage[5 + k] = src[k];
    } else {
      if (type == defl::kFixed) {
        defl::fill_fixed_lengths(&s_b, lane, 64);
        defl::assign_codes(s_b.len, infl::kFixedLens, s_b.code, &s_b, lane, 64);
        defl::assign_codes(s_b.len + defl::kDistBase, infl::kFixedDists, s_b.code + defl::kDistBase, &s_b, lane, 64);
      } else {
        defl::assign_codes(s_b.len, defl::kLitSyms, s_b.code, &s_b, lane, 64);
        defl::assign_codes(s_b.len + defl::kDistBase, defl::kDistSyms, s_b.code + defl::kDistBase, &s_b, lane, 64);
      }
      for (u32 w = lane; w < kWinWords; w += 64) s_win[w] = 0;
      wave_lds_fence();
      Emit em{s_win, stage, granules(n), 0, 0};
      // (lane 0's result goes through LDS, not through a readfirstlane the
      // compiler could place on lane 0's side of the branch alone)
      if (lane == 0) s_pass = defl::write_block_header(&s_b, type, last, s_win);
      wave_lds_fence();
      em.bits = rfl(s_pass);
      em.flush(lane, false);
      // the tokens were stored by this wave: wait for the stores, read through L2
      wait_all_memory();
      for (u32 g = 0; g < ntok; g += 64) {
        const u32 t = g + lane;
        u32 nb = 0;
        u64 v = 0;
        if (t < ntok) v = defl::token_bits(&s_b, __builtin_amdgcn_raw_buffer_load_b32(tok_rs, t * 4, 0, 16), &nb);
        const u32 incl = dpp_incl_scan(nb);
        defl::put_bits(s_win, em.bits + incl - nb, v, nb);
        em.bits += readlane(incl, 63);
        em.flush(lane, false);
      }
      wave_lds_fence();
      if (lane == 0) s_pass = defl::write_block_tail(last, em.bits, s_win);
      wave_lds_fence();
      const u32 rel = rfl(s_pass);
      if (em.blocks * 16 + rel != c.bytes) type = kBroken;
      em.bits = rel * 8;
      em.flush(lane, true);
    }
    if (lane == 0) {
      e[kUOutLen] = c.bytes;
      e[kUType] = type;
      atomicAdd(&hdr[type == defl::kStored ? kHdrStored : type == defl::kFixed ? kHdrFixed : kHdrDynamic], 1u);
    }
  }
}

}  // namespace

// Levels 0 and 2 (deflate_level.hip); level 1 is launched by deflate.hip itself.
hipError_t launch_deflate_units_level(u32 level, u32 waves, const u8* in, const u64* in_off, u32* hdr, u32* units,
                                      u32* tokens, u8* stage, hipStream_t stream);

}  // namespace fsg
