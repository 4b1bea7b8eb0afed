// deflate.hip -- batched deflate compress (raw deflate, zlib, gzip bodies) for
// gfx950: fsg_deflate_batch (include/flare_deflate_compress_gpu.h).  The bytes
// are those of the host model (host/deflate_cpu.cc); deflate_format.h holds
// every rule, and this file is the wave-parallel order of the same steps.
// DESIGN.md section 4, "Deflate compress".
//
// Launches, all on the caller's stream:
//   plan      one wave: units and staging granules per body, prefix sums, the
//             bodies the workspace holds; then a wave per body lists its units
//   unit      persistent grid, a wave per workgroup, units from one counter.
//             Phase 1, the window parse: 64 positions a step, one per lane
//             (hash, candidate from the LDS position table, common prefix
//             through the unit's buffer descriptor), the greedy chain walked
//             over the 64 successors, tokens to the wave's token region,
//             symbol counts to LDS.  Phase 2, the codes: build_lengths and its
//             kin from deflate_format.h, the sorts and assignments strided by
//             lane, the merge wave-uniform; the three sizes and the choice.
//             Phase 3, emit: 64 tokens a step, each lane forms its bits, a DPP
//             prefix sum places them, lanes OR them into the LDS bit window,
//             whole 16-byte blocks go to the unit's staging slot.  A stored
//             unit is a cooperative copy.
//   checksum  inflate_sum.h's kernel over the input bodies (zlib, gzip only)
//   assemble  a wave per body: the units' places, wrapper head and trailer,
//             d_out_len, d_status; then a wave per unit copies its bytes
// No wave waits on another wave.
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

constexpr u32 kMaxWaves = 1024;               // token regions the workspace holds at most
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

struct Plan {
  u32 cap_units, waves;
  u64 cap_granules;
  size_t off_cols, off_units, off_tokens, off_stage, bytes;
};

// The workspace for n_msgs bodies and `extra` units beyond one per body.
Plan plan_for(u32 n_msgs, u64 extra) {
  Plan p;
  const u64 units = (u64)n_msgs + extra;
  p.cap_units = units > 0xffffffffull ? 0xffffffffu : (u32)units;
  p.waves = units < kMaxWaves ? (u32)units : kMaxWaves;
  p.cap_granules = (extra + 1) * (defl::kUnit / 16) + 3 * units;
  auto up = [](size_t v) { return (v + 15) & ~(size_t)15; };
  p.off_cols = 256;
  p.off_units = up(p.off_cols + (size_t)n_msgs * 24);
  p.off_tokens = up(p.off_units + (size_t)units * kUnitWords * 4);
  p.off_stage = p.off_tokens + (size_t)p.waves * kTokCap * 4;
  p.bytes = p.off_stage + (size_t)p.cap_granules * 16;
  return p;
}

__device__ __forceinline__ u32 rfl(u32 v) { return (u32)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ u64 rfl64(u64 v) { return (u64)rfl((u32)(v >> 32)) << 32 | rfl((u32)v); }
__device__ __forceinline__ u64 readlane64(u64 v, u32 l) {
  return (u64)readlane((u32)(v >> 32), l) << 32 | readlane((u32)v, l);
}
__device__ __forceinline__ u64 wave_incl_scan64(u64 v, u32 lane) {
#pragma unroll
  for (u32 d = 1; d < 64; d <<= 1) {
    const u32 lo = __shfl_up((u32)v, d, 64), hi = __shfl_up((u32)(v >> 32), d, 64);
    if (lane >= d) v += (u64)hi << 32 | lo;
  }
  return v;
}
__device__ __forceinline__ u32 granules(u32 len) { return (len + 5 + 15) / 16 + 1; }

// ---- plan.  Per body: [stage granule u64][unit base u32][unit count u32][checksum u32][pad]
struct Cols {
  u64* stage;
  u32 *ubase, *ucount, *sum;
};
__host__ __device__ inline Cols cols_at(u8* ws, size_t off, u32 n_msgs) {
  Cols c;
  c.stage = reinterpret_cast<u64*>(ws + off);
  c.ubase = reinterpret_cast<u32*>(ws + off + (size_t)n_msgs * 8);
  c.ucount = c.ubase + n_msgs;
  c.sum = c.ucount + n_msgs;
  return c;
}

// One wave.  A body takes part when its slot length fits 32 bits; the bodies
// the workspace holds are a prefix of those (both sums only grow), the others
// get no unit and are answered FSG_CORRUPT by the assemble kernel.
__global__ __launch_bounds__(64) void deflate_plan_kernel(const u32* __restrict__ in_len, u32 n_msgs, u32 format,
                                                          u32* hdr, Cols c, u32 cap_units, u64 cap_granules) {
  const u32 lane = threadIdx.x;
  hdr[lane] = 0;
  u64 run_u = 0, run_g = 0;
  u32 total = 0, overflow = 0;
  for (u32 base = 0; base < n_msgs; base += 64) {
    const u32 m = base + lane;
    const bool have = m < n_msgs;
    const u32 n = have ? in_len[m] : 0u;
    const bool sized = have && defl::max_length(n, format) <= 0xffffffffull;
    const u32 u = sized ? (u32)defl::unit_count(n) : 0u;
    const u64 g = sized ? (u64)(u - 1) * kGranulesFull + granules(n - (u - 1) * defl::kUnit) : 0ull;
    const u64 iu = run_u + wave_incl_scan64(u, lane), ig = run_g + wave_incl_scan64(g, lane);
    const bool fits = sized && iu <= cap_units && ig <= cap_granules;
    if (have) {
      c.stage[m] = ig - g;
      c.ubase[m] = (u32)(iu - u);
      c.ucount[m] = fits ? u : 0u;
    }
    const u64 b = __ballot(fits);
    if (b) total = (u32)readlane64(iu, 63u - (u32)__builtin_clzll(b));
    overflow += (u32)__builtin_popcountll(__ballot(have && !fits));
    run_u = readlane64(iu, 63);
    run_g = readlane64(ig, 63);
  }
  if (lane == 0) {
    hdr[kHdrUnits] = total;
    hdr[kHdrOverflow] = overflow;
  }
}

// A wave per body (grid stride): its units' entries.
__global__ __launch_bounds__(64) void deflate_list_kernel(const u32* __restrict__ in_len, u32 n_msgs, Cols c,
                                                          u32* __restrict__ units) {
  const u32 lane = threadIdx.x;
  for (u32 m = blockIdx.x; m < n_msgs; m += gridDim.x) {
    const u32 cnt = c.ucount[m], n = in_len[m], ub = c.ubase[m];
    const u64 sg = c.stage[m];
    for (u32 k = lane; k < cnt; k += 64) {
      u32* e = units + (size_t)(ub + k) * kUnitWords;
      const u64 g = sg + (u64)k * kGranulesFull;
      e[kUBody] = m;
      e[kUFirst] = k * defl::kUnit;
      e[kULen] = k + 1 == cnt ? n - k * defl::kUnit : defl::kUnit;
      e[kULast] = k + 1 == cnt ? 1u : 0u;
      e[kUStageLo] = (u32)g;
      e[kUStageHi] = (u32)(g >> 32);
    }
  }
}

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

__global__ __launch_bounds__(64) void deflate_unit_kernel(const u8* __restrict__ in, const u64* __restrict__ in_off,
                                                          u32* hdr, u32* units, u32* tokens, u8* stage_base) {
  __shared__ u16 s_table[defl::kTableEntries];
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

    // ---- phase 1: the window parse
    {
      u32* t32 = reinterpret_cast<u32*>(s_table);
      for (u32 k = lane; k < defl::kTableEntries / 2; k += 64) t32[k] = defl::kNoPos | defl::kNoPos << 16;
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
      const u32 rec = active ? defl::token_at(rd, n, p, s_table) : defl::kTokLit;
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
      if (active && n - p >= defl::kMinMatch) s_table[defl::hash4(rd.load32(p))] = (u16)p;
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

// ---- assemble.  A wave per body (grid stride): where each unit's bytes go,
// the wrapper, the result columns.
__global__ __launch_bounds__(64) void deflate_place_kernel(const u32* __restrict__ in_len, u32 n_msgs, u32 format,
                                                           Cols c, u32* units, u8* out,
                                                           const u64* __restrict__ out_off, u32* __restrict__ out_len,
                                                           i32* __restrict__ status) {
  const u32 lane = threadIdx.x;
  const u32 head = defl::wrapper_head(format), tail = defl::wrapper_tail(format);
  for (u32 m = blockIdx.x; m < n_msgs; m += gridDim.x) {
    const u32 cnt = rfl(c.ucount[m]), ub = rfl(c.ubase[m]);
    u64 run = 0;
    bool broken = cnt == 0;
    for (u32 k0 = 0; k0 < cnt; k0 += 64) {
      const u32 k = k0 + lane;
      u32* e = units + (size_t)(ub + (k < cnt ? k : 0)) * kUnitWords;
      const u32 len = k < cnt ? e[kUOutLen] : 0u;
      broken = broken || __ballot(k < cnt && e[kUType] == kBroken) != 0;
      const u32 incl = dpp_incl_scan(len);
      if (k < cnt) {
        const u64 pos = run + incl - len;
        e[kUPosLo] = (u32)pos;
        e[kUPosHi] = (u32)(pos >> 32);
      }
      run += readlane(incl, 63);
    }
    if (lane == 0) {
      if (broken) {
        out_len[m] = 0;
        status[m] = kCorrupt;
      } else {
        u8* d = out + out_off[m];
        u8 w[10];
        defl::write_wrapper_head(format, w);
        for (u32 k = 0; k < head; ++k) d[k] = w[k];
        defl::write_wrapper_tail(format, c.sum[m], in_len[m], w);
        for (u32 k = 0; k < tail; ++k) d[head + run + k] = w[k];
        out_len[m] = (u32)(head + run + tail);
        status[m] = kOk;
      }
    }
  }
}

// A wave per unit (grid stride): the staged bytes to their place in the slot.
__global__ __launch_bounds__(64) void deflate_copy_kernel(const u32* hdr, const u32* __restrict__ units, u32 format,
                                                          const u8* __restrict__ stage_base, u8* out,
                                                          const u64* __restrict__ out_off) {
  const u32 lane = threadIdx.x;
  const u32 total = rfl(hdr[kHdrUnits]), head = defl::wrapper_head(format);
  for (u32 ui = blockIdx.x; ui < total; ui += gridDim.x) {
    const u32* e = units + (size_t)ui * kUnitWords;
    if (rfl(e[kUType]) == kBroken) continue;
    const u32 len = rfl(e[kUOutLen]);
    const u8* s = stage_base + ((u64)rfl(e[kUStageHi]) << 32 | rfl(e[kUStageLo])) * 16;
    u8* d = out + rfl64(out_off[rfl(e[kUBody])]) + head + ((u64)rfl(e[kUPosHi]) << 32 | rfl(e[kUPosLo]));
    for (u32 k = lane; k < (len >> 4); k += 64) copy16(d + 16 * k, s + 16 * k);
    for (u32 k = (len & ~15u) + lane; k < len; k += 64) d[k] = s[k];
  }
}

}  // namespace

size_t deflate_workspace_bytes(u32 n_msgs, u64 total_in_bytes) {
  return plan_for(n_msgs, total_in_bytes / defl::kUnit).bytes;
}

// The units a workspace of ws_bytes holds for n_msgs bodies: n_msgs plus the
// largest `extra` whose plan fits; 0 when not even plan_for(n_msgs, 0) does.
static bool deflate_plan(u32 n_msgs, size_t ws_bytes, Plan* out) {
  if (plan_for(n_msgs, 0).bytes > ws_bytes) return false;
  u64 lo = 0, hi = 1ull << 36;  // plan_for is increasing in extra
  while (lo < hi) {
    const u64 mid = lo + (hi - lo + 1) / 2;
    if (plan_for(n_msgs, mid).bytes <= ws_bytes)
      lo = mid;
    else
      hi = mid - 1;
  }
  *out = plan_for(n_msgs, lo);
  return true;
}

u64 deflate_unit_capacity(u32 n_msgs, size_t ws_bytes) {
  Plan p;
  return deflate_plan(n_msgs, ws_bytes, &p) ? p.cap_units : 0;
}

hipError_t launch_deflate(const u8* in, const u64* in_off, const u32* in_len, u32 n_msgs, u8* out, const u64* out_off,
                          u32* out_len, i32* status, u32 format, void* ws_, size_t ws_bytes, hipStream_t stream) {
  if (n_msgs == 0) return hipSuccess;
  Plan p;
  if (!deflate_plan(n_msgs, ws_bytes, &p)) return hipErrorInvalidValue;
  u8* ws = static_cast<u8*>(ws_);
  u32* hdr = reinterpret_cast<u32*>(ws);
  const Cols c = cols_at(ws, p.off_cols, n_msgs);
  u32* units = reinterpret_cast<u32*>(ws + p.off_units);
  u32* tokens = reinterpret_cast<u32*>(ws + p.off_tokens);
  u8* stage = ws + p.off_stage;
  const u32 body_grid = n_msgs < 65536 ? n_msgs : 65536;
  hipError_t e;
  deflate_plan_kernel<<<1, 64, 0, stream>>>(in_len, n_msgs, format, hdr, c, p.cap_units, p.cap_granules);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  deflate_list_kernel<<<body_grid, 64, 0, stream>>>(in_len, n_msgs, c, units);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  deflate_unit_kernel<<<p.waves, 64, 0, stream>>>(in, in_off, hdr, units, tokens, stage);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if (format != defl::kRaw) {
    e = launch_inflate_sum(in, in_off, in_len, n_msgs, c.sum, format == defl::kZlib, stream);
    if (e != hipSuccess) return e;
  }
  deflate_place_kernel<<<body_grid, 64, 0, stream>>>(in_len, n_msgs, format, c, units, out, out_off, out_len, status);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  deflate_copy_kernel<<<p.cap_units < 65536 ? p.cap_units : 65536, 64, 0, stream>>>(hdr, units, format, stage, out,
                                                                                  out_off);
  return hipGetLastError();
}

void deflate_header_counts(const void* header, DeflateHeaderCounts* c) {
  const u32* h = static_cast<const u32*>(header);
  c->units = h[kHdrUnits];
  c->stored = h[kHdrStored];
  c->fixed = h[kHdrFixed];
  c->dynamic = h[kHdrDynamic];
  c->overflow = h[kHdrOverflow];
}

}  // namespace fsg
