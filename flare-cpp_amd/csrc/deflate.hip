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
//             d_out_len, d_status; then a wave per unit copies its bytes.
//             With FSG_DEFLATE_FLAG_UNIT_INDEX (fsg_deflate_batch_flags,
//             include/flare_deflate_index_gpu.h) a gzip body's head is
//             gzip_index.h's, 22 + 2 * units bytes: its length follows from
//             the unit count, its size entries are the units' lengths
// No wave waits on another wave.
//
// The unit kernel is deflate_unit.h's, a template over the level
// (fsg_deflate_batch_level, include/flare_deflate_level_gpu.h): level 1 is
// launched here, levels 0 and 2 by deflate_level.hip; every other launch is
// the same at all levels.
#include "deflate_unit.h"
#include "gzip_index.h"

namespace fsg {

namespace {

constexpr u32 kMaxWaves = 1024;  // token regions the workspace holds at most

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

// ---- assemble.  A wave per body (grid stride): where each unit's bytes go,
// the wrapper, the result columns.
__global__ __launch_bounds__(64) void deflate_place_kernel(const u32* __restrict__ in_len, u32 n_msgs, u32 format,
                                                           u32 flags, Cols c, u32* units, u8* out,
                                                           const u64* __restrict__ out_off, u32* __restrict__ out_len,
                                                           i32* __restrict__ status) {
  const u32 lane = threadIdx.x;
  const u32 tail = defl::wrapper_tail(format);
  for (u32 m = blockIdx.x; m < n_msgs; m += gridDim.x) {
    const u32 cnt = rfl(c.ucount[m]), ub = rfl(c.ubase[m]);
    const bool index = gzidx::writes_index(format, flags, cnt);
    const u32 head = index ? gzidx::head_bytes(cnt) : defl::wrapper_head(format);
    u8* const d = out + out_off[m];
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
    if (index && !broken)  // the size entries, behind the head's first 22 bytes
      for (u32 k = lane; k < cnt; k += 64) gzidx::wr16(d + 22 + 2 * k, units[(size_t)(ub + k) * kUnitWords + kUOutLen]);
    if (lane == 0) {
      if (broken) {
        out_len[m] = 0;
        status[m] = kCorrupt;
      } else {
        u8 w[22];
        if (index)
          gzidx::write_head(cnt, defl::kUnit, w);
        else
          defl::write_wrapper_head(format, w);
        for (u32 k = 0; k < (index ? 22u : head); ++k) d[k] = w[k];
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
                                                          u32 flags, const u32* __restrict__ ucount,
                                                          const u8* __restrict__ stage_base, u8* out,
                                                          const u64* __restrict__ out_off) {
  const u32 lane = threadIdx.x;
  const u32 total = rfl(hdr[kHdrUnits]);
  for (u32 ui = blockIdx.x; ui < total; ui += gridDim.x) {
    const u32* e = units + (size_t)ui * kUnitWords;
    if (rfl(e[kUType]) == kBroken) continue;
    const u32 len = rfl(e[kUOutLen]), cnt = rfl(ucount[rfl(e[kUBody])]);
    const u32 head = gzidx::writes_index(format, flags, cnt) ? gzidx::head_bytes(cnt) : defl::wrapper_head(format);
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
                          u32* out_len, i32* status, u32 format, u32 level, u32 flags, void* ws_, size_t ws_bytes,
                          hipStream_t stream) {
  if (level > defl::kMaxLevel) return hipErrorInvalidValue;
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
  if (level == defl::kLevelFast) {
    deflate_unit_kernel<defl::kLevelFast><<<p.waves, 64, 0, stream>>>(in, in_off, hdr, units, tokens, stage);
    e = hipGetLastError();
  } else {
    e = launch_deflate_units_level(level, p.waves, in, in_off, hdr, units, tokens, stage, stream);
  }
  if (e != hipSuccess) return e;
  if (format != defl::kRaw) {
    e = launch_inflate_sum(in, in_off, in_len, n_msgs, c.sum, format == defl::kZlib, stream);
    if (e != hipSuccess) return e;
  }
  deflate_place_kernel<<<body_grid, 64, 0, stream>>>(in_len, n_msgs, format, flags, c, units, out, out_off, out_len,
                                                     status);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  deflate_copy_kernel<<<p.cap_units < 65536 ? p.cap_units : 65536, 64, 0, stream>>>(hdr, units, format, flags,
                                                                                  c.ucount, stage, out, out_off);
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
