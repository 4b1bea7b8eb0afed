// inflate_units.hip -- batched inflate with a wave per UNIT for gzip bodies
// that carry a unit index (gzip_index.h): fsg_inflate_units_batch and
// fsg_inflate_units_lengths_batch (include/flare_deflate_index_gpu.h).  The
// block loop is inflate_walk.h's, the one inflate.hip runs with a wave per
// body; the verdict rules are inflate_format.h's.  host/gzip_index_cpu.cc is
// the serial model of the routes.  DESIGN.md section 4, "Deflate: unit index".
//
// The rule: status, length and bytes of every body are what fsg_inflate_batch
// gives.  A body is decoded by units only where that provably is the serial
// walk: unit 0 starts where the stream starts, every unit in front of the last
// ends on a block boundary exactly where the next one starts, meets no BFINAL,
// gives exactly CHLEN bytes and holds no distance below its own first byte,
// and the last unit ends the stream under the serial walk's end rule.  Then
// the serial walk meets the same blocks at the same places and writes the same
// bytes.  Everything else is walked again as one whole stream.
//
// Launches, all on the caller's stream:
//   classify  a wave per body: wrapper, index, units wanted; the bodies the
//             wrapper decides get their status here
//   plan      one wave: prefix sums of the unit entries, the bodies whose
//             units the workspace holds (a prefix of the indexed ones), the
//             counts that need no decode
//   list      a wave per body: its unit entries (start byte, stop byte, slot
//             base); a body without a usable index is one whole-stream entry.
//             The units in front of the last come first in the list, body by
//             body, then one entry per body: its last unit or whole stream
//   units     a wave per entry: inflate_walk.  A whole-stream entry writes the
//             body's status and length; a unit writes them into its entry
//   resolve   a wave per indexed body: all units clean and the total within
//             the slot is FSG_OK; anything else appends a whole-stream entry
//             to the redo list
//   units     the same kernel over the redo list
//   checksum  inflate.hip's trailer judge, unchanged (decode call only)
// No wave waits on another wave.  Units of one body write disjoint ranges of
// the slot and load only bytes of their own range, so the ordering note at the
// top of inflate.hip holds per unit.
#include "gzip_index.h"
#include "inflate_format.h"
#include "inflate_walk.h"
#include "launch.h"
#include "wave_util.h"

namespace fsg {
namespace {

constexpr u32 kEntryWords = 8;
enum : u32 { kEBody, kEStart, kEStop, kEBase, kEKind, kEClean, kELenLo, kELenHi };
enum : u32 { kKindWhole = 0, kKindUnit = 1, kKindLast = 2 };
// the workspace header (64 words)
enum : u32 { kHEntries = 1, kHRedo, kHParBodies, kHParUnits, kHNoIndex, kHUnusable, kHMismatch, kHOverflow, kHFront };
enum : u32 { kClsDecided = 0, kClsNoIndex, kClsUnusable, kClsIndexed, kClsOverflow };
constexpr u32 kMaxGrid = 1u << 20;

struct Plan {
  u32 cap_entries;
  size_t off_cols, off_entries, off_redo, bytes;
};
constexpr u32 kColWords = 8;

Plan plan_for(u32 n_msgs, u64 extra) {
  Plan p;
  const u64 entries = (u64)n_msgs + extra;
  p.cap_entries = entries > 0xffffffffull ? 0xffffffffu : (u32)entries;
  auto up = [](size_t v) { return (v + 15) & ~(size_t)15; };
  p.off_cols = 256;
  p.off_entries = up(p.off_cols + (size_t)n_msgs * kColWords * 4);
  p.off_redo = p.off_entries + (size_t)p.cap_entries * kEntryWords * 4;
  p.bytes = p.off_redo + (size_t)n_msgs * kEntryWords * 4;
  return p;
}

bool plan_in(u32 n_msgs, size_t ws_bytes, Plan* out) {
  const Plan p0 = plan_for(n_msgs, 0);
  if (p0.bytes > ws_bytes) return false;
  *out = plan_for(n_msgs, (ws_bytes - p0.bytes) / (kEntryWords * 4));
  return true;
}

// Per body: units wanted, first front entry, entries, class, stream begin,
// CHLEN, first size entry's byte, rank among the tail entries
struct Cols {
  u32 *want, *ubase, *ucount, *cls, *begin, *chlen, *sizes_at, *tail;
};
Cols cols_at(u8* ws, size_t off, u32 n_msgs) {
  u32* b = reinterpret_cast<u32*>(ws + off);
  return Cols{b, b + n_msgs, b + 2 * (size_t)n_msgs, b + 3 * (size_t)n_msgs, b + 4 * (size_t)n_msgs,
              b + 5 * (size_t)n_msgs, b + 6 * (size_t)n_msgs, b + 7 * (size_t)n_msgs};
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

// ---- classify.  A wave per body (grid stride).
template <bool kStore>
__global__ __launch_bounds__(64) void inflate_units_classify_kernel(const u8* __restrict__ in,
                                                                    const u64* __restrict__ in_off,
                                                                    const u32* __restrict__ in_len, u32 n_msgs,
                                                                    u32* __restrict__ out_len,
                                                                    u64* __restrict__ lengths,
                                                                    i32* __restrict__ status, u32 format, Cols c) {
  const u32 lane = threadIdx.x;
  for (u32 m = blockIdx.x; m < n_msgs; m += gridDim.x) {
    const u8* p = in + in_off[m];
    const u32 n = uniform(in_len[m]);
    u32 cls = kClsDecided, want = 0, begin = 0, chlen = 0, sizes_at = 0;
    i32 st;
    if (n == 0 || n > kMaxBody) {
      st = n == 0 && format != infl::kRaw ? infl::kStBadHeader : infl::kStCorrupt;
    } else {
      const infl::Wrapper w = infl::parse_wrapper(format, p, n);
      st = w.status;
      if (st == infl::kStOk) {
        cls = kClsNoIndex;
        want = 1;
        begin = uniform(w.begin);
        if (format == infl::kGzip) {
          const gzidx::Head h = gzidx::find_head(p);
          const u32 state = uniform(h.state);
          if (state == gzidx::kUnusable) cls = kClsUnusable;
          if (state == gzidx::kUsable) {
            const u32 cnt = uniform(h.chcnt);
            u32 part = 0;  // at most 32,761 entries of at most 65,535
            for (u32 k = lane; k + 1 < cnt; k += 64) part += gzidx::size_at(p, h, k);
            const u32 sum = readlane(dpp_incl_scan(part), 63);
            if (gzidx::placed(begin, sum, n)) {
              cls = kClsIndexed;
              want = cnt;
              chlen = uniform(h.chlen);
              sizes_at = uniform(h.sizes_at);
            } else {
              cls = kClsUnusable;
            }
          }
        }
      }
    }
    if (lane == 0) {
      c.want[m] = want;
      c.cls[m] = cls;
      c.begin[m] = begin;
      c.chlen[m] = chlen;
      c.sizes_at[m] = sizes_at;
      if (cls == kClsDecided) {
        status[m] = st;
        if (kStore)
          out_len[m] = 0;
        else
          lengths[m] = 0;
      }
    }
  }
}

// ---- plan.  One wave.  An indexed body keeps its units while the units
// beyond one per body of all indexed bodies up to and including it fit the
// workspace's extra entries; from the first that does not, indexed bodies are
// one whole-stream entry each.
// The entry list has two parts.  Front: the units in front of a body's last,
// body by body.  Tail: one entry per body, its last unit or its whole stream.
// Front units all decode CHLEN bytes; a last unit may be a few bytes.  With a
// body's entries kept together, a batch of two-unit bodies alternates long and
// short entries, and 4,096 bodies of 64 KiB took twice the time of the
// one-wave-per-body call; with the list in two parts they take its time
// ("Deflate: unit index").  The likely cause: workgroups
// are dealt out in turn, so every other SIMD got the short entries.
__global__ __launch_bounds__(64) void inflate_units_plan_kernel(u32 n_msgs, u32* hdr, Cols c, u64 extra_cap) {
  const u32 lane = threadIdx.x;
  hdr[lane] = 0;
  u64 run_e = 0, run_f = 0;
  u32 run_t = 0, no_index = 0, unusable = 0, overflow = 0;
  for (u32 base = 0; base < n_msgs; base += 64) {
    const u32 m = base + lane;
    const bool have = m < n_msgs;
    const u32 want = have ? c.want[m] : 0u;
    u32 cls = have ? c.cls[m] : kClsDecided;
    const u64 extra = cls == kClsIndexed ? want - 1 : 0u;
    const u64 ie = run_e + wave_incl_scan64(extra, lane);
    if (cls == kClsIndexed && ie > extra_cap) cls = kClsOverflow;
    const u32 front = cls == kClsIndexed ? want - 1 : 0u, tail = have && want ? 1u : 0u;
    const u64 jf = run_f + wave_incl_scan64(front, lane);
    const u32 jt = run_t + dpp_incl_scan(tail);
    if (have) {
      c.ubase[m] = (u32)(jf - front);
      c.ucount[m] = front + tail;
      c.tail[m] = jt - tail;
      c.cls[m] = cls;
    }
    no_index += (u32)__builtin_popcountll(__ballot(have && (cls == kClsNoIndex || cls == kClsDecided)));
    unusable += (u32)__builtin_popcountll(__ballot(cls == kClsUnusable));
    overflow += (u32)__builtin_popcountll(__ballot(cls == kClsOverflow));
    run_e = readlane64(ie, 63);
    run_f = readlane64(jf, 63);
    run_t = readlane(jt, 63);
  }
  if (lane == 0) {
    hdr[kHFront] = (u32)run_f;  // at most extra_cap
    hdr[kHEntries] = (u32)run_f + run_t;  // at most n_msgs + extra_cap
    hdr[kHNoIndex] = no_index;
    hdr[kHUnusable] = unusable;
    hdr[kHOverflow] = overflow;
  }
}

// ---- list.  A wave per body (grid stride): its entries.
__global__ __launch_bounds__(64) void inflate_units_list_kernel(const u8* __restrict__ in,
                                                                const u64* __restrict__ in_off,
                                                                const u32* __restrict__ in_len, u32 n_msgs,
                                                                const u32* hdr, Cols c, u32* __restrict__ entries) {
  const u32 lane = threadIdx.x;
  const u32 front = uniform(hdr[kHFront]);
  for (u32 m = blockIdx.x; m < n_msgs; m += gridDim.x) {
    const u32 cnt = uniform(c.ucount[m]), ub = uniform(c.ubase[m]), tail = front + uniform(c.tail[m]);
    if (cnt == 0) continue;
    if (uniform(c.cls[m]) != kClsIndexed) {
      if (lane == 0) {
        u32* e = entries + (size_t)tail * kEntryWords;
        e[kEBody] = m;
        e[kEKind] = kKindWhole;
      }
      continue;
    }
    const u8* p = in + in_off[m];
    const u32 n = uniform(in_len[m]), chlen = uniform(c.chlen[m]);
    gzidx::Head h;
    h.sizes_at = uniform(c.sizes_at[m]);
    u32 run = uniform(c.begin[m]);
    for (u32 k0 = 0; k0 < cnt; k0 += 64) {
      const u32 k = k0 + lane;
      const u32 size = k + 1 < cnt ? gzidx::size_at(p, h, k) : 0u;  // the last entry places nothing
      const u32 incl = dpp_incl_scan(size);
      if (k < cnt) {
        u32* e = entries + (size_t)(k + 1 < cnt ? ub + k : tail) * kEntryWords;
        const u32 start = run + incl - size;  // <= n - 8: classify's sum rule
        e[kEBody] = m;
        e[kEStart] = start;
        e[kEStop] = k + 1 < cnt ? start + size : n - 8;
        e[kEBase] = k * chlen;  // below 32,762 * 65,535
        e[kEKind] = k + 1 < cnt ? kKindUnit : kKindLast;
      }
      run += readlane(incl, 63);
    }
  }
}

// ---- units.  A wave per entry (grid stride) of the list whose length is
// hdr[count_at].  Four waves per SIMD, as inflate.hip's kernel has: a batch of
// many one-unit bodies must not take more rounds here than there.
template <bool kStore>
__global__ __launch_bounds__(64, 4) void inflate_units_kernel(const u8* __restrict__ in, const u64* __restrict__ in_off,
                                                           const u32* __restrict__ in_len, u8* out,
                                                           const u64* __restrict__ out_off,
                                                           const u32* __restrict__ out_cap,
                                                           u32* __restrict__ out_len, u64* __restrict__ lengths,
                                                           i32* __restrict__ status, u32 format, const u32* hdr,
                                                           u32 count_at, u32* entries, Cols c) {
  const u32 lane = threadIdx.x;
  const u32 total = uniform(hdr[count_at]);
  const u32 trailer = format == infl::kZlib ? 4u : format == infl::kGzip ? 8u : 0u;
  for (u32 ei = blockIdx.x; ei < total; ei += gridDim.x) {
    u32* e = entries + (size_t)ei * kEntryWords;
    const u32 m = uniform(e[kEBody]), kind = uniform(e[kEKind]);
    const u8* p = in + in_off[m];
    const u32 n = uniform(in_len[m]);
    const u32 cap = kStore ? uniform(out_cap[m]) : 0u;
    u8* slot = kStore ? out + out_off[m] : nullptr;
    u64 outpos = 0;
    const bool whole = kind == kKindWhole, nonlast = kind == kKindUnit;
    const u32 chlen = uniform(c.chlen[m]);
    // a whole stream: from the wrapper's end to the trailer, the whole slot
    u32 at = uniform(c.begin[m]), n_end = n - trailer, base = 0, ucap = cap;
    bool ok = !whole || n >= at + trailer;
    if (!whole) {
      at = uniform(e[kEStart]);
      n_end = uniform(e[kEStop]);
      base = uniform(e[kEBase]);
      const u32 room = cap > base ? cap - base : 0u;  // the last unit may run to the slot's end
      ucap = nonlast && chlen < room ? chlen : room;
    }
    ok = ok && inflate_walk<kStore, true>(lane, p, n, at, n_end, nonlast, chlen, kStore ? slot + base : nullptr, ucap,
                                          outpos);
    if (lane == 0) {
      if (whole) {
        const i32 st = !ok ? infl::kStCorrupt : kStore && outpos > cap ? infl::kStSlotTooSmall : infl::kStOk;
        status[m] = st;
        if (kStore)
          out_len[m] = st == infl::kStOk || st == infl::kStSlotTooSmall
                           ? (outpos > 0xffffffffull ? 0xffffffffu : (u32)outpos)
                           : 0u;
        else
          lengths[m] = st == infl::kStOk ? outpos : 0ull;
      } else {
        e[kEClean] = ok ? 1u : 0u;
        e[kELenLo] = (u32)outpos;
        e[kELenHi] = (u32)(outpos >> 32);
      }
    }
    wave_lds_fence();
  }
}

// ---- resolve.  A wave per body (grid stride).
template <bool kStore>
__global__ __launch_bounds__(64) void inflate_units_resolve_kernel(u32 n_msgs, const u32* __restrict__ out_cap,
                                                                   u32* __restrict__ out_len,
                                                                   u64* __restrict__ lengths,
                                                                   i32* __restrict__ status, u32* hdr, Cols c,
                                                                   const u32* __restrict__ entries,
                                                                   u32* __restrict__ redo) {
  const u32 lane = threadIdx.x;
  for (u32 m = blockIdx.x; m < n_msgs; m += gridDim.x) {
    if (uniform(c.cls[m]) != kClsIndexed) continue;
    const u32 cnt = uniform(c.ucount[m]), ub = uniform(c.ubase[m]);
    const u32* last = entries + (size_t)(uniform(hdr[kHFront]) + uniform(c.tail[m])) * kEntryWords;
    bool clean = last[kEClean] == 1u;
    for (u32 k = lane; k + 1 < cnt; k += 64) clean = clean && entries[(size_t)(ub + k) * kEntryWords + kEClean] == 1u;
    const bool all = __ballot(!clean) == 0;
    if (lane == 0) {
      // clean units in front of the last gave CHLEN bytes each
      const u64 total = (u64)(cnt - 1) * c.chlen[m] + ((u64)last[kELenHi] << 32 | last[kELenLo]);
      if (all && (!kStore || total <= out_cap[m])) {
        status[m] = infl::kStOk;
        if (kStore)
          out_len[m] = (u32)total;
        else
          lengths[m] = total;
        atomicAdd(&hdr[kHParBodies], 1u);
        atomicAdd(&hdr[kHParUnits], cnt);
      } else {
        u32* e = redo + (size_t)atomicAdd(&hdr[kHRedo], 1u) * kEntryWords;
        e[kEBody] = m;
        e[kEKind] = kKindWhole;
        atomicAdd(&hdr[kHMismatch], 1u);
      }
    }
  }
}

template <bool kStore>
hipError_t launch_units(const u8* in, const u64* in_off, const u32* in_len, u32 n_msgs, u8* out, const u64* out_off,
                        const u32* out_cap, u32* out_len, u64* lengths, i32* status, u32 format, void* ws_,
                        size_t ws_bytes, hipStream_t stream) {
  if (n_msgs == 0) return hipSuccess;
  Plan p;
  if (!plan_in(n_msgs, ws_bytes, &p)) return hipErrorInvalidValue;
  u8* ws = static_cast<u8*>(ws_);
  u32* hdr = reinterpret_cast<u32*>(ws);
  const Cols c = cols_at(ws, p.off_cols, n_msgs);
  u32* entries = reinterpret_cast<u32*>(ws + p.off_entries);
  u32* redo = reinterpret_cast<u32*>(ws + p.off_redo);
  const u32 body_grid = n_msgs < 65536 ? n_msgs : 65536;
  hipError_t e;
  inflate_units_classify_kernel<kStore><<<body_grid, 64, 0, stream>>>(in, in_off, in_len, n_msgs, out_len, lengths,
                                                                       status, format, c);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  inflate_units_plan_kernel<<<1, 64, 0, stream>>>(n_msgs, hdr, c, (u64)p.cap_entries - n_msgs);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  inflate_units_list_kernel<<<body_grid, 64, 0, stream>>>(in, in_off, in_len, n_msgs, hdr, c, entries);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  inflate_units_kernel<kStore><<<p.cap_entries < kMaxGrid ? p.cap_entries : kMaxGrid, 64, 0, stream>>>(
      in, in_off, in_len, out, out_off, out_cap, out_len, lengths, status, format, hdr, kHEntries, entries, c);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if (format != infl::kGzip) return hipSuccess;  // no index: every body was one whole-stream entry
  inflate_units_resolve_kernel<kStore><<<body_grid, 64, 0, stream>>>(n_msgs, out_cap, out_len, lengths, status, hdr,
                                                                      c, entries, redo);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  inflate_units_kernel<kStore><<<n_msgs < kMaxGrid ? n_msgs : kMaxGrid, 64, 0, stream>>>(
      in, in_off, in_len, out, out_off, out_cap, out_len, lengths, status, format, hdr, kHRedo, redo, c);
  return hipGetLastError();
}

}  // namespace

size_t inflate_units_workspace_bytes(u32 n_msgs, u64 extra_units) { return plan_for(n_msgs, extra_units).bytes; }

u64 inflate_units_entry_capacity(u32 n_msgs, size_t ws_bytes) {
  Plan p;
  return plan_in(n_msgs, ws_bytes, &p) ? p.cap_entries : 0;
}

hipError_t launch_inflate_units(const u8* in, const u64* in_off, const u32* in_len, u32 n_msgs, u8* out,
                                const u64* out_off, const u32* out_cap, u32* out_len, i32* status, u32 format,
                                void* ws, size_t ws_bytes, hipStream_t stream) {
  const hipError_t e = launch_units<true>(in, in_off, in_len, n_msgs, out, out_off, out_cap, out_len, nullptr, status,
                                          format, ws, ws_bytes, stream);
  if (e != hipSuccess || n_msgs == 0 || format == infl::kRaw) return e;
  return launch_inflate_judge(in, in_off, in_len, n_msgs, out, out_off, out_len, status, format, stream);
}

hipError_t launch_inflate_units_lengths(const u8* in, const u64* in_off, const u32* in_len, u32 n_msgs, u64* lengths,
                                        i32* status, u32 format, void* ws, size_t ws_bytes, hipStream_t stream) {
  return launch_units<false>(in, in_off, in_len, n_msgs, nullptr, nullptr, nullptr, nullptr, lengths, status, format,
                             ws, ws_bytes, stream);
}

void inflate_units_header_counts(const void* header, InflateUnitsHeaderCounts* c) {
  const u32* h = static_cast<const u32*>(header);
  c->parallel_bodies = h[kHParBodies];
  c->parallel_units = h[kHParUnits];
  c->no_index = h[kHNoIndex];
  c->unusable = h[kHUnusable];
  c->mismatch = h[kHMismatch];
  c->overflow = h[kHOverflow];
}

}  // namespace fsg
