// lz4_encode_wave.hip -- LZ4 compress, one wave per body, position table in LDS.
//
// The default LZ4 block compressor (lz4.hip: lz4_compress_block, the oracle's
// lz4o_compress_block) is one serial greedy chain per body, and its serial
// time is the match search: probes at cur_0 = ip, cur_1, ... with a step that
// grows every 64 misses; EVERY probe reads the table slot of its hash and
// overwrites it with its own position, and the search ends at the first probe
// whose candidate is near enough and has the same 4 bytes.  This kernel runs
// that chain exactly, 64 probes of one search at a time:
//
//   window  lane k holds probe k of the next 64.  Its position comes from the
//           step schedule carried across windows (fwd, step, nb); its
//           candidate is the position of the highest lane j < k with the same
//           hash, else the table entry as of the window's start (all probes
//           before a probe insert).  The first lane that hits, or whose next
//           position passes mflimit + 1, ends the window.  Lanes up to and
//           including a hit commit their positions in one LDS store (the
//           highest lane wins a shared slot, as the newest write does:
//           tools/probes/lds_overlap_probe.hip, and snappy_encode_wave.hip's
//           commit); a lane that ended the window at the limit does not.
//   between windows, wave-uniform: backward extension and match count are
//           wave-parallel compares with a ballot; token, length bytes,
//           literals, offset are written cooperatively; the ip - 2 insert and
//           the immediate re-match test follow.
//
// Same-hash lanes of a window are found through the table itself: the live
// lanes store their positions and read the slot back; if every lane reads its
// own, no two share a slot and every candidate is the table's (the common
// case; a window that then runs to its end has also committed already).
// Otherwise a readlane loop finds each lane's predecessor, and a window that
// ends early restores the slots before its commit.
//
// Input is read through a buffer descriptor of the body (bytes past it read
// 0); literal copies read the body's own bytes.  Every store is exact-length
// inside the body's slot.  CPU model, checked block for block against the
// oracle: tools/l4wenc_model.cc.
#include "launch.h"
#include "snappy_device.h"

namespace fsg {

namespace {

constexpr u32 kMinMatch = 4, kMfLimit = 12, kLastLiterals = 5, kHashLog = 12, kSkipTrigger = 6;
constexpr u32 kDistanceMax = 65535, kLimit64K = 65536 + kMfLimit - 1;
constexpr u32 kMaxInput = 0x7E000000u;  // LZ4_MAX_INPUT_SIZE
constexpr u32 kTableBytes = kLz4EncTableBytes;  // 8,192 x u16 or 4,096 x u32

// ---- the header of the routed call's workspace (its layout: lz4_plan.h)
constexpr u32 kCtrListed = 0;  // bodies on the list
constexpr u32 kCtrNext = 1;    // the wave kernel's work counter
constexpr u32 kCtrDone = 2;    // bodies the wave kernel encoded
constexpr u32 kCtrBytes = 4;   // their input bytes (u64: words 4, 5)

__device__ __forceinline__ u32 rl(u32 v, u32 l) { return (u32)__builtin_amdgcn_readlane((int)v, (int)l); }
__device__ __forceinline__ u32 rfl(u32 v) { return (u32)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ void lds_fence() { __builtin_amdgcn_wave_barrier(); }

// The body as a buffer: offset fal + p is byte p (the base is the dword below
// the body's first byte, the size the dword above its last).
struct Body {
  __amdgpu_buffer_rsrc_t r;
  u32 fal;
};
// 4 bytes at p; *b4 = the 5th
__device__ __forceinline__ u32 w5(const Body& s, u32 p, u32* b4) {
  const u32 a = s.fal + p;
  const u32x2 d = __builtin_amdgcn_raw_buffer_load_b64(s.r, (int)(a & ~3u), 0, 0);
  *b4 = (d[1] >> (8 * (a & 3u))) & 0xffu;
  return __builtin_amdgcn_alignbyte(d[1], d[0], a & 3u);
}
__device__ __forceinline__ u32 w4(const Body& s, u32 p) {
  u32 b4;
  return w5(s, p, &b4);
}
__device__ __forceinline__ u32 b1(const Body& s, u32 p) {
  return (u32)__builtin_amdgcn_raw_buffer_load_b8(s.r, (int)(s.fal + p), 0, 0);
}

__device__ __forceinline__ u32 l4_hash(u32 lo, u32 b4, bool small) {
  if (small) return (lo * 2654435761u) >> (32 - (kHashLog + 1));
  const u64 x = (u64)lo | (u64)b4 << 32;
  return (u32)(((x << 24) * 889523592379ull) >> (64 - kHashLog));
}

// sum of (t >> 6) for t in [0, x): the step schedule's running total
__device__ __forceinline__ u32 step_sum(u32 x) {
  const u32 q = x >> kSkipTrigger, r = x & 63u;
  return 32u * q * (q - 1u) + r * q;
}

// One block of n bytes, encoded by the calling wave to dst (at most cap
// bytes); returns the block's length, or 0xffffffff if it would not fit (it
// always does: the slot holds LZ4_compressBound(n)).  tab: the wave's 16 KiB
// of LDS, zeroed.
__device__ u32 wave_block(const Body& s, const u8* src, u32 n, u8* dst, u32 cap, u8* tab, u32 lane) {
  const bool small = n < kLimit64K;
  u16* const t16 = reinterpret_cast<u16*>(tab);
  u32* const t32 = reinterpret_cast<u32*>(tab);
  auto get = [&](u32 h) -> u32 { return small ? (u32)t16[h] : t32[h]; };
  auto put = [&](u32 h, u32 v) {
    if (small) t16[h] = (u16)v;
    else t32[h] = v;
  };
  u32 op = 0, anchor = 0;
  bool fits = true;
  // token, length bytes, literals [lit_at, lit_at + lit); with has_match the
  // offset and the match length bytes
  auto emit = [&](u32 lit_at, u32 lit, bool has_match, u32 off, u32 ml) {
    const u32 nl = lit >= 15 ? (lit - 15) / 255 + 1 : 0u;
    const u32 nm = has_match && ml >= 15 ? (ml - 15) / 255 + 1 : 0u;
    const u32 size = 1 + nl + lit + (has_match ? 2 + nm : 0u);
    if (size > cap - op || lit > n - lit_at) {
      fits = false;
      return;
    }
    u8* d = dst + op;
    if (lane == 0) d[0] = (u8)((lit >= 15 ? 15u : lit) << 4 | (has_match ? (ml >= 15 ? 15u : ml) : 0u));
    for (u32 i = lane; i < nl; i += 64) d[1 + i] = i + 1 < nl ? (u8)255 : (u8)((lit - 15) % 255);
    d += 1 + nl;
    const u8* from = src + lit_at;
    if (lit <= 64) {
      if (lane < lit) d[lane] = from[lane];
    } else {
      for (u32 k0 = 0; k0 < lit; k0 += 1024) {  // 1 KiB a step, 16 bytes a lane
        const u32 k = k0 + 16 * lane;
        if (k + 16 <= lit) {
          copy16(d + k, from + k);
        } else {
          for (u32 i = k; i < lit; ++i) d[i] = from[i];
        }
      }
    }
    if (has_match) {
      d += lit;
      if (lane < 2) d[lane] = (u8)(off >> (8 * lane));
      for (u32 i = lane; i < nm; i += 64) d[2 + i] = i + 1 < nm ? (u8)255 : (u8)((ml - 15) % 255);
    }
    op += size;
  };

  if (n >= kMfLimit + 1) {
    const u32 mflimit1 = n - kMfLimit + 1;  // a match starts before this
    const u32 matchlimit = n - kLastLiterals;
    // (the reference's first insert, position 0 at hash(0), leaves the zeroed table as it is)
    u32 ip = 1;
    u32 guard = 0;  // every window and every sequence advances the parse
    for (;;) {
      // ---- match search: windows of 64 probes
      u32 fwd = ip, step = 1, nb = 1u << kSkipTrigger, match = 0;
      bool at_limit = false;
      for (;;) {
        if (++guard > n) {
          fits = false;
          break;
        }
        const u32 f0 = step_sum(nb);
        const u32 cur = fwd + (lane ? step + step_sum(nb + lane - 1) - f0 : 0u);
        const u32 nxt = fwd + step + step_sum(nb + lane) - f0;
        const bool live = cur <= mflimit1;  // the probe before it passed the limit test
        const bool ok = nxt <= mflimit1;
        u32 b4;
        const u32 iw = w5(s, live ? cur : 0u, &b4);
        const u32 h = live ? l4_hash(iw, b4, small) : 0u;
        const u32 T = get(h);
        lds_fence();
        if (live) put(h, cur);
        lds_fence();
        const u32 rb = get(h);
        lds_fence();
        u32 mi = T;
        if (__ballot(live && rb != cur)) {  // lanes sharing a slot: each lane's predecessor
          const u32 nlive = (u32)__builtin_popcountll(__ballot(live));
          for (u32 j = 0; j + 1 < nlive; ++j) {
            const u32 hj = rl(h, j), cj = rl(cur, j);
            mi = j < lane && hj == h ? cj : mi;
          }
        }
        const u32 cw = w4(s, live && ok ? mi : 0u);
        const bool hit = live && ok && (small || mi + kDistanceMax >= cur) && cw == iw;
        const u64 E = __ballot(live && (hit || !ok));
        if (!E) {  // (the slots already hold the window's commit)
          fwd = rl(nxt, 63);
          step = (nb + 63) >> kSkipTrigger;
          nb += 64;
          continue;
        }
        const u32 e = (u32)__builtin_ctzll(E);
        at_limit = !((__ballot(ok) >> e) & 1ull);
        if (live) put(h, T);
        lds_fence();
        if (lane < e + (at_limit ? 0u : 1u)) put(h, cur);
        lds_fence();
        ip = rl(cur, e);
        match = rl(mi, e);
        break;
      }
      if (at_limit || !fits) break;
      // ---- backward extension, 64 bytes a step
      {
        const u32 maxb = ip - anchor < match ? ip - anchor : match;
        u32 ext = 0;
        while (maxb) {
          const u32 i = ext + lane;
          const bool in = i < maxb;
          const u32 a = b1(s, in ? ip - 1 - i : 0u), b = b1(s, in ? match - 1 - i : 0u);
          const u64 ne = __ballot(!(in && a == b));
          if (ne) {
            ext += (u32)__builtin_ctzll(ne);
            break;
          }
          ext += 64;
        }
        ip -= ext;
        match -= ext;
      }
      u32 lit_at = anchor, lit = ip - anchor;
      bool last = false;
      for (;;) {  // a match at ip from `match`, then possibly another at once
        if (++guard > n) {
          fits = false;
          break;
        }
        // ---- match count, 4 bytes a lane (LZ4_count up to matchlimit)
        u32 m = 0;
        for (;;) {
          const u32 o = kMinMatch + m + 4 * lane;
          const u32 left = ip + o < matchlimit ? matchlimit - (ip + o) : 0u;
          const u32 x = w4(s, left ? ip + o : 0u) ^ w4(s, left ? match + o : 0u);
          u32 eqb = x ? (u32)__builtin_ctz(x) >> 3 : 4u;
          eqb = eqb < left ? eqb : left;
          const u64 stop = __ballot(eqb < 4);
          if (stop) {
            const u32 l = (u32)__builtin_ctzll(stop);
            m += 4 * l + rl(eqb, l);
            break;
          }
          m += 256;
        }
        emit(lit_at, lit, true, ip - match, m);
        if (!fits) break;
        ip += m + kMinMatch;
        anchor = ip;
        if (ip >= mflimit1) {
          last = true;
          break;
        }
        // ---- the ip - 2 insert and the test at ip (uniform: every lane the same values)
        u32 b4a, b4b;
        const u32 wa = w5(s, ip - 2, &b4a), wb = w5(s, ip, &b4b);
        const u32 ha = l4_hash(wa, b4a, small), hb = l4_hash(wb, b4b, small);
        if (lane == 0) put(ha, ip - 2);
        lds_fence();
        const u32 mi = get(hb);
        lds_fence();
        if (lane == 0) put(hb, ip);
        lds_fence();
        if ((small || mi + kDistanceMax >= ip) && w4(s, mi) == wb) {
          match = mi;
          lit_at = ip;
          lit = 0;
          continue;
        }
        break;
      }
      if (last || !fits) break;
      ++ip;
    }
  }
  if (fits) emit(anchor, n - anchor, false, 0, 0);
  return fits ? op : 0xffffffffu;
}

// One lane per message: the indices of the bodies of at least wave_min bytes,
// appended by ballot and one atomic per wave.
__global__ __launch_bounds__(256) void lz4_encode_list_kernel(const u32* __restrict__ in_len, u32 n_msgs, u64 wave_min,
                                                            u32* __restrict__ hdr, u32* __restrict__ list) {
  const u32 m = blockIdx.x * 256 + threadIdx.x;
  const u32 lane = threadIdx.x & 63;
  const bool mine = m < n_msgs && (u64)in_len[m] >= wave_min;
  const u64 b = __ballot(mine);
  if (!b) return;
  const u32 first = (u32)__builtin_ctzll(b);
  u32 base = 0;
  if (lane == first) base = atomicAdd(&hdr[kCtrListed], (u32)__builtin_popcountll(b));
  base = rl(base, first);
  if (mine) list[base + (u32)__builtin_popcountll(b & ((1ull << lane) - 1))] = m;
}

// Persistent grid, one wave a workgroup: the listed bodies from one work
// counter.  Header, d_out_len and d_status as lz4_encode_kernel writes them.
__global__ __launch_bounds__(64) void lz4_encode_wave_kernel(const u8* __restrict__ in, const u64* __restrict__ in_off,
                                                           const u32* __restrict__ in_len, u8* out,
                                                           const u64* __restrict__ out_off, u32* __restrict__ out_len,
                                                           i32* __restrict__ status, u32* hdr,
                                                           const u32* __restrict__ list) {
  __shared__ __attribute__((aligned(16))) u8 tab[kTableBytes];
  const u32 lane = threadIdx.x;
  const u32 n_list = rfl(hdr[kCtrListed]);
  for (;;) {
    // (every lane takes part, lane 0 adding 1: a fetch under `lane == 0` next to
    // the lane-0 stores that end the previous body lets the compiler route
    // lane 0 round the loop apart from the others, which then read a stale
    // first lane -- snappy_encode_wave.hip fetches its units the same way)
    const u32 w = rfl(atomicAdd(&hdr[kCtrNext], lane == 0 ? 1u : 0u));
    if (w >= n_list) break;
    const u32 m = rfl(list[w]);
    const u32 n = rfl(in_len[m]);
    if (lane == 0) {
      atomicAdd(&hdr[kCtrDone], 1u);
      atomicAdd(reinterpret_cast<unsigned long long*>(hdr + kCtrBytes), (unsigned long long)n);
    }
    if (n > kMaxInput) {
      if (lane == 0) {
        out_len[m] = 0;
        status[m] = kCorrupt;
      }
      continue;
    }
    u8* const ob = out + out_off[m];
    const u32 hl = (u32)varint32_len(n);
    if (lane == 0) {
      u8* hp = ob;
      u32 v = n;
      while (v >= 0x80) {
        *hp++ = (u8)(v | 0x80);
        v >>= 7;
      }
      *hp = (u8)v;
    }
    const u8* src = in + in_off[m];
    Body s;
    s.fal = (u32)(reinterpret_cast<uintptr_t>(src) & 3);
    s.r = __builtin_amdgcn_make_buffer_rsrc(const_cast<u8*>(src - s.fal), (short)0, (int)((s.fal + n + 3) & ~3u),
                                            0x00020000);
    for (u32 i = 16 * lane; i < kTableBytes; i += 1024) *reinterpret_cast<u32x4*>(tab + i) = u32x4{0, 0, 0, 0};
    lds_fence();
    // the slot: 5 + LZ4_compressBound(n) (fsg_lz4_max_compressed_length)
    const u32 len = wave_block(s, src, n, ob + hl, 5 + n + n / 255 + 16 - hl, tab, lane);
    lds_fence();
    if (lane == 0) {
      out_len[m] = len != 0xffffffffu ? hl + len : 0u;
      status[m] = len != 0xffffffffu ? kOk : kCorrupt;
    }
  }
}

}  // namespace

void lz4_encode_header_counts(const void* header, Lz4EncodeHeaderCounts* c) {
  u32 ctr[kCtrBytes + 2];
  __builtin_memcpy(ctr, header, sizeof(ctr));
  c->listed = ctr[kCtrListed];
  c->wave_messages = ctr[kCtrDone];
  c->wave_bytes = (u64)ctr[kCtrBytes] | (u64)ctr[kCtrBytes + 1] << 32;
}

// fsg_lz4_compress_batch, every size and decision from lz4_encode_plan
// (lz4_plan.h).  Route 0: the bodies of at least wave_min bytes on the wave
// encoder, the others on the lanes, both on `stream`.  Route 1: the lanes
// only, as before the wave encoder.  Either way the launch zeroes what it
// uses.
hipError_t launch_lz4_encode(const u8* in, const u64* in_off, const u32* in_len, u32 n_msgs, u8* out,
                             const u64* out_off, u32* out_len, i32* status, void* ws, hipStream_t stream,
                             const Lz4EncodePlan& p) {
  if (n_msgs == 0) return hipSuccess;
  hipError_t e = hipMemsetAsync(ws, 0, p.zero_bytes, stream);
  if (e != hipSuccess) return e;
  u8* const tables = static_cast<u8*>(ws) + p.tables_off;
  if (p.wave_min >= kLz4WaveNone)
    return launch_lz4_encode_lanes(in, in_off, in_len, n_msgs, out, out_off, out_len, status, tables, kLz4WaveNone,
                                   stream);
  u32* hdr = static_cast<u32*>(ws);
  u32* list = reinterpret_cast<u32*>(static_cast<u8*>(ws) + p.list_off);
  lz4_encode_list_kernel<<<p.list_grid, 256, 0, stream>>>(in_len, n_msgs, p.wave_min, hdr, list);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  lz4_encode_wave_kernel<<<p.wave_grid, 64, 0, stream>>>(in, in_off, in_len, out, out_off, out_len, status, hdr, list);
  e = hipGetLastError();
  if (e != hipSuccess || p.wave_min == 0) return e;  // (0: no body is left for the lanes)
  return launch_lz4_encode_lanes(in, in_off, in_len, n_msgs, out, out_off, out_len, status, tables, p.wave_min, stream);
}

}  // namespace fsg
