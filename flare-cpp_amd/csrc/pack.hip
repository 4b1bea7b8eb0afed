// pack.hip -- device-side pack (compaction) of a batch's outputs: n byte
// ranges that lie spread over worst-case slots become one dense buffer plus
// an offsets column, the form a sender puts on the wire and the form that
// makes the D2H copy move result bytes only (fsg_pack_batch,
// include/flare_snappy_gpu.h).  Codec-agnostic: Snappy and LZ4 bodies, or
// decode outputs with the rejected messages masked out by their status.
//
//   eff[i]      = (status && status[i] != FSG_OK) ? 0 : len[i]
//   pack_off[i] = sum_{j<i} round_up(eff[j], align)       (u64)
//   total       = sum over all j of round_up(eff[j], align)
//   dst[pack_off[i] .. + eff[i]) = src[src_off[i] .. + eff[i])
//
// Two parts, every kernel free of inter-workgroup waiting (no look-back, no
// ticket: a workgroup never reads what another one of the same launch wrote):
//   scan  reduce / scan-of-block-sums / add over kPackScanBlock items per
//         workgroup, one more level whenever the block sums exceed one
//         workgroup (n = 2^32 - 1 takes four levels);
//   copy  byte-balanced over the DESTINATION: a wave owns tiles of
//         kPackTileBytes of it whatever the message sizes are, so a million bodies of a few
//         hundred bytes next to bodies of megabytes (CM, C5) load every wave
//         alike, where a wave per message would serialise on the large ones.
#include "../../include/flare_snappy_gpu.h"
#include "launch.h"
#include "snappy_device.h"
#include "wave_util.h"

namespace fsg {
namespace {

constexpr u32 kPackScanThreads = 256;
constexpr u32 kPackScanPerThread = 4;
constexpr u32 kPackScanBlock = kPackScanThreads * kPackScanPerThread;  // items per workgroup (1024)
constexpr u32 kPackTileBytes = 4096;   // a tile of the destination: 4 steps of 64 lanes x 16 bytes
constexpr u32 kPackTilesPerWave = 4;   // consecutive tiles a wave takes at a time (one full search per 16 KiB)
constexpr u32 kPackCopyBlocks = 2048;  // 256 CUs x 8 workgroups of 4 waves; the waves stride over the tiles

// Inclusive prefix sum of a u64 over the 64 lanes: three DPP scans
// (wave_util.h) over limbs of 24, 24 and 16 bits, whose 64-lane sums stay
// below 2^30, recombined modulo 2^64 (exact whenever the true sum fits).
__device__ __forceinline__ u64 wave_incl_scan_u64(u64 t) {
  const u32 s0 = dpp_incl_scan((u32)t & 0xffffffu);
  const u32 s1 = dpp_incl_scan((u32)(t >> 24) & 0xffffffu);
  const u32 s2 = dpp_incl_scan((u32)(t >> 48));
  return (u64)s0 + ((u64)s1 << 24) + ((u64)s2 << 48);
}

// Exclusive prefix of `t` over the workgroup's 256 threads and the
// workgroup's sum.  Every thread of the workgroup calls it.
__device__ __forceinline__ u64 block_excl_scan(u64 t, u64* block_total) {
  __shared__ u64 wsum[kPackScanThreads / 64];
  const u64 inc = wave_incl_scan_u64(t);
  const u32 wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 63) wsum[wave] = inc;
  __syncthreads();
  u64 pre = 0, tot = 0;
#pragma unroll
  for (u32 w = 0; w < kPackScanThreads / 64; ++w) {
    const u64 s = wsum[w];
    pre += w < wave ? s : 0;
    tot += s;
  }
  *block_total = tot;
  return pre + inc - t;
}

// This thread's kPackScanPerThread consecutive items.  Leaf: the messages'
// padded effective lengths; otherwise the sums of the level below.
template <bool Leaf>
__device__ __forceinline__ void load_items(u64 (&v)[kPackScanPerThread], const u32* len, const i32* status,
                                           const u64* in, u64 n, u64 first, u32 amask) {
#pragma unroll
  for (u32 k = 0; k < kPackScanPerThread; ++k) {
    const u64 i = first + k;
    u64 x = 0;
    if (i < n) {
      if (Leaf) {
        const u32 e = (status && status[i] != kOk) ? 0u : len[i];
        x = ((u64)e + amask) & ~(u64)amask;
      } else {
        x = in[i];
      }
    }
    v[k] = x;
  }
}

template <bool Leaf>
__global__ __launch_bounds__(kPackScanThreads) void pack_reduce_kernel(const u32* len, const i32* status,
                                                                       const u64* in, u64 n, u32 amask,
                                                                       u64* sums) {
  u64 v[kPackScanPerThread];
  load_items<Leaf>(v, len, status, in, n, (u64)blockIdx.x * kPackScanBlock + threadIdx.x * kPackScanPerThread,
                   amask);
  u64 tot;
  (void)block_excl_scan(v[0] + v[1] + v[2] + v[3], &tot);
  if (threadIdx.x == 0) sums[blockIdx.x] = tot;
}

// Exclusive scan of one workgroup's items plus base[blockIdx.x] (the scanned
// sums of the level above; null for the single workgroup of the top level,
// which also writes the grand total).  `out` may be `in` (the sums are
// scanned in place: a thread reads its four items before it writes them and
// touches no other thread's).
template <bool Leaf>
__global__ __launch_bounds__(kPackScanThreads) void pack_scan_kernel(const u32* len, const i32* status,
                                                                     const u64* in, u64 n, u32 amask,
                                                                     const u64* base, u64* out, u64* total) {
  u64 v[kPackScanPerThread];
  const u64 first = (u64)blockIdx.x * kPackScanBlock + threadIdx.x * kPackScanPerThread;
  load_items<Leaf>(v, len, status, in, n, first, amask);
  u64 tot;
  u64 run = block_excl_scan(v[0] + v[1] + v[2] + v[3], &tot) + (base ? base[blockIdx.x] : 0);
#pragma unroll
  for (u32 k = 0; k < kPackScanPerThread; ++k) {
    if (first + k < n) out[first + k] = run;
    run += v[k];
  }
  if (total && threadIdx.x == 0) *total = tot;
}

__device__ __forceinline__ u32 eff_len(const u32* len, const i32* status, u64 j) {
  return (status && status[j] != kOk) ? 0u : len[j];
}

// First index in [lo, hi] whose off[] exceeds pos (hi if none), for the whole
// wave at once: each lane probes the end of one 64th of the range and a
// ballot keeps the 64th that holds the answer, so a million offsets take four
// dependent loads where a binary search takes twenty.  All 64 lanes call it
// with the same arguments.
__device__ __forceinline__ u64 wave_upper_bound(const u64* off, u64 lo, u64 hi, u64 pos, u32 lane) {
  while (lo < hi) {
    const u64 step = (hi - lo + 63) >> 6;
    u64 idx = lo + (u64)(lane + 1) * step - 1;
    if (idx > hi - 1) idx = hi - 1;
    const u64 mask = __ballot(off[idx] > pos);
    if (mask == 0) return hi;
    const u32 f = (u32)__ffsll((unsigned long long)mask) - 1;
    u64 nhi = lo + (u64)(f + 1) * step - 1;
    if (nhi > hi - 1) nhi = hi - 1;
    lo += (u64)f * step;  // lane f-1's probe (the element before) is <= pos
    hi = nhi;             // lane f's probe is > pos
  }
  return lo;
}

// Last index in [m, n) whose off[] is <= pos, given off[m] <= pos, for the
// whole wave: the 64 entries behind m first (one load; the answer is there
// whenever fewer than 64 messages start between the two positions), else the
// 64-ary search over the rest.
__device__ __forceinline__ u64 wave_last_le_from(const u64* off, u64 m, u64 n, u64 pos, u32 lane) {
  const u64 idx = m + 1 + lane;
  const u64 le = __ballot(idx < n && off[idx] <= pos);  // sorted: a prefix of the lanes
  const u32 c = (u32)__popcll((unsigned long long)le);
  if (c < 64) return m + c;
  return wave_upper_bound(off, m + 65, n, pos, lane) - 1;
}

// Last index in [lo, hi] whose off[] is <= q, given off[lo] <= q (one lane).
__device__ __forceinline__ u64 last_le(const u64* off, u64 lo, u64 hi, u64 q) {
  while (lo < hi) {
    const u64 mid = lo + ((hi - lo + 1) >> 1);
    if (off[mid] <= q) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// A wave takes kPackTilesPerWave consecutive tiles of kPackTileBytes of the
// packed destination at a time.  The first message of a tile is the last one
// whose offset is <= the tile's start: among a run of empty messages sharing
// an offset that is the non-empty one behind them.  It is searched for over
// all offsets once per run of tiles and from the previous tile's message on
// after that.
// Each lane then takes one 16-byte destination block per step:
//   * a block wholly inside one message: one 16-byte load, one 16-byte store.
//     The store is aligned when d_dst is; the load is not whenever align or
//     src_off is no multiple of 16.  It is issued as ONE unaligned 16-byte
//     global load (gfx950 runs in unaligned-access mode, snappy_device.h;
//     the alternative, two aligned loads and a byte-align, doubles the load
//     count for the same cache lines) and reads message bytes only;
//   * any other block (a message's head or tail, a block several messages
//     share when align < 16, padding): byte by byte, bytes of no message
//     are not written.
// A tile past `total` does not exist, so nothing is stored from there on.
__global__ __launch_bounds__(256) void pack_copy_kernel(const u8* __restrict__ src, const u64* __restrict__ src_off,
                                                        const u32* __restrict__ len,
                                                        const i32* __restrict__ status, u32 n,
                                                        const u64* __restrict__ pack_off,
                                                        const u64* __restrict__ total_p, u8* __restrict__ dst) {
  const u32 lane = threadIdx.x & 63;
  const u64 wave = ((u64)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const u64 nwaves = ((u64)gridDim.x * blockDim.x) >> 6;
  const u64 total = *total_p;
  constexpr u64 kSpan = (u64)kPackTileBytes * kPackTilesPerWave;
  for (u64 w0 = wave * kSpan; w0 < total; w0 += nwaves * kSpan) {
    u64 mf = wave_upper_bound(pack_off, 0, n, w0, lane) - 1;  // pack_off[0] = 0 <= w0
    for (u64 t0 = w0; t0 < w0 + kSpan && t0 < total; t0 += kPackTileBytes) {
      const u64 t1 = t0 + kPackTileBytes < total ? t0 + kPackTileBytes : total;
      if (t0 != w0) mf = wave_last_le_from(pack_off, mf, n, t0, lane);  // on from the tile before
      const u64 pf = pack_off[mf];
      if (pf + eff_len(len, status, mf) >= t0 + kPackTileBytes) {  // the tile lies inside message mf
        const u8* s = src + src_off[mf] + (t0 - pf) + 16 * lane;
        u8* d = dst + t0 + 16 * lane;
        u32x4 v[4];
#pragma unroll
        for (u32 k = 0; k < 4; ++k) __builtin_memcpy(&v[k], s + 1024 * k, 16);
#pragma unroll
        for (u32 k = 0; k < 4; ++k) __builtin_memcpy(d + 1024 * k, &v[k], 16);
        continue;
      }
      const u64 ml = wave_last_le_from(pack_off, mf, n, t1 - 1, lane);  // last message starting in the tile
      u64 j = mf;
      for (u32 k = 0; k < 4; ++k) {
        const u64 p = t0 + 1024 * k + 16 * lane;
        if (p >= t1) break;
        j = last_le(pack_off, j, ml, p);
        u64 pj = pack_off[j];
        u32 ej = eff_len(len, status, j);
        const u8* sj = src + src_off[j];
        if (p + 16 <= pj + ej) {
          u32x4 v;
          __builtin_memcpy(&v, sj + (p - pj), 16);
          __builtin_memcpy(dst + p, &v, 16);
          continue;
        }
        const u64 pe = p + 16 < t1 ? p + 16 : t1;
        for (u64 q = p; q < pe; ++q) {
          if (j < ml && pack_off[j + 1] <= q) {
            j = last_le(pack_off, j + 1, ml, q);
            pj = pack_off[j];
            ej = eff_len(len, status, j);
            sj = src + src_off[j];
          }
          if (q - pj < ej) dst[q] = sj[q - pj];
        }
      }
    }
  }
}

// Items of scan level k (level 0 = the messages) and where level k's sums
// start in the workspace; returns the number of levels above 0.
struct PackLevels {
  u64 m[8];
  size_t at[8];
  int top;
  size_t bytes;
};
PackLevels pack_levels(u32 n) {
  PackLevels L{};
  L.m[0] = n;
  L.top = 0;
  size_t pos = 0;
  while (L.m[L.top] > kPackScanBlock) {
    const u64 next = (L.m[L.top] + kPackScanBlock - 1) / kPackScanBlock;
    ++L.top;
    L.m[L.top] = next;
    L.at[L.top] = pos;
    pos += (size_t)next * sizeof(u64);
  }
  L.bytes = pos + sizeof(u64);
  return L;
}

}  // namespace

size_t pack_workspace_bytes(u32 n_msgs) { return pack_levels(n_msgs).bytes; }

// d_src and d_dst must not overlap (not checked).  The caller has checked
// the pointers, `align` and the workspace size.
hipError_t launch_pack(const u8* src, const u64* src_off, const u32* len, const i32* status, u32 n, u32 align,
                       u8* dst, u64* pack_off, u64* total, void* ws, hipStream_t stream) {
  if (n == 0) return hipMemsetAsync(total, 0, sizeof(u64), stream);
  const PackLevels L = pack_levels(n);
  const u32 amask = align - 1;
  u8* w = static_cast<u8*>(ws);
  auto sums = [&](int k) { return reinterpret_cast<u64*>(w + L.at[k]); };
  if (L.top == 0) {
    pack_scan_kernel<true><<<1, kPackScanThreads, 0, stream>>>(len, status, nullptr, n, amask, nullptr, pack_off,
                                                              total);
  } else {
    pack_reduce_kernel<true><<<(u32)L.m[1], kPackScanThreads, 0, stream>>>(len, status, nullptr, n, amask, sums(1));
    for (int k = 1; k < L.top; ++k)
      pack_reduce_kernel<false><<<(u32)L.m[k + 1], kPackScanThreads, 0, stream>>>(nullptr, nullptr, sums(k),
                                                                                 L.m[k], 0, sums(k + 1));
    pack_scan_kernel<false><<<1, kPackScanThreads, 0, stream>>>(nullptr, nullptr, sums(L.top), L.m[L.top], 0,
                                                               nullptr, sums(L.top), total);
    for (int k = L.top - 1; k >= 1; --k)
      pack_scan_kernel<false><<<(u32)L.m[k + 1], kPackScanThreads, 0, stream>>>(
          nullptr, nullptr, sums(k), L.m[k], 0, sums(k + 1), sums(k), nullptr);
    pack_scan_kernel<true><<<(u32)L.m[1], kPackScanThreads, 0, stream>>>(len, status, nullptr, n, amask, sums(1),
                                                                        pack_off, nullptr);
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || !dst) return e;
  pack_copy_kernel<<<kPackCopyBlocks, 256, 0, stream>>>(src, src_off, len, status, n, pack_off, total, dst);
  return hipGetLastError();
}

}  // namespace fsg
