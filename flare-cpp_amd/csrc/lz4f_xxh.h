// lz4f_xxh.h -- XXH32 of many byte ranges at once, a quad of lanes per range:
// the checksum kernel of the LZ4 frame calls (lz4_frame_encode.hip,
// lz4_frame_decode.hip) and of
// fsg_lz4f_xxh32_batch.  lz4f::xxh32 (lz4_frame_format.h) stays the serial
// text; this gives the same words.
//
// A unit is one byte range [p, p + n) with one checksum.  XXH32 cuts it into
// 16-byte stripes; word q of every stripe feeds accumulator q, and the rotate
// between the add and the multiply leaves no scan over one accumulator, so a
// unit has exactly four chains.  Lane q of a quad holds accumulator q, a wave
// carries 16 units.  Per step each lane of the quad loads one stripe (64
// contiguous bytes per quad), and a 4x4 transpose in two DPP quad_perm
// exchanges gives lane q word q of the four stripes in order.  The merge of
// the four accumulators is two more quad_perm adds; the tail (up to three
// words, then up to three bytes) is the serial text on every lane of the
// quad, and lane 0 stores the result.
//
// Loads: 16-byte loads only for whole stripes of the unit, the tail by words
// and bytes, so no load touches a byte outside [p, p + n); p may have any
// alignment (gfx950 runs in unaligned-access mode).  Every loop is bounded by
// the unit's length or the unit count; all control flow is uniform within a
// quad (it depends on the unit alone), so the four lanes of a quad are active
// together at every DPP.  No wave waits for another.
#pragma once

#include "lz4_frame_format.h"
#include "snappy_device.h"

namespace fsg {
namespace {

constexpr u32 kXxhUnitsPerWave = 16;

// quad_perm [1,0,3,2] and [2,3,0,1]: the lane whose index differs in bit 0, bit 1
__device__ __forceinline__ u32 quad_xor1(u32 v) {
  return (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xf, 0xf, true);
}
__device__ __forceinline__ u32 quad_xor2(u32 v) {
  return (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xf, 0xf, true);
}

// In: w[i] = word i of this lane's stripe (lane j of the quad: stripe j).
// Out: w[j] = word q of stripe j.  Two exchanges of 2x2 blocks.
__device__ __forceinline__ void quad_transpose(u32x4& w, u32 q) {
  const bool b0 = q & 1, b1 = q & 2;
  const u32 r01 = quad_xor1(b0 ? w[0] : w[1]);
  const u32 r23 = quad_xor1(b0 ? w[2] : w[3]);
  if (b0) {
    w[0] = r01;
    w[2] = r23;
  } else {
    w[1] = r01;
    w[3] = r23;
  }
  const u32 r02 = quad_xor2(b1 ? w[0] : w[2]);
  const u32 r13 = quad_xor2(b1 ? w[1] : w[3]);
  if (b1) {
    w[0] = r02;
    w[1] = r13;
  } else {
    w[2] = r02;
    w[3] = r13;
  }
}

__device__ __forceinline__ u32x4 xxh_load_stripe(const u8* p) {
  u32x4 v;
  __builtin_memcpy(&v, p, 16);
  return v;
}

// K steps of four stripes from stripe s on, as long as they are whole: the
// loads of a round first, so that K * 64 bytes per quad are in flight.
template <int K>
__device__ __forceinline__ void xxh_steps(const u8* p, u32 q, u64& s, u64 stripes, u32& acc) {
  for (; s + 4 * K <= stripes; s += 4 * K) {
    u32x4 w[K];
#pragma unroll
    for (int k = 0; k < K; ++k) w[k] = xxh_load_stripe(p + 16 * (s + 4 * k + q));
#pragma unroll
    for (int k = 0; k < K; ++k) {
      quad_transpose(w[k], q);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc = lz4f::xxh_round(acc, w[k][j]);
    }
  }
}

// XXH32 of [p, p + n) with `seed`, by the quad this lane is lane q of.  All
// four lanes call it with the same arguments and get the result.
__device__ __forceinline__ u32 quad_xxh32(const u8* p, u64 n, u32 seed, u32 q) {
  u32 h;
  u64 i = 0;
  if (n >= 16) {
    const u64 stripes = n >> 4;
    u32 acc = q == 0 ? seed + lz4f::kP1 + lz4f::kP2 : q == 1 ? seed + lz4f::kP2 : q == 2 ? seed : seed - lz4f::kP1;
    u64 s = 0;
    xxh_steps<16>(p, q, s, stripes, acc);
    xxh_steps<4>(p, q, s, stripes, acc);
    xxh_steps<1>(p, q, s, stripes, acc);
    const u32 rest = (u32)(stripes - s);  // 0..3 stripes: lanes below `rest` load one
    if (rest) {
      u32x4 w{0, 0, 0, 0};
      if (q < rest) w = xxh_load_stripe(p + 16 * (s + q));
      quad_transpose(w, q);
      acc = lz4f::xxh_round(acc, w[0]);
      if (rest > 1) acc = lz4f::xxh_round(acc, w[1]);
      if (rest > 2) acc = lz4f::xxh_round(acc, w[2]);
    }
    h = lz4f::rotl(acc, q == 0 ? 1 : q == 1 ? 7 : q == 2 ? 12 : 18);
    h += quad_xor1(h);
    h += quad_xor2(h);
    i = stripes << 4;
  } else {
    h = seed + lz4f::kP5;
  }
  h += (u32)n;
  for (; i + 4 <= n; i += 4) h = lz4f::rotl(h + ldu32(p + i) * lz4f::kP3, 17) * lz4f::kP4;
  for (; i < n; ++i) h = lz4f::rotl(h + p[i] * lz4f::kP5, 11) * lz4f::kP1;
  h ^= h >> 15;
  h *= lz4f::kP2;
  h ^= h >> 13;
  h *= lz4f::kP3;
  h ^= h >> 16;
  return h;
}

// One quad per unit, 16 units per wave, a wave per block; a grid of at most
// kXxhMaxGrid blocks strides over the units.  Units: a struct with
//   bool any() const                                          false: no unit has anything to do
//   bool get(u32 u, const u8** p, u64* n, u32* seed) const   false: nothing to do for unit u
//   void put(u32 u, u32 h) const                              called by lane 0 of the quad
// any and get must not depend on the lane, so that a quad stays together.  A
// launch whose units have nothing to do (any() false: a decode batch without
// checksums) costs kXxhMaxGrid waves that read one word each.
constexpr u32 kXxhMaxGrid = 8192;

template <typename Units>
__global__ __launch_bounds__(64) void lz4f_xxh_quad_kernel(Units units, u32 count) {
  if (!units.any()) return;
  const u32 q = threadIdx.x & 3;
  for (u32 u = blockIdx.x * kXxhUnitsPerWave + (threadIdx.x >> 2); u < count; u += gridDim.x * kXxhUnitsPerWave) {
    const u8* p;
    u64 n;
    u32 seed;
    if (!units.get(u, &p, &n, &seed)) continue;
    const u32 h = quad_xxh32(p, n, seed, q);
    if (q == 0) units.put(u, h);
  }
}

template <typename Units>
hipError_t launch_xxh_quads(const Units& units, u32 count, hipStream_t stream) {
  if (count == 0) return hipSuccess;
  const u32 waves = (count + kXxhUnitsPerWave - 1) / kXxhUnitsPerWave;
  lz4f_xxh_quad_kernel<<<waves < kXxhMaxGrid ? waves : kXxhMaxGrid, 64, 0, stream>>>(units, count);
  return hipGetLastError();
}

}  // namespace
}  // namespace fsg
