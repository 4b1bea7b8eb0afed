// snappy_device.h -- device-side constants and helpers shared by the gfx950
// Snappy kernels.  Format constants follow the reference's vendored Snappy
// 1.1.3 (/root/reference/flare/io/snappy/).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "encode_v3_plan.h"  // kBlockLog .. kInputMarginBytes, table_size_for, kWaveEncMaxWaves, wave_quota_of

namespace fsg {

typedef uint8_t u8;
typedef uint16_t u16;
typedef uint32_t u32;
typedef uint64_t u64;
typedef int32_t i32;
typedef int64_t i64;

// (kBlockLog, kBlockSize, kMaxHashTableSize, kInputMarginBytes: encode_v3_plan.h)
constexpr u32 kHashMul = 0x1e35a7bdu;            // snappy.cc:47
constexpr int kWave = 64;                        // CDNA wavefront

// Status words (mirrors include/flare_snappy_gpu.h).
constexpr i32 kOk = 0;
constexpr i32 kCorrupt = 1;
constexpr i32 kBadHeader = 2;
constexpr i32 kSlotTooSmall = 3;
// Internal: message not indexed by the two-pass decoder (its bitmap did not
// fit the workspace); finished by v4's fallback_kernel (one lane, serial tag
// loop), or by the v3 kernel under kFlagFallbackOnly.
constexpr i32 kNeedFallback = 0x40000000;
constexpr u32 kFlagFallbackOnly = 0x80000000u;
// Internal: a large message left by the lane-per-message index pass for the
// wave-per-message one (decode v4), which writes its final status.
constexpr i32 kNeedBigIndex = 0x20000000;
// Internal: listed by the decode v4 plan pass for the lane walk.
constexpr i32 kNeedLaneWalk = 0x10000000;

__host__ __device__ inline u64 max_compressed_length(u64 n) {
  return 32 + n + n / 6;  // snappy.cc:55-77
}

__host__ __device__ inline int varint32_len(u32 v) {
  return v < (1u << 7) ? 1 : v < (1u << 14) ? 2 : v < (1u << 21) ? 3
       : v < (1u << 28) ? 4 : 5;
}

// Unaligned little-endian loads/stores on global memory.  gfx950 runs in
// unaligned-access mode, so these lower to single dword/dwordx2/dwordx4 ops.
__device__ __forceinline__ u32 ldu32(const u8* p) {
  u32 v;
  __builtin_memcpy(&v, p, 4);
  return v;
}
__device__ __forceinline__ u64 ldu64(const u8* p) {
  u64 v;
  __builtin_memcpy(&v, p, 8);
  return v;
}
__device__ __forceinline__ void stu64(u8* p, u64 v) { __builtin_memcpy(p, &v, 8); }
__device__ __forceinline__ void stu32(u8* p, u32 v) { __builtin_memcpy(p, &v, 4); }

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void copy16(u8* d, const u8* s) {
  u32x4 v;
  __builtin_memcpy(&v, s, 16);
  __builtin_memcpy(d, &v, 16);
}

__device__ __forceinline__ u32 hash_bytes(u32 bytes, int shift) {
  return (bytes * kHashMul) >> shift;  // snappy.cc:46-49
}

__device__ __forceinline__ int lane_id() { return __lane_id(); }

// ---- encode work units (encode_plan_kernel's long list)
constexpr u32 kWholeUnit = 0x80000000u;  // unit = a whole message (not a fragment of a split one)

// Units [0, quota) of the long list go to the wave encoder, the rest to the
// lane encoder (wave_quota_of, encode_v3_plan.h), from the plan pass's counters.
__device__ __forceinline__ u32 wave_quota(const u32* ctr, u32 share_permille, u64 all_bytes) {
  return wave_quota_of(ctr[1], *reinterpret_cast<const unsigned long long*>(ctr + 6), share_permille, all_bytes);
}

// Staging regions of a split message (more than one 64 KiB fragment): fragment
// k is encoded at dst + hdr + k * stride and may fill *room bytes; the gather
// pass then moves the fragments together.  Every full fragment gets the same
// stride, 64 bytes short of 64 KiB + 1/6, and the last one the rest of the
// slot: with f bytes it has at least f + f/6 + 64 * (fragments - 1) + 22 (the
// encoders keep 48 bytes of spill room), so an incompressible fragment (its
// bytes + 3) fits whatever the message length.  (An even split of the slot,
// the earlier rule, left a 70,000-byte body two regions of 40,832 bytes, and
// every incompressible body whose length is not near a multiple of 64 KiB
// went to the whole-message fallback.)  region_cap != 0 (test knob) caps
// every region.  total > kBlockSize.
__host__ __device__ __forceinline__ u32 split_region(u32 total, u32 hdr, u32 nfr, u32 region_cap, u32 k,
                                                     u32* room) {
  const u32 slot = (u32)max_compressed_length(total) - hdr;
  u32 stride = ((kBlockSize + kBlockSize / 6) & ~15u) - 64;
  u32 last = slot - (nfr - 1) * stride;
  if (region_cap && region_cap < stride) stride = region_cap;
  if (region_cap && region_cap < last) last = region_cap;
  *room = k == nfr - 1 ? last : stride;
  return stride;
}

// (The host entry points -- launch_*, workspace sizes, the path report's
// header counts -- are declared in launch.h.)

}  // namespace fsg
