// decode_v4_exec_common.h -- what the three execution headers of the two-pass
// Snappy decoder share (decode_v4_exec4.h, decode_v4_exec5.h,
// decode_v4_packed.h): the tag ring's geometry, which also sizes the LDS of
// exec_kernel and exec_packed_kernel (snappy_decode_v4.hip), and the phase
// stamps of the diagnostic build.
#pragma once

#include "snappy_device.h"

namespace fsg {

namespace {

// ---- pass 2 geometry
#ifndef FSG_TAG_RING
#define FSG_TAG_RING 512
#endif
constexpr u32 kTagRing = FSG_TAG_RING;       // tag positions per wave (LDS)
constexpr u32 kFillWords = kTagRing / 32;    // bitmap words per fill (<= kTagRing / 2 tags)
constexpr u32 kMaxPieces = 64;

// Diagnostic build only (-DFSG_STAMPS): per-phase cycle totals of exec_kernel,
// summed over waves, read back with fsg_debug_stamps.
#ifdef FSG_STAMPS
__device__ unsigned long long g_stamps[24];  // 0-7 exec5_message phases; 8-15 exec5_packed phases, 16 its set-up, 17-20 counts
#define STAMP(k) do { const u64 t_ = __builtin_amdgcn_s_memtime(); st_[k] += t_ - t_last_; t_last_ = t_; } while (0)
#else
#define STAMP(k) do { } while (0)
#endif

// ceil(len / step) for a pattern copy: len <= 64 and step >= 9 (pat_step of
// offsets 1..15), so the answer is 1..8 -- counted instead of divided.
__device__ __forceinline__ u32 pattern_pieces(u32 len, u32 step) {
  u32 pc = 1;
#pragma unroll
  for (u32 k = 1; k < 8; ++k) pc += len > k * step ? 1u : 0u;
  return pc;
}

}  // namespace

}  // namespace fsg
