// inflate.hip -- batched inflate (raw deflate, zlib, gzip) for gfx950, one wave
// per body; the checksum kernel behind it; fsg_crc32_batch / fsg_adler32_batch.
// include/flare_deflate_gpu.h states the acceptance rule; inflate_format.h
// holds the verdict rules and the table build, shared with the host model
// (host/inflate_cpu.cc), which this kernel is written from.  DESIGN.md
// section 4, "Deflate".
//
// The block loop itself is inflate_walk.h's (shared with inflate_units.hip,
// which runs it with a wave per unit of an indexed gzip body); what follows
// describes it.  A body's wave alternates between two phases.
//   Symbol phase: wave-uniform code (every lane holds the same bit buffer;
//   table entries and input words go through readfirstlane, so the compiler
//   keeps them in scalar registers) decodes up to 64 Huffman symbols with the
//   LDS tables; symbol k's record -- a literal byte, or a length and a
//   distance -- stays in lane k.
//   Execute phase: a DPP prefix sum over the lengths places the records; the
//   records and their first positions go to LDS, and the group's output bytes
//   are produced 64 at a time, one per lane.  A lane finds the record that owns
//   its byte (binary search over the 64 first positions).  A literal gives the
//   byte.  A copy gives a source position below the record's first byte
//   (dst - dist + (i mod dist): an overlapping copy is its period repeated);
//   a source below the group's first byte is loaded from the slot, one inside
//   the group is resolved again through the record that owns it, which lies
//   earlier in the group, so at most 64 times.  No byte a group reads from the
//   slot is one it stores, so the copies of a group need no order among them.
//
// Ordering of the slot reads ("Ordering, far copies"):
// the bytes a group loads were stored by earlier groups of the same wave; the
// wave waits for all its outstanding stores (s_waitcnt 0) before the first
// load of each group, and the loads are sc1 buffer loads, served by L2, so
// nothing relies on the L1.
//
// Count-only mode: kStore = false compiles the execute phase out (the lengths
// call); the decode kernel skips it once a group starts at or past the slot's
// capacity, and stores are predicated on the capacity before that.
//
// No loop waits on another wave.
#include "inflate_format.h"
#include "inflate_sum.h"
#include "inflate_walk.h"
#include "launch.h"
#include "wave_util.h"

namespace fsg {
namespace {

template <bool kStore>
__global__ __launch_bounds__(64) void inflate_kernel(const u8* __restrict__ in, const u64* __restrict__ in_off,
                                                     const u32* __restrict__ in_len, u32 n_msgs, u8* out,
                                                     const u64* __restrict__ out_off,
                                                     const u32* __restrict__ out_cap, u32* __restrict__ out_len,
                                                     u64* __restrict__ lengths, i32* __restrict__ status,
                                                     u32 format) {
  const u32 lane = threadIdx.x, m = blockIdx.x;
  if (m >= n_msgs) return;
  const u8* p = in + in_off[m];
  const u32 n = uniform(in_len[m]);
  const u32 cap = kStore ? uniform(out_cap[m]) : 0u;
  u8* dst = kStore ? out + out_off[m] : nullptr;
  i32 st = infl::kStOk;
  u64 outpos = 0;

  [&] {
    if (n == 0 || n > kMaxBody) {
      st = n == 0 && format != infl::kRaw ? infl::kStBadHeader : infl::kStCorrupt;
      return;
    }
    const infl::Wrapper w = infl::parse_wrapper(format, p, n);
    if (w.status != infl::kStOk) {
      st = w.status;
      return;
    }
    st = infl::kStCorrupt;  // every early return below
    if (n < w.begin + w.trailer) return;
    const u32 n_end = n - w.trailer;  // where the deflate stream must end
    if (!inflate_walk<kStore, false>(lane, p, n, w.begin, n_end, false, 0u, dst, cap, outpos)) return;
    st = kStore && outpos > cap ? infl::kStSlotTooSmall : infl::kStOk;
  }();

  if (lane == 0) {
    status[m] = st;
    if (kStore)
      out_len[m] = st == infl::kStOk || st == infl::kStSlotTooSmall
                       ? (outpos > 0xffffffffull ? 0xffffffffu : (u32)outpos)
                       : 0u;
    else
      lengths[m] = st == infl::kStOk ? outpos : 0ull;
  }
}

// The checksum kernel, a wave per body.  mode 0 / 1: zlib's crc32 / adler32 of
// [in + in_off[m], + in_len[m]) into sum[m].  mode 2 / 3 judge the bodies the
// decode kernel left FSG_OK: the Adler-32 of the decoded bytes against the
// zlib trailer (big endian, the body's last 4 bytes), or their CRC-32 and
// length mod 2^32 against the gzip trailer (little endian, the last 8); a
// mismatch is FSG_CORRUPT with length 0.
constexpr u32 kSumCrc = 0, kSumAdler = 1, kSumJudgeZlib = 2, kSumJudgeGzip = 3;
constexpr u32 kSumMaxGrid = 1u << 20;

__global__ __launch_bounds__(64) void inflate_sum_kernel(const u8* __restrict__ in, const u64* __restrict__ in_off,
                                                         const u32* __restrict__ in_len, u32 n_msgs, const u8* out,
                                                         const u64* __restrict__ out_off, u32* out_len, i32* status,
                                                         u32* __restrict__ sum, u32 mode) {
  __shared__ u32 s_crc[256];
  const u32 lane = threadIdx.x;
  const bool crc = mode == kSumCrc || mode == kSumJudgeGzip;
  if (crc) crc_table_init(s_crc, lane);
  for (u32 m = blockIdx.x; m < n_msgs; m += gridDim.x) {
    const u8* body = in + in_off[m];
    const u32 n = uniform(in_len[m]);
    if (mode <= kSumAdler) {
      const u32 v = crc ? wave_crc32(body, n, s_crc, lane) : wave_adler32(body, n, lane);
      if (lane == 0) sum[m] = v;
      continue;
    }
    if (uniform((u32)status[m]) != (u32)infl::kStOk) continue;
    const u8* d = out + out_off[m];
    const u32 len = uniform(out_len[m]);
    bool ok;
    if (mode == kSumJudgeZlib) {
      const u8* t = body + n - 4;  // the decode kernel found n >= header + 4
      const u32 want = (u32)t[0] << 24 | (u32)t[1] << 16 | (u32)t[2] << 8 | t[3];
      ok = wave_adler32(d, len, lane) == want;
    } else {
      const u8* t = body + n - 8;
      const u32 want = t[0] | (u32)t[1] << 8 | (u32)t[2] << 16 | (u32)t[3] << 24;
      const u32 isize = t[4] | (u32)t[5] << 8 | (u32)t[6] << 16 | (u32)t[7] << 24;
      ok = wave_crc32(d, len, s_crc, lane) == want && isize == len;
    }
    if (!ok && lane == 0) {
      status[m] = infl::kStCorrupt;
      out_len[m] = 0;
    }
  }
}

}  // namespace

hipError_t launch_inflate(const u8* in, const u64* in_off, const u32* in_len, u32 n_msgs, u8* out, const u64* out_off,
                          const u32* out_cap, u32* out_len, i32* status, u32 format, hipStream_t stream) {
  if (n_msgs == 0) return hipSuccess;
  inflate_kernel<true><<<n_msgs, 64, 0, stream>>>(in, in_off, in_len, n_msgs, out, out_off, out_cap, out_len, nullptr,
                                                   status, format);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || format == infl::kRaw) return e;
  return launch_inflate_judge(in, in_off, in_len, n_msgs, out, out_off, out_len, status, format, stream);
}

hipError_t launch_inflate_judge(const u8* in, const u64* in_off, const u32* in_len, u32 n_msgs, const u8* out,
                                const u64* out_off, u32* out_len, i32* status, u32 format, hipStream_t stream) {
  inflate_sum_kernel<<<n_msgs < kSumMaxGrid ? n_msgs : kSumMaxGrid, 64, 0, stream>>>(
      in, in_off, in_len, n_msgs, out, out_off, out_len, status, nullptr,
      format == infl::kZlib ? kSumJudgeZlib : kSumJudgeGzip);
  return hipGetLastError();
}

hipError_t launch_inflate_lengths(const u8* in, const u64* in_off, const u32* in_len, u32 n_msgs, u64* lengths,
                                  i32* status, u32 format, hipStream_t stream) {
  if (n_msgs == 0) return hipSuccess;
  inflate_kernel<false><<<n_msgs, 64, 0, stream>>>(in, in_off, in_len, n_msgs, nullptr, nullptr, nullptr, nullptr,
                                                    lengths, status, format);
  return hipGetLastError();
}

hipError_t launch_inflate_sum(const u8* in, const u64* in_off, const u32* in_len, u32 n_msgs, u32* sum, bool adler,
                              hipStream_t stream) {
  if (n_msgs == 0) return hipSuccess;
  inflate_sum_kernel<<<n_msgs < kSumMaxGrid ? n_msgs : kSumMaxGrid, 64, 0, stream>>>(
      in, in_off, in_len, n_msgs, nullptr, nullptr, nullptr, nullptr, sum, adler ? kSumAdler : kSumCrc);
  return hipGetLastError();
}

}  // namespace fsg
