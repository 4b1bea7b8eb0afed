// inflate.hip -- batched inflate (raw deflate, zlib, gzip) for gfx950, one wave
// per body; the checksum kernel behind it; fsg_crc32_batch / fsg_adler32_batch.
// include/flare_deflate_gpu.h states the acceptance rule; inflate_format.h
// holds the verdict rules and the table build, shared with the host model
// (host/inflate_cpu.cc), which this kernel is written from.  DESIGN.md
// section 4, "Deflate".
//
// A body's wave alternates between two phases.
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
#include "launch.h"
#include "wave_util.h"

namespace fsg {
namespace {

using infl::e_bits;
using infl::e_op;
using infl::e_val;

// LDS decode tables: the dynamic block's, then the fixed code's
constexpr u32 kTabLit = 0, kTabDist = infl::kEnoughLens, kTabFixLit = kTabDist + infl::kEnoughDists,
              kTabFixDist = kTabFixLit + 512, kTabEntries = kTabFixDist + 32;
// Bodies above this are FSG_CORRUPT: byte positions are 32 bits wide and run
// up to one group's bits past the input's end.
constexpr u32 kMaxBody = 0xFFFF0000u;

__device__ __forceinline__ u32 uniform(u32 v) { return (u32)__builtin_amdgcn_readfirstlane((int)v); }

// Wave-uniform 64-bit bit buffer over a body.  Input words come through the
// body's buffer descriptor (wave_util.h msg_rsrc: dwords past the body read 0
// and touch no memory) and the bytes at and past n are masked to 0.
struct WaveReader {
  __amdgpu_buffer_rsrc_t rs;
  u32 base;  // the body's first byte in the descriptor
  u32 n;
  u32 pos;   // next byte to load
  u64 hold;
  u32 nbits;
  __device__ __forceinline__ void need() {
    if (nbits < 32) {
      const u32 P = base + pos, s = P & 3u;
      const u32x2 d = __builtin_amdgcn_raw_buffer_load_b64(rs, P & ~3u, 0, 0);
      u32 w = __builtin_amdgcn_alignbyte(d[1], d[0], s);
      const u32 keep = pos < n ? n - pos : 0u;
      if (keep < 4) w &= (1u << (8 * keep)) - 1u;
      hold |= (u64)uniform(w) << nbits;
      nbits += 32;
      pos += 4;
    }
  }
  __device__ __forceinline__ void restart(u32 at) {
    pos = at;
    hold = 0;
    nbits = 0;
  }
  __device__ __forceinline__ u32 peek(u32 k) const { return (u32)hold & ((1u << k) - 1u); }
  __device__ __forceinline__ void drop(u32 k) {
    hold >>= k;
    nbits -= k;
  }
  __device__ __forceinline__ u32 bits(u32 k) {
    const u32 v = peek(k);
    drop(k);
    return v;
  }
  __device__ __forceinline__ u64 consumed() const { return 8ull * pos - nbits; }
};

__device__ __forceinline__ u32 lookup(WaveReader& r, const u32* tab, u32 root) {
  u32 e = uniform(tab[r.peek(root)]);
  if (e_op(e) & infl::kOpLink) {
    r.drop(e_bits(e));
    e = uniform(tab[e_val(e) + r.peek(e_op(e) & 15u)]);
  }
  r.drop(e_bits(e));
  return e;
}

constexpr u32 kRecLiteral = 0x80000000u;  // | the byte; a copy: length | distance << 9

// The execute phase of one group: cnt records (lane k: rec, len; the other
// lanes 0, 0) whose first output byte is slot position g < cap.
__device__ __forceinline__ void execute_group(u32 lane, u32 rec, u32 len, u32 g, u32 cap,
                                              __amdgpu_buffer_rsrc_t slot, u32* s_start, u32* s_rec) {
  const u32 incl = dpp_incl_scan(len);
  const u32 total = readlane(incl, 63);
  s_start[lane] = incl - len;  // lanes past the last record: total, above every position
  s_rec[lane] = rec;
  wave_lds_fence();
  wait_all_memory();  // the earlier groups' stores, before this group's loads
  for (u32 j = lane; j < total; j += 64) {
    const u32 at = g + j;
    if (at >= cap || at < g) break;  // count-only from the capacity on
    u32 p = j, val;
    for (;;) {  // every round moves to an earlier record: 64 rounds at most
      u32 r = 0;
#pragma unroll
      for (u32 step = 32; step; step >>= 1)
        if (s_start[r + step] <= p) r += step;
      const u32 rc = s_rec[r], first = s_start[r];
      if (rc & kRecLiteral) {
        val = rc & 0xffu;
        break;
      }
      const u32 dist = (rc >> 9) & 0xffffu, i = p - first;
      const u32 back = dist - (i < dist ? i : i % dist);  // 1 .. dist bytes below the record
      if (back > first) {  // below the group: g + first >= dist was checked when the record was decoded
        val = __builtin_amdgcn_raw_buffer_load_b8(slot, g + first - back, 0, 16);
        break;
      }
      p = first - back;
    }
    __builtin_amdgcn_raw_buffer_store_b8((u8)val, slot, at, 0, 0);
  }
  wave_lds_fence();
}

template <bool kStore>
__global__ __launch_bounds__(64) void inflate_kernel(const u8* __restrict__ in, const u64* __restrict__ in_off,
                                                     const u32* __restrict__ in_len, u32 n_msgs, u8* out,
                                                     const u64* __restrict__ out_off,
                                                     const u32* __restrict__ out_cap, u32* __restrict__ out_len,
                                                     u64* __restrict__ lengths, i32* __restrict__ status,
                                                     u32 format) {
  __shared__ u32 s_tab[kTabEntries];
  __shared__ u8 s_lens[infl::kLensArray];
  __shared__ u16 s_work[infl::kLensArray];
  __shared__ infl::TableScratch s_scr;
  __shared__ u32 s_start[64], s_rec[64];
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
    const u32 bal = (u32)(reinterpret_cast<uintptr_t>(p) & 15u);
    WaveReader r;
    r.rs = msg_rsrc(p - bal, bal + n);
    r.base = bal;
    r.n = n;
    r.restart(w.begin);
    const __amdgpu_buffer_rsrc_t slot =
        __builtin_amdgcn_make_buffer_rsrc(dst, (short)0, (int)cap, 0x00020000);
    bool have_fixed = false;
    u32 last;
    // Termination: every block takes at least 3 bits, every symbol at least
    // one, every stored block lies inside the input, and the bit position is
    // compared with the stream's end after every group of at most 64 symbols
    // (48 bits each at most), so it stays below 8 * (n + 400) and each loop
    // below ends; a body's time is bounded by its length and the bytes it
    // declares (258 per symbol at most).
    do {
      r.need();
      last = r.bits(1);
      const u32 type = r.bits(2);
      if (type == 3) return;
      if (type == 0) {  // stored: cooperative 16-byte copies
        r.drop(r.nbits & 7u);
        r.need();
        const u32 len = r.bits(16), nlen = r.bits(16);
        if ((len ^ 0xffffu) != nlen) return;
        const u64 start = r.consumed() >> 3;
        if (start + len > n_end) return;
        if (kStore && outpos < cap) {
          const u32 room = cap - (u32)outpos, ne = len < room ? len : room;
          const u8* s = p + start;
          u8* d = dst + outpos;
          for (u32 c = lane; c < (ne >> 4); c += 64) copy16(d + 16 * c, s + 16 * c);
          for (u32 t = (ne & ~15u) + lane; t < ne; t += 64) d[t] = s[t];
        }
        outpos += len;
        r.restart((u32)start + len);
        continue;
      }
      u32 lit, dist, lroot = infl::kLenRoot, droot = infl::kDistRoot;
      if (type == 1) {  // fixed: built on first use, kept for the body
        lit = kTabFixLit;
        dist = kTabFixDist;
        if (!have_fixed) {
          for (u32 k = lane; k < infl::kFixedLens + infl::kFixedDists; k += 64) s_lens[k] = (u8)infl::fixed_length(k);
          wave_lds_fence();
          infl::build_table(infl::kLens, s_lens, infl::kFixedLens, s_tab + lit, 512, &lroot, s_work, &s_scr, lane, 64);
          infl::build_table(infl::kDists, s_lens + infl::kFixedLens, infl::kFixedDists, s_tab + dist, 32, &droot,
                            s_work, &s_scr, lane, 64);
          have_fixed = true;
        }
        lroot = 9;
        droot = 5;
      } else {
        lit = kTabLit;
        dist = kTabDist;
        u32 nl, nd;
        if (!infl::read_dynamic_header(r, s_lens, &nl, &nd, s_tab + dist, s_work, &s_scr, lane, 64)) return;
        if (infl::build_table(infl::kLens, s_lens, nl, s_tab + lit, infl::kEnoughLens, &lroot, s_work, &s_scr, lane,
                              64) != infl::kTableOk)
          return;
        if (infl::build_table(infl::kDists, s_lens + nl, nd, s_tab + dist, infl::kEnoughDists, &droot, s_work, &s_scr,
                              lane, 64) != infl::kTableOk)
          return;
      }
      lroot = uniform(lroot);
      droot = uniform(droot);
      bool eob = false;
      while (!eob) {
        // ---- symbol phase
        const u64 gstart = outpos;
        u32 cnt = 0, rec = 0, len = 0;
        while (cnt < 64) {
          r.need();
          u32 e = lookup(r, s_tab + lit, lroot);
          u32 op = e_op(e), rc, ln;
          if (op == infl::kOpLit) {
            rc = kRecLiteral | e_val(e);
            ln = 1;
          } else {
            if (op == infl::kOpEnd) {
              eob = true;
              break;
            }
            if (!(op & infl::kOpBase)) return;  // a symbol with no code
            ln = e_val(e) + r.bits(op & 15u);
            r.need();
            e = lookup(r, s_tab + dist, droot);
            op = e_op(e);
            if (!(op & infl::kOpBase)) return;
            const u32 distance = e_val(e) + r.bits(op & 15u);
            if (distance > outpos) return;  // before the body's first byte
            rc = ln | distance << 9;
          }
          if (lane == cnt) {
            rec = rc;
            len = ln;
          }
          outpos += ln;
          ++cnt;
        }
        if (r.consumed() > 8ull * n_end) return;
        // ---- execute phase
        if (kStore && cnt && gstart < cap) execute_group(lane, rec, len, (u32)gstart, cap, slot, s_start, s_rec);
      }
    } while (!last);
    const u64 used = r.consumed();
    if (used > 8ull * n_end || (used + 7) / 8 != n_end) return;  // cut short, or bytes after the stream
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
