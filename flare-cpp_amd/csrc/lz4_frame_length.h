// lz4_frame_length.h -- the decoded length of one LZ4 block by a whole wave:
// lz4f::block_length (lz4_frame_format.h) for a block of a frame that states
// no content size, where the sequences are the only place a block's length is
// written.  Included by lz4_frame_decode.hip alone.  The shape is lz4_walk_big's
// (lz4_decode2.hip), the code is its own: nothing here needs offsets, output
// positions per sequence or the block decoder's end rules, only lengths.
//
// The wave stages the block through an 8 KiB LDS ring and takes 64 input bytes
// per step.  Lane i decodes the sequence that would start at byte pos + i:
// token, one literal-length byte, the literals and the offset field skipped,
// one match-length byte.  That gives the lane a successor and lit + ml output
// bytes.  Pointer doubling over (successor lane, output bytes, last lane)
// from lane 0 -- the real position -- reaches the chain's last sequence in
// the window with the output bytes before it; what that sequence is decides
// the step: it leaves the window (go on there), it ends the block, it breaks a
// rule of block_length, or the window cannot decode it (a 255 length byte)
// and one wave-uniform serial step takes it, reading the length bytes 64 at a
// time.
//
// Why one comparison at the end is block_length's answer: every failure of
// block_length is the same `false`, and its running output count never
// shrinks, so "some count on the way exceeded the limit" and "the count at
// the end, or where the walk broke off, exceeded it" give the same verdict.
// The count is cut to limit + 1 after every step, so nothing wraps: a block
// has at most 4 MiB (the index pass checked its size word against the block
// maximum), one length field is below 255 * 4 Mi + 19 < 2^31, and a step adds
// at most two of them to a count of at most 4 Mi + 1.
#pragma once

#include "lz4_frame_format.h"
#include "wave_util.h"

namespace fsg {
namespace {

constexpr u32 kLenRing = 8192;  // bytes of LDS per wave
constexpr u32 kLenHalf = kLenRing / 2;
constexpr u32 kLenWaves = 4;    // waves per workgroup of lz4f_length_wave_kernel
// the furthest byte a lane reads past its own: token, length byte, 15 + 254
// literals, offset field, match-length byte
constexpr u32 kLenReach = 2 + 269 + 2;
static_assert(64 + kLenReach < kLenHalf, "a window's reads must lie inside the staged half");

// what the sequence at a lane is
constexpr u32 kSeqNext = 0;    // complete: successor and output bytes known
constexpr u32 kSeqDone = 1;    // its literals end at the block's last byte
constexpr u32 kSeqFail = 2;    // block_length returns false here
constexpr u32 kSeqSerial = 3;  // a 255 length byte: the serial step

// true and *len: lz4f::block_length(src, n, limit, len), for 0 < n <= 4 MiB
// and limit <= 4 MiB.  Wave-uniform arguments and result; ring: kLenRing bytes
// of LDS of this wave's own.
__device__ inline bool lz4f_wave_block_length(const u8* __restrict__ src, u32 n, u32 limit, u32* ring, u32 lane,
                                              u32* len) {
  const u32 bal = (u32)(reinterpret_cast<uintptr_t>(src) & 15);
  const u8* abase = src - bal;  // 16-byte chunks from here; the block is [bal, bal + n)
  const u32 last_chunk = (bal + n - 1) >> 4;
  const u8* ring8 = reinterpret_cast<const u8*>(ring);
  // ring slots of chunks [c0, c0 + nch); a chunk past the block's last one is
  // never read from memory (its slot gets the last chunk's bytes, which no
  // lane trusts: every byte a lane uses lies below n)
  auto stage = [&](u32 c0, u32 nch) {
    wave_lds_fence();
    for (u32 r = 0; r < nch; r += 64) {
      const u32 k = c0 + r + lane;
      const u32 kk = k <= last_chunk ? k : last_chunk;
      const u32x4 v = *reinterpret_cast<const u32x4*>(abase + 16 * (u64)kk);
      *reinterpret_cast<u32x4*>(ring + ((4 * k) & (kLenRing / 4 - 1))) = v;
    }
    wave_lds_fence();
  };
  u32 sb = 0;  // the ring holds [sb, sb + kLenRing) from abase
  stage(0, kLenRing / 16);
  // afterwards P < sb + kLenHalf: the ring holds at least [P, P + kLenHalf)
  auto keep = [&](u32 P) {
    if (P >= sb + kLenHalf) {
      const u32 nsb = P & ~(kLenHalf - 1);
      if (nsb == sb + kLenHalf)
        stage((sb + kLenRing) >> 4, kLenHalf / 16);
      else
        stage(nsb >> 4, kLenRing / 16);
      sb = nsb;
    }
  };
  auto rb = [&](u32 p) -> u32 { return ring8[(p + bal) & (kLenRing - 1)]; };
  // A run of length bytes from ip on, read from memory 64 at a time
  // (wave-uniform): v += the bytes up to and including the first that is not
  // 255, ip past it.  false: the input ends first.
  auto run = [&](u32& ip, u32& v) -> bool {
    for (;;) {
      const u32 a = ip + lane;
      const u32 b = a < n ? (u32)src[a] : 256u;
      const u64 stop = __ballot(b != 255u);
      if (!stop) {
        v += 255u * 64u;
        ip += 64;
        continue;
      }
      const u32 k = (u32)__builtin_ctzll(stop);
      const u32 bk = readlane(b, k);
      if (bk == 256u) return false;
      v += 255u * k + bk;
      ip += k + 1;
      return true;
    }
  };

  u32 pos = 0, op = 0;
  for (;;) {
    pos = (u32)__builtin_amdgcn_readfirstlane((int)pos);
    op = (u32)__builtin_amdgcn_readfirstlane((int)op);
    sb = (u32)__builtin_amdgcn_readfirstlane((int)sb);
    if (pos >= n || op > limit) return false;
    keep(pos + bal);
    // ---------- every lane: the sequence that would start at p
    const u32 p = pos + lane;
    const bool in = p < n;
    const u32 tok = in ? rb(p) : 0u;
    const u32 l0 = tok >> 4, nib = tok & 15u;
    const bool lx = l0 == 15u, mx = nib == 15u;
    const bool have1 = p + 1 < n;
    const u32 b1 = lx && have1 ? rb(p + 1) : 0u;
    const u32 lit = l0 + b1;
    const u32 ipl = p + 1 + (lx ? 1u : 0u);  // <= n unless the token or its length byte is missing
    u32 kind = kSeqNext, succ = 0, w = 0;
    if (!in || (lx && !have1)) {
      kind = kSeqFail;  // the input ends inside the token or its extension
    } else if (lx && b1 == 255u) {
      kind = kSeqSerial;
    } else if (lit > n - ipl) {
      kind = kSeqFail;  // the literals overrun the input
    } else if (lit == n - ipl) {
      kind = kSeqDone;
    } else {
      const u32 q = ipl + lit;  // the offset field; q < n
      if (q + 2 > n || (mx && q + 2 >= n)) {
        kind = kSeqFail;  // the input ends inside the offset field or the extension
      } else {
        const u32 b2 = mx ? rb(q + 2) : 0u;
        if (mx && b2 == 255u) kind = kSeqSerial;
        succ = q + 2 + (mx ? 1u : 0u);
        w = lit + nib + 4u + b2;
      }
    }
    // ---------- the chain from lane 0: J the next lane (64: none in this
    // window), T the last lane reached, W the output bytes of the sequences
    // before T.  A sequence has at least 3 bytes, so at most 22 start in a
    // window: 5 rounds.  W < 22 * 543 fits 16 bits.
    const bool hop = kind == kSeqNext && succ < pos + 64;
    u32 J = hop ? succ - pos : 64u, T = lane, W = hop ? w : 0u;
#pragma unroll
    for (int r = 0; r < 5; ++r) {
      const u32 pk = (W << 16) | (T << 8) | J;
      const u32 o = (u32)__shfl((int)pk, (int)(J < 64 ? J : lane), 64);
      if (J < 64) {
        W += o >> 16;
        T = (o >> 8) & 0xffu;
        J = o & 0xffu;
      }
    }
    const u32 t = readlane(T, 0);
    const u32 before = op + readlane(W, 0);
    const u32 tkind = readlane(kind, t);
    if (tkind == kSeqFail) return false;
    if (tkind == kSeqDone) {
      const u32 total = before + readlane(lit, t);
      *len = total;
      return total <= limit;
    }
    if (tkind == kSeqNext) {
      pos = readlane(succ, t);
      op = before + readlane(w, t);
      op = op > limit ? limit + 1 : op;
      continue;
    }
    // ---------- one sequence at pos + t, wave-uniform, lengths from memory:
    // block_length's loop body
    op = before;
    u32 ip = pos + t;  // < n: the lane had its token
    const u32 tk = src[ip++];
    u32 sl = tk >> 4;
    if (sl == 15u && !run(ip, sl)) return false;
    if (sl > n - ip) return false;
    if (ip + sl == n) {
      const u32 total = op + sl;
      *len = total;
      return total <= limit;
    }
    ip += sl + 2;
    if (ip > n) return false;
    u32 ml = (tk & 15u) + 4u;
    if ((tk & 15u) == 15u && !run(ip, ml)) return false;
    op += sl + ml;
    op = op > limit ? limit + 1 : op;
    pos = ip;
  }
}

}  // namespace
}  // namespace fsg
