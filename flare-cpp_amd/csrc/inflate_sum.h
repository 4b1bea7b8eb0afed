// inflate_sum.h -- CRC-32 and Adler-32 of one byte range by one wave: the
// checksum kernel of the inflate calls (inflate.hip) and of fsg_crc32_batch /
// fsg_adler32_batch.  infl::crc32_serial / adler32_serial (inflate_format.h)
// stay the serial text; these give the same words.
//
// Both cut the range into 16-byte pieces; piece k goes to lane k % 64, so a
// step of the wave is one coalesced 1 KiB read.  Only whole pieces are loaded
// with 16-byte loads and the last n % 16 bytes one by one, so no byte outside
// [p, p + n) is read; p may have any alignment (unaligned-access mode).
//
// CRC-32 (reflected 0xEDB88320).  For zlib's crc values crc(A || B) =
// crc(A) * x^(8 |B|) + crc(B) mod P.  A lane keeps S = the crc of its pieces
// as if nothing lay between them and its last piece ended the range: per
// piece S = S * x^(8 * 1024) + crc(piece), the piece's crc by a 256-entry LDS
// table; at the end S * x^(8 * (bytes after the lane's last piece)) is the
// lane's share, and the shares and the tail's crc add up (xor) over the wave.
//
// Adler-32.  s1 = 1 + sum b_j, s2 = n + sum (n - j) b_j mod 65521.  A piece
// at offset o adds (n - o) * (sum of its bytes) - sum j * b_j to s2; both
// partial sums are reduced mod 65521 at every piece (the largest term is
// 65,520 * 4,080 + 65,521 < 2^29), and the lanes' sums add up over the wave
// (64 * 65,520 < 2^23).
#pragma once

#include "inflate_format.h"
#include "snappy_device.h"

namespace fsg {
namespace {

__device__ __forceinline__ u32 wave_xor_all(u32 v) {
#pragma unroll
  for (int d = 32; d; d >>= 1) v ^= __shfl_xor(v, d, 64);
  return v;
}
__device__ __forceinline__ u32 wave_add_all(u32 v) {
#pragma unroll
  for (int d = 32; d; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

// tab[b] = the register after byte b from register 0; 64 lanes fill it
__device__ __forceinline__ void crc_table_init(u32* tab, u32 lane) {
#pragma unroll
  for (u32 k = 0; k < 4; ++k) tab[4 * lane + k] = infl::crc32_byte(0, 4 * lane + k);
  __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ u32 crc_piece(const u32* tab, const u32x4& v) {  // zlib's crc32 of the 16 bytes
  u32 reg = ~0u;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    reg ^= v[w];
#pragma unroll
    for (int b = 0; b < 4; ++b) reg = tab[reg & 0xffu] ^ (reg >> 8);
  }
  return ~reg;
}

__device__ __forceinline__ u32x4 sum_load16(const u8* p) {
  u32x4 v;
  __builtin_memcpy(&v, p, 16);
  return v;
}

// zlib's crc32(0, p, n) on all lanes.  The loop runs n / 1024 + 1 times at most.
__device__ __forceinline__ u32 wave_crc32(const u8* p, u32 n, const u32* tab, u32 lane) {
  const u32 pieces = n >> 4;
  constexpr u32 kStep = infl::CrcXpow8<10>::v;  // x^(8 * 1024)
  u32 s = 0, last = 0;
  for (u32 k = lane; k < pieces; k += 64) {
    s = infl::crc_mulmod(s, kStep) ^ crc_piece(tab, sum_load16(p + 16 * (size_t)k));
    last = k;
  }
  u32 c = 0;
  if (lane < pieces) c = infl::crc_mulmod(s, infl::crc_xpow8(n - 16 * (last + 1)));
  if (lane == 0 && (n & 15)) {
    u32 reg = ~0u;
    for (u32 i = pieces << 4; i < n; ++i) reg = tab[(reg ^ p[i]) & 0xffu] ^ (reg >> 8);
    c ^= ~reg;
  }
  return wave_xor_all(c);
}

// zlib's adler32(1, p, n) on all lanes.
__device__ __forceinline__ u32 wave_adler32(const u8* p, u32 n, u32 lane) {
  constexpr u32 M = infl::kAdlerMod;
  const u32 pieces = n >> 4;
  u32 a = 0, b = 0;
  for (u32 k = lane; k < pieces; k += 64) {
    const u32x4 v = sum_load16(p + 16 * (size_t)k);
    u32 psum = 0, wsum = 0;
#pragma unroll
    for (u32 j = 0; j < 16; ++j) {
      const u32 x = (v[j >> 2] >> (8 * (j & 3))) & 0xffu;
      psum += x;
      wsum += j * x;
    }
    a = (a + psum) % M;
    b = (b + ((n - 16 * k) % M) * psum + M - wsum) % M;
  }
  if (lane == 0) {
    for (u32 i = pieces << 4; i < n; ++i) {
      a += p[i];
      b += (n - i) * p[i];
    }
  }
  const u32 s1 = (1 + wave_add_all(a)) % M;
  const u32 s2 = (n % M + wave_add_all(b)) % M;
  return s2 << 16 | s1;
}

}  // namespace
}  // namespace fsg
