// inflate_format.h -- deflate (RFC 1951) and its zlib (RFC 1950) and gzip
// (RFC 1952) wrappers in plain C++: the wrapper-header parsers, the code-set
// checks and the decode-table build, the length and distance base / extra
// rules, the dynamic block header, and the serial CRC-32 and Adler-32.  One
// text for three users: the device decoder (inflate.hip, where INFL_HD is
// __host__ __device__), the host model (host/inflate_cpu.cc, compiled by g++)
// and tests/cpp/inflate_check.cc, which runs the model under AddressSanitizer.
// include/flare_deflate_gpu.h states the acceptance rule: the verdicts are
// those of zlib 1.2.11's inflate.
//
// Lanes.  build_table and read_dynamic_header take (lane, nlanes).  The host
// passes (0, 1).  On the device all 64 lanes of a wave call them together with
// the same arguments and their own lane: control flow and every value that
// decides it are the same on all lanes (wave-uniform), the arrays live in LDS,
// lanes write the same value where they all write one address, and the loops
// over symbols or table entries that carry no dependency are strided by lane.
#pragma once

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define INFL_HD __host__ __device__ inline
#else
#define INFL_HD inline
#endif

#if defined(__HIP_DEVICE_COMPILE__)
// one wave: LDS accesses execute in issue order, the barrier pins the schedule
#define INFL_FENCE() __builtin_amdgcn_wave_barrier()
#define INFL_COUNT(p) __hip_atomic_fetch_add((p), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)
#else
#define INFL_FENCE() ((void)0)
#define INFL_COUNT(p) (++*(p))
#endif

namespace infl {

constexpr uint32_t kRaw = 0, kZlib = 1, kGzip = 2;  // FSG_INFLATE_*
constexpr int32_t kStOk = 0, kStCorrupt = 1, kStBadHeader = 2, kStSlotTooSmall = 3;

// zlib's proven table bounds (ENOUGH_LENS, ENOUGH_DISTS: root 9 and 6, 15-bit codes)
constexpr uint32_t kEnoughLens = 852, kEnoughDists = 592;
constexpr uint32_t kLenRoot = 9, kDistRoot = 6, kCodeRoot = 7;
constexpr uint32_t kMaxLens = 286, kMaxDists = 30;   // symbols a dynamic block may declare
constexpr uint32_t kFixedLens = 288, kFixedDists = 32;
constexpr uint32_t kLensArray = 320;                 // 288 + 32 >= 286 + 30
constexpr uint32_t kWindow = 32768;

enum TableType : uint32_t { kCodes = 0, kLens = 1, kDists = 2 };

// ---- decode-table entries: val | bits << 16 | op << 24
//   kOpLit        val = the literal byte (or the code-length symbol)
//   kOpBase | e   val = the length or distance base, e extra bits follow
//   kOpEnd        end of block
//   kOpBad        no symbol has this code (286, 287, distance 30, 31, the
//                 unused half of a single-code set)
//   kOpLink | b   val = offset of a sub-table indexed by the next b bits
// bits = what to drop for this entry (a link: the root bits).
constexpr uint32_t kOpLit = 0x00, kOpBase = 0x10, kOpEnd = 0x20, kOpBad = 0x40, kOpLink = 0x80;
INFL_HD uint32_t entry(uint32_t op, uint32_t bits, uint32_t val) { return val | bits << 16 | op << 24; }
INFL_HD uint32_t e_op(uint32_t e) { return e >> 24; }
INFL_HD uint32_t e_bits(uint32_t e) { return (e >> 16) & 0xffu; }
INFL_HD uint32_t e_val(uint32_t e) { return e & 0xffffu; }

// ---- length symbols 257..285 and distance symbols 0..29 (RFC 1951, 3.2.5)
INFL_HD uint32_t length_extra(uint32_t sym) { return sym < 265 || sym == 285 ? 0u : (sym - 261) >> 2; }
INFL_HD uint32_t length_base(uint32_t sym) {
  if (sym < 261) return sym - 254;
  if (sym == 285) return 258;
  return 3 + ((4 + ((sym - 261) & 3)) << ((sym - 261) >> 2));
}
INFL_HD uint32_t dist_extra(uint32_t sym) { return sym < 4 ? 0u : (sym >> 1) - 1; }
INFL_HD uint32_t dist_base(uint32_t sym) { return sym < 4 ? 1 + sym : 1 + ((2 + (sym & 1)) << ((sym >> 1) - 1)); }

// the order of the code-length code lengths: 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
INFL_HD uint32_t cl_order(uint32_t i) {
  constexpr uint64_t lo = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 |
                          6ull << 35 | 10ull << 40 | 5ull << 45 | 11ull << 50 | 4ull << 55;
  constexpr uint64_t hi = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
  return (uint32_t)((i < 12 ? lo >> (5 * i) : hi >> (5 * (i - 12))) & 31u);
}

// the fixed code's lengths (3.2.6): 288 literal/length symbols, then 32 distances
INFL_HD uint32_t fixed_length(uint32_t i) {
  return i < 144 ? 8u : i < 256 ? 9u : i < 280 ? 7u : i < 288 ? 8u : 5u;
}

INFL_HD uint32_t bitrev(uint32_t v, uint32_t n) {  // the low n (1..15) bits of v, reversed
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_bitreverse32(v) >> (32 - n);
#else
  uint32_t r = 0;
  for (uint32_t i = 0; i < n; ++i, v >>= 1) r = r << 1 | (v & 1);
  return r;
#endif
}

INFL_HD uint32_t symbol_entry(uint32_t type, uint32_t sym, uint32_t bits) {
  if (type == kCodes) return entry(kOpLit, bits, sym);
  if (type == kLens) {
    if (sym < 256) return entry(kOpLit, bits, sym);
    if (sym == 256) return entry(kOpEnd, bits, 0);
    if (sym < kMaxLens) return entry(kOpBase | length_extra(sym), bits, length_base(sym));
    return entry(kOpBad, bits, 0);
  }
  if (sym < kMaxDists) return entry(kOpBase | dist_extra(sym), bits, dist_base(sym));
  return entry(kOpBad, bits, 0);
}

// ---- the code-set checks and the table build (zlib's inflate_table: same
// verdicts, same table shape, so its proven bounds hold)
struct TableScratch {
  uint32_t count[16];  // symbols of each length
  uint32_t offs[16];   // first index of each length in `work`
  uint32_t first[16];  // first canonical code of each length
};
constexpr int kTableOk = 0, kTableOver = 1, kTableIncomplete = 2, kTableTooLarge = 3;

// Builds the decode table of the code whose lengths are lens[0 .. codes) into
// tab[0 .. cap): a root table of 2^root entries (root = *root_io clamped to
// the shortest and longest code, written back), then the sub-tables of the
// longer codes.  Verdicts: an over-subscribed set is kTableOver; an incomplete
// one is kTableIncomplete, except a single code of length 1 in a
// literal/length or distance set, whose other half reads kOpBad; a set with
// no code at all is accepted as two kOpBad entries (any use of it is an
// error; the code-length code with no code is rejected by the caller).
// work: `codes` entries.
INFL_HD int build_table(uint32_t type, const uint8_t* lens, uint32_t codes, uint32_t* tab, uint32_t cap,
                        uint32_t* root_io, uint16_t* work, TableScratch* s, uint32_t lane, uint32_t nlanes) {
  for (uint32_t l = lane; l < 16; l += nlanes) s->count[l] = 0;
  INFL_FENCE();
  for (uint32_t sym = lane; sym < codes; sym += nlanes) INFL_COUNT(&s->count[lens[sym]]);
  INFL_FENCE();
  uint32_t max = 15;
  while (max >= 1 && s->count[max] == 0) --max;
  if (max == 0) {
    tab[0] = tab[1] = entry(kOpBad, 1, 0);
    *root_io = 1;
    INFL_FENCE();
    return kTableOk;
  }
  uint32_t min = 1;
  while (s->count[min] == 0) ++min;
  uint32_t root = *root_io;
  if (root > max) root = max;
  if (root < min) root = min;
  int left = 1;
  for (uint32_t len = 1; len <= 15; ++len) {
    left <<= 1;
    left -= (int)s->count[len];
    if (left < 0) return kTableOver;
  }
  if (left > 0 && (type == kCodes || max != 1)) return kTableIncomplete;
  uint32_t code = 0, nsym = 0;
  for (uint32_t len = 1; len <= 15; ++len) {
    s->first[len] = code;
    s->offs[len] = nsym;
    nsym += s->count[len];
    code = (code + s->count[len]) << 1;
  }
  INFL_FENCE();
  // symbols in order of (length, symbol): one length per lane
  for (uint32_t len = 1 + lane; len <= 15; len += nlanes) {
    if (s->count[len] == 0) continue;
    uint32_t k = s->offs[len];
    for (uint32_t sym = 0; sym < codes; ++sym)
      if (lens[sym] == len) work[k++] = (uint16_t)sym;
  }
  INFL_FENCE();
  // codes no longer than the root: every one on its own, 2^(root - len) entries each
  const uint32_t nroot = root < 15 ? s->offs[root + 1] : nsym;
  for (uint32_t i = lane; i < nroot; i += nlanes) {
    const uint32_t sym = work[i], len = lens[sym];
    const uint32_t rev = bitrev(s->first[len] + (i - s->offs[len]), len);
    const uint32_t e = symbol_entry(type, sym, len);
    for (uint32_t k = rev; k < (1u << root); k += 1u << len) tab[k] = e;
  }
  if (left > 0) tab[1] = entry(kOpBad, 1, 0);  // the single code is tab[0], root is 1
  // longer codes, in order: a sub-table per root prefix, sized by zlib's rule
  // (grow it while the codes still to come do not complete it)
  uint32_t used = 1u << root, sub = 0, subbits = 0, prev = ~0u;
  for (uint32_t i = nroot; i < nsym; ++i) {
    const uint32_t sym = work[i], len = lens[sym], rank = i - s->offs[len];
    const uint32_t rev = bitrev(s->first[len] + rank, len);
    const uint32_t prefix = rev & ((1u << root) - 1);
    if (prefix != prev) {
      uint32_t curr = len - root;
      int lf = 1 << curr;
      for (uint32_t cl = len; cl < max; ++cl) {
        lf -= (int)(cl == len ? s->count[len] - rank : s->count[cl]);
        if (lf <= 0) break;
        ++curr;
        lf <<= 1;
      }
      sub = used;
      subbits = curr;
      used += 1u << curr;
      if (used > cap) return kTableTooLarge;
      tab[prefix] = entry(kOpLink | curr, root, sub);
      prev = prefix;
    }
    const uint32_t e = symbol_entry(type, sym, len - root);
    const uint32_t step = 1u << (len - root);
    for (uint32_t k = (rev >> root) + lane * step; k < (1u << subbits); k += nlanes * step) tab[sub + k] = e;
  }
  *root_io = root;
  INFL_FENCE();
  return kTableOk;
}

// ---- the dynamic block header (3.2.7).  R is a bit reader:
//   void need()             at least 32 bits are in the buffer (bytes past the input read 0)
//   uint32_t peek(n) / void drop(n) / uint32_t bits(n)      n <= 16
// Reads HLIT, HDIST, HCLEN, the code-length code and the nlen + ndist code
// lengths into lens[0 .. nlen + ndist).  codetab: 128 entries.  false: corrupt
// (too many symbols, a bad code-length code, a repeat with nothing to repeat
// or past the end, no end-of-block code).  Every step of the loop takes at
// least one bit, so it ends within 316 symbols whatever the input holds.
template <class R>
INFL_HD bool read_dynamic_header(R& r, uint8_t* lens, uint32_t* nlen_out, uint32_t* ndist_out, uint32_t* codetab,
                                 uint16_t* work, TableScratch* s, uint32_t lane, uint32_t nlanes) {
  r.need();
  const uint32_t nlen = r.bits(5) + 257, ndist = r.bits(5) + 1, ncode = r.bits(4) + 4;
  if (nlen > kMaxLens || ndist > kMaxDists) return false;
  for (uint32_t i = 0; i < 19; ++i) {
    if ((i & 7) == 0) r.need();
    lens[cl_order(i)] = (uint8_t)(i < ncode ? r.bits(3) : 0);
  }
  INFL_FENCE();
  uint32_t root = kCodeRoot;
  if (build_table(kCodes, lens, 19, codetab, 128, &root, work, s, lane, nlanes) != kTableOk) return false;
  uint32_t have = 0;
  const uint32_t total = nlen + ndist;
  while (have < total) {
    r.need();
    const uint32_t e = codetab[r.peek(root)];
    if (e_op(e) != kOpLit) return false;  // a code-length code without codes
    r.drop(e_bits(e));
    const uint32_t sym = e_val(e);
    if (sym < 16) {
      lens[have++] = (uint8_t)sym;
      continue;
    }
    uint32_t prevlen = 0, rep;
    if (sym == 16) {
      if (have == 0) return false;
      prevlen = lens[have - 1];
      rep = 3 + r.bits(2);
    } else if (sym == 17) {
      rep = 3 + r.bits(3);
    } else {
      rep = 11 + r.bits(7);
    }
    if (have + rep > total) return false;
    for (uint32_t k = 0; k < rep; ++k) lens[have + k] = (uint8_t)prevlen;
    have += rep;
    INFL_FENCE();
  }
  INFL_FENCE();
  if (lens[256] == 0) return false;
  *nlen_out = nlen;
  *ndist_out = ndist;
  return true;
}

// ---- serial checksums
constexpr uint32_t kCrcPoly = 0xEDB88320u;  // reflected
constexpr uint32_t kAdlerMod = 65521u;

INFL_HD uint32_t crc32_byte(uint32_t reg, uint32_t b) {  // the register, not the inverted value
  reg ^= b;
  for (int k = 0; k < 8; ++k) reg = (reg >> 1) ^ (kCrcPoly & (0u - (reg & 1u)));
  return reg;
}
INFL_HD uint32_t crc32_serial(uint32_t crc, const uint8_t* p, uint64_t n) {  // zlib's crc32(crc, p, n)
  uint32_t reg = ~crc;
  for (uint64_t i = 0; i < n; ++i) reg = crc32_byte(reg, p[i]);
  return ~reg;
}
INFL_HD uint32_t adler32_serial(uint32_t adler, const uint8_t* p, uint64_t n) {  // zlib's adler32(adler, p, n)
  uint32_t a = adler & 0xffffu, b = adler >> 16;
  uint64_t i = 0;
  while (i < n) {
    const uint64_t end = n - i > 5552 ? i + 5552 : n;  // 5552: the sums stay below 2^32
    for (; i < end; ++i) {
      a += p[i];
      b += a;
    }
    a %= kAdlerMod;
    b %= kAdlerMod;
  }
  return b << 16 | a;
}

// Polynomials mod P in the reflected form (bit 31 is x^0).  crc(A || B) =
// crc(A) * x^(8 |B|) + crc(B) for zlib's crc32 values, which is what lets
// the checksum kernel (inflate_sum.h) give each lane its own pieces.
INFL_HD uint32_t crc_mulmod(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (int k = 0; k < 32; ++k) {
    p ^= b & (0u - (a >> 31));
    a <<= 1;
    b = (b >> 1) ^ (kCrcPoly & (0u - (b & 1u)));
  }
  return p;
}
constexpr uint32_t crc_mulmod_c(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (int k = 0; k < 32; ++k) {
    p ^= b & (0u - (a >> 31));
    a <<= 1;
    b = (b >> 1) ^ (kCrcPoly & (0u - (b & 1u)));
  }
  return p;
}
// x^(8 * 2^J) mod P, a compile-time constant
template <int J>
struct CrcXpow8 {
  static constexpr uint32_t v = crc_mulmod_c(CrcXpow8<J - 1>::v, CrcXpow8<J - 1>::v);
};
template <>
struct CrcXpow8<0> {
  static constexpr uint32_t v = 0x00800000u;  // x^8
};
template <int J>
INFL_HD uint32_t crc_xpow8_from(uint64_t n, uint32_t r) {
  if ((n >> J) & 1) r = crc_mulmod(r, CrcXpow8<J>::v);
  if constexpr (J < 32) return crc_xpow8_from<J + 1>(n, r);
  return r;
}
// x^(8 n) mod P for n < 2^33: the product of the x^(8 * 2^j) of n's bits
INFL_HD uint32_t crc_xpow8(uint64_t n) { return crc_xpow8_from<0>(n, 0x80000000u); }

// ---- wrappers
struct Wrapper {
  int32_t status;    // kStOk or kStBadHeader
  uint32_t begin;    // first byte of the deflate stream
  uint32_t trailer;  // bytes after it: 0, 4 (Adler-32, big endian) or 8 (CRC-32, ISIZE, little endian)
};

// What zlib's inflate accepts as the head of a stream of `format`; a head cut
// short by the input's end is kStBadHeader too.
INFL_HD Wrapper parse_wrapper(uint32_t format, const uint8_t* p, uint64_t n) {
  Wrapper w{kStOk, 0, 0};
  if (format == kRaw) return w;
  w.status = kStBadHeader;
  if (format == kZlib) {
    w.trailer = 4;
    if (n < 2) return w;
    const uint32_t cmf = p[0], flg = p[1];
    if (((cmf << 8) + flg) % 31) return w;  // header check
    if ((cmf & 15) != 8) return w;          // CM
    if ((cmf >> 4) > 7) return w;           // CINFO: a window above 32 KiB
    if (flg & 0x20) return w;               // FDICT: no dictionaries here
    w.begin = 2;
    w.status = kStOk;
    return w;
  }
  w.trailer = 8;
  if (n < 10) return w;
  if (p[0] != 0x1f || p[1] != 0x8b || p[2] != 8) return w;
  const uint32_t flg = p[3];
  if (flg & 0xe0) return w;  // reserved bits
  uint64_t at = 10;
  if (flg & 4) {  // FEXTRA
    if (n < at + 2) return w;
    const uint64_t xlen = p[at] | (uint64_t)p[at + 1] << 8;
    at += 2;
    if (n - at < xlen) return w;
    at += xlen;
  }
  for (uint32_t bit = 8; bit <= 16; bit <<= 1) {  // FNAME, FCOMMENT: zero-terminated
    if (!(flg & bit)) continue;
    for (;;) {
      if (at >= n) return w;
      if (p[at++] == 0) break;
    }
  }
  if (flg & 2) {  // FHCRC: the low 16 bits of the CRC-32 of the header so far
    if (n - at < 2) return w;
    const uint32_t want = p[at] | (uint32_t)p[at + 1] << 8;
    if ((crc32_serial(0, p, at) & 0xffffu) != want) return w;
    at += 2;
  }
  w.begin = (uint32_t)at;
  w.status = kStOk;
  return w;
}

}  // namespace infl
