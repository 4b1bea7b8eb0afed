// gzip_index.h -- the unit index of a gzip body, in plain C++ for the device
// (inflate_units.hip, deflate.hip), the host model (host/gzip_index_cpu.cc,
// host/deflate_cpu.cc) and tests/cpp/gzip_index_check.cc.
// include/flare_deflate_index_gpu.h is the public statement.
//
// The index is dictzip's `RA` random-access subfield of the gzip header's
// extra field (RFC 1952, 2.3.1.1): FLG.FEXTRA is set, the XLEN bytes hold a
// chain of subfields SI1 SI2 LEN(2) data, and the index is the FIRST subfield
// with SI1 = 'R', SI2 = 'A'.  Its data:
//   VER(2) = 1   CHLEN(2)   CHCNT(2)   CHCNT x size(2)      all little endian
// CHLEN is the decoded length of every unit but the last, size k the
// compressed length of unit k.  Unit k starts at begin + sum(size[< k]), where
// begin is the first byte of the deflate stream (parse_wrapper), and its
// output starts at k * CHLEN.  The last size entry places nothing.
//
// An index is USABLE when the chain up to it is well-formed inside XLEN,
// VER == 1, CHLEN >= 1, CHCNT >= 1, LEN == 6 + 2 * CHCNT and
// begin + sum(size[0 .. CHCNT-2]) <= n - 8.  A body whose chain breaks before
// an RA subfield was seen, or whose first RA subfield misses one of these, has
// an UNUSABLE index; one without FEXTRA or without an RA subfield has NO
// index.  Neither is an error: every inflate skips the extra field, and so
// does the decision which bytes and which verdict a body gets.
//
// What a writer of this project puts in front of the deflate stream
// (FSG_DEFLATE_FLAG_UNIT_INDEX): head_bytes(units) = 22 + 2 * units bytes,
//   1f 8b 08 04  00 00 00 00  00 03   XLEN = 10 + 2 * units
//   'R' 'A'  LEN = 6 + 2 * units  VER = 1  CHLEN = 65,472  CHCNT = units  sizes
// XLEN is 16 bits wide, so a body of more than kMaxUnits units is written
// without the index (the plain 10-byte head).
#pragma once

#include "inflate_format.h"

namespace gzidx {

constexpr uint32_t kFlagUnitIndex = 1;  // FSG_DEFLATE_FLAG_UNIT_INDEX
constexpr uint32_t kMaxUnits = 32762;   // 10 + 2 * units <= 65,535
constexpr uint32_t kNone = 0, kUnusable = 1, kUsable = 2;

INFL_HD uint32_t rd16(const uint8_t* p) { return p[0] | (uint32_t)p[1] << 8; }
INFL_HD void wr16(uint8_t* p, uint32_t v) {
  p[0] = (uint8_t)v;
  p[1] = (uint8_t)(v >> 8);
}

struct Head {
  uint32_t state;     // kNone, kUnusable, or kUsable once placed() holds as well
  uint32_t chlen, chcnt;
  uint32_t sizes_at;  // the first size entry's byte in the body
};

// Every rule but the last (the sum) for a gzip body p[0 .. n) whose wrapper
// parse_wrapper accepted, so the XLEN bytes lie inside the body.
INFL_HD Head find_head(const uint8_t* p) {
  Head h{kNone, 0, 0, 0};
  if (!(p[3] & 4)) return h;
  uint32_t at = 12;
  const uint32_t end = at + rd16(p + 10);
  while (at < end) {
    h.state = kUnusable;  // a chain that breaks here
    if (end - at < 4) return h;
    const uint32_t len = rd16(p + at + 2);
    if (end - at - 4 < len) return h;
    if (p[at] == 'R' && p[at + 1] == 'A') {
      if (len < 6) return h;
      const uint32_t ver = rd16(p + at + 4);
      h.chlen = rd16(p + at + 6);
      h.chcnt = rd16(p + at + 8);
      h.sizes_at = at + 10;
      if (ver != 1 || h.chlen == 0 || h.chcnt == 0 || len != 6 + 2 * h.chcnt) return h;
      h.state = kUsable;
      return h;
    }
    at += 4 + len;
    h.state = kNone;
  }
  return h;
}

INFL_HD uint32_t size_at(const uint8_t* p, const Head& h, uint32_t k) { return rd16(p + h.sizes_at + 2 * k); }

// The sum rule.  before_last = sum(size[0 .. CHCNT-2]), at most 32,761 * 65,535.
INFL_HD bool placed(uint32_t begin, uint64_t before_last, uint64_t n) { return n >= 8 && begin + before_last <= n - 8; }

// ---- the writer's side
INFL_HD bool writes_index(uint32_t format, uint32_t flags, uint64_t units) {
  return format == infl::kGzip && (flags & kFlagUnitIndex) && units <= kMaxUnits;
}
INFL_HD uint32_t head_bytes(uint32_t units) { return 22 + 2 * units; }
// The 22 bytes in front of the sizes.
INFL_HD void write_head(uint32_t units, uint32_t chlen, uint8_t* h) {
  h[0] = 0x1f;
  h[1] = 0x8b;
  h[2] = 8;
  h[3] = 4;  // FEXTRA
  for (uint32_t i = 4; i < 8; ++i) h[i] = 0;
  h[8] = 0;
  h[9] = 3;
  wr16(h + 10, 10 + 2 * units);
  h[12] = 'R';
  h[13] = 'A';
  wr16(h + 14, 6 + 2 * units);
  wr16(h + 16, 1);
  wr16(h + 18, chlen);
  wr16(h + 20, units);
}

}  // namespace gzidx
