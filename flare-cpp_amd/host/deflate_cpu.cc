// deflate_cpu.cc -- see deflate_cpu.h.  A serial reading of
// csrc/deflate_format.h: every rule is a function of that header called with
// (lane, nlanes) = (0, 1); what is written here is only the order of the
// steps, which csrc/deflate.hip follows phase by phase.
#include "deflate_cpu.h"

#include <cstdlib>
#include <cstring>
#include <vector>

#include "../csrc/deflate_format.h"
#include "../csrc/gzip_index.h"
#include "inflate_cpu.h"

namespace {

using namespace defl;

struct UnitReader {
  const uint8_t* p;
  uint32_t n;
  uint32_t load32(uint32_t q) const {
    uint32_t v = 0;
    if (q + 4 <= n) {
      memcpy(&v, p + q, 4);
      return v;
    }
    for (uint32_t i = 0; i < 4 && q + i < n; ++i) v |= (uint32_t)p[q + i] << (8 * i);
    return v;
  }
};

struct Scratch {
  uint16_t table[kTableEntries];
  uint32_t pairs[kTableEntries];  // level 2's table
  Build b;
  std::vector<uint32_t> tokens, win;
};

// Phase 1: the window parse.  Tokens (the end-of-block token last) and symbol counts.
void parse_unit(const UnitReader& rd, Scratch& s) {
  for (uint32_t i = 0; i < kTableEntries; ++i) s.table[i] = (uint16_t)kNoPos;
  memset(&s.b, 0, sizeof s.b);
  s.tokens.clear();
  const uint32_t n = rd.n;
  uint32_t entry = 0;
  for (uint32_t base = 0; base < n; base += kWindow) {
    const uint32_t cnt = n - base < kWindow ? n - base : kWindow;
    uint32_t rec[kWindow];
    for (uint32_t i = 0; i < cnt; ++i) rec[i] = token_at(rd, n, base + i, s.table);
    uint32_t cur = entry;
    while (cur < cnt) {
      s.tokens.push_back(rec[cur]);
      count_token(&s.b, rec[cur]);
      cur += tok_advance(rec[cur]);
    }
    entry = cur - cnt;  // 0 in the last window: no token passes the unit's end
    for (uint32_t i = 0; i < cnt; ++i)
      if (n - (base + i) >= kMinMatch) s.table[hash4(rd.load32(base + i))] = (uint16_t)(base + i);
  }
  s.tokens.push_back(kTokEnd);
  count_token(&s.b, kTokEnd);
}

// Phase 1 at level 2: two candidates per slot and one lazy step inside the
// window (deflate_format.h, "levels").
void parse_unit2(const UnitReader& rd, Scratch& s) {
  for (uint32_t i = 0; i < kTableEntries; ++i) s.pairs[i] = kEmptyPair;
  memset(&s.b, 0, sizeof s.b);
  s.tokens.clear();
  const uint32_t n = rd.n;
  uint32_t entry = 0;
  for (uint32_t base = 0; base < n; base += kWindow) {
    const uint32_t cnt = n - base < kWindow ? n - base : kWindow;
    uint32_t r[kWindow + 1], rec[kWindow], four[kWindow], word[kWindow];
    for (uint32_t i = 0; i < cnt; ++i) r[i] = token_at2(rd, n, base + i, s.pairs, &four[i], &word[i]);
    r[cnt] = kTokLit;
    for (uint32_t i = 0; i < cnt; ++i) rec[i] = defer_token(r[i], r[i + 1], i + 1 < cnt, four[i]);
    uint32_t cur = entry;
    while (cur < cnt) {
      s.tokens.push_back(rec[cur]);
      count_token(&s.b, rec[cur]);
      cur += tok_advance(rec[cur]);
    }
    entry = cur - cnt;
    // every word comes from the state before the window; the highest position of a slot lands last
    for (uint32_t i = 0; i < cnt; ++i)
      if (n - (base + i) >= kMinMatch) s.pairs[hash4(four[i])] = insert_word(word[i], base + i);
  }
  s.tokens.push_back(kTokEnd);
  count_token(&s.b, kTokEnd);
}

void write_stored_unit(const uint8_t* in, uint32_t n, bool last, std::vector<uint8_t>* out) {
  uint8_t h[5];
  write_stored_head(n, last, h);
  out->insert(out->end(), h, h + 5);
  out->insert(out->end(), in, in + n);
}

// Phases 2 and 3 for one unit; its bytes are appended to out.
uint32_t compress_unit(uint32_t level, const uint8_t* in, uint32_t n, bool last, Scratch& s,
                       std::vector<uint8_t>* out) {
  if (level == kLevelStored) {
    if (out) write_stored_unit(in, n, last, out);
    return kStored;
  }
  const UnitReader rd{in, n};
  if (level == kLevelBest)
    parse_unit2(rd, s);
  else
    parse_unit(rd, s);
  Build* b = &s.b;
  build_lengths(b->hist, kLitSyms, 15, b->len, b, 0, 1);
  build_lengths(b->hist + kDistBase, kDistSyms, 15, b->len + kDistBase, b, 0, 1);
  const uint32_t header = build_dynamic_header(b, 0, 1);
  uint32_t dyn, fix;
  symbol_bits(b, 0, 1, &dyn, &fix);
  const Choice c = choose_block(n, last, dyn + header, fix);
  if (!out) return c.type;
  if (c.type == kStored) {
    write_stored_unit(in, n, last, out);
    return c.type;
  }
  if (c.type == kFixed) {
    fill_fixed_lengths(b, 0, 1);
    assign_codes(b->len, infl::kFixedLens, b->code, b, 0, 1);
    assign_codes(b->len + kDistBase, infl::kFixedDists, b->code + kDistBase, b, 0, 1);
  } else {
    assign_codes(b->len, kLitSyms, b->code, b, 0, 1);
    assign_codes(b->len + kDistBase, kDistSyms, b->code + kDistBase, b, 0, 1);
  }
  s.win.assign(c.bytes / 4 + 4, 0);
  uint32_t pos = write_block_header(b, c.type, last, s.win.data());
  for (const uint32_t t : s.tokens) {
    uint32_t nb;
    const uint64_t v = token_bits(b, t, &nb);
    put_bits(s.win.data(), pos, v, nb);
    pos += nb;
  }
  const uint32_t bytes = write_block_tail(last, pos, s.win.data());
  if (bytes != c.bytes) abort();  // the size formulas and the writer disagree
  const uint8_t* w = reinterpret_cast<const uint8_t*>(s.win.data());
  out->insert(out->end(), w, w + bytes);
  return c.type;
}

}  // namespace

extern "C" {

size_t fsh_cpu_deflate_bound(size_t n, uint32_t format) { return (size_t)defl::max_length(n, format); }

int fsh_cpu_deflate(uint32_t format, const void* in, size_t n, void* out, size_t cap, uint64_t* len) {
  return fsh_cpu_deflate_level(format, kLevelFast, in, n, out, cap, len);
}

int fsh_cpu_deflate_level(uint32_t format, uint32_t level, const void* in, size_t n, void* out, size_t cap,
                          uint64_t* len) {
  return fsh_cpu_deflate_flags(format, level, 0, in, n, out, cap, len);
}

size_t fsh_cpu_deflate_bound_flags(size_t n, uint32_t format, uint32_t flags) {
  if (format > kGzip || (flags & ~gzidx::kFlagUnitIndex) || (flags && format != kGzip)) return 0;
  const uint64_t units = unit_count(n);
  return (size_t)(max_length(n, format) +
                  (gzidx::writes_index(format, flags, units) ? gzidx::head_bytes((uint32_t)units) - 10 : 0));
}

int fsh_cpu_deflate_flags(uint32_t format, uint32_t level, uint32_t flags, const void* in_, size_t n, void* out_,
                          size_t cap, uint64_t* len) {
  *len = 0;
  if (format > kGzip || level > kMaxLevel) return infl::kStCorrupt;
  if ((flags & ~gzidx::kFlagUnitIndex) || (flags && format != kGzip)) return infl::kStCorrupt;
  const uint8_t* in = static_cast<const uint8_t*>(in_);
  const uint64_t units = unit_count(n);
  const bool index = gzidx::writes_index(format, flags, units);
  const uint32_t head = index ? gzidx::head_bytes((uint32_t)units) : wrapper_head(format);
  std::vector<uint8_t> body(head);
  if (index)
    gzidx::write_head((uint32_t)units, kUnit, body.data());
  else
    write_wrapper_head(format, body.data());
  std::vector<Scratch> scratch(1);
  for (uint64_t u = 0; u < units; ++u) {
    const uint64_t first = u * kUnit;
    const uint32_t un = (uint32_t)(n - first < kUnit ? n - first : kUnit);
    const size_t before = body.size();
    compress_unit(level, in + first, un, u + 1 == units, scratch[0], &body);
    if (index) gzidx::wr16(body.data() + 22 + 2 * u, (uint32_t)(body.size() - before));  // at most 65,477
  }
  uint8_t tail[8];
  const uint32_t sum = format == kZlib ? fsh_cpu_adler32(in, n) : format == kGzip ? fsh_cpu_crc32(in, n) : 0u;
  write_wrapper_tail(format, sum, (uint32_t)n, tail);
  body.insert(body.end(), tail, tail + wrapper_tail(format));
  if (body.size() > cap) return infl::kStSlotTooSmall;
  if (!body.empty()) memcpy(out_, body.data(), body.size());
  *len = body.size();
  return infl::kStOk;
}

void fsh_cpu_deflate_unit_types(const void* in, size_t n, uint64_t counts[3]) {
  fsh_cpu_deflate_unit_types_level(kLevelFast, in, n, counts);
}

void fsh_cpu_deflate_unit_types_level(uint32_t level, const void* in_, size_t n, uint64_t counts[3]) {
  if (level > kMaxLevel) return;
  const uint8_t* in = static_cast<const uint8_t*>(in_);
  std::vector<Scratch> scratch(1);
  const uint64_t units = unit_count(n);
  for (uint64_t u = 0; u < units; ++u) {
    const uint64_t first = u * kUnit;
    const uint32_t un = (uint32_t)(n - first < kUnit ? n - first : kUnit);
    ++counts[compress_unit(level, in + first, un, u + 1 == units, scratch[0], nullptr)];
  }
}

size_t fsh_cpu_deflate_tokens(const void* in, size_t n, uint32_t* tokens, size_t cap) {
  return fsh_cpu_deflate_tokens_level(kLevelFast, in, n, tokens, cap);
}

size_t fsh_cpu_deflate_tokens_level(uint32_t level, const void* in_, size_t n, uint32_t* tokens, size_t cap) {
  if (n > kUnit || level < kLevelFast || level > kMaxLevel) return 0;
  std::vector<Scratch> scratch(1);
  const UnitReader rd{static_cast<const uint8_t*>(in_), (uint32_t)n};
  if (level == kLevelBest)
    parse_unit2(rd, scratch[0]);
  else
    parse_unit(rd, scratch[0]);
  const size_t cnt = scratch[0].tokens.size() - 1;
  if (cnt > cap) return 0;
  if (cnt) memcpy(tokens, scratch[0].tokens.data(), cnt * 4);
  return cnt;
}

uint64_t fsh_cpu_deflate_limited(const void* in_, size_t n) {
  const uint8_t* in = static_cast<const uint8_t*>(in_);
  std::vector<Scratch> scratch(1);
  uint64_t limited = 0;
  const uint64_t units = unit_count(n);
  for (uint64_t u = 0; u < units; ++u) {
    const uint64_t first = u * kUnit;
    const uint32_t un = (uint32_t)(n - first < kUnit ? n - first : kUnit);
    compress_unit(kLevelFast, in + first, un, u + 1 == units, scratch[0], nullptr);
    limited += scratch[0].b.limited;
  }
  return limited;
}

}  // extern "C"
