// deflate_format.h -- the deflate streams this project WRITES (raw, zlib, gzip
// bodies; include/flare_deflate_compress_gpu.h, fsg_deflate_batch), in plain C++: the
// unit rule, the hash and the window parse, the length and distance symbols,
// code construction and limiting, the dynamic header, the three block sizes
// and the choice, the wrappers and the slot bound.  One text for three users,
// as inflate_format.h is for the reading side: the device encoder
// (deflate.hip), the host model (host/deflate_cpu.cc, the definition of the
// bytes) and tests/cpp/deflate_check.cc.  Every stream is legal under RFC
// 1950 / 1951 / 1952; the bytes are ours, not zlib's (DESIGN.md section 4,
// "Deflate compress").
//
// The stream.
//   Units.  A body is cut into units of kUnit input bytes, the last one
//   shorter; an empty body is one empty unit.  No match reaches below its
//   unit's first byte, so units are compressed independently.
//   Blocks.  A unit is one deflate block -- stored, fixed or dynamic,
//   choose_block() says which -- that starts on a byte boundary.  A coded
//   block that is not the body's last is followed by an empty stored block
//   (three zero bits, zero bits to the byte, 00 00 FF FF), which restores the
//   boundary; a stored block ends on one by itself.  The last unit's block
//   has BFINAL set and is padded with zero bits.  A unit's output is
//   therefore a byte string and a body is the concatenation of its units'.
//   Parse.  Positions are taken in aligned windows of 64.  A position with 4
//   bytes left in the unit hashes them and reads one candidate from a
//   position table that holds every position of the EARLIER windows (highest
//   position per slot); its match length is the common prefix with the
//   candidate, at most 258 and at most the bytes left, valid from 4 bytes and
//   up to distance 32,768.  The tokens are the greedy chain: from the current
//   position, a match moves by its length, a literal by 1; a match that
//   crosses the window's end sets the next window's first position.  All
//   positions of a window are inserted after it, in ascending order.
//   Levels.  That is level 1, what fsg_deflate_batch writes.  Level 0 (stored
//   units only) and level 2 (another parse, everything else unchanged) are
//   stated at "levels" below.
//
// Lanes.  Functions with (lane, nlanes) are called by the host with (0, 1) and
// by all 64 lanes of a wave together, arrays in LDS, under the rules
// inflate_format.h states: wave-uniform control flow, same value where all
// lanes write one address, independent loops strided by lane; what is serial
// (the merge, the length counts, the header's run lengths) is done by lane 0
// alone between two fences.  Between two such calls the device places a
// fence; the calls themselves place the ones they need inside.
#pragma once

#include "inflate_format.h"

#if defined(DEFL_ADD)
// the includer's own (tests/cpp/deflate_check.cc emulates the lanes with threads)
#elif defined(__HIP_DEVICE_COMPILE__)
#define DEFL_ADD(p, v) __hip_atomic_fetch_add((p), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)
#define DEFL_OR(p, v) __hip_atomic_fetch_or((p), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)
#else
#define DEFL_ADD(p, v) (*(p) += (v))
#define DEFL_OR(p, v) (*(p) |= (v))
#endif

namespace defl {

using infl::kGzip;
using infl::kRaw;
using infl::kZlib;

// ---- units, windows, matches
constexpr uint32_t kUnit = 65472;  // a multiple of 64, above 32,768, one stored block (LEN is 16 bits)
constexpr uint32_t kWindow = 64;
constexpr uint32_t kHashBits = 13, kTableEntries = 1u << kHashBits;
constexpr uint32_t kNoPos = 0xffffu;  // an empty table slot: no unit position reaches it
constexpr uint32_t kMinMatch = 4, kMaxMatch = 258, kMaxDist = 32768;
static_assert(kUnit % kWindow == 0 && kUnit > kMaxDist && kUnit <= 65535 && kUnit <= kNoPos, "unit rule");

// ---- the slot bound: n + 5 per unit + the wrapper (0 for an unknown format)
INFL_HD uint32_t wrapper_head(uint32_t format) { return format == kZlib ? 2u : format == kGzip ? 10u : 0u; }
INFL_HD uint32_t wrapper_tail(uint32_t format) { return format == kZlib ? 4u : format == kGzip ? 8u : 0u; }
INFL_HD uint64_t unit_count(uint64_t n) { return n == 0 ? 1 : (n + kUnit - 1) / kUnit; }
INFL_HD uint64_t max_length(uint64_t n, uint32_t format) {
  if (format > kGzip) return 0;
  return n + 5 * unit_count(n) + wrapper_head(format) + wrapper_tail(format);
}

// The wrapper's first bytes into h (wrapper_head(format) of them).  zlib: CM 8,
// CINFO 7, FLEVEL 0, no FDICT, FCHECK so that the pair is a multiple of 31.
// gzip: no flags, no mtime, XFL 0, OS 3.
INFL_HD void write_wrapper_head(uint32_t format, uint8_t* h) {
  if (format == kZlib) {
    h[0] = 0x78;
    h[1] = 0x01;
  } else if (format == kGzip) {
    h[0] = 0x1f;
    h[1] = 0x8b;
    h[2] = 8;
    for (uint32_t i = 3; i < 9; ++i) h[i] = 0;
    h[9] = 3;
  }
}
// The trailer (wrapper_tail(format) bytes): big-endian Adler-32, or
// little-endian CRC-32 and the length mod 2^32.  sum: the checksum of the input.
INFL_HD void write_wrapper_tail(uint32_t format, uint32_t sum, uint32_t isize, uint8_t* t) {
  if (format == kZlib) {
    for (uint32_t i = 0; i < 4; ++i) t[i] = (uint8_t)(sum >> (24 - 8 * i));
  } else if (format == kGzip) {
    for (uint32_t i = 0; i < 4; ++i) {
      t[i] = (uint8_t)(sum >> (8 * i));
      t[4 + i] = (uint8_t)(isize >> (8 * i));
    }
  }
}

// ---- symbols (the inverse of infl::length_base / dist_base)
INFL_HD uint32_t log2_floor(uint32_t v) { return 31u - (uint32_t)__builtin_clz(v); }
INFL_HD uint32_t length_symbol(uint32_t len) {  // len 3 .. 258
  if (len == 258) return 285;
  const uint32_t l = len - 3;
  if (l < 8) return 257 + l;
  const uint32_t e = log2_floor(l) - 2;
  return 261 + 4 * e + ((l >> e) & 3u);
}
INFL_HD uint32_t dist_symbol(uint32_t dist) {  // dist 1 .. 32768
  const uint32_t d = dist - 1;
  if (d < 4) return d;
  const uint32_t hb = log2_floor(d);
  return 2 * hb + ((d >> (hb - 1)) & 1u);
}

// ---- tokens: a literal (kTokLit | byte), a match (length | distance << 9),
// or the end of the block (kTokEnd), which closes every unit's token list
constexpr uint32_t kTokLit = 0x80000000u, kTokEnd = 0x40000000u;
INFL_HD uint32_t tok_length(uint32_t t) { return t & 511u; }
INFL_HD uint32_t tok_dist(uint32_t t) { return (t >> 9) & 0x1ffffu; }
INFL_HD uint32_t tok_advance(uint32_t t) { return (t & kTokLit) ? 1u : tok_length(t); }

INFL_HD uint32_t hash4(uint32_t four) { return (four * 2654435761u) >> (32 - kHashBits); }

// The token at unit position p < n.  R reads the unit: load32(q) = the bytes
// q .. q+3, little endian (what it returns for bytes at or past n is never
// used).  table: kTableEntries positions, the state before p's window.
template <class R>
INFL_HD uint32_t token_at(const R& rd, uint32_t n, uint32_t p, const uint16_t* table) {
  const uint32_t mine = rd.load32(p);
  const uint32_t lit = kTokLit | (mine & 0xffu);
  if (n - p < kMinMatch) return lit;
  const uint32_t c = table[hash4(mine)];
  if (c == kNoPos || p - c > kMaxDist) return lit;
  const uint32_t limit = n - p < kMaxMatch ? n - p : kMaxMatch;
  uint32_t k = 0;
  while (k < limit) {
    const uint32_t x = rd.load32(p + k) ^ rd.load32(c + k);
    if (x) {
      k += (uint32_t)__builtin_ctz(x) >> 3;
      break;
    }
    k += 4;
  }
  if (k > limit) k = limit;
  return k >= kMinMatch ? (k | (p - c) << 9) : lit;
}

// ---- levels.  Level 1 is the stream above.  Level 0 writes every unit as a
// stored block, with no parse and no code build: a body's length is exactly
// max_length(n, format).  Level 2 keeps units, blocks, choice, codes, header,
// emit, wrappers and bound; only the parse differs:
//   Table.  kTableEntries 32-bit words: the low half is the newer candidate
//   position of the slot, the high half the older one, kNoPos in a half that
//   is empty.  The hash is hash4.
//   Token.  Both candidates are tried under level 1's validity rule; each
//   one's length is the common prefix, at most 258 and the bytes left.  The
//   longer wins, the newer (nearer) on equal lengths; a match from 4 bytes on.
//   One lazy step.  With r[] the window's tokens as just defined, position i
//   becomes the literal of its byte when r[i] is a match, i + 1 lies in the
//   same window, r[i + 1] is a match and longer than r[i].  The decision
//   reads the undeferred r[i + 1]; the window's last position never defers.
//   The greedy chain then walks the deferred tokens as at level 1.
//   Insert.  After the window, every slot that a position of the window (4
//   bytes left) hashes to becomes insert_word(old, highest such position):
//   one new entry per slot and window, the previous older candidate drops out.
constexpr uint32_t kLevelStored = 0, kLevelFast = 1, kLevelBest = 2, kMaxLevel = 2;
constexpr uint32_t kEmptyPair = kNoPos | kNoPos << 16;

// The common prefix of the unit's bytes at p and at c < p, at most limit.
template <class R>
INFL_HD uint32_t common_prefix(const R& rd, uint32_t p, uint32_t c, uint32_t limit) {
  uint32_t k = 0;
  while (k < limit) {
    const uint32_t x = rd.load32(p + k) ^ rd.load32(c + k);
    if (x) {
      k += (uint32_t)__builtin_ctz(x) >> 3;
      break;
    }
    k += 4;
  }
  return k > limit ? limit : k;
}

// Level 2's token at unit position p < n, before the lazy step.  table: the
// kTableEntries words of the state before p's window.  *four: the bytes
// p .. p+3.  *word: the slot's word when p has 4 bytes left (what insert_word
// takes after the window), else untouched.  The second compare is skipped
// when the first reached the limit: an equal length would lose to it.
template <class R>
INFL_HD uint32_t token_at2(const R& rd, uint32_t n, uint32_t p, const uint32_t* table, uint32_t* four,
                           uint32_t* word) {
  const uint32_t mine = rd.load32(p);
  *four = mine;
  const uint32_t lit = kTokLit | (mine & 0xffu);
  if (n - p < kMinMatch) return lit;
  const uint32_t w = table[hash4(mine)];
  *word = w;
  const uint32_t newer = w & 0xffffu, older = w >> 16;
  const uint32_t limit = n - p < kMaxMatch ? n - p : kMaxMatch;
  uint32_t k = 0, c = newer;
  if (newer != kNoPos && p - newer <= kMaxDist) k = common_prefix(rd, p, newer, limit);
  if (k < limit && older != kNoPos && p - older <= kMaxDist) {
    const uint32_t k1 = common_prefix(rd, p, older, limit);
    if (k1 > k) {
      k = k1;
      c = older;
    }
  }
  return k >= kMinMatch ? (k | (p - c) << 9) : lit;
}

// The lazy step: position i's token from r = r[i] and next = r[i + 1]
// (has_next: i + 1 is a position of the same window); byte: the byte at i.
INFL_HD uint32_t defer_token(uint32_t r, uint32_t next, bool has_next, uint32_t byte) {
  const bool defer = has_next && !(r & kTokLit) && !(next & kTokLit) && tok_length(next) > tok_length(r);
  return defer ? (kTokLit | (byte & 0xffu)) : r;
}

// The slot's word after a window whose highest position in the slot is p.
INFL_HD uint32_t insert_word(uint32_t old, uint32_t p) { return (old & 0xffffu) << 16 | p; }

// ---- the arrays of one unit's code build (LDS on the device, 8 KiB)
constexpr uint32_t kLitSyms = 286, kDistSyms = 30, kClSyms = 19;
constexpr uint32_t kDistBase = 288;  // distance symbol d is entry kDistBase + d (the layout of the fixed code)
constexpr uint32_t kSyms = 320;
constexpr uint32_t kMaxNodes = 2 * kLitSyms;

struct Build {
  uint32_t hist[kSyms];        // symbol counts: literal/length 0 .. 285, distance at kDistBase
  uint32_t nfreq[kMaxNodes];   // tree nodes: the leaves in sorted order, then the merged nodes
  uint16_t parent[kMaxNodes];
  uint16_t order[kSyms];       // the used symbols by (frequency, symbol)
  uint16_t code[kSyms];        // bit-reversed codes, as they go into the stream
  uint16_t cl_seq[kSyms];      // the header's code-length symbols: symbol | extra value << 5
  uint8_t depth[kMaxNodes];
  uint8_t len[kSyms];          // code lengths, the layout of hist
  uint32_t cl_hist[kClSyms + 1];
  uint16_t cl_code[kClSyms + 1];
  uint8_t cl_len[kClSyms + 1];
  uint32_t count[16];          // codes of each length
  uint32_t first[16];          // a length's first rank (build_lengths) or first code (assign_codes)
  uint32_t n_seq, hlit, hdist, hclen;
  uint32_t limited;            // literal/length and distance code sets of this unit the 15-bit limiter changed
};

// Code lengths of at most maxbits for the n symbols with counts freq[] into
// len[0 .. n); unused symbols get 0.  At least two symbols get a code: with
// fewer than two in use, symbol 0 and then symbol 1 are counted once (those
// not in use already), as zlib's build_tree forces two codes, so the set is
// complete with every length >= 1 and the decoder's single-code exception is
// never met.  The code is Huffman's where its depth fits; where it does not,
// the lengths above maxbits are cut to it and the Kraft sum is repaired by
// moving one code of the longest shorter length down for each unit of excess.
// Sorting is by (frequency, symbol), the merge prefers a leaf on equal
// weight, lengths go to the symbols in sorted order, longest first: integers
// only, one result on every machine.
INFL_HD void build_lengths(const uint32_t* freq, uint32_t n, uint32_t maxbits, uint8_t* len, Build* b, uint32_t lane,
                           uint32_t nlanes) {
  // the forced symbols
  uint32_t used = 0, first_used = 0;
  for (uint32_t s = 0; s < n; ++s)
    if (freq[s]) {
      if (!used) first_used = s;
      ++used;
    }
  uint32_t fa = n, fb = n;
  if (used == 0) {
    fa = 0;
    fb = 1;
  } else if (used == 1) {
    fa = first_used == 0 ? 1 : 0;
  }
  const uint32_t m = used < 2 ? 2 : used;
  auto eff = [&](uint32_t s) { return freq[s] ? freq[s] : (s == fa || s == fb) ? 1u : 0u; };
  // rank sort: a symbol's place is the number of used symbols below it
  for (uint32_t s = lane; s < n; s += nlanes) {
    len[s] = 0;
    const uint32_t f = eff(s);
    if (!f) continue;
    uint32_t r = 0;
    for (uint32_t t = 0; t < n; ++t) {
      const uint32_t g = eff(t);
      r += (g && (g < f || (g == f && t < s))) ? 1u : 0u;
    }
    b->order[r] = (uint16_t)s;
    b->nfreq[r] = f;
  }
  INFL_FENCE();
  if (lane == 0) {  // the serial part: one lane
    // two-queue merge: leaves 0 .. m-1, merged nodes m .. 2m-2 in order of creation
    uint32_t i = 0, j = m, k = m;
    while (k < 2 * m - 1) {
      uint32_t pick[2];
      for (uint32_t q = 0; q < 2; ++q) {
        if (i < m && (j >= k || b->nfreq[i] <= b->nfreq[j]))
          pick[q] = i++;
        else
          pick[q] = j++;
      }
      b->nfreq[k] = b->nfreq[pick[0]] + b->nfreq[pick[1]];
      b->parent[pick[0]] = (uint16_t)k;
      b->parent[pick[1]] = (uint16_t)k;
      ++k;
    }
    // depths from the root down (a parent is created after its children), cut to 255
    b->depth[2 * m - 2] = 0;
    for (uint32_t x = 2 * m - 2; x-- > 0;) {
      const uint32_t d = b->depth[b->parent[x]] + 1u;
      b->depth[x] = (uint8_t)(d > 255 ? 255 : d);
    }
    // codes per length, the lengths above maxbits cut to it
    for (uint32_t l = 0; l < 16; ++l) b->count[l] = 0;
    uint64_t kraft = 0;  // in units of 2^-maxbits
    for (uint32_t x = 0; x < m; ++x) {
      uint32_t d = b->depth[x];
      if (d > maxbits) d = maxbits;
      b->count[d] += 1;
      kraft += 1ull << (maxbits - d);
    }
    const uint64_t full = 1ull << maxbits;
    if (kraft > full && maxbits == 15) b->limited += 1;
    while (kraft > full) {
      uint32_t l = maxbits - 1;
      while (l > 1 && b->count[l] == 0) --l;
      // one code of length l moves to l + 1 and takes a code of length maxbits
      // with it as its sibling: the sum falls by 2^-maxbits
      b->count[l] -= 1;
      b->count[l + 1] += 2;
      b->count[maxbits] -= 1;
      --kraft;
    }
    // lengths in sorted order: the rarest symbols get the longest codes
    uint32_t at = 0;
    for (uint32_t l = maxbits; l >= 1; --l) {
      b->first[l] = at;
      at += b->count[l];
    }
  }
  INFL_FENCE();
  for (uint32_t r = lane; r < m; r += nlanes) {
    uint32_t l = maxbits;
    while (l > 1 && r >= b->first[l] + b->count[l]) --l;
    len[b->order[r]] = (uint8_t)l;
  }
  INFL_FENCE();
}

// Canonical codes (RFC 1951, 3.2.2) of the lengths len[0 .. n), bit-reversed,
// into code[0 .. n).
INFL_HD void assign_codes(const uint8_t* len, uint32_t n, uint16_t* code, Build* b, uint32_t lane, uint32_t nlanes) {
  for (uint32_t l = lane; l < 16; l += nlanes) b->count[l] = 0;
  INFL_FENCE();
  for (uint32_t s = lane; s < n; s += nlanes)
    if (len[s]) DEFL_ADD(&b->count[len[s]], 1u);
  INFL_FENCE();
  if (lane == 0) {
    uint32_t c = 0;
    for (uint32_t l = 1; l <= 15; ++l) {
      b->first[l] = c;
      c = (c + b->count[l]) << 1;
    }
  }
  INFL_FENCE();
  for (uint32_t s = lane; s < n; s += nlanes) {
    const uint32_t l = len[s];
    if (!l) {
      code[s] = 0;
      continue;
    }
    uint32_t r = 0;
    for (uint32_t t = 0; t < s; ++t) r += len[t] == l ? 1u : 0u;
    code[s] = (uint16_t)infl::bitrev(b->first[l] + r, l);
  }
  INFL_FENCE();
}

// ---- the dynamic header (3.2.7).  The lengths of the HLIT literal/length and
// HDIST distance codes are one sequence; a run of zeros takes symbol 18 (11 to
// 138) or 17 (3 to 10) greedily, a run of one non-zero length its first
// entry and then symbol 16 (3 to 6) greedily, what is left goes one by one.
INFL_HD uint32_t cl_extra_bits(uint32_t sym) { return sym == 16 ? 2u : sym == 17 ? 3u : sym == 18 ? 7u : 0u; }

// After build_lengths for both code sets: hlit, hdist, the symbol sequence,
// its counts, the code-length code, hclen.  Returns the header's bits from
// HLIT on (the three block-header bits not counted).
INFL_HD uint32_t build_dynamic_header(Build* b, uint32_t lane, uint32_t nlanes) {
  uint32_t hlit = kLitSyms, hdist = kDistSyms;
  while (hlit > 257 && b->len[hlit - 1] == 0) --hlit;
  while (hdist > 1 && b->len[kDistBase + hdist - 1] == 0) --hdist;
  for (uint32_t s = lane; s <= kClSyms; s += nlanes) b->cl_hist[s] = 0;
  INFL_FENCE();
  const uint32_t total = hlit + hdist;
  auto seq = [&](uint32_t q) -> uint32_t { return q < hlit ? b->len[q] : b->len[kDistBase + q - hlit]; };
  if (lane == 0) {  // serial: one lane
    uint32_t n_seq = 0, q = 0;
    auto emit = [&](uint32_t sym, uint32_t extra) {
      b->cl_seq[n_seq++] = (uint16_t)(sym | extra << 5);
      b->cl_hist[sym] += 1;
    };
    while (q < total) {
      const uint32_t v = seq(q);
      uint32_t run = 1;
      while (q + run < total && seq(q + run) == v) ++run;
      if (v == 0) {
        uint32_t left = run;
        while (left >= 11) {
          const uint32_t r = left < 138 ? left : 138;
          emit(18, r - 11);
          left -= r;
        }
        if (left >= 3) {
          emit(17, left - 3);
          left = 0;
        }
        while (left--) emit(0, 0);
      } else {
        emit(v, 0);
        uint32_t left = run - 1;
        while (left >= 3) {
          const uint32_t r = left < 6 ? left : 6;
          emit(16, r - 3);
          left -= r;
        }
        while (left--) emit(v, 0);
      }
      q += run;
    }
    b->n_seq = n_seq;
    b->hlit = hlit;
    b->hdist = hdist;
  }
  INFL_FENCE();
  build_lengths(b->cl_hist, kClSyms, 7, b->cl_len, b, lane, nlanes);
  assign_codes(b->cl_len, kClSyms, b->cl_code, b, lane, nlanes);
  uint32_t hclen = kClSyms;
  while (hclen > 4 && b->cl_len[infl::cl_order(hclen - 1)] == 0) --hclen;
  uint32_t bits = 5 + 5 + 4 + 3 * hclen;
  for (uint32_t s = 0; s < kClSyms; ++s) bits += b->cl_hist[s] * (b->cl_len[s] + cl_extra_bits(s));
  if (lane == 0) b->hclen = hclen;
  INFL_FENCE();
  return bits;
}

// ---- sizes.  The bits of the unit's symbols (end of block included: the
// parse counts it) under the built code and under the fixed code: this lane's
// share, to be summed over the lanes.
INFL_HD void symbol_bits(const Build* b, uint32_t lane, uint32_t nlanes, uint32_t* dyn, uint32_t* fix) {
  uint32_t d = 0, f = 0;
  for (uint32_t s = lane; s < kLitSyms; s += nlanes) {
    const uint32_t c = b->hist[s], x = s > 256 ? infl::length_extra(s) : 0u;
    d += c * (b->len[s] + x);
    f += c * (infl::fixed_length(s) + x);
  }
  for (uint32_t s = lane; s < kDistSyms; s += nlanes) {
    const uint32_t c = b->hist[kDistBase + s], x = infl::dist_extra(s);
    d += c * (b->len[kDistBase + s] + x);
    f += c * (5 + x);
  }
  *dyn = d;
  *fix = f;
}

// The choice.  A unit of n bytes whose symbols take dyn_bits (header included)
// or fix_bits, both without the 3 block-header bits.  Of the two coded forms
// the shorter in bits, the fixed one on a tie; the coded form only if its
// bytes, the empty stored block behind a non-final unit included, are FEWER
// than the stored form's n + 5 (so stored on a tie: it decodes as a copy).
constexpr uint32_t kStored = 0, kFixed = 1, kDynamic = 2;
struct Choice {
  uint32_t type;
  uint32_t bytes;  // the unit's output
};
INFL_HD Choice choose_block(uint32_t n, bool last, uint32_t dyn_bits, uint32_t fix_bits) {
  const bool fixed = fix_bits <= dyn_bits;
  const uint32_t bits = 3 + (fixed ? fix_bits : dyn_bits);
  const uint32_t coded = last ? (bits + 7) / 8 : (bits + 3 + 7) / 8 + 4;
  if (coded < n + 5) return Choice{fixed ? kFixed : kDynamic, coded};
  return Choice{kStored, n + 5};
}

// The fixed code's lengths into b->len (288 + 32 entries, contiguous).
INFL_HD void fill_fixed_lengths(Build* b, uint32_t lane, uint32_t nlanes) {
  for (uint32_t s = lane; s < kSyms; s += nlanes) b->len[s] = (uint8_t)infl::fixed_length(s);
  INFL_FENCE();
}

// ---- bits.  The output window is an array of zeroed 32-bit words, bit k of
// the stream in word k / 32 at k % 32 (deflate's order on a little-endian
// machine).  Lanes OR their bits in: any order gives the same words.
INFL_HD void put_bits(uint32_t* win, uint32_t pos, uint64_t v, uint32_t nbits) {
  if (!nbits) return;
  const uint32_t w = pos >> 5, s = pos & 31u;
  const uint64_t lo = v << s;
  DEFL_OR(&win[w], (uint32_t)lo);
  if (s + nbits > 32) DEFL_OR(&win[w + 1], (uint32_t)(lo >> 32));
  if (s + nbits > 64) DEFL_OR(&win[w + 2], (uint32_t)(v >> (64 - s)));
}

// A token's bits under the codes of b (at most 48) and their count.
INFL_HD uint64_t token_bits(const Build* b, uint32_t tok, uint32_t* nbits) {
  if (tok & kTokLit) {
    const uint32_t s = tok & 0xffu;
    *nbits = b->len[s];
    return b->code[s];
  }
  if (tok & kTokEnd) {
    *nbits = b->len[256];
    return b->code[256];
  }
  const uint32_t len = tok_length(tok), dist = tok_dist(tok);
  const uint32_t ls = length_symbol(len), ds = dist_symbol(dist);
  uint64_t v = b->code[ls];
  uint32_t at = b->len[ls];
  v |= (uint64_t)(len - infl::length_base(ls)) << at;
  at += infl::length_extra(ls);
  v |= (uint64_t)b->code[kDistBase + ds] << at;
  at += b->len[kDistBase + ds];
  v |= (uint64_t)(dist - infl::dist_base(ds)) << at;
  at += infl::dist_extra(ds);
  *nbits = at;
  return v;
}

// The symbols a token counts: literal/length into hist[0 ..), distance at kDistBase.
INFL_HD void count_token(Build* b, uint32_t tok) {
  if (tok & kTokLit) {
    DEFL_ADD(&b->hist[tok & 0xffu], 1u);
  } else if (tok & kTokEnd) {
    DEFL_ADD(&b->hist[256], 1u);
  } else {
    DEFL_ADD(&b->hist[length_symbol(tok_length(tok))], 1u);
    DEFL_ADD(&b->hist[kDistBase + dist_symbol(tok_dist(tok))], 1u);
  }
}

// The block header of a coded block at bit 0 of the window: BFINAL, BTYPE and,
// for a dynamic block, the header build_dynamic_header prepared.  One caller
// (the device: one lane).  Returns the bits written: at most 3 + 14 + 57 +
// 316 * 14.
constexpr uint32_t kMaxHeaderBits = 3 + 14 + 57 + 316 * 14;
INFL_HD uint32_t write_block_header(const Build* b, uint32_t type, bool last, uint32_t* win) {
  uint32_t pos = 0;
  put_bits(win, pos, (last ? 1u : 0u) | type << 1, 3);
  pos += 3;
  if (type != kDynamic) return pos;
  put_bits(win, pos, (b->hlit - 257) | (b->hdist - 1) << 5 | (b->hclen - 4) << 10, 14);
  pos += 14;
  for (uint32_t i = 0; i < b->hclen; ++i, pos += 3) put_bits(win, pos, b->cl_len[infl::cl_order(i)], 3);
  for (uint32_t i = 0; i < b->n_seq; ++i) {
    const uint32_t sym = b->cl_seq[i] & 31u, extra = b->cl_seq[i] >> 5;
    put_bits(win, pos, b->cl_code[sym], b->cl_len[sym]);
    pos += b->cl_len[sym];
    put_bits(win, pos, extra, cl_extra_bits(sym));
    pos += cl_extra_bits(sym);
  }
  return pos;
}

// What follows a coded block's end-of-block code at bit `pos`: for the last
// unit zero bits to the byte, otherwise the empty stored block.  Returns the
// unit's length in bytes.
INFL_HD uint32_t write_block_tail(bool last, uint32_t pos, uint32_t* win) {
  if (last) return (pos + 7) / 8;
  pos = (pos + 3 + 7) & ~7u;
  put_bits(win, pos, 0xffff0000u, 32);
  return pos / 8 + 4;
}

// The five bytes in front of a stored unit's data.
INFL_HD void write_stored_head(uint32_t n, bool last, uint8_t* h) {
  h[0] = last ? 1 : 0;
  h[1] = (uint8_t)n;
  h[2] = (uint8_t)(n >> 8);
  h[3] = (uint8_t)~n;
  h[4] = (uint8_t)(~n >> 8);
}

}  // namespace defl
