// l4wenc_model.cc -- CPU model of the LZ4 wave encoder
// (flare-cpp_amd/csrc/lz4_encode_wave.hip): the default LZ4 block compressor's
// greedy parse run 64 probes at a time, the per-lane quantities held in arrays
// of 64.  The kernel is written from this file; tests/test_lz4_wave_model.py
// builds it with AddressSanitizer and compares every block with
// oracle/lz4_oracle.c.
//
//   l4wenc_model IN OUT   : IN = records [u32 n][n bytes]; OUT = blocks [u32 len][bytes]
//   (the convention of tests/cpp/lz4_host_check.hip, mode c)
//
// Window: the 64 next probes of one match search.  Probe k reads the table
// slot of its hash and overwrites it with its own position, every probe, hit
// or miss; so probe k's candidate is the position of the highest probe j < k
// of the window with the same hash, else the table entry as of the window's
// start.  The first probe that hits, or whose successor passes mflimit + 1,
// ends the window; the probes up to and including a hit commit their table
// writes in position order (the highest probe wins a shared slot), a probe
// that ended the window at the limit does not.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

typedef uint8_t u8;
typedef uint16_t u16;
typedef uint32_t u32;
typedef uint64_t u64;

namespace {

constexpr u32 kW = 64;
constexpr u32 kMinMatch = 4, kMfLimit = 12, kLastLiterals = 5, kHashLog = 12, kSkipTrigger = 6;
constexpr u32 kDistanceMax = 65535, kLimit64K = 65536 + kMfLimit - 1;

struct Body {
  const u8* src;
  u32 n;
  // the kernel reads its input through a buffer descriptor: bytes past the body read 0
  u32 b(u64 p) const { return p < n ? src[p] : 0u; }
  u32 w4(u64 p) const { return b(p) | b(p + 1) << 8 | b(p + 2) << 16 | b(p + 3) << 24; }
};

// sum of (t >> 6) for t in [0, x)
u32 F(u32 x) {
  const u32 q = x >> kSkipTrigger, r = x & (kW - 1);
  return 32 * q * (q - 1) + r * q;
}

struct Table {
  bool small;
  u16 t16[8192];
  u32 t32[4096];
  void clear() {
    memset(t16, 0, sizeof(t16));
    memset(t32, 0, sizeof(t32));
  }
  u32 get(u32 h) const { return small ? (u32)t16[h] : t32[h]; }
  void put(u32 h, u32 v) {
    if (small) t16[h] = (u16)v;
    else t32[h] = v;
  }
  u32 hash(const Body& s, u32 p) const {
    const u32 lo = s.w4(p);
    if (small) return (lo * 2654435761u) >> (32 - (kHashLog + 1));
    const u64 x = (u64)lo | (u64)s.b((u64)p + 4) << 32;
    return (u32)(((x << 24) * 889523592379ull) >> (64 - kHashLog));
  }
};

u32 ctz64(u64 x) { return (u32)__builtin_ctzll(x); }

// token, length bytes, literals [lit_at, lit_at + lit); then, when has_match,
// the offset and the match length bytes.  One call per sequence: the kernel
// writes these cooperatively (runs of 255 are a parallel fill).
u32 emit(u8* dst, u32 op, const Body& s, u32 lit_at, u32 lit, bool has_match, u32 off, u32 ml) {
  const u32 nl = lit >= 15 ? (lit - 15) / 255 + 1 : 0;
  const u32 nm = has_match && ml >= 15 ? (ml - 15) / 255 + 1 : 0;
  dst[op] = (u8)((lit >= 15 ? 15u : lit) << 4 | (has_match ? (ml >= 15 ? 15u : ml) : 0u));
  u32 o = op + 1;
  for (u32 i = 0; i < nl; ++i) dst[o + i] = i + 1 < nl ? 255 : (u8)((lit - 15) % 255);
  o += nl;
  for (u32 i = 0; i < lit; ++i) dst[o + i] = s.src[lit_at + i];
  o += lit;
  if (has_match) {
    dst[o] = (u8)off;
    dst[o + 1] = (u8)(off >> 8);
    o += 2;
    for (u32 i = 0; i < nm; ++i) dst[o + i] = i + 1 < nm ? 255 : (u8)((ml - 15) % 255);
    o += nm;
  }
  return o;
}

u32 compress_block(const u8* src, u32 n, u8* dst, Table& tb) {
  const Body s{src, n};
  tb.small = n < kLimit64K;
  tb.clear();
  u32 op = 0, anchor = 0;
  if (n >= kMfLimit + 1) {
    const u32 mflimit1 = n - kMfLimit + 1, matchlimit = n - kLastLiterals;
    // (the reference's first insert, position 0 at hash(0), leaves the zeroed table as it is)
    u32 ip = 1;
    for (;;) {
      // ---- match search: windows of 64 probes
      u32 fwd = ip, step = 1, nb = 1u << kSkipTrigger, match = 0;
      bool at_limit = false;
      for (;;) {
        u32 cur[kW], nxt[kW], h[kW], T[kW], mi[kW];
        bool live[kW], ok[kW], hit[kW];
        for (u32 k = 0; k < kW; ++k) {
          cur[k] = fwd + (k ? step + F(nb + k - 1) - F(nb) : 0u);
          nxt[k] = fwd + step + F(nb + k) - F(nb);
          live[k] = cur[k] <= mflimit1;  // the probe before it passed the limit test
          ok[k] = nxt[k] <= mflimit1;
          h[k] = live[k] ? tb.hash(s, cur[k]) : 0u;
          T[k] = tb.get(h[k]);
        }
        for (u32 k = 0; k < kW; ++k) {
          mi[k] = T[k];
          for (u32 j = 0; j < k; ++j)
            if (live[j] && h[j] == h[k]) mi[k] = cur[j];
          hit[k] = live[k] && ok[k] && (tb.small || mi[k] + kDistanceMax >= cur[k]) && s.w4(mi[k]) == s.w4(cur[k]);
        }
        u64 E = 0;
        for (u32 k = 0; k < kW; ++k)
          if (live[k] && (hit[k] || !ok[k])) E |= 1ull << k;
        if (!E) {
          for (u32 k = 0; k < kW; ++k) tb.put(h[k], cur[k]);
          fwd = nxt[kW - 1];
          step = (nb + kW - 1) >> kSkipTrigger;
          nb += kW;
          continue;
        }
        const u32 e = ctz64(E);
        at_limit = !ok[e];
        for (u32 k = 0; k < e + (at_limit ? 0u : 1u); ++k) tb.put(h[k], cur[k]);
        ip = cur[e];
        match = mi[e];
        break;
      }
      if (at_limit) break;
      // ---- backward extension, 64 bytes a step
      {
        const u32 maxb = ip - anchor < match ? ip - anchor : match;
        u32 ext = 0;
        for (;;) {
          u64 ne = 0;
          for (u32 k = 0; k < kW; ++k) {
            const u32 i = ext + k;
            if (!(i < maxb && s.b(ip - 1 - i) == s.b(match - 1 - i))) ne |= 1ull << k;
          }
          if (ne) {
            ext += ctz64(ne);
            break;
          }
          ext += kW;
        }
        ip -= ext;
        match -= ext;
      }
      u32 lit_at = anchor, lit = ip - anchor;
      bool last = false;
      for (;;) {  // a match at ip from `match`, then possibly another at once
        // ---- match count, 4 bytes a lane
        u32 m = 0;
        for (;;) {
          u64 stop = 0;
          u32 eqb[kW];
          for (u32 k = 0; k < kW; ++k) {
            const u64 a = (u64)ip + kMinMatch + m + 4 * k, b = (u64)match + kMinMatch + m + 4 * k;
            const u32 left = a < matchlimit ? (u32)(matchlimit - a) : 0u;
            const u32 x = s.w4(a) ^ s.w4(b);
            eqb[k] = x ? (u32)__builtin_ctz(x) >> 3 : 4u;
            if (eqb[k] > left) eqb[k] = left;
            if (eqb[k] < 4) stop |= 1ull << k;
          }
          if (stop) {
            const u32 l = ctz64(stop);
            m += 4 * l + eqb[l];
            break;
          }
          m += 4 * kW;
        }
        op = emit(dst, op, s, lit_at, lit, true, ip - match, m);
        ip += m + kMinMatch;
        anchor = ip;
        if (ip >= mflimit1) {
          last = true;
          break;
        }
        tb.put(tb.hash(s, ip - 2), ip - 2);
        const u32 h = tb.hash(s, ip), mi = tb.get(h);
        tb.put(h, ip);
        if ((tb.small || mi + kDistanceMax >= ip) && s.w4(mi) == s.w4(ip)) {
          match = mi;
          lit_at = ip;
          lit = 0;
          continue;
        }
        break;
      }
      if (last) break;
      ++ip;
    }
  }
  return emit(dst, op, s, anchor, n - anchor, false, 0, 0);
}

bool rd(FILE* f, void* p, size_t n) { return fread(p, 1, n, f) == n; }

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: l4wenc_model IN OUT\n");
    return 2;
  }
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) return 2;
  std::vector<Table> tb(1);
  for (;;) {
    uint32_t n;
    if (!rd(in, &n, 4)) break;
    // exact sizes: the sanitizer sees any access past the input or the slot
    std::vector<u8> src(n), dst((size_t)n + n / 255 + 16);
    if (n && !rd(in, src.data(), n)) return 3;
    const uint32_t len = compress_block(src.data(), n, dst.data(), tb[0]);
    fwrite(&len, 4, 1, out);
    fwrite(dst.data(), 1, len, out);
  }
  fclose(out);
  fclose(in);
  return 0;
}
