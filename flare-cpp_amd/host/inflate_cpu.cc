// inflate_cpu.cc -- see inflate_cpu.h.
#include "inflate_cpu.h"

#include "../csrc/inflate_format.h"

namespace {

using namespace infl;

// 64-bit bit buffer over p[0 .. n); bytes past n read 0 (a stream that needs
// them is corrupt: the caller compares consumed() with the stream's end).
struct Reader {
  const uint8_t* p;
  uint64_t n, pos = 0;
  uint64_t hold = 0;
  uint32_t nbits = 0;
  Reader(const uint8_t* p_, uint64_t n_, uint64_t at) : p(p_), n(n_), pos(at) {}
  void need() {
    while (nbits <= 56) {
      hold |= (uint64_t)(pos < n ? p[pos] : 0) << nbits;
      ++pos;
      nbits += 8;
    }
  }
  uint32_t peek(uint32_t k) const { return (uint32_t)hold & ((1u << k) - 1); }
  void drop(uint32_t k) {
    hold >>= k;
    nbits -= k;
  }
  uint32_t bits(uint32_t k) {
    const uint32_t v = peek(k);
    drop(k);
    return v;
  }
  uint64_t consumed() const { return 8 * pos - nbits; }  // bits
  void restart(uint64_t at) {
    pos = at;
    hold = 0;
    nbits = 0;
  }
};

struct Tables {
  uint32_t lit[kEnoughLens], dist[kEnoughDists];
  uint32_t fixlit[512], fixdist[32];
  uint8_t lens[kLensArray];
  uint16_t work[kLensArray];
  TableScratch s;
  bool have_fixed = false;
};

inline uint32_t lookup(Reader& r, const uint32_t* tab, uint32_t root) {
  uint32_t e = tab[r.peek(root)];
  if (e_op(e) & kOpLink) {
    r.drop(e_bits(e));
    e = tab[e_val(e) + r.peek(e_op(e) & 15)];
  }
  r.drop(e_bits(e));
  return e;
}

// The block loop over p[at ..): blocks until BFINAL, which must end in byte
// n_end - 1 (a whole stream, or the last unit of an indexed gzip body).  With
// `nonlast` it is a unit before the last (csrc/gzip_index.h): it ends clean
// after the block whose last bit is bit 8 * n_end - 1, having given exactly
// chlen bytes and met no BFINAL; everything else is kStCorrupt.  Distances are
// counted from the walk's first output byte, out[0]; cap is the room at out.
int walk(const uint8_t* p, uint64_t n, uint64_t at, uint64_t n_end, bool nonlast, uint64_t chlen, uint8_t* out,
         uint64_t cap, bool store, uint64_t* outpos_out) {
  Reader r(p, n, at);
  Tables t;
  uint64_t outpos = 0;
  uint32_t last = 0;
  auto unit_end = [&]() -> int {  // a non-last unit after each block; -1: go on
    *outpos_out = outpos;
    if (last || outpos > chlen) return kStCorrupt;
    if (r.consumed() == 8 * n_end) return outpos == chlen ? kStOk : kStCorrupt;
    return -1;
  };
  do {
    r.need();
    last = r.bits(1);
    const uint32_t type = r.bits(2);
    if (type == 3) return kStCorrupt;
    if (type == 0) {
      r.drop(r.nbits & 7);
      r.need();
      const uint32_t len = r.bits(16), nlen = r.bits(16);
      if ((len ^ 0xffffu) != nlen) return kStCorrupt;
      const uint64_t start = r.consumed() / 8;
      if (start + len > n_end) return kStCorrupt;
      for (uint32_t i = 0; i < len; ++i, ++outpos)
        if (store && outpos < cap) out[outpos] = p[start + i];
      r.restart(start + len);
      if (nonlast) {
        const int v = unit_end();
        if (v >= 0) return v;
      }
      continue;
    }
    const uint32_t *lt, *dt;
    uint32_t lroot = kLenRoot, droot = kDistRoot;
    if (type == 1) {
      if (!t.have_fixed) {
        for (uint32_t i = 0; i < kFixedLens + kFixedDists; ++i) t.lens[i] = (uint8_t)fixed_length(i);
        build_table(kLens, t.lens, kFixedLens, t.fixlit, 512, &lroot, t.work, &t.s, 0, 1);
        build_table(kDists, t.lens + kFixedLens, kFixedDists, t.fixdist, 32, &droot, t.work, &t.s, 0, 1);
        t.have_fixed = true;
      }
      lroot = 9;
      droot = 5;
      lt = t.fixlit;
      dt = t.fixdist;
    } else {
      uint32_t nlen, ndist;
      if (!read_dynamic_header(r, t.lens, &nlen, &ndist, t.dist, t.work, &t.s, 0, 1)) return kStCorrupt;
      if (build_table(kLens, t.lens, nlen, t.lit, kEnoughLens, &lroot, t.work, &t.s, 0, 1) != kTableOk)
        return kStCorrupt;
      if (build_table(kDists, t.lens + nlen, ndist, t.dist, kEnoughDists, &droot, t.work, &t.s, 0, 1) != kTableOk)
        return kStCorrupt;
      lt = t.lit;
      dt = t.dist;
    }
    // Every step takes at least one bit and the bit position is checked
    // against the stream's end at each, so the loop ends within 8 * n steps.
    for (;;) {
      if (r.consumed() > 8 * n_end) return kStCorrupt;
      r.need();
      uint32_t e = lookup(r, lt, lroot);
      uint32_t op = e_op(e);
      if (op == kOpLit) {
        if (store && outpos < cap) out[outpos] = (uint8_t)e_val(e);
        ++outpos;
        continue;
      }
      if (op == kOpEnd) break;
      if (!(op & kOpBase)) return kStCorrupt;  // a symbol with no code
      const uint32_t length = e_val(e) + r.bits(op & 15);
      r.need();
      e = lookup(r, dt, droot);
      op = e_op(e);
      if (!(op & kOpBase)) return kStCorrupt;
      const uint32_t distance = e_val(e) + r.bits(op & 15);
      if (distance > outpos) return kStCorrupt;  // before the first byte (at most 32,768 by the code itself)
      for (uint32_t i = 0; i < length; ++i, ++outpos)
        if (store && outpos < cap) out[outpos] = out[outpos - distance];
    }
    if (nonlast) {
      const int v = unit_end();
      if (v >= 0) return v;
    }
  } while (!last);
  *outpos_out = outpos;
  const uint64_t used = r.consumed();
  if (used > 8 * n_end || (used + 7) / 8 != n_end) return kStCorrupt;  // cut short, or bytes after the stream
  return kStOk;
}

int inflate_body(uint32_t format, const uint8_t* p, uint64_t n, uint8_t* out, uint64_t cap, bool store,
                 uint64_t* len_out) {
  *len_out = 0;
  if (format > kGzip || n > 0xffff0000ull) return kStCorrupt;  // the device decoder's limit (4 GiB - 64 KiB)
  const Wrapper w = parse_wrapper(format, p, n);
  if (w.status != kStOk) return w.status;
  if (n < (uint64_t)w.begin + w.trailer) return kStCorrupt;
  const uint64_t n_end = n - w.trailer;  // where the deflate stream must end
  uint64_t outpos = 0;
  if (walk(p, n, w.begin, n_end, false, 0, out, cap, store, &outpos) != kStOk) return kStCorrupt;
  if (!store) {
    *len_out = outpos;
    return kStOk;
  }
  if (outpos > cap) {
    *len_out = outpos > 0xffffffffull ? 0xffffffffull : outpos;
    return kStSlotTooSmall;
  }
  if (format == kZlib) {
    const uint32_t want = (uint32_t)p[n_end] << 24 | (uint32_t)p[n_end + 1] << 16 | (uint32_t)p[n_end + 2] << 8 |
                          p[n_end + 3];
    if (adler32_serial(1, out, outpos) != want) return kStCorrupt;
  } else if (format == kGzip) {
    const uint8_t* q = p + n_end;
    const uint32_t crc = q[0] | (uint32_t)q[1] << 8 | (uint32_t)q[2] << 16 | (uint32_t)q[3] << 24;
    const uint32_t isize = q[4] | (uint32_t)q[5] << 8 | (uint32_t)q[6] << 16 | (uint32_t)q[7] << 24;
    if (crc32_serial(0, out, outpos) != crc || (uint32_t)outpos != isize) return kStCorrupt;
  }
  *len_out = outpos;
  return kStOk;
}

}  // namespace

extern "C" {

int fsh_cpu_inflate(uint32_t format, const void* in, size_t n, void* out, size_t cap, uint64_t* len) {
  uint64_t l = 0;
  const int st = inflate_body(format, static_cast<const uint8_t*>(in), n, static_cast<uint8_t*>(out), cap, true, &l);
  if (len) *len = l;
  return st;
}

int fsh_cpu_inflate_length(uint32_t format, const void* in, size_t n, uint64_t* len) {
  uint64_t l = 0;
  const int st = inflate_body(format, static_cast<const uint8_t*>(in), n, nullptr, 0, false, &l);
  if (len) *len = l;
  return st;
}

int fsh_cpu_inflate_unit(const void* in, size_t n, size_t start, size_t stop, int nonlast, uint32_t chlen, void* out,
                         size_t cap, int store, uint64_t* len) {
  uint64_t l = 0;
  const int st = walk(static_cast<const uint8_t*>(in), n, start, stop, nonlast != 0, chlen, static_cast<uint8_t*>(out),
                      cap, store != 0, &l);
  if (len) *len = l;
  return st;
}

uint32_t fsh_cpu_crc32(const void* p, size_t n) { return infl::crc32_serial(0, static_cast<const uint8_t*>(p), n); }
uint32_t fsh_cpu_adler32(const void* p, size_t n) { return infl::adler32_serial(1, static_cast<const uint8_t*>(p), n); }

}  // extern "C"
