// deflate_check.cc -- the host deflate model (host/deflate_cpu.cc over
// csrc/deflate_format.h) under AddressSanitizer and UBSan, stand-alone: built
// and run by tests/test_deflate.py, never loaded into Python.
//
// Input: a file of records { u32 format, n, want_len, flags } + n input bytes
// + want_len body bytes (what the unsanitized library gave).  Per record:
//   1. fsh_cpu_deflate gives exactly those bytes, into a buffer of exactly
//      the bound, and fsh_cpu_inflate gives the input back;
//   2. (flags & 2) the wide functions of deflate_format.h -- symbol counts,
//      code lengths, code assignment, the header, the sizes, bit placement --
//      run by 64 lanes give what their (0, 1) form gives, for every unit of
//      the input.  The lanes are 64 threads; INFL_FENCE is a barrier of all
//      64, so a function that needs a fence it does not have shows up as a
//      difference (or under the sanitizer);
//   3. (flags & 1) the length limiter ran.
// Prints "ok <records> <units emulated>".
#include <pthread.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>
#include <thread>
#include <vector>

#include "../../flare-cpp_amd/csrc/inflate_format.h"

// this translation unit's own reading of deflate_format.h: fences are
// barriers, counts and ORs are atomic, and the namespace has another name so
// that the model's copy (deflate_cpu.cc, linked in) stays what it is
static pthread_barrier_t g_barrier;
static thread_local bool t_in_lanes = false;
static void lane_fence() {
  if (t_in_lanes) pthread_barrier_wait(&g_barrier);
}
#undef INFL_FENCE
#define INFL_FENCE() lane_fence()
#define DEFL_ADD(p, v) __atomic_fetch_add((p), (v), __ATOMIC_RELAXED)
#define DEFL_OR(p, v) __atomic_fetch_or((p), (v), __ATOMIC_RELAXED)
#define defl defl_lanes
#include "../../flare-cpp_amd/csrc/deflate_format.h"
#undef defl
namespace E = defl_lanes;

#include "deflate_cpu.h"
#include "inflate_cpu.h"

namespace {

constexpr uint32_t kLanes = 64;

void run_lanes(const std::function<void(uint32_t)>& fn) {
  std::vector<std::thread> t;
  for (uint32_t lane = 0; lane < kLanes; ++lane)
    t.emplace_back([&fn, lane] {
      t_in_lanes = true;
      fn(lane);
    });
  for (auto& x : t) x.join();
}

#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      printf("record %zu: %s (line %d)\n", g_rec, #c, __LINE__);  \
      return false;                                               \
    }                                                             \
  } while (0)
size_t g_rec = 0;

struct Outcome {
  E::Build b;
  uint32_t header, dyn, fix;
  E::Choice c;
  std::vector<uint32_t> win;
  uint32_t bytes;
};

// Phases 2 and 3 of one unit from its tokens, by `nl` lanes.
void encode(const std::vector<uint32_t>& tok, uint32_t n, bool last, uint32_t nl, Outcome* o) {
  memset(&o->b, 0, sizeof o->b);
  E::Build* b = &o->b;
  std::vector<uint32_t> pd(nl), pf(nl), hdr(nl);
  auto phase2 = [&](uint32_t lane) {
    for (size_t i = lane; i < tok.size(); i += nl) E::count_token(b, tok[i]);
    lane_fence();
    E::build_lengths(b->hist, E::kLitSyms, 15, b->len, b, lane, nl);
    lane_fence();
    E::build_lengths(b->hist + E::kDistBase, E::kDistSyms, 15, b->len + E::kDistBase, b, lane, nl);
    lane_fence();
    hdr[lane] = E::build_dynamic_header(b, lane, nl);
    lane_fence();
    E::symbol_bits(b, lane, nl, &pd[lane], &pf[lane]);
  };
  if (nl == 1) phase2(0); else run_lanes(phase2);
  o->header = hdr[0];
  o->dyn = o->fix = 0;
  for (uint32_t l = 0; l < nl; ++l) {
    if (hdr[l] != hdr[0]) o->header = ~0u;  // the lanes must agree
    o->dyn += pd[l];
    o->fix += pf[l];
  }
  o->c = E::choose_block(n, last, o->dyn + o->header, o->fix);
  o->win.assign(o->c.bytes / 4 + 8, 0);
  o->bytes = o->c.bytes;
  if (o->c.type == E::kStored) return;
  std::vector<uint32_t> at(tok.size() + 1, 0);
  uint32_t pos0 = 0;
  auto phase3 = [&](uint32_t lane) {
    if (o->c.type == E::kFixed) {
      E::fill_fixed_lengths(b, lane, nl);
      E::assign_codes(b->len, infl::kFixedLens, b->code, b, lane, nl);
      lane_fence();
      E::assign_codes(b->len + E::kDistBase, infl::kFixedDists, b->code + E::kDistBase, b, lane, nl);
    } else {
      E::assign_codes(b->len, E::kLitSyms, b->code, b, lane, nl);
      lane_fence();
      E::assign_codes(b->len + E::kDistBase, E::kDistSyms, b->code + E::kDistBase, b, lane, nl);
    }
    lane_fence();
    if (lane == 0) {
      pos0 = E::write_block_header(b, o->c.type, last, o->win.data());
      uint32_t p = pos0;  // the prefix sum the device takes with DPP
      for (size_t i = 0; i < tok.size(); ++i) {
        uint32_t nb;
        E::token_bits(b, tok[i], &nb);
        at[i] = p;
        p += nb;
      }
      at[tok.size()] = p;
    }
    lane_fence();
    for (size_t i = lane; i < tok.size(); i += nl) {
      uint32_t nb;
      const uint64_t v = E::token_bits(b, tok[i], &nb);
      E::put_bits(o->win.data(), at[i], v, nb);
    }
    lane_fence();
    if (lane == 0) o->bytes = E::write_block_tail(last, at[tok.size()], o->win.data());
  };
  if (nl == 1) phase3(0); else run_lanes(phase3);
}

bool same(const Outcome& s, const Outcome& w) {
  CHECK(memcmp(s.b.hist, w.b.hist, sizeof s.b.hist) == 0);
  CHECK(w.header == s.header && w.dyn == s.dyn && w.fix == s.fix);
  CHECK(w.c.type == s.c.type && w.c.bytes == s.c.bytes && w.bytes == s.bytes && s.bytes == s.c.bytes);
  CHECK(memcmp(s.b.cl_len, w.b.cl_len, E::kClSyms) == 0 && memcmp(s.b.cl_code, w.b.cl_code, 2 * E::kClSyms) == 0);
  CHECK(s.b.n_seq == w.b.n_seq && s.b.hlit == w.b.hlit && s.b.hdist == w.b.hdist && s.b.hclen == w.b.hclen);
  CHECK(memcmp(s.b.cl_seq, w.b.cl_seq, 2 * s.b.n_seq) == 0);
  CHECK(s.b.limited == w.b.limited);
  if (s.c.type != E::kStored) {
    const uint32_t nlit = s.c.type == E::kFixed ? 288 : E::kLitSyms, nd = s.c.type == E::kFixed ? 32 : E::kDistSyms;
    CHECK(memcmp(s.b.len, w.b.len, nlit) == 0 && memcmp(s.b.code, w.b.code, 2 * nlit) == 0);
    CHECK(memcmp(s.b.len + E::kDistBase, w.b.len + E::kDistBase, nd) == 0);
    CHECK(memcmp(s.b.code + E::kDistBase, w.b.code + E::kDistBase, 2 * nd) == 0);
    CHECK(s.win == w.win);
  }
  return true;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  pthread_barrier_init(&g_barrier, nullptr, kLanes);
  size_t units = 0;
  for (;; ++g_rec) {
    uint32_t h[4];
    if (fread(h, 4, 4, f) != 4) break;
    const uint32_t fmt = h[0], n = h[1], want_len = h[2], flags = h[3];
    std::vector<uint8_t> in(n), want(want_len);
    if (n && fread(in.data(), 1, n, f) != n) return 2;
    if (want_len && fread(want.data(), 1, want_len, f) != want_len) return 2;
    auto fail = [&](const char* what) {
      printf("record %zu (format %u, %u bytes): %s\n", g_rec, fmt, n, what);
      return 1;
    };
    // 1. the model, into a heap buffer of exactly the bound (ASan guards its end)
    const size_t cap = fsh_cpu_deflate_bound(n, fmt);
    std::vector<uint8_t> out(cap);
    uint64_t len = 99;
    if (fsh_cpu_deflate(fmt, in.data(), n, out.data(), cap, &len) != 0) return fail("status");
    if (len != want_len || memcmp(out.data(), want.data(), len) != 0) return fail("bytes differ from the library's");
    if (len) {
      uint64_t l2 = 7;
      std::vector<uint8_t> tiny(len - 1);
      if (fsh_cpu_deflate(fmt, in.data(), n, tiny.data(), len - 1, &l2) != 3 || l2 != 0) return fail("small cap");
    }
    std::vector<uint8_t> back(n);
    uint64_t blen = 0;
    if (fsh_cpu_inflate(fmt, out.data(), len, back.data(), n, &blen) != 0 || blen != n ||
        (n && memcmp(back.data(), in.data(), n) != 0))
      return fail("fsh_cpu_inflate does not return the input");
    if ((flags & 1) && fsh_cpu_deflate_limited(in.data(), n) == 0) return fail("the length limiter did not run");
    // 2. 64 lanes against (0, 1), unit by unit
    if (!(flags & 2)) continue;
    const uint64_t nu = n == 0 ? 1 : (n + E::kUnit - 1) / E::kUnit;
    for (uint64_t u = 0; u < nu; ++u, ++units) {
      const uint32_t first = (uint32_t)(u * E::kUnit), un = n - first < E::kUnit ? n - first : E::kUnit;
      std::vector<uint32_t> tok(un + 1);
      const size_t k = fsh_cpu_deflate_tokens(in.data() + first, un, tok.data(), un);
      if (un && !k) return fail("tokens");
      tok.resize(k);
      tok.push_back(E::kTokEnd);
      Outcome s, w;
      encode(tok, un, u + 1 == nu, 1, &s);
      encode(tok, un, u + 1 == nu, kLanes, &w);
      if (!same(s, w)) return 1;
    }
  }
  fclose(f);
  printf("ok %zu %zu\n", g_rec, units);
  return 0;
}
