// gzip_index_cpu.cc -- see gzip_index_cpu.h.
#include "gzip_index_cpu.h"

#include "../csrc/gzip_index.h"
#include "inflate_cpu.h"

namespace {

// The usable index of a gzip body whose wrapper is accepted; kNone / kUnusable otherwise.
gzidx::Head usable_index(const uint8_t* p, uint64_t n, const infl::Wrapper& w, uint64_t* before_last) {
  gzidx::Head h = gzidx::find_head(p);
  if (h.state != gzidx::kUsable) return h;
  uint64_t sum = 0;
  for (uint32_t k = 0; k + 1 < h.chcnt; ++k) sum += gzidx::size_at(p, h, k);
  if (!gzidx::placed(w.begin, sum, n)) h.state = gzidx::kUnusable;
  *before_last = sum;
  return h;
}

}  // namespace

extern "C" {

int fsh_cpu_gzip_index(const void* in, size_t n, uint32_t* chlen, uint32_t* chcnt, uint64_t* starts,
                       size_t starts_cap) {
  const uint8_t* p = static_cast<const uint8_t*>(in);
  const infl::Wrapper w = infl::parse_wrapper(infl::kGzip, p, n);
  if (w.status != infl::kStOk) return FSH_GZIP_INDEX_NONE;
  uint64_t sum = 0;
  const gzidx::Head h = usable_index(p, n, w, &sum);
  if (h.state != gzidx::kUsable) return (int)h.state;
  if (chlen) *chlen = h.chlen;
  if (chcnt) *chcnt = h.chcnt;
  uint64_t at = w.begin;
  for (uint32_t k = 0; k < h.chcnt && k < starts_cap; ++k) {
    starts[k] = at;
    at += gzidx::size_at(p, h, k);
  }
  return FSH_GZIP_INDEX_USABLE;
}

int fsh_cpu_inflate_units_route(uint32_t format, const void* in, size_t n, size_t cap, int store, uint32_t* units) {
  const uint8_t* p = static_cast<const uint8_t*>(in);
  uint32_t cnt = 1;
  int route = FSH_UNITS_ROUTE_NO_INDEX;
  [&] {
    if (n == 0 || n > 0xffff0000ull || format > infl::kGzip) {  // decided without a walk
      cnt = 0;
      return;
    }
    const infl::Wrapper w = infl::parse_wrapper(format, p, n);
    if (w.status != infl::kStOk) {
      cnt = 0;
      return;
    }
    if (format != infl::kGzip) return;
    uint64_t sum = 0;
    const gzidx::Head h = usable_index(p, n, w, &sum);
    if (h.state == gzidx::kNone) return;
    route = FSH_UNITS_ROUTE_UNUSABLE;
    if (h.state != gzidx::kUsable) return;
    cnt = h.chcnt;
    route = FSH_UNITS_ROUTE_MISMATCH;
    uint64_t at = w.begin, total = 0;
    for (uint32_t k = 0; k < h.chcnt; ++k) {
      const bool nonlast = k + 1 < h.chcnt;
      const uint64_t stop = nonlast ? at + gzidx::size_at(p, h, k) : n - 8;
      uint64_t len = 0;
      if (fsh_cpu_inflate_unit(p, n, at, stop, nonlast, h.chlen, nullptr, 0, 0, &len) != infl::kStOk) return;
      total += len;
      at = stop;
    }
    if (store && total > cap) return;
    route = FSH_UNITS_ROUTE_PARALLEL;
  }();
  if (units) *units = cnt;
  return route;
}

}  // extern "C"
