// The launch arithmetic of the LZ4 block codec and of LZ4 frames
// (csrc/lz4_plan.h, csrc/lz4_frame_plan.h: workspace layouts, capacities,
// routes, thresholds, grid sizes) on the CPU.  Stand-alone: includes only
// those headers and the recorded table; tests/test_lz4_plan.py builds it with
// g++ and runs one part per test ("table", "layout", "sizing", "contracts",
// "rules").
#include "lz4_frame_plan.h"

#include <cstdio>
#include <cstring>
#include <initializer_list>

using namespace fsg;
typedef unsigned long long ull;

static int g_fail = 0;
#define CHECK(cond, ...)                                   \
  do {                                                     \
    if (!(cond)) {                                         \
      ++g_fail;                                            \
      std::printf("FAIL %s:%d %s | ", __FILE__, __LINE__, #cond); \
      std::printf(__VA_ARGS__);                            \
      std::printf("\n");                                   \
    }                                                      \
  } while (0)

// ---- what the C ABI answered before the arithmetic moved into the plan
// headers: tools/lz4_plan_golden.py, run against the library built from the
// commit before them (fsg_lz4_compress_workspace_bytes,
// fsg_lz4_decompress_workspace_bytes, fsg_lz4f_compress_workspace_bytes,
// fsg_lz4f_decompress_workspace_bytes; path and bitmap_words_capacity of
// fsg_lz4_decompress_report; path and wave_min of fsg_lz4_compress_report
// under option lz4_encode_wave_min; block_entries and block_wave_min of
// fsg_lz4f_compress_report, the latter also under option lz4f_block_wave_min;
// block_entries of fsg_lz4f_decompress_report).  A size of 0: over the limit
// of 2^30 block entries.  block_entries 0: the workspace is too small.
struct EncWs { u32 n; u64 ws; };
struct DecWs { u32 n; u64 total, ws; };
struct FrameEncWs { u32 n; u64 total; u32 id; u64 ws; };
struct FrameDecWs { u32 n; u64 total, ws; };
struct DecCap { u32 n; u64 ws; u32 path; u64 cap_words; };
struct EncRoute { i64 opt; u32 n; u64 ws; u32 path; u64 wave_min; };
struct FrameEncCap { u32 n, id; u64 ws; u32 entries; u64 block_wave_min; };
struct FrameEncWave { i64 opt; u32 n; u64 ws; u32 entries; u64 block_wave_min; };
struct FrameDecCap { u32 n; u64 ws; u32 entries; };
#include "lz4_plan_golden.inc"

template <typename T, size_t N>
constexpr size_t count_of(const T (&)[N]) { return N; }

static u64 report_wave_min(u64 wave_min) { return wave_min < 0xFFFFFFFFull ? wave_min : 0xFFFFFFFFull; }

static void test_table() {
  const Lz4Opts dflt;
  for (const EncWs& r : kEncWs)
    CHECK(lz4_compress_workspace_bytes(r.n) == r.ws, "n %u: %llu, recorded %llu", r.n,
          (ull)lz4_compress_workspace_bytes(r.n), (ull)r.ws);
  for (const DecWs& r : kDecWs)
    CHECK(lz4_decode_workspace_bytes(r.n, r.total) == r.ws, "n %u total %llu: %llu, recorded %llu", r.n, (ull)r.total,
          (ull)lz4_decode_workspace_bytes(r.n, r.total), (ull)r.ws);
  for (const FrameEncWs& r : kFrameEncWs)
    CHECK(lz4f_compress_workspace_bytes(r.n, r.total, r.id) == r.ws, "n %u total %llu id %u: %llu, recorded %llu", r.n,
          (ull)r.total, r.id, (ull)lz4f_compress_workspace_bytes(r.n, r.total, r.id), (ull)r.ws);
  for (const FrameDecWs& r : kFrameDecWs)
    CHECK(lz4f_decompress_workspace_bytes(r.n, r.total) == r.ws, "n %u total %llu: %llu, recorded %llu", r.n,
          (ull)r.total, (ull)lz4f_decompress_workspace_bytes(r.n, r.total), (ull)r.ws);
  // the over-limit rows are in the tables, and answer 0
  CHECK(lz4f_compress_workspace_bytes(1, 1ull << 46, 4) == 0, "2^30 + 1 entries");
  CHECK(lz4f_decompress_workspace_bytes(1, 1ull << 38) == 0, "2^30 + 1 entries");

  for (const DecCap& r : kDecCap) {  // fsg_lz4_decompress_report: path 0 = two passes, 1 = the one-pass kernel
    const Lz4DecodePlan p = lz4_decode_plan(r.n, (size_t)r.ws, 0, dflt);
    const bool two = r.ws != 0 && p.two_pass;
    CHECK(two == (r.path == 0), "n %u ws %llu: two_pass %d, recorded path %u", r.n, (ull)r.ws, (int)two, r.path);
    if (two) CHECK(p.valid && p.cap_words == r.cap_words, "n %u ws %llu: %llu words, recorded %llu", r.n, (ull)r.ws,
                   (ull)p.cap_words, (ull)r.cap_words);
    else CHECK(r.cap_words == 0, "n %u ws %llu", r.n, (ull)r.ws);
  }
  for (const EncRoute& r : kEncRoute) {
    Lz4Opts o;
    o.lz4_encode_wave_min = r.opt;
    const Lz4EncodePlan p = lz4_encode_plan(r.n, (size_t)r.ws, o);
    CHECK((u32)p.route == r.path && report_wave_min(p.wave_min) == r.wave_min,
          "opt %lld n %u ws %llu: route %d wave_min %llu, recorded %u %llu", (long long)r.opt, r.n, (ull)r.ws, p.route,
          (ull)p.wave_min, r.path, (ull)r.wave_min);
  }
  for (const FrameEncCap& r : kFrameEncCap) {
    const Lz4fEncodePlan p = lz4f_encode_plan(r.n, (size_t)r.ws, r.id, dflt);
    CHECK(p.valid == (r.entries != 0), "n %u id %u ws %llu: valid %d, recorded %u entries", r.n, r.id, (ull)r.ws,
          (int)p.valid, r.entries);
    if (!p.valid) continue;
    CHECK(p.w.nb_cap == r.entries && report_wave_min(p.inner.wave_min) == r.block_wave_min,
          "n %u id %u ws %llu: %u entries wave_min %llu, recorded %u %llu", r.n, r.id, (ull)r.ws, p.w.nb_cap,
          (ull)p.inner.wave_min, r.entries, (ull)r.block_wave_min);
  }
  for (const FrameEncWave& r : kFrameEncWave) {
    Lz4Opts o;
    o.lz4f_block_wave_min = r.opt;
    const Lz4fEncodePlan p = lz4f_encode_plan(r.n, (size_t)r.ws, 4, o);
    CHECK(p.valid && p.w.nb_cap == r.entries && report_wave_min(p.inner.wave_min) == r.block_wave_min,
          "opt %lld n %u ws %llu: %u entries wave_min %llu, recorded %u %llu", (long long)r.opt, r.n, (ull)r.ws,
          p.w.nb_cap, (ull)p.inner.wave_min, r.entries, (ull)r.block_wave_min);
  }
  for (const FrameDecCap& r : kFrameDecCap) {
    const Lz4fDecodePlan p = lz4f_decode_plan(r.n, (size_t)r.ws, dflt);
    CHECK(p.valid == (r.entries != 0) && (!p.valid || p.w.nb_cap == r.entries),
          "n %u ws %llu: valid %d %u entries, recorded %u", r.n, (ull)r.ws, (int)p.valid, p.w.nb_cap, r.entries);
  }
  std::printf("table: %zu + %zu + %zu + %zu sizes, %zu + %zu + %zu + %zu + %zu report rows\n", count_of(kEncWs),
              count_of(kDecWs), count_of(kFrameEncWs), count_of(kFrameDecWs), count_of(kDecCap), count_of(kEncRoute),
              count_of(kFrameEncCap), count_of(kFrameEncWave), count_of(kFrameDecCap));
}

// ---- the points of the other parts
static const u32 kNs[] = {1, 63, 64, 65, 256, 257, 65536};
static const u64 kTotals[] = {0, 1, 255, 256, 4095, 4096, 65535, 65536, 1ull << 20, (1ull << 32) + 12345, 1ull << 40};

struct Region {
  const char* name;
  u64 begin, end, align;
};
// ascending, disjoint, aligned; returns the end of the last
static u64 check_regions(const char* what, u32 n, u64 total, const Region* r, size_t count) {
  u64 at = 0;
  for (size_t i = 0; i < count; ++i) {
    CHECK(r[i].begin >= at && r[i].end >= r[i].begin, "%s n %u total %llu: %s [%llu, %llu) begins below %llu", what, n,
          (ull)total, r[i].name, (ull)r[i].begin, (ull)r[i].end, (ull)at);
    CHECK(r[i].begin % r[i].align == 0, "%s n %u total %llu: %s at %llu, alignment %llu", what, n, (ull)total, r[i].name,
          (ull)r[i].begin, (ull)r[i].align);
    at = r[i].end;
  }
  return at;
}

static void check_frame_layout(const char* what, u32 n, u64 total, const Lz4fLayout& w, bool enc) {
  const u64 lb = lz4f_list_bytes(n), nb = w.nb_cap;
  const Lz4fBlockColOff o = lz4f_block_col_off(nb);
  const Region r[] = {
      {"header", 0, kLz4fHead, 256},
      {"route", w.off_msg, w.off_msg + 4ull * n, 256},
      {"first", w.off_msg + lb, w.off_msg + lb + 4ull * n, 256},
      {"nb", w.off_msg + 2 * lb, w.off_msg + 2 * lb + 4ull * n, 256},
      {"xxh", w.off_msg + 3 * lb, w.off_msg + 3 * lb + 4ull * n, 256},
      {"in_off", w.off_blk + o.in_off, w.off_blk + o.in_off + 8 * nb, 16},  // the block columns begin 16-aligned
      {"out_off", w.off_blk + o.out_off, w.off_blk + o.out_off + 8 * nb, 8},
      {"src_off", w.off_blk + o.src_off, w.off_blk + o.src_off + 8 * nb, 8},
      {"in_len", w.off_blk + o.in_len, w.off_blk + o.in_len + 4 * nb, 4},
      {"out_cap", w.off_blk + o.out_cap, w.off_blk + o.out_cap + 4 * nb, 4},
      {"out_len", w.off_blk + o.out_len, w.off_blk + o.out_len + 4 * nb, 4},
      {"status", w.off_blk + o.status, w.off_blk + o.status + 4 * nb, 4},
      {"src_len", w.off_blk + o.src_len, w.off_blk + o.src_len + 4 * nb, 4},
      {"flags", w.off_blk + o.flags, w.off_blk + o.flags + 4 * nb, 4},
      {"entry slots", w.off_dummy, w.off_dummy + (enc ? 64 * nb : 0), 256},
      {"inner", w.off_inner, w.off_inner + w.inner_bytes, 256},
      {"staging", w.off_stage, w.off_stage + w.stage_cap, 256},
  };
  const u64 end = check_regions(what, n, total, r, count_of(r));
  CHECK(w.off_blk + lz4f_block_cols_bytes(nb) == w.off_dummy && o.flags + 4 * nb == nb * kLz4fBlockColBytes,
        "%s n %u total %llu: block columns", what, n, (ull)total);
  CHECK(w.total >= end && w.total - end < 256 && w.total % 256 == 0, "%s n %u total %llu: total %llu, last region ends %llu",
        what, n, (ull)total, (ull)w.total, (ull)end);
}

static void test_layout() {
  const Lz4Opts dflt;
  size_t points = 0;
  for (u32 n : kNs) {
    for (u64 total : kTotals) {
      // block decode
      const size_t ws = lz4_decode_workspace_bytes(n, total);
      const Lz4DecodePlan d = lz4_decode_plan(n, ws, 0, dflt);
      CHECK(d.valid && d.two_pass, "n %u total %llu", n, (ull)total);
      const Region dr[] = {{"counters", 0, kL4Head, 256},
                           {"bm_base", d.bm_base, d.bm_base + 4ull * n, 256},
                           {"hdr", d.hdr, d.hdr + 4ull * n, 256},
                           {"big_list", d.big_list, d.big_list + 4ull * n, 256},
                           {"bitmap", d.bitmap, d.bitmap + 4 * d.cap_words, 16}};
      const u64 dend = check_regions("decode", n, total, dr, count_of(dr));
      CHECK(dend <= ws && ws - dend < 16, "decode n %u total %llu: ws %llu, bitmap ends %llu", n, (ull)total, (ull)ws,
            (ull)dend);
      CHECK(4 * kL4CtrFallback + 4 <= kL4Head, "the fallback counter is in the header");
      ++points;
      // frames: the layout made for `total`, and the one found again from its size
      Lz4fLayout w;
      if (lz4f_dec_layout(n, total, &w)) {
        check_frame_layout("frame decode", n, total, w, false);
        const Lz4fDecodePlan p = lz4f_decode_plan(n, (size_t)w.total, dflt);
        CHECK(p.valid && p.w.total <= w.total && p.w.nb_cap >= w.nb_cap, "frame decode n %u total %llu", n, (ull)total);
        check_frame_layout("frame decode plan", n, total, p.w, false);
        ++points;
      }
      for (u32 id = 4; id <= 7; ++id) {
        if (!lz4f_enc_layout(n, total, id, &w)) continue;
        check_frame_layout("frame encode", n, total, w, true);
        const Lz4fEncodePlan p = lz4f_encode_plan(n, (size_t)w.total, id, dflt);
        CHECK(p.valid && p.w.total <= w.total && p.w.nb_cap >= w.nb_cap, "frame encode n %u total %llu id %u", n,
              (ull)total, id);
        check_frame_layout("frame encode plan", n, total, p.w, true);
        ++points;
      }
    }
    // block encode, both routes
    const size_t ws = lz4_compress_workspace_bytes(n);
    const Lz4EncodePlan e = lz4_encode_plan(n, ws, dflt);
    const Region er[] = {{"header", 0, kLz4EncHead, 256},
                         {"list", e.list_off, e.list_off + 4ull * n, 256},
                         {"tables", e.tables_off, e.tables_off + (u64)n * kLz4EncTableBytes, 256}};
    const u64 eend = check_regions("encode", n, 0, er, count_of(er));
    CHECK(e.valid && e.route == 0 && eend == ws && e.zero_bytes == ws, "encode n %u: ws %llu, tables end %llu, zeroed %llu",
          n, (ull)ws, (ull)eend, (ull)e.zero_bytes);
    const Lz4EncodePlan t = lz4_encode_plan(n, lz4_compress_tables_bytes(n), dflt);
    CHECK(t.valid && t.route == 1 && t.tables_off == 0 && t.zero_bytes == lz4_compress_tables_bytes(n) &&
              t.wave_min == kLz4WaveNone,
          "encode n %u, the tables alone", n);
    CHECK(!lz4_encode_plan(n, lz4_compress_tables_bytes(n) - 1, dflt).valid, "encode n %u, below the tables", n);
  }
  std::printf("layout: %zu points\n", points);
}

static void test_sizing() {
  const Lz4Opts dflt;
  for (u32 n : kNs) {
    for (u64 total : kTotals) {
      // block decode: a workspace sized for (n, T) holds T / 32 + 4 n bitmap words
      const Lz4DecodePlan d = lz4_decode_plan(n, lz4_decode_workspace_bytes(n, total), 0, dflt);
      CHECK(d.cap_words >= total / 32 + 4ull * n, "n %u total %llu: %llu words", n, (ull)total, (ull)d.cap_words);
      // frames: a workspace sized for (n, T) holds a block per message and per full block
      for (u32 id = 4; id <= 7; ++id) {
        const size_t ws = lz4f_compress_workspace_bytes(n, total, id);
        if (!ws) continue;
        const Lz4fEncodePlan p = lz4f_encode_plan(n, ws, id, dflt);
        CHECK(p.valid && p.w.nb_cap >= n + total / lz4f::block_bytes(id), "n %u total %llu id %u: %u entries", n,
              (ull)total, id, p.w.nb_cap);
        CHECK(p.w.stage_cap >= total + total / 255 + (u64)n * enc_slot(0), "n %u total %llu id %u: staging %llu", n,
              (ull)total, id, (ull)p.w.stage_cap);
      }
      if (const size_t ws = lz4f_decompress_workspace_bytes(n, total)) {
        const Lz4fDecodePlan p = lz4f_decode_plan(n, ws, dflt);
        CHECK(p.valid && p.w.nb_cap >= n + total / 256, "n %u total %llu: %u entries", n, (ull)total, p.w.nb_cap);
        CHECK(p.w.stage_cap >= total + (u64)n * dec_slot(0), "n %u total %llu: staging %llu", n, (ull)total,
              (ull)p.w.stage_cap);
      }
    }
    // the smallest workspace, and one byte less
    for (u32 id = 4; id <= 7; ++id) {
      const size_t lo = lz4f_compress_workspace_bytes(n, 0, id);
      CHECK(lz4f_encode_plan(n, lo, id, dflt).valid && !lz4f_encode_plan(n, lo - 1, id, dflt).valid, "n %u id %u", n, id);
    }
    const size_t lo = lz4f_decompress_workspace_bytes(n, 0);
    CHECK(lz4f_decode_plan(n, lo, dflt).valid && !lz4f_decode_plan(n, lo - 1, dflt).valid, "n %u", n);
    CHECK(!lz4f_encode_plan(n, lz4f_compress_workspace_bytes(n, 0, 4), 3, dflt).valid &&
              !lz4f_encode_plan(n, lz4f_compress_workspace_bytes(n, 0, 7), 8, dflt).valid,
          "n %u: block size ids 3 and 8", n);
    // more workspace, never fewer entries
    u32 enc_prev = 0, dec_prev = 0;
    for (u64 add = 0; add < (1ull << 34); add = add < 4096 ? add + 97 : add * 3 + 1) {
      const Lz4fEncodePlan pe = lz4f_encode_plan(n, lz4f_compress_workspace_bytes(n, 0, 4) + add, 4, dflt);
      const Lz4fDecodePlan pd = lz4f_decode_plan(n, lo + add, dflt);
      CHECK(pe.valid && pe.w.nb_cap >= enc_prev && pd.valid && pd.w.nb_cap >= dec_prev,
            "n %u + %llu bytes: %u after %u, %u after %u entries", n, (ull)add, pe.w.nb_cap, enc_prev, pd.w.nb_cap, dec_prev);
      enc_prev = pe.w.nb_cap;
      dec_prev = pd.w.nb_cap;
    }
    CHECK(enc_prev > n && dec_prev > n, "n %u: 16 GiB more hold more entries", n);
  }
  std::printf("sizing ok\n");
}

// what the frame launches rely on in the block codec's launches
static void test_contracts() {
  Lz4Opts o;
  for (int linked = 0; linked < 2; ++linked) {
    o.lz4f_linked_fast = linked;
    for (u32 n : kNs) {
      for (u64 total : kTotals) {
        Lz4fLayout w;
        if (lz4f_dec_layout(n, total, &w)) {
          // the inner size, as lz4_frame.hip wrote it before the block decoder's layout had named pieces
          CHECK(w.inner_bytes == lz4_decode_workspace_bytes(w.nb_cap, 0) - 16ull * w.nb_cap +
                                     16 * ((u64)n + total / 4096) + 4 * (total / 32),
                "n %u total %llu: inner %llu", n, (ull)total, (ull)w.inner_bytes);
          const Lz4fDecodePlan p = lz4f_decode_plan(n, (size_t)w.total, o);
          // the block decoder never answers hipErrorInvalidValue, and sees the bitmap the layout paid for
          CHECK(p.valid && p.w.inner_bytes >= lz4_decode_fixed_bytes(p.w.nb_cap) && p.inner.valid,
                "n %u total %llu: inner %llu", n, (ull)total, (ull)p.w.inner_bytes);
          CHECK(p.inner.cap_words == lz4_decode_bitmap_capacity_words(p.w.nb_cap, (size_t)p.w.inner_bytes) &&
                    4 * (p.inner.cap_words + 4) > 4 * lz4_decode_bitmap_words((u64)n + total / 4096, total) &&
                    p.inner.bitmap + 4 * p.inner.cap_words <= p.w.inner_bytes,
                "n %u total %llu: %llu words", n, (ull)total, (ull)p.inner.cap_words);
          CHECK(p.inner.chain_grid == (linked ? (n + 3) / 4 : 0u) && p.inner.exec_grid == (p.w.nb_cap + 3) / 4,
                "n %u total %llu linked %d: chain grid %u", n, (ull)total, linked, p.inner.chain_grid);
        }
        for (u32 id = 4; id <= 7; ++id) {
          if (!lz4f_enc_layout(n, total, id, &w)) continue;
          const Lz4fEncodePlan p = lz4f_encode_plan(n, (size_t)w.total, id, o);
          // the block encoders' route is always 0
          CHECK(p.valid && p.w.inner_bytes == lz4_compress_workspace_bytes(p.w.nb_cap) && p.inner.valid &&
                    p.inner.route == 0 && p.inner.zero_bytes == p.w.inner_bytes,
                "n %u total %llu id %u: inner %llu", n, (ull)total, id, (ull)p.w.inner_bytes);
        }
      }
    }
  }
  std::printf("contracts ok\n");
}

static void test_rules() {
  const Lz4Opts dflt;
  Lz4Opts o;
  // big_min: -1 (and anything outside [0, 2^32)) = 2 KiB up to 256 messages, 64 KiB above
  for (i64 v : {(i64)-1, (i64)-2, (i64)1 << 32, (i64)1 << 40}) {
    o = Lz4Opts{};
    o.lz4_big_min = v;
    CHECK(lz4_decode_plan(1, 1 << 20, 0, o).big_min == 2048 && lz4_decode_plan(256, 1 << 20, 0, o).big_min == 2048 &&
              lz4_decode_plan(257, 1 << 20, 0, o).big_min == 65536 && lz4_decode_plan(65536, 1 << 20, 0, o).big_min == 65536,
          "lz4_big_min %lld", (long long)v);
  }
  for (i64 v : {(i64)0, (i64)1, (i64)2048, (i64)65536, (i64)0xFFFFFFFE, (i64)0xFFFFFFFF}) {
    o = Lz4Opts{};
    o.lz4_big_min = v;
    CHECK(lz4_decode_plan(1, 1 << 20, 0, o).big_min == (u32)v && lz4_decode_plan(257, 1 << 20, 0, o).big_min == (u32)v,
          "lz4_big_min %lld", (long long)v);
  }
  // ... and a frame's blocks follow it, with the block entries as the batch
  o = Lz4Opts{};
  o.lz4_big_min = 777;
  CHECK(lz4f_decode_plan(5, lz4f_decompress_workspace_bytes(5, 1 << 20), o).inner.big_min == 777, "frames, lz4_big_min");
  CHECK(lz4f_decode_plan(5, lz4f_decompress_workspace_bytes(5, 0), dflt).inner.big_min == 2048 &&
            lz4f_decode_plan(5, lz4f_decompress_workspace_bytes(5, 1 << 20), dflt).inner.big_min == 65536,
        "frames, lz4_big_min automatic: 5 entries, 4,101 entries");

  // wave_min of the block call and of a frame's blocks
  struct { i64 opt; u64 at256, at257; } const wm[] = {{-1, 8192, kLz4WaveNone},
                                                       {-5, 8192, kLz4WaveNone},
                                                       {0, 0, 0},
                                                       {0xFFFFFFFEll, 0xFFFFFFFEull, 0xFFFFFFFEull},
                                                       {0xFFFFFFFFll, kLz4WaveNone, kLz4WaveNone},
                                                       {1ll << 40, kLz4WaveNone, kLz4WaveNone}};
  for (const auto& r : wm) {
    CHECK(lz4_encode_wave_min(r.opt, 256) == r.at256 && lz4_encode_wave_min(r.opt, 257) == r.at257 &&
              lz4_encode_wave_min(r.opt, 1) == r.at256,
          "wave_min %lld", (long long)r.opt);
    o = Lz4Opts{};
    o.lz4_encode_wave_min = r.opt;
    CHECK(lz4_encode_plan(256, lz4_compress_workspace_bytes(256), o).wave_min == r.at256 &&
              lz4_encode_plan(257, lz4_compress_workspace_bytes(257), o).wave_min == r.at257,
          "lz4_encode_wave_min %lld", (long long)r.opt);
    // a frame's blocks: option lz4f_block_wave_min, not lz4_encode_wave_min; 256 and 257 entries
    o = Lz4Opts{};
    o.lz4f_block_wave_min = r.opt;
    o.lz4_encode_wave_min = 4242;
    const Lz4fEncodePlan a = lz4f_encode_plan(256, lz4f_compress_workspace_bytes(256, 0, 4), 4, o);
    const Lz4fEncodePlan b = lz4f_encode_plan(257, lz4f_compress_workspace_bytes(257, 0, 4), 4, o);
    CHECK(a.valid && a.w.nb_cap == 256 && a.inner.wave_min == r.at256 && b.valid && b.w.nb_cap == 257 &&
              b.inner.wave_min == r.at257,
          "lz4f_block_wave_min %lld: %u entries %llu, %u entries %llu", (long long)r.opt, a.w.nb_cap,
          (ull)a.inner.wave_min, b.w.nb_cap, (ull)b.inner.wave_min);
  }
  // length_wave_min
  CHECK(lz4f_length_wave_min(-1) == 2048 && lz4f_length_wave_min(-7) == 2048 && lz4f_length_wave_min(0) == 0 &&
            lz4f_length_wave_min(0xFFFFFFFEll) == 0xFFFFFFFEu && lz4f_length_wave_min(0xFFFFFFFFll) == 0xFFFFFFFFu &&
            lz4f_length_wave_min(1ll << 40) == 0xFFFFFFFFu,
        "lz4f_length_wave_min");
  CHECK(lz4f_decode_plan(1, 1 << 20, dflt).length_wave_min == 2048, "lz4f_length_wave_min, default");
  // the three switches
  o = Lz4Opts{};
  o.lz4f_nosize_fast = 1;
  const Lz4fDecodePlan sw = lz4f_decode_plan(1, 1 << 20, o);
  CHECK(!sw.force_serial && sw.nosize_fast && !sw.linked_fast, "lz4f_nosize_fast");
  const Lz4fDecodePlan sd = lz4f_decode_plan(1, 1 << 20, dflt);
  CHECK(!sd.force_serial && !sd.nosize_fast && !sd.linked_fast, "defaults");

  // the wave encoder's grid: min(n, 256 CUs x waves per CU), nine waves of 16 KiB per CU unless the option says fewer
  struct { i64 opt; u32 waves; } const pc[] = {{-1, 2304}, {0, 2304}, {1, 256}, {8, 2048}, {9, 2304}, {10, 2304}, {1ll << 40, 2304}};
  for (const auto& r : pc) {
    o = Lz4Opts{};
    o.lz4_encode_wave_min = 0;
    o.lz4f_block_wave_min = 0;
    o.lz4_encode_wave_per_cu = r.opt;
    for (u32 n : {1u, 255u, 256u, 257u, 2047u, 2048u, 2049u, 2303u, 2304u, 2305u, 65536u}) {
      CHECK(lz4_encode_plan(n, lz4_compress_workspace_bytes(n), o).wave_grid == (n < r.waves ? n : r.waves),
            "lz4_encode_wave_per_cu %lld n %u", (long long)r.opt, n);
      const Lz4fEncodePlan f = lz4f_encode_plan(n, lz4f_compress_workspace_bytes(n, 0, 4), 4, o);
      CHECK(f.valid && f.w.nb_cap == n && f.inner.wave_grid == (n < r.waves ? n : r.waves),
            "frames, lz4_encode_wave_per_cu %lld, %u entries", (long long)r.opt, f.w.nb_cap);
    }
  }

  // grids.  A frame workspace of the smallest size for n messages has n block entries.
  struct { u32 n, by4, by64, by256, stage, lane; } const g[] = {
      {1, 1, 1, 1, 1, 1},           {63, 16, 1, 1, 16, 1},           {64, 16, 1, 1, 16, 1},
      {65, 17, 2, 1, 17, 2},        {256, 64, 4, 1, 64, 4},          {257, 65, 5, 2, 65, 5},
      {32764, 8191, 512, 128, 8191, 512}, {32765, 8192, 512, 128, 8192, 512}, {32768, 8192, 512, 128, 8192, 512},
      {32769, 8193, 513, 129, 8192, 513}, {262080, 65520, 4095, 1024, 8192, 4095}, {262081, 65521, 4096, 1024, 8192, 4096},
      {262144, 65536, 4096, 1024, 8192, 4096}, {262145, 65537, 4097, 1025, 8192, 4096}};
  for (const auto& r : g) {
    o = Lz4Opts{};
    o.lz4f_linked_fast = 1;
    const Lz4DecodePlan d = lz4_decode_plan(r.n, lz4_decode_workspace_bytes(r.n, 0), r.n, o);
    CHECK(d.index_grid == r.by64 && d.index_big_grid == 256 && d.exec_grid == r.by4 && d.chain_grid == r.by4, "decode n %u",
          r.n);
    CHECK(lz4_decode_plan(r.n, lz4_decode_workspace_bytes(r.n, 0), 0, o).chain_grid == 0, "decode n %u, no chains", r.n);
    const Lz4EncodePlan e = lz4_encode_plan(r.n, lz4_compress_workspace_bytes(r.n), dflt);
    CHECK(e.list_grid == r.by256, "encode n %u: list grid %u", r.n, e.list_grid);
    const Lz4fEncodePlan fe = lz4f_encode_plan(r.n, lz4f_compress_workspace_bytes(r.n, 0, 4), 4, o);
    CHECK(fe.valid && fe.w.nb_cap == r.n && fe.prefill_grid == r.by256 && fe.plan_grid == r.by64 && fe.assemble_grid == r.n &&
              fe.inner.list_grid == r.by256,
          "frame encode n %u: %u entries", r.n, fe.w.nb_cap);
    const Lz4fDecodePlan fd = lz4f_decode_plan(r.n, lz4f_decompress_workspace_bytes(r.n, 0), o);
    CHECK(fd.valid && fd.w.nb_cap == r.n, "frame decode n %u: %u entries", r.n, fd.w.nb_cap);
    CHECK(fd.msg_grid == r.by64 && fd.place_grid == r.by4 && fd.length_wave_grid == 256 && fd.verdict_grid == r.by64 &&
              fd.stage_grid == r.stage && fd.length_lane_grid == r.lane,
          "frame decode n %u: stage %u lane %u", r.n, fd.stage_grid, fd.length_lane_grid);
    CHECK(fd.inner.index_grid == r.by64 && fd.inner.exec_grid == r.by4 && fd.inner.chain_grid == r.by4,
          "frame decode n %u: inner grids", r.n);
  }
  std::printf("rules ok\n");
}

int main(int argc, char** argv) {
  const char* part = argc > 1 ? argv[1] : "all";
  const bool all = !std::strcmp(part, "all");
  if (all || !std::strcmp(part, "table")) test_table();
  if (all || !std::strcmp(part, "layout")) test_layout();
  if (all || !std::strcmp(part, "sizing")) test_sizing();
  if (all || !std::strcmp(part, "contracts")) test_contracts();
  if (all || !std::strcmp(part, "rules")) test_rules();
  std::printf("%s: %d failure(s)\n", part, g_fail);
  return g_fail ? 1 : 0;
}
