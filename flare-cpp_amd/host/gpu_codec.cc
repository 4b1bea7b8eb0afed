// gpu_codec.cc -- see gpu_codec.h.
#include "gpu_codec.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

#include "../../include/flare_snappy_gpu.h"
#include "batch_plan.h"
#include "pinned.h"
#include "snappy_cpu.h"

namespace flare::gpu {

namespace {

// A grow-only buffer: device memory, or pinned host memory (so
// hipMemcpyAsync is a true DMA).
template <bool kPinned>
struct Buf {
  void* p = nullptr;
  size_t cap = 0;
  bool reserve(size_t n) {
    if (n <= cap) return true;
    release();
    size_t want = n + n / 4 + 4096;
    if ((kPinned ? hipHostMalloc(&p, want, hipHostMallocDefault) : hipMalloc(&p, want)) != hipSuccess) {
      p = nullptr;
      return false;
    }
    cap = want;
    return true;
  }
  void release() {
    if (p) (void)(kPinned ? hipHostFree(p) : hipFree(p));
    p = nullptr;
    cap = 0;
  }
  template <class T>
  T* as() const { return static_cast<T*>(p); }
};
using DevBuf = Buf<false>;
using HostBuf = Buf<true>;

struct Request {
  const cord_buf* in;
  cord_buf* out;
  Kind kind;
  bool ok = false;       // the verdict
  bool handled = false;  // a device (or the host codec) produced it
  bool done = false;
  void* latch = nullptr;
  void (*signal)(void*) = nullptr;
};

// Host threads for gather / scatter of large chunks (copies into pinned
// staging are CPU memcpy; one core moves ~10 GB/s).
unsigned host_threads() {
  static const unsigned t = [] {
    if (const char* e = getenv("FLARE_SNAPPY_GPU_HOST_THREADS")) return (unsigned)std::max(1, atoi(e));
    const unsigned hw = std::thread::hardware_concurrency();
    return std::min(16u, std::max(1u, hw));
  }();
  return t;
}

// fn(i) for i in [a, b), split over host threads when `bytes` is large.
template <class F>
void parallel_for(uint32_t a, uint32_t b, size_t bytes, F&& fn) {
  const unsigned nt = bytes < (8u << 20) ? 1u : std::min<unsigned>(host_threads(), b - a);
  if (nt <= 1) {
    for (uint32_t i = a; i < b; ++i) fn(i);
    return;
  }
  std::vector<std::thread> th;
  th.reserve(nt);
  for (unsigned t = 0; t < nt; ++t) {
    const uint32_t lo = a + (uint32_t)((uint64_t)(b - a) * t / nt);
    const uint32_t hi = a + (uint32_t)((uint64_t)(b - a) * (t + 1) / nt);
    th.emplace_back([lo, hi, &fn] {
      for (uint32_t i = lo; i < hi; ++i) fn(i);
    });
  }
  for (auto& x : th) x.join();
}

// Flat copy of a cord_buf (the host codec works on contiguous bytes).
const uint8_t* flatten(const cord_buf& in, std::vector<uint8_t>* tmp) {
  if (in.backing_block_num() == 1) return reinterpret_cast<const uint8_t*>(in.backing_block(0).data());
  tmp->resize(in.size() + 1);
  in.copy_to(tmp->data(), in.size());
  return tmp->data();
}

bool cpu_run(Kind kind, const cord_buf& in, cord_buf* out) {
  std::vector<uint8_t> tin, tout;  // per call: no thread_local (see snappy_cpu.cc)
  const uint8_t* p = flatten(in, &tin);
  const size_t n = in.size();
  if (kind == kCompress) {
    tout.resize(snappy::cpu::MaxCompressedLength(n));
    out->append(tout.data(), snappy::cpu::Compress(p, n, tout.data()));
    return true;
  }
  if (kind == kValidate) return snappy::cpu::IsValid(p, n);
  uint32_t ulen = 0;
  const size_t h = snappy::cpu::ReadHeader(p, n, &ulen, /*strict=*/false);
  if (h == 0 || !plausible_length(ulen, n)) return false;
  tout.resize((size_t)ulen + 32);
  if (!snappy::cpu::Decode(p, n, h, tout.data(), ulen, nullptr, tout.size())) return false;
  out->append(tout.data(), ulen);
  return true;
}

constexpr int kSlots = 3;
// Outputs at least this long are adopted from the pinned slab; shorter ones
// are copied (an adopted range costs a block header and a slab reference).
constexpr uint32_t kAdoptMin = 2048;

struct Counters {
  std::atomic<uint64_t> batches{0}, messages{0}, bytes_in{0}, bytes_out{0}, max_batch{0},
      failures{0}, cpu_messages{0}, fallbacks{0}, adopted{0}, d2h_bytes{0}, packed_chunks{0},
      device_fallback_messages{0}, device_single_pass_messages{0}, device_fallback_batches{0};
};

static_assert(FSG_OK == kStatusOk, "batch_plan.h's packed_layout tests the device's status");

// What a slot's batch call was given (path report: its workspace's header
// follows the results down on the same stream when it had a workspace).
struct CallArgs {
  uint32_t n = 0, max_len = 0;
  size_t ws_bytes = 0;  // 0: no workspace
};

// Chunk k of a batch: bodies [a, b) on stream `slot`, input bytes [ia, ib)
// of the staging buffers, output slots [oa, ob).
struct Chunk {
  size_t k;
  int slot;
  uint32_t a, b, cn;
  size_t ia, ib, oa, ob;
  uint64_t staged = 0, direct = 0;  // gather_chunk: input bytes staged / left to the device gather
};

// One device batch: what the stages of Device::run share.
struct Batch {
  const std::vector<Request*>& reqs;
  const Kind kind;
  const uint32_t n;
  BatchPlan plan;
  MetaColumns h{}, d{};  // host (pinned) and device metadata columns
  GatherColumns hg{}, dg{};
  // The unpacked chunks' D2H target: a pinned slab the outputs are adopted
  // from, else staging.
  OutSlab* slab = nullptr;
  bool adopt = false;
  uint8_t* hout = nullptr;
  bool failed = false;
  int pending[kSlots];  // chunk in flight on each stream
  CallArgs call[kSlots];
  std::vector<uint64_t> poff;  // a packed chunk's offsets (packed_layout)
  uint64_t bytes_in = 0, bytes_out = 0, adopted = 0, corrupt = 0, d2h = 0, packed_chunks = 0;
  uint64_t fb_messages = 0, fb_batches = 0, single_pass = 0;

  Batch(const std::vector<Request*>& r, Kind k) : reqs(r), kind(k), n((uint32_t)r.size()) {
    std::fill(pending, pending + kSlots, -1);
  }
  bool compress() const { return kind == kCompress; }
  bool validate() const { return kind == kValidate; }
  Chunk chunk(size_t k) const {
    const uint32_t a = plan.cut[k], b = plan.cut[k + 1];
    return Chunk{k, (int)(k % kSlots), a, b, b - a, plan.in_begin(k), plan.in_end(k), plan.out_begin(k),
                 plan.out_end(k)};
  }
};

// What the plan needs of each request: sizes, and for decode kinds the
// length header's verdict.
std::vector<PlanBody> plan_bodies(const std::vector<Request*>& reqs, Kind kind) {
  std::vector<PlanBody> bodies(reqs.size());
  for (size_t i = 0; i < reqs.size(); ++i) {
    const cord_buf& in = *reqs[i]->in;
    bodies[i] = PlanBody{in.size(), (uint32_t)in.backing_block_num(), 0, true};
    if (kind == kCompress) continue;
    uint8_t hdr[5];
    const size_t k = in.copy_to(hdr, sizeof(hdr));
    bodies[i].header_ok = fsg_get_uncompressed_length(hdr, k, &bodies[i].ulen, /*lenient=*/1) != 0;
  }
  return bodies;
}

// One HIP device's runtime.
struct Device {
  int id = -1;
  hipStream_t streams[kSlots] = {};
  // Decode is copy-bound end to end and pipelines well in 256 MiB chunks;
  // encode is latency-bound on the GPU and needs every message of the batch
  // in one launch, so it is not chunked.  FLARE_SNAPPY_GPU_CHUNK_BYTES
  // overrides both (tests force many small chunks).
  size_t chunk_bytes = 256ull << 20;
  size_t chunk_bytes_compress = ~size_t(0);
  // Compress chunks whose output slots hold at least this many bytes are
  // packed on the device before the D2H (fsg_pack_batch), so the copy and the
  // pinned slab carry compressed bytes instead of worst-case slots; smaller
  // ones take the one-synchronisation path.  FLARE_SNAPPY_GPU_PACK_MIN_BYTES.
  size_t pack_min_bytes = kPackMinBytesDefault;
  DevBuf d_in, d_meta, d_out, d_ws[kSlots], d_gath;
  // per stream, packed path: the dense outputs; total u64 | pack_off u64[n] | scan workspace
  DevBuf d_pack[kSlots], d_pmeta[kSlots];
  HostBuf h_in, h_meta, h_out, h_gath, h_total, h_pack;
  // per stream: the workspace's counter header after the batch call (path report)
  HostBuf h_rep;

  bool start(int dev, std::string* err) {
    id = dev;
    if (fsg_init(dev) != FSG_SUCCESS) {
      *err = std::string("fsg_init failed: ") + fsg_last_error();
      return false;
    }
    for (auto& st : streams) {
      if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) {
        st = nullptr;
        *err = "hipStreamCreate failed";
        return false;
      }
    }
    if (const char* cb = getenv("FLARE_SNAPPY_GPU_CHUNK_BYTES")) {
      chunk_bytes = std::max<size_t>(1, strtoull(cb, nullptr, 10));
      chunk_bytes_compress = chunk_bytes;
    }
    pack_min_bytes = PackMinBytesFromEnv();
    return true;
  }

  void stop() {
    if (id < 0) return;
    (void)hipSetDevice(id);
    for (auto& st : streams)
      if (st) {
        (void)hipStreamSynchronize(st);
        (void)hipStreamDestroy(st);
        st = nullptr;
      }
    for (DevBuf* b : {&d_in, &d_meta, &d_out, &d_gath}) b->release();
    for (auto* per_slot : {d_ws, d_pack, d_pmeta})
      for (int s = 0; s < kSlots; ++s) per_slot[s].release();
    for (HostBuf* b : {&h_total, &h_pack, &h_rep, &h_in, &h_meta, &h_out, &h_gath}) b->release();
    id = -1;
  }

  // Runs one device batch for `reqs` (all of `kind`).  Every request it
  // finishes gets handled = true; returns false after a device error (the
  // unfinished requests are left to the host codec).
  bool run(const std::vector<Request*>& reqs, Kind kind, Counters* ctr);

  // run's stages, in a chunk's order.  A stage that returns false has
  // reported the error; the batch has then failed.
  bool reserve(Batch& bt);
  void gather_chunk(Batch& bt, Chunk* c);
  bool upload_chunk(Batch& bt, const Chunk& c);
  bool launch_chunk(Batch& bt, const Chunk& c);
  bool download_chunk(Batch& bt, const Chunk& c);
  void finish_chunk(Batch& bt, int slot);
  void read_report(Batch& bt, int slot);
  void drain(Batch& bt);
  static void add_counters(const Batch& bt, Counters* ctr);
};

std::atomic<int> g_inject_errors{0};  // test hook: fail the next n device batches

bool Device::run(const std::vector<Request*>& reqs, Kind kind, Counters* ctr) {
  if (reqs.empty()) return true;
  for (int k = g_inject_errors.load(); k > 0;)
    if (g_inject_errors.compare_exchange_weak(k, k - 1)) return false;
  if (hipSetDevice(id) != hipSuccess) return false;
  Batch bt(reqs, kind);
  bt.plan = plan_batch(kind, plan_bodies(reqs, kind).data(), bt.n,
                       bt.compress() ? chunk_bytes_compress : chunk_bytes, pack_min_bytes);
  if (!reserve(bt)) return false;
  for (size_t k = 0; k < bt.plan.n_chunks(); ++k) {
    Chunk c = bt.chunk(k);
    finish_chunk(bt, c.slot);  // its previous chunk (staging regions are disjoint, streams are not)
    if (bt.failed) break;
    gather_chunk(bt, &c);
    if (!upload_chunk(bt, c) || !launch_chunk(bt, c) || !download_chunk(bt, c)) {
      bt.failed = true;
      break;
    }
    bt.pending[c.slot] = (int)k;
  }
  drain(bt);
  if (bt.slab) OutSlabRelease(bt.slab);  // the adopted ranges keep it alive
  add_counters(bt, ctr);
  return !bt.failed;
}

// The batch's buffers, its column views with the plan's columns in them, and
// the unpacked chunks' D2H target.  False (nothing held) when memory is short.
bool Device::reserve(Batch& bt) {
  const BatchPlan& p = bt.plan;
  const size_t n = bt.n;
  if (!h_in.reserve(p.total_in + 16) || !h_meta.reserve(p.meta_bytes) || !h_gath.reserve(p.gath_bytes + 16) ||
      !d_in.reserve(p.total_in + 16) || !d_meta.reserve(p.meta_bytes) || !d_gath.reserve(p.gath_bytes + 16) ||
      !d_out.reserve(p.total_out + 16) || !h_rep.reserve(kSlots * fsg_report_header_bytes()))
    return false;
  bt.h = MetaColumns::at(h_meta.p, n);
  bt.d = MetaColumns::at(d_meta.p, n);
  bt.hg = GatherColumns::at(h_gath.p, p.blk_base[n]);
  bt.dg = GatherColumns::at(d_gath.p, p.blk_base[n]);
  memcpy(bt.h.in_off, p.in_off.data(), 8 * n);
  memcpy(bt.h.out_off, p.out_off.data(), 8 * n);
  memcpy(bt.h.in_len, p.in_len.data(), 4 * n);
  memcpy(bt.h.out_cap, p.out_cap.data(), 4 * n);
  if (p.any_packed && !h_total.reserve(kSlots * sizeof(uint64_t))) return false;
  bt.slab = bt.validate() || !p.any_unpacked ? nullptr : AcquireOutSlab(p.host_out + 16);
  // under slab pressure outputs are copied, so this slab returns to the pool
  // right after the batch instead of being held by long-lived cord_bufs
  bt.adopt = bt.slab && !OutSlabsUnderPressure();
  if (!bt.validate() && p.any_unpacked && bt.slab == nullptr && !h_out.reserve(p.host_out + 16)) return false;
  bt.hout = bt.slab ? OutSlabData(bt.slab) : h_out.as<uint8_t>();
  return true;
}

// cord_buf backing blocks (cord_buf.cc:1469-1475): pinned ones become
// descriptors for the device gather, the rest is staged.
void Device::gather_chunk(Batch& bt, Chunk* c) {
  const BatchPlan& p = bt.plan;
  const GatherColumns g = bt.hg;
  uint8_t* hin = h_in.as<uint8_t>();
  // The host threads add to these once per body.  Each fills a cache line of
  // its own, so the adds do not take away the line that holds the pointers
  // every block reads (16,384 x 64 KiB from pinned blocks, compress: 101-103
  // ms, against 105-110 with the two sums next to those pointers; DESIGN.md
  // section 5, "Host batch plan").
  struct alignas(64) Sum {
    std::atomic<uint64_t> v{0};
  } staged, direct;
  parallel_for(c->a, c->b, c->ib - c->ia, [&](uint32_t i) {
    if (p.skip[i]) return;
    const cord_buf& in = *bt.reqs[i]->in;
    size_t w = 0;
    uint64_t st = 0, dr = 0;
    for (size_t blk = 0; blk < in.backing_block_num(); ++blk) {
      std::string_view v = in.backing_block(blk);
      const uint32_t j = p.blk_base[i] + (uint32_t)blk;
      g.dst[j] = p.in_off[i] + w;
      if (v.size() >= 1024 && IsPinned(v.data(), v.size())) {
        g.src[j] = reinterpret_cast<uint64_t>(v.data());
        g.len[j] = (uint32_t)v.size();
        dr += v.size();
      } else {
        g.src[j] = 0;
        g.len[j] = 0;
        memcpy(hin + p.in_off[i] + w, v.data(), v.size());
        st += v.size();
      }
      w += v.size();
    }
    staged.v += st;
    direct.v += dr;
  });
  c->staged = staged.v.load();
  c->direct = direct.v.load();
}

// H2D: the staged input, the descriptors and the device gather, the columns.
bool Device::upload_chunk(Batch& bt, const Chunk& c) {
  const BatchPlan& p = bt.plan;
  const MetaColumns &h = bt.h, &d = bt.d;
  const GatherColumns &hg = bt.hg, &dg = bt.dg;
  hipStream_t st = streams[c.slot];
  bool ok = true;
  if (c.staged && c.ib > c.ia)
    ok = hipMemcpyAsync(d_in.as<uint8_t>() + c.ia, h_in.as<uint8_t>() + c.ia, c.ib - c.ia, hipMemcpyHostToDevice,
                        st) == hipSuccess;
  const uint32_t ja = p.blk_base[c.a], jn = p.blk_base[c.b] - p.blk_base[c.a];
  if (ok && c.direct && jn) {
    ok = hipMemcpyAsync(dg.src + ja, hg.src + ja, 8ull * jn, hipMemcpyHostToDevice, st) == hipSuccess &&
         hipMemcpyAsync(dg.dst + ja, hg.dst + ja, 8ull * jn, hipMemcpyHostToDevice, st) == hipSuccess &&
         hipMemcpyAsync(dg.len + ja, hg.len + ja, 4ull * jn, hipMemcpyHostToDevice, st) == hipSuccess &&
         fsg_gather_blocks(dg.src + ja, dg.len + ja, dg.dst + ja, jn, d_in.as<uint8_t>(), st) == FSG_SUCCESS;
  }
  // this chunk's offsets, lengths and caps: four column slices, or (one
  // chunk: the whole batch) the four columns in one copy -- per-copy
  // latency dominates a small batch
  const uint32_t a = c.a, cn = c.cn;
  if (p.n_chunks() == 1) {
    ok = ok && hipMemcpyAsync(d.in_off, h.in_off, MetaColumns::kUpBytesPerBody * (size_t)bt.n,
                              hipMemcpyHostToDevice, st) == hipSuccess;
  } else {
    ok = ok && hipMemcpyAsync(d.in_off + a, h.in_off + a, 8ull * cn, hipMemcpyHostToDevice, st) == hipSuccess;
    ok = ok && hipMemcpyAsync(d.out_off + a, h.out_off + a, 8ull * cn, hipMemcpyHostToDevice, st) == hipSuccess;
    ok = ok && hipMemcpyAsync(d.in_len + a, h.in_len + a, 4ull * cn, hipMemcpyHostToDevice, st) == hipSuccess;
    ok = ok && hipMemcpyAsync(d.out_cap + a, h.out_cap + a, 4ull * cn, hipMemcpyHostToDevice, st) == hipSuccess;
  }
  if (!ok) fprintf(stderr, "[flare-snappy-gpu] H2D copy failed on device %d\n", id);
  return ok;
}

// The batch call (compress, then the pack pass of a packed chunk; or decode /
// validate) and the workspace's report header behind it.
bool Device::launch_chunk(Batch& bt, const Chunk& c) {
  const MetaColumns& d = bt.d;
  const bool validate = bt.validate();
  const uint32_t a = c.a, cn = c.cn;
  const int slot = c.slot;
  hipStream_t st = streams[slot];
  int rc;
  if (bt.compress()) {
    uint32_t cmax = 0;
    for (uint32_t i = a; i < c.b; ++i) cmax = std::max(cmax, bt.plan.in_len[i]);
    const size_t ws = fsg_compress_workspace_bytes(cn, cmax);
    void* wsp = d_ws[slot].reserve(ws) ? d_ws[slot].p : nullptr;  // no workspace -> LDS-table kernel
    rc = fsg_compress_batch(d_in.as<uint8_t>(), d.in_off + a, d.in_len + a, cn, cmax, d_out.as<uint8_t>(),
                            d.out_off + a, d.out_len + a, d.status + a, wsp, wsp ? ws : 0, st);
    bt.call[slot] = CallArgs{cn, cmax, wsp ? ws : 0};
    if (rc == FSG_SUCCESS && bt.plan.packed[c.k]) {
      // dense copies of the outputs, 16-byte aligned (an adopted output that
      // later feeds a decode keeps fsg_gather_blocks' 16-byte path)
      const size_t pws = fsg_pack_workspace_bytes(cn);
      if (d_pack[slot].reserve(c.ob - c.oa) && d_pmeta[slot].reserve(8 + 8ull * cn + pws)) {
        auto* d_total = d_pmeta[slot].as<uint64_t>();
        rc = fsg_pack_batch(d_out.as<uint8_t>(), d.out_off + a, d.out_len + a, d.status + a, cn, 16,
                            d_pack[slot].as<uint8_t>(), d_total + 1, d_total, d_total + 1 + cn, pws, st);
      } else {
        rc = FSG_ERR_HIP;
      }
    }
  } else {
    // two-pass decoder workspace (tag bitmap); without it the single-pass kernel runs
    const size_t ws = validate ? 0 : fsg_decompress_workspace_bytes(cn, c.ib - c.ia);
    void* wsp = ws && d_ws[slot].reserve(ws) ? d_ws[slot].p : nullptr;
    rc = fsg_decompress_batch(d_in.as<uint8_t>(), d.in_off + a, d.in_len + a, cn,
                              validate ? nullptr : d_out.as<uint8_t>(), validate ? nullptr : d.out_off + a,
                              validate ? nullptr : d.out_cap + a, d.out_len + a, d.status + a,
                              validate ? FSG_FLAG_VALIDATE_ONLY : 0u, wsp, wsp ? ws : 0, st);
    bt.call[slot] = CallArgs{cn, 0, wsp ? ws : 0};
  }
  // the workspace's counter header, behind the batch's passes on its stream
  // (a failed reserve() left no workspace: the routing rule alone reports it)
  const size_t rep_bytes = fsg_report_header_bytes();
  if (rc == FSG_SUCCESS && bt.call[slot].ws_bytes >= rep_bytes &&
      hipMemcpyAsync(h_rep.as<uint8_t>() + rep_bytes * slot, d_ws[slot].p, rep_bytes, hipMemcpyDeviceToHost, st) !=
          hipSuccess)
    rc = FSG_ERR_HIP;
  if (rc != FSG_SUCCESS)
    fprintf(stderr, "[flare-snappy-gpu] batch launch failed on device %d: %s\n", id, fsg_last_error());
  return rc == FSG_SUCCESS;
}

// D2H: the lengths and statuses (one chunk: both columns in one copy), then
// the chunk's output slots, or a packed chunk's total.
bool Device::download_chunk(Batch& bt, const Chunk& c) {
  const BatchPlan& p = bt.plan;
  const MetaColumns &h = bt.h, &d = bt.d;
  const uint32_t a = c.a, cn = c.cn;
  const bool packed = p.packed[c.k];
  hipStream_t st = streams[c.slot];
  const bool ok =
      (p.n_chunks() == 1
           ? hipMemcpyAsync(h.out_len, d.out_len, MetaColumns::kDownBytesPerBody * (size_t)bt.n,
                            hipMemcpyDeviceToHost, st) == hipSuccess
           : hipMemcpyAsync(h.out_len + a, d.out_len + a, 4ull * cn, hipMemcpyDeviceToHost, st) == hipSuccess &&
                 hipMemcpyAsync(h.status + a, d.status + a, 4ull * cn, hipMemcpyDeviceToHost, st) == hipSuccess) &&
      (bt.validate() || c.ob == c.oa ||
       (packed ? hipMemcpyAsync(h_total.as<uint64_t>() + c.slot, d_pmeta[c.slot].p, sizeof(uint64_t),
                                hipMemcpyDeviceToHost, st)
               : hipMemcpyAsync(bt.hout + p.hbase[c.k], d_out.as<uint8_t>() + c.oa, c.ob - c.oa,
                                hipMemcpyDeviceToHost, st)) == hipSuccess);
  if (ok && !bt.validate() && !packed) bt.d2h += c.ob - c.oa;
  if (!ok) fprintf(stderr, "[flare-snappy-gpu] D2H copy failed on device %d\n", id);
  return ok;
}

// Path report of the slot's finished batch call.
void Device::read_report(Batch& bt, int slot) {
  const CallArgs& call = bt.call[slot];
  const void* hdr = call.ws_bytes ? h_rep.as<uint8_t>() + fsg_report_header_bytes() * slot : nullptr;
  uint64_t fb = 0, sp = 0;
  if (bt.compress()) {
    fsg_encode_report r;
    if (fsg_compress_report(hdr, call.n, call.max_len, call.ws_bytes, &r) != FSG_SUCCESS) return;
    fb = r.fallback_messages;
    sp = r.no_workspace_messages;
  } else {
    fsg_decode_report r;
    if (fsg_decompress_report(hdr, call.n, call.ws_bytes, bt.validate() ? FSG_FLAG_VALIDATE_ONLY : 0u, &r) !=
        FSG_SUCCESS)
      return;
    fb = r.fallback_messages;
    // validate-only is single-pass by design
    sp = r.path == FSG_PATH_NO_WORKSPACE || r.path == FSG_PATH_FORCED ? r.single_pass_messages : 0;
  }
  bt.fb_messages += fb;
  bt.fb_batches += fb ? 1 : 0;
  bt.single_pass += sp;
}

// Waits for the slot's chunk (if one is in flight), downloads a packed
// chunk's outputs, and scatters the results to the callers' cord_bufs.
void Device::finish_chunk(Batch& bt, int slot) {
  const int k = bt.pending[slot];
  if (k < 0) return;
  bt.pending[slot] = -1;
  if (hipStreamSynchronize(streams[slot]) != hipSuccess) {
    fprintf(stderr, "[flare-snappy-gpu] stream error on device %d\n", id);
    bt.failed = true;
    return;
  }
  read_report(bt, slot);
  const BatchPlan& p = bt.plan;
  const uint32_t* out_len = bt.h.out_len;
  const int32_t* status = bt.h.status;
  // where message i's bytes are on the host, the slab they are adopted from
  const uint32_t ka = p.cut[k], kb = p.cut[k + 1];
  const bool packed = p.packed[k];
  uint8_t* obase = bt.hout + p.hbase[k];
  OutSlab* oslab = bt.slab;
  bool oadopt = bt.adopt;
  if (packed) {
    // the lengths and statuses are here: lay the packed outputs out as the
    // device did, take a slab for exactly that many bytes, download them
    bt.poff.resize(kb - ka);
    const uint64_t tot = packed_layout(status, out_len, ka, kb, bt.poff.data());
    if (tot != h_total.as<uint64_t>()[slot]) {
      fprintf(stderr, "[flare-snappy-gpu] packed size mismatch on device %d\n", id);
      bt.failed = true;
      return;
    }
    oslab = AcquireOutSlab(tot + 16);
    oadopt = oslab && !OutSlabsUnderPressure();
    obase = oslab ? OutSlabData(oslab) : (h_pack.reserve(tot + 16) ? h_pack.as<uint8_t>() : nullptr);
    if (obase == nullptr ||
        (tot && (hipMemcpyAsync(obase, d_pack[slot].p, tot, hipMemcpyDeviceToHost, streams[slot]) != hipSuccess ||
                 hipStreamSynchronize(streams[slot]) != hipSuccess))) {
      fprintf(stderr, "[flare-snappy-gpu] packed D2H failed on device %d\n", id);
      if (oslab) OutSlabRelease(oslab);
      bt.failed = true;
      return;
    }
    bt.d2h += tot;
    ++bt.packed_chunks;
  }
  // ---- scatter: append results to the callers' cord_bufs (serial: page
  // faults from many threads at once measured 3x slower than one thread)
  for (uint32_t i = ka; i < kb; ++i) {
    Request* r = bt.reqs[i];
    if (p.skip[i] == 2) continue;  // for the host codec
    r->handled = true;
    if (p.skip[i] || status[i] != FSG_OK) {
      r->ok = false;
      ++bt.corrupt;
      continue;
    }
    r->ok = true;
    bt.bytes_in += p.in_len[i];
    if (bt.validate()) continue;
    const uint32_t L = out_len[i];
    uint8_t* bytes = obase + (packed ? bt.poff[i - ka] : p.out_off[i] - p.out_off[ka]);
    if (oadopt && L >= kAdoptMin) {
      OutSlabRef(oslab);
      r->out->append_user_data(bytes, L, AdoptedDeleter);
      ++bt.adopted;
    } else {
      r->out->append(bytes, L);
    }
    bt.bytes_out += L;
  }
  if (packed && oslab) OutSlabRelease(oslab);  // the adopted ranges keep it alive
}

// Finishes the chunks still in flight; a failed batch only waits for their
// streams and leaves them, like every later chunk, unhandled.
void Device::drain(Batch& bt) {
  for (int slot = 0; slot < kSlots; ++slot) {
    if (bt.failed) {
      if (bt.pending[slot] >= 0) (void)hipStreamSynchronize(streams[slot]);
      bt.pending[slot] = -1;
    } else {
      finish_chunk(bt, slot);
    }
  }
}

void Device::add_counters(const Batch& bt, Counters* ctr) {
  ctr->batches += 1;
  ctr->messages += bt.n;
  ctr->bytes_in += bt.bytes_in;
  ctr->bytes_out += bt.bytes_out;
  ctr->adopted += bt.adopted;
  ctr->failures += bt.corrupt;
  ctr->d2h_bytes += bt.d2h;
  ctr->packed_chunks += bt.packed_chunks;
  ctr->device_fallback_messages += bt.fb_messages;
  ctr->device_single_pass_messages += bt.single_pass;
  ctr->device_fallback_batches += bt.fb_batches;
  uint64_t mb = ctr->max_batch.load();
  while (bt.n > mb && !ctr->max_batch.compare_exchange_weak(mb, bt.n)) {
  }
}

// Devices from FLARE_SNAPPY_GPU_DEVICES ("0x3" / "3" = a mask, "0,2" = a
// list) or FLARE_SNAPPY_GPU_DEVICE (one index); default device 0.
uint64_t env_device_mask() {
  if (const char* e = getenv("FLARE_SNAPPY_GPU_DEVICES")) {
    if (strchr(e, ',')) {
      uint64_t m = 0;
      for (const char* p = e; *p;) {
        m |= 1ull << (strtoul(p, nullptr, 10) & 63);
        p = strchr(p, ',');
        if (!p) break;
        ++p;
      }
      return m;
    }
    return strtoull(e, nullptr, 0);
  }
  if (const char* d = getenv("FLARE_SNAPPY_GPU_DEVICE")) return 1ull << (atoi(d) & 63);
  return 1;
}

size_t env_min_bytes() {
  const char* e = getenv("FLARE_SNAPPY_GPU_MIN_BYTES");
  return e ? (size_t)strtoull(e, nullptr, 10) : 16384;
}

}  // namespace

struct SnappyGpuCodec::Impl {
  std::mutex mu;
  std::condition_variable cv;
  std::deque<Request*> queue;
  std::vector<std::unique_ptr<Device>> devs;
  std::vector<char> busy;
  // double-checked start: read without the lock on every handler call,
  // published with release once start_locked has set the devices up
  std::atomic<bool> started{false};
  std::string err;
  std::atomic<int> n_devs{0};
  std::atomic<size_t> min_bytes{env_min_bytes()};
  ParkHooks hooks;
  Counters ctr;

  void ensure_started() {
    if (started.load(std::memory_order_acquire)) return;
    std::unique_lock<std::mutex> lk(mu);
    if (!started.load(std::memory_order_relaxed)) start_locked(env_device_mask());
  }

  int start_locked(uint64_t mask) {
    const int n = start_devices_locked(mask);
    started.store(true, std::memory_order_release);
    return n;
  }

  int start_devices_locked(uint64_t mask) {
    err.clear();
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count == 0) {
      err = "no HIP device";
      return 0;
    }
    for (int d = 0; d < 64 && d < count; ++d) {
      if (!(mask & (1ull << d))) continue;
      auto dev = std::make_unique<Device>();
      std::string e;
      if (dev->start(d, &e)) {
        devs.push_back(std::move(dev));
      } else {
        dev->stop();
        err += "device " + std::to_string(d) + ": " + e + "; ";
      }
    }
    busy.assign(devs.size(), 0);
    n_devs.store((int)devs.size());
    if (devs.empty() && err.empty()) err = "no device in the mask";
    return (int)devs.size();
  }

  // Waits until no device runs and nothing is queued (caller holds lk).
  void quiesce(std::unique_lock<std::mutex>& lk) {
    cv.wait(lk, [&] {
      return queue.empty() && std::none_of(busy.begin(), busy.end(), [](char b) { return b != 0; });
    });
  }

  void stop_locked() {
    for (auto& d : devs) d->stop();
    devs.clear();
    busy.clear();
    n_devs.store(0);
  }

  // Runs a mixed batch on device d; the host codec takes whatever the device
  // could not finish.
  void run_batch(Device& dev, const std::vector<Request*>& batch) {
    std::vector<Request*> by[3];
    for (Request* q : batch) by[q->kind].push_back(q);
    for (int k = 0; k < 3; ++k) {
      if (by[k].empty()) continue;
      dev.run(by[k], (Kind)k, &ctr);
      for (Request* q : by[k]) {
        if (q->handled) continue;
        q->ok = cpu_run(q->kind, *q->in, q->out);
        q->handled = true;
        ctr.fallbacks += 1;
        ctr.cpu_messages += 1;
      }
    }
  }

  // Leads device d (busy[d] set by the caller, lk held) until the queue is
  // empty, finishing and waking every request it takes.
  void lead(int d, std::unique_lock<std::mutex>& lk) {
    while (!queue.empty()) {
      std::vector<Request*> batch(queue.begin(), queue.end());
      queue.clear();
      lk.unlock();
      run_batch(*devs[d], batch);
      lk.lock();
      for (Request* q : batch) {
        q->done = true;
        if (q->latch) q->signal(q->latch);
      }
      cv.notify_all();
    }
  }

  // Queues r and returns once it is done; false if no device is running.
  bool submit(Request* r) {
    std::unique_lock<std::mutex> lk(mu);
    if (devs.empty()) return false;
    queue.push_back(r);
    int d = -1;
    for (size_t i = 0; i < busy.size(); ++i)
      if (!busy[i]) {
        d = (int)i;
        break;
      }
    if (d >= 0) {
      busy[d] = 1;
      lead(d, lk);
      busy[d] = 0;
      cv.notify_all();
      return true;
    }
    // follower: a leader (or an explicit batch releasing its device) drains
    // the queue before it lets its device go, so someone finishes r
    if (hooks.create && hooks.wait && hooks.signal && hooks.destroy) {
      const ParkHooks h = hooks;
      r->latch = h.create();
      r->signal = h.signal;
      lk.unlock();
      h.wait(r->latch);
      h.destroy(r->latch);
      lk.lock();
      cv.wait(lk, [&] { return r->done; });  // a latch that woke early
    } else {
      cv.wait(lk, [&] { return r->done; });
    }
    return true;
  }

  bool process(const cord_buf& in, cord_buf* out, Kind kind) {
    // devices start on the first body that needs one: a process whose bodies
    // all stay below the threshold never initialises HIP
    if (in.size() >= min_bytes.load(std::memory_order_relaxed)) {
      ensure_started();
      if (n_devs.load(std::memory_order_relaxed) > 0) {
        Request r{&in, out, kind};
        if (submit(&r)) return r.ok;
      }
    }
    ctr.cpu_messages += 1;
    return cpu_run(kind, in, out);
  }

  // Explicit batches: split by bytes over the devices, each part run on its
  // device as one batch (the part's thread then drains the queue before it
  // releases the device).
  bool explicit_batch(const std::vector<const cord_buf*>& in, const std::vector<cord_buf*>& out,
                      std::vector<bool>* ok, Kind kind) {
    if (in.size() != out.size()) return false;
    ensure_started();
    std::vector<Request> rs(in.size());
    for (size_t i = 0; i < in.size(); ++i) rs[i] = Request{in[i], out[i], kind};
    const size_t nd = (size_t)n_devs.load();
    if (nd == 0) {
      for (auto& r : rs) {
        r.ok = cpu_run(kind, *r.in, r.out);
        ctr.cpu_messages += 1;
      }
    } else {
      // contiguous ranges balanced by input bytes, a body counting 64 more than its size
      std::vector<uint64_t> sizes(rs.size());
      for (size_t i = 0; i < rs.size(); ++i) sizes[i] = rs[i].in->size() + 64;
      const std::vector<size_t> cuts = byte_balanced_cuts(sizes.data(), sizes.size(), nd);
      auto part = [&](size_t p) {
        std::vector<Request*> batch;
        for (size_t i = cuts[p]; i < cuts[p + 1]; ++i) batch.push_back(&rs[i]);
        std::unique_lock<std::mutex> lk(mu);
        const size_t d = p % std::max<size_t>(1, devs.size());
        if (devs.empty()) {
          lk.unlock();
          for (Request* q : batch) {
            q->ok = cpu_run(kind, *q->in, q->out);
            ctr.cpu_messages += 1;
          }
          return;
        }
        cv.wait(lk, [&] { return !busy[d]; });
        busy[d] = 1;
        lk.unlock();
        run_batch(*devs[d], batch);
        lk.lock();
        lead((int)d, lk);
        busy[d] = 0;
        cv.notify_all();
      };
      const size_t parts = cuts.size() - 1;
      if (parts == 1) {
        part(0);
      } else {
        std::vector<std::thread> th;
        for (size_t p = 0; p < parts; ++p) th.emplace_back(part, p);
        for (auto& t : th) t.join();
      }
    }
    ok->assign(rs.size(), false);
    bool all = true;
    for (size_t i = 0; i < rs.size(); ++i) {
      (*ok)[i] = rs[i].ok;
      all = all && rs[i].ok;
    }
    return all;
  }
};

SnappyGpuCodec& SnappyGpuCodec::Instance() {
  static SnappyGpuCodec* inst = new SnappyGpuCodec();  // never destroyed: handlers may run at exit
  return *inst;
}

SnappyGpuCodec::SnappyGpuCodec() : impl_(new Impl) {}

SnappyGpuCodec::~SnappyGpuCodec() { delete impl_; }

int SnappyGpuCodec::InitDevices(uint64_t mask) {
  std::unique_lock<std::mutex> lk(impl_->mu);
  impl_->quiesce(lk);
  impl_->stop_locked();
  return impl_->start_locked(mask ? mask : env_device_mask());
}

void SnappyGpuCodec::Shutdown() {
  std::unique_lock<std::mutex> lk(impl_->mu);
  impl_->quiesce(lk);
  impl_->stop_locked();
  impl_->started.store(true, std::memory_order_release);  // stay on the host codec until InitDevices
  impl_->err = "shut down";
}

bool SnappyGpuCodec::available() {
  impl_->ensure_started();
  return impl_->n_devs.load() > 0;
}

std::string SnappyGpuCodec::error() {
  std::lock_guard<std::mutex> lk(impl_->mu);
  return impl_->err;
}

int SnappyGpuCodec::device_count() {
  impl_->ensure_started();
  return impl_->n_devs.load();
}

void SnappyGpuCodec::SetMinGpuBytes(size_t bytes) { impl_->min_bytes.store(bytes); }
size_t SnappyGpuCodec::min_gpu_bytes() const { return impl_->min_bytes.load(); }

void SnappyGpuCodec::SetParkHooks(const ParkHooks& hooks) {
  std::lock_guard<std::mutex> lk(impl_->mu);
  impl_->hooks = hooks;
}

bool SnappyGpuCodec::Compress(const cord_buf& in, cord_buf* out) { return impl_->process(in, out, kCompress); }
bool SnappyGpuCodec::Uncompress(const cord_buf& in, cord_buf* out) { return impl_->process(in, out, kDecompress); }
bool SnappyGpuCodec::IsValid(const cord_buf& in) { return impl_->process(in, nullptr, kValidate); }

bool SnappyGpuCodec::CompressBatch(const std::vector<const cord_buf*>& in, const std::vector<cord_buf*>& out,
                                   std::vector<bool>* ok) {
  return impl_->explicit_batch(in, out, ok, kCompress);
}

bool SnappyGpuCodec::UncompressBatch(const std::vector<const cord_buf*>& in, const std::vector<cord_buf*>& out,
                                     std::vector<bool>* ok) {
  return impl_->explicit_batch(in, out, ok, kDecompress);
}

CodecStats SnappyGpuCodec::stats() const {
  const Counters& c = impl_->ctr;
  CodecStats s;
  s.batches = c.batches.load();
  s.messages = c.messages.load();
  s.bytes_in = c.bytes_in.load();
  s.bytes_out = c.bytes_out.load();
  s.max_batch = c.max_batch.load();
  s.failures = c.failures.load();
  s.cpu_messages = c.cpu_messages.load();
  s.fallbacks = c.fallbacks.load();
  s.adopted = c.adopted.load();
  s.d2h_bytes = c.d2h_bytes.load();
  s.packed_chunks = c.packed_chunks.load();
  s.device_fallback_messages = c.device_fallback_messages.load();
  s.device_single_pass_messages = c.device_single_pass_messages.load();
  s.device_fallback_batches = c.device_fallback_batches.load();
  return s;
}

size_t PackMinBytesFromEnv() {
  const char* e = getenv("FLARE_SNAPPY_GPU_PACK_MIN_BYTES");
  if (e == nullptr || *e == '\0') return kPackMinBytesDefault;
  char* end = nullptr;
  const unsigned long long v = strtoull(e, &end, 10);
  return end == e ? kPackMinBytesDefault : (size_t)v;  // not a number: the default
}

void InjectDeviceErrorsForTesting(int n) { g_inject_errors.store(n); }

bool CpuCompress(const cord_buf& in, cord_buf* out) { return cpu_run(kCompress, in, out); }
bool CpuUncompress(const cord_buf& in, cord_buf* out) { return cpu_run(kDecompress, in, out); }

}  // namespace flare::gpu
