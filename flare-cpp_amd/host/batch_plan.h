// batch_plan.h -- the host runtime's device batch (gpu_codec.cc, Device::run)
// as plain host arithmetic: which bodies the device takes, where each one's
// input and output slot lie, where the batch is cut into chunks, which chunks
// pack their outputs on the device, the layout of the shared D2H target and
// of a packed chunk, the metadata and gather column views, and the split of
// an explicit batch across devices.  No HIP include and no cord_buf:
// Device::run fills one PlanBody per request and drives its stages from the
// plan; tests/cpp/test_batch_plan.cc checks it on the CPU.  DESIGN.md
// section 1, "Host C++ mirror".
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace flare::gpu {

enum Kind { kCompress = 0, kDecompress = 1, kValidate = 2 };

inline size_t align16(size_t x) { return (x + 15) & ~size_t(15); }

// A valid stream expands at most 64/3x (a 3-byte COPY_2 of length 64) plus
// its header: a longer header length cannot decode (the reference would run
// out of input and return false), so nothing is allocated for it.
inline bool plausible_length(uint32_t ulen, size_t in_len) { return (uint64_t)ulen <= 22ull * in_len + 64; }

// The value of fsg_max_compressed_length (the GPU library's, which this
// header cannot call; tests/cpp/test_rpc_snappy_compress.cc ties the two).
inline size_t max_compressed_length(size_t n) { return 32 + n + n / 6; }

// The status of a body the device coded (FSG_OK, include/flare_snappy_gpu.h).
constexpr int32_t kStatusOk = 0;

// ---- column views
// Metadata columns, back to back in this order on host and device (a
// one-chunk batch copies in_off..out_cap up as one span of 24n bytes and
// out_len..status down as one of 8n bytes, so the order and the packing are
// load-bearing):
//   in_off u64[n] | out_off u64[n] | in_len u32[n] | out_cap u32[n] | out_len u32[n] | status i32[n]
struct MetaColumns {
  uint64_t* in_off;
  uint64_t* out_off;
  uint32_t* in_len;
  uint32_t* out_cap;
  uint32_t* out_len;
  int32_t* status;

  static constexpr size_t kInOff = 0, kOutOff = 8, kInLen = 16, kOutCap = 20, kOutLen = 24, kStatus = 28;
  static constexpr size_t kBytesPerBody = 32, kUpBytesPerBody = 24, kDownBytesPerBody = 8;
  static_assert(kOutOff == kInOff + 8 && kInLen == kOutOff + 8 && kOutCap == kInLen + 4 && kOutLen == kOutCap + 4 &&
                    kStatus == kOutLen + 4 && kBytesPerBody == kStatus + 4 && kUpBytesPerBody == kOutLen - kInOff &&
                    kDownBytesPerBody == kBytesPerBody - kOutLen,
                "the combined H2D (24n bytes from in_off) and D2H (8n bytes from out_len) copies need these "
                "columns contiguous and in this order");

  // The columns of n bodies in the buffer at `base` (host or device memory).
  static MetaColumns at(void* base, size_t n) {
    uint8_t* m = static_cast<uint8_t*>(base);
    return MetaColumns{reinterpret_cast<uint64_t*>(m + kInOff * n),  reinterpret_cast<uint64_t*>(m + kOutOff * n),
                       reinterpret_cast<uint32_t*>(m + kInLen * n),  reinterpret_cast<uint32_t*>(m + kOutCap * n),
                       reinterpret_cast<uint32_t*>(m + kOutLen * n), reinterpret_cast<int32_t*>(m + kStatus * n)};
  }
};

// Pinned-block descriptors of the device gather, one per backing block:
//   src u64[n_blk] | dst offset u64[n_blk] | length u32[n_blk] (0 = staged)
struct GatherColumns {
  uint64_t* src;
  uint64_t* dst;
  uint32_t* len;

  static constexpr size_t kBytesPerBlock = 8 + 8 + 4;

  static GatherColumns at(void* base, size_t n_blk) {
    uint8_t* g = static_cast<uint8_t*>(base);
    return GatherColumns{reinterpret_cast<uint64_t*>(g), reinterpret_cast<uint64_t*>(g + 8 * n_blk),
                         reinterpret_cast<uint32_t*>(g + 16 * n_blk)};
  }
};

// ---- the plan
// What the plan needs to know of one body.  For decode kinds, header_ok and
// ulen are the verdict and the value of the lenient length-header parse of
// the body's first bytes; compress ignores both.
struct PlanBody {
  uint64_t len;     // input bytes
  uint32_t blocks;  // backing blocks (gather descriptors)
  uint32_t ulen;
  bool header_ok;
};

struct BatchPlan {
  // 0: the device codes it; 1: the header already decides it (the reference
  // returns false); 2: beyond the u32 formats, the host codec takes it
  std::vector<uint8_t> skip;
  std::vector<uint32_t> blk_base;  // [n + 1]: first gather descriptor of each body
  // the host metadata columns (skipped bodies: length and capacity 0, and
  // they advance neither offset)
  std::vector<uint64_t> in_off, out_off;
  std::vector<uint32_t> in_len, out_cap;
  size_t pos_in = 0, pos_out = 0;  // ends of the input and the output slots
  // chunks: body ranges [cut[k], cut[k + 1]) of >= chunk_bytes of input offsets
  std::vector<uint32_t> cut;
  // Which chunks pack their outputs on the device.  The others download
  // their slot ranges, back to back in chunk order (hbase), into one D2H
  // target of host_out bytes.  A packed chunk gets a target of its own once
  // its total is known (packed_layout).
  std::vector<uint8_t> packed;
  std::vector<size_t> hbase;
  size_t host_out = 0;
  bool any_packed = false, any_unpacked = false;
  // buffer sizes (the caller adds its own slack)
  size_t total_in = 0, total_out = 0, meta_bytes = 0, gath_bytes = 0;

  size_t n_chunks() const { return cut.size() - 1; }
  // chunk k's input and output slot ranges
  size_t in_begin(size_t k) const { return in_off[cut[k]]; }
  size_t in_end(size_t k) const { return cut[k + 1] < in_off.size() ? in_off[cut[k + 1]] : pos_in; }
  size_t out_begin(size_t k) const { return out_off[cut[k]]; }
  size_t out_end(size_t k) const { return cut[k + 1] < out_off.size() ? out_off[cut[k + 1]] : pos_out; }
};

// n >= 1 bodies of one kind.  chunk_bytes >= 1.
inline BatchPlan plan_batch(Kind kind, const PlanBody* bodies, uint32_t n, size_t chunk_bytes,
                            size_t pack_min_bytes) {
  const bool compress = kind == kCompress, validate = kind == kValidate;
  BatchPlan p;
  p.skip.assign(n, 0);
  p.blk_base.assign(n + 1, 0);
  p.in_off.resize(n);
  p.out_off.resize(n);
  p.in_len.resize(n);
  p.out_cap.resize(n);
  // ---- layout; bodies whose verdict the header already decides are skipped
  for (uint32_t i = 0; i < n; ++i) {
    const PlanBody& b = bodies[i];
    p.in_off[i] = p.pos_in;
    p.out_off[i] = p.pos_out;
    p.in_len[i] = 0;
    p.out_cap[i] = 0;
    p.blk_base[i + 1] = p.blk_base[i];
    // beyond the format's uint32 lengths, or (compress) a worst-case output
    // the u32 slot sizes cannot describe: the host codec takes these
    if (b.len > 0xffffffffu || (compress && max_compressed_length(b.len) > 0xffffffffu)) {
      p.skip[i] = 2;
      continue;
    }
    if (!compress && (!b.header_ok || !plausible_length(b.ulen, b.len))) {
      p.skip[i] = 1;  // the reference returns false
      continue;
    }
    p.blk_base[i + 1] += b.blocks;
    p.in_len[i] = (uint32_t)b.len;
    p.pos_in += align16(b.len);
    const size_t cap = compress ? max_compressed_length(b.len) : (validate ? 0 : b.ulen);
    p.out_cap[i] = (uint32_t)cap;
    p.pos_out += align16(cap);
  }
  p.total_in = p.pos_in;
  p.total_out = p.pos_out;
  p.meta_bytes = (size_t)n * MetaColumns::kBytesPerBody;
  p.gath_bytes = (size_t)p.blk_base[n] * GatherColumns::kBytesPerBlock;
  // ---- chunks
  p.cut.push_back(0);
  for (uint32_t i = 0; i < n; ++i)
    if (i + 1 < n && p.in_off[i + 1] - p.in_off[p.cut.back()] >= chunk_bytes) p.cut.push_back(i + 1);
  p.cut.push_back(n);
  // ---- packed or not, and the unpacked chunks' places in the D2H target
  p.packed.assign(p.n_chunks(), 0);
  p.hbase.assign(p.n_chunks(), 0);
  for (size_t k = 0; k < p.n_chunks(); ++k) {
    const size_t oa = p.out_begin(k), ob = p.out_end(k);
    if (compress && ob > oa && ob - oa >= pack_min_bytes) {
      p.packed[k] = 1;
      p.any_packed = true;
    } else {
      p.hbase[k] = p.host_out;
      p.host_out += ob - oa;
      p.any_unpacked = true;
    }
  }
  return p;
}

// A packed chunk's outputs as the device's pack pass lays them out: bodies
// [a, b) back to back, each 16-byte aligned, a rejected body taking no room.
// poff[i - a] receives body i's offset; returns the total, which must equal
// the device's.
inline uint64_t packed_layout(const int32_t* status, const uint32_t* out_len, uint32_t a, uint32_t b,
                              uint64_t* poff) {
  uint64_t tot = 0;
  for (uint32_t i = a; i < b; ++i) {
    poff[i - a] = tot;
    tot += align16(status[i] != kStatusOk ? 0 : out_len[i]);
  }
  return tot;
}

// An explicit batch across `parts` devices: cuts {0, ..., n} of at most
// `parts` contiguous ranges balanced by `sizes` (shard.byte_balanced_ranges).
// Range r ends at the first body whose prefix reaches r / parts of the total,
// and a body ends one range at most, so no range is empty.
inline std::vector<size_t> byte_balanced_cuts(const uint64_t* sizes, size_t n, size_t parts) {
  uint64_t total = 0;
  for (size_t i = 0; i < n; ++i) total += sizes[i];
  std::vector<size_t> cuts{0};
  uint64_t acc = 0;
  for (size_t i = 0; i < n && cuts.size() < parts; ++i) {
    acc += sizes[i];
    if (acc * parts >= total * cuts.size() && i + 1 < n) cuts.push_back(i + 1);
  }
  cuts.push_back(n);
  return cuts;
}

}  // namespace flare::gpu
