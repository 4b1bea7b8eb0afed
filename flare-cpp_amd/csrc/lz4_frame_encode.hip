// lz4_frame_encode.hip -- LZ4 frame bodies (LZ4 Frame Format 1.6.x, what
// LZ4F_compressFrame and the lz4 command write) on the batch layout of the
// block codec, the compress side: include/flare_lz4_gpu.h, "LZ4 frames".
//
// A frame with independent blocks is a list of small LZ4 blocks, so the block
// codecs this library already has (lz4.hip, lz4_encode_wave.hip,
// lz4_decode2.hip) run a frame's blocks as if they were messages, called as
// they are on the plans the frame's plan holds for them; the kernels here only
// cut messages into blocks and put frames together.  Workspace layouts,
// capacities and grid sizes: lz4_frame_plan.h (tests/cpp/test_lz4_plan.cc).
//
// Compress: plan (a lane per message: its blocks' columns, staging slots from
// two counters) -> launch_lz4_encode on the block columns -> XXH32 of the
// inputs when a content checksum is asked for, and of every block's bytes as
// stored when block checksums are (the checksum kernel, lz4f_xxh.h: a quad of
// lanes per unit) -> assemble (a wave per message: prefix sum of the stored
// sizes, size words, block copies, block checksums, descriptor, end mark).
#include "launch.h"
#include "lz4_frame_cols.h"
#include "lz4_frame_format.h"
#include "lz4f_xxh.h"

namespace fsg {

namespace {

// ---- workspace header (the first 256 bytes; u32 indices)
constexpr u32 kFcBlocks = 0;    // blocks asked for (past the capacity when a message did not fit)
constexpr u32 kFcRaw = 1;       // blocks stored raw
constexpr u32 kFcOverflow = 2;  // messages whose blocks did not fit the workspace
constexpr u32 kFcListed = 3;    // blocks of the messages that fitted
constexpr u32 kFcStage = 4;     // u64: staging bytes asked for

constexpr u32 kNoFit = 0xFFFFFFFFu;

// (the staging slot of a block, enc_slot: lz4_frame_plan.h)

// every block entry: an empty input and a 64-byte slot of its own, so that
// the entries past the batch's blocks encode to nothing anybody reads
__global__ __launch_bounds__(256) void lz4f_prefill_kernel(BlockCols c, u32 nb_cap, u64 dummy_off) {
  const u32 e = blockIdx.x * 256 + threadIdx.x;
  if (e >= nb_cap) return;
  c.in_off[e] = 0;
  c.in_len[e] = 0;
  c.out_off[e] = dummy_off + 64ull * e;
}

__global__ __launch_bounds__(64) void lz4f_plan_kernel(const u64* __restrict__ in_off, const u32* __restrict__ in_len,
                                                     u32 n_msgs, u32 bs, u32* hdr, MsgCols mc, BlockCols c, u32 nb_cap,
                                                     u64 stage_off, u64 stage_cap) {
  const u32 m = blockIdx.x * 64 + threadIdx.x;
  if (m >= n_msgs) return;
  const u32 n = in_len[m];
  const u32 nb = (u32)(((u64)n + bs - 1) / bs);
  mc.nb[m] = nb;
  mc.first[m] = 0;
  if (nb == 0) return;
  const u32 last = n - (nb - 1) * bs;
  const u64 need = (u64)(nb - 1) * enc_slot(bs) + enc_slot(last);
  const u32 base = atomicAdd(&hdr[kFcBlocks], nb);
  u64 sb = atomicAdd(reinterpret_cast<unsigned long long*>(hdr + kFcStage), (unsigned long long)need);
  if ((u64)base + nb > nb_cap || sb + need > stage_cap) {
    mc.first[m] = kNoFit;
    atomicAdd(&hdr[kFcOverflow], 1u);
    return;
  }
  mc.first[m] = base;
  atomicAdd(&hdr[kFcListed], nb);
  const u64 io = in_off[m];
  for (u32 k = 0; k < nb; ++k) {
    const u32 L = k + 1 < nb ? bs : last;
    c.in_off[base + k] = io + (u64)k * bs;
    c.in_len[base + k] = L;
    c.out_off[base + k] = stage_off + sb;
    sb += enc_slot(L);
  }
}

// ---- units of the checksum kernel (lz4f_xxh.h)
// each body of a batch: the content checksum of compress, fsg_lz4f_xxh32_batch
struct BodyUnits {
  const u8* in;
  const u64* in_off;
  const u32* in_len;
  u32 seed;
  u32* xxh;
  __device__ bool any() const { return true; }
  __device__ bool get(u32 m, const u8** p, u64* n, u32* sd) const {
    *p = in + in_off[m];
    *n = in_len[m];
    *sd = seed;
    return true;
  }
  __device__ void put(u32 m, u32 h) const { xxh[m] = h; }
};

// compress, block checksums: every block entry that holds a block (the
// prefilled rest is empty), over the bytes as stored -- the choice of
// lz4f_assemble_kernel; the word goes to src_len, idle on this side
struct StoredUnits {
  const u8* in;
  const u8* ws;
  BlockCols c;
  __device__ bool any() const { return true; }
  __device__ bool get(u32 e, const u8** p, u64* n, u32* sd) const {
    const u32 L = c.in_len[e];
    if (L == 0) return false;
    const u32 hl = (u32)varint32_len(L);
    const u32 csize = c.out_len[e] - hl;
    const bool raw = csize >= L;
    *p = raw ? in + c.in_off[e] : ws + c.out_off[e] + hl;
    *n = raw ? L : csize;
    *sd = 0;
    return true;
  }
  __device__ void put(u32 e, u32 h) const { c.src_len[e] = h; }
};

// One wave per message: the frame from the staged blocks.
__global__ __launch_bounds__(64) void lz4f_assemble_kernel(const u8* __restrict__ in, const u32* __restrict__ in_len,
                                                         u8* out, const u64* __restrict__ out_off,
                                                         u32* __restrict__ out_len, i32* __restrict__ status, u32 id,
                                                         u32 flags, u32* hdr, MsgCols mc, BlockCols c,
                                                         const u8* ws) {
  const u32 m = blockIdx.x;
  const u32 lane = threadIdx.x;
  const u32 n = in_len[m];
  const u32 first = mc.first[m], nb = mc.nb[m];
  if (first == kNoFit || lz4f::max_frame_length(n, id, flags) > 0xFFFFFFFFull) {
    if (lane == 0) {
      out_len[m] = 0;
      status[m] = kCorrupt;
    }
    return;
  }
  u8* const ob = out + out_off[m];
  if (lane == 0) lz4f::write_header(ob, n, id, flags);
  const u32 bsum = (flags & lz4f::kOptBlockSums) ? 4 : 0;
  u64 pos = n && !(flags & lz4f::kOptNoSize) ? 15 : 7;
  u32 raws = 0;
  for (u32 k0 = 0; k0 < nb; k0 += 64) {
    const u32 k = k0 + lane;
    const bool valid = k < nb;
    u32 L = 0, stored = 0, hl = 0;
    bool raw = false;
    u64 src = 0;
    if (valid) {
      const u32 e = first + k;
      L = c.in_len[e];
      hl = (u32)varint32_len(L);
      const u32 csize = c.out_len[e] - hl;
      raw = csize >= L;
      stored = raw ? L : csize;
      src = raw ? c.in_off[e] : c.out_off[e] + hl;
    }
    const u32 sz = valid ? 4 + stored + bsum : 0;
    const u32 incl = wave_scan(sz);
    const u64 at = pos + (incl - sz);
    if (valid) {
      lz4f::wr32(ob + at, raw ? (L | lz4f::kRawBit) : stored);
      if (bsum) lz4f::wr32(ob + at + 4 + stored, c.src_len[first + k]);
    }
    raws += (u32)__builtin_popcountll(__ballot(valid && raw));
    const u32 cnt = nb - k0 < 64 ? nb - k0 : 64;
    for (u32 j = 0; j < cnt; ++j) {
      const u64 s = __shfl(src, j, 64), a = __shfl(at, j, 64);
      const u32 len = __shfl(stored, j, 64);
      const bool r = __shfl((int)raw, j, 64);
      wave_copy(ob + a + 4, (r ? in : ws) + s, len, lane);
    }
    pos += __shfl(incl, 63, 64);
  }
  if (lane == 0) {
    lz4f::wr32(ob + pos, 0);
    pos += 4;
    if (flags & lz4f::kOptContentSum) {
      lz4f::wr32(ob + pos, mc.xxh[m]);
      pos += 4;
    }
    out_len[m] = (u32)pos;
    status[m] = kOk;
    if (raws) atomicAdd(&hdr[kFcRaw], raws);
  }
}

}  // namespace

void lz4f_encode_header_counts(const void* header, Lz4fEncodeHeaderCounts* c) {
  u32 ctr[8];
  __builtin_memcpy(ctr, header, sizeof(ctr));
  c->blocks = ctr[kFcListed];
  c->raw_blocks = ctr[kFcRaw];
  c->overflow_messages = ctr[kFcOverflow];
}

// every size and decision from lz4f_encode_plan (lz4_frame_plan.h)
hipError_t launch_lz4f_encode(const u8* in, const u64* in_off, const u32* in_len, u32 n_msgs, u8* out,
                              const u64* out_off, u32* out_len, i32* status, u32 id, u32 flags, void* ws,
                              hipStream_t stream, const Lz4fEncodePlan& plan) {
  if (n_msgs == 0) return hipSuccess;
  if (!plan.valid) return hipErrorInvalidValue;
  const Lz4fLayout& p = plan.w;
  u8* const w = static_cast<u8*>(ws);
  u32* const hdr = reinterpret_cast<u32*>(w);
  const MsgCols mc = msg_cols(w + p.off_msg, n_msgs);
  const BlockCols c = block_cols(w + p.off_blk, p.nb_cap);
  const u32 bs = lz4f::block_bytes(id);
  hipError_t e = hipMemsetAsync(w, 0, kLz4fHead, stream);
  if (e != hipSuccess) return e;
  lz4f_prefill_kernel<<<plan.prefill_grid, 256, 0, stream>>>(c, p.nb_cap, p.off_dummy);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  lz4f_plan_kernel<<<plan.plan_grid, 64, 0, stream>>>(in_off, in_len, n_msgs, bs, hdr, mc, c, p.nb_cap, p.off_stage,
                                                     p.stage_cap);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  // the block encoders on the block columns, with their own routing
  e = launch_lz4_encode(in, c.in_off, c.in_len, p.nb_cap, w, c.out_off, c.out_len, c.status, w + p.off_inner, stream,
                        plan.inner);
  if (e != hipSuccess) return e;
  // the checksum kernel: the messages, and the entries' bytes as stored
  if (flags & lz4f::kOptContentSum) {
    if ((e = launch_xxh_quads(BodyUnits{in, in_off, in_len, 0u, mc.xxh}, n_msgs, stream)) != hipSuccess) return e;
  }
  if (flags & lz4f::kOptBlockSums) {
    if ((e = launch_xxh_quads(StoredUnits{in, w, c}, p.nb_cap, stream)) != hipSuccess) return e;
  }
  lz4f_assemble_kernel<<<plan.assemble_grid, 64, 0, stream>>>(in, in_len, out, out_off, out_len, status, id, flags, hdr,
                                                             mc, c, w);
  return hipGetLastError();
}

hipError_t launch_lz4f_xxh32(const u8* in, const u64* in_off, const u32* in_len, u32 n_msgs, u32 seed, u32* xxh,
                             hipStream_t stream) {
  return launch_xxh_quads(BodyUnits{in, in_off, in_len, seed, xxh}, n_msgs, stream);
}

}  // namespace fsg
