// lz4_frame_format.h -- the LZ4 frame format (1.6.x) in plain C++: XXH32, the
// descriptor, the walk over a frame's size words and the serial frame decoder.
// One text for three users: the device code (lz4_frame_encode.hip,
// lz4_frame_decode.hip, where LZ4F_HD is __host__ __device__), the host codec
// (host/lz4_cpu.cc, compiled by g++) and the stand-alone programs that run it
// on the CPU under AddressSanitizer (tests/cpp/lz4f_host_check.hip: the
// decoder; tests/cpp/test_lz4f_walk.cc: the walk under every reader's rules).
// include/flare_lz4_gpu.h states the rules ("LZ4 frames").
#pragma once

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define LZ4F_HD __host__ __device__ inline
#else
#define LZ4F_HD inline
#endif

namespace lz4f {

constexpr uint32_t kMagic = 0x184D2204u;
constexpr uint32_t kRawBit = 0x80000000u;   // block size word: the block is stored raw
constexpr uint32_t kMinBlockId = 4, kMaxBlockId = 7;
constexpr uint64_t kNoSize = ~0ull;         // content size: the frame states none
// status words (include/flare_snappy_gpu.h)
constexpr int32_t kStOk = 0, kStCorrupt = 1, kStBadHeader = 2, kStSlotTooSmall = 3;
// FLG bits
constexpr uint32_t kFlgIndep = 0x20, kFlgBlockSum = 0x10, kFlgSize = 0x08, kFlgSum = 0x04, kFlgReserved = 0x02,
                   kFlgDict = 0x01;

LZ4F_HD uint32_t block_bytes(uint32_t id) { return 1u << (8 + 2 * id); }  // 4..7: 64 KiB, 256 KiB, 1 MiB, 4 MiB

LZ4F_HD uint32_t rd32(const uint8_t* p) {
  return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}
LZ4F_HD void wr32(uint8_t* p, uint32_t v) {
  p[0] = (uint8_t)v;
  p[1] = (uint8_t)(v >> 8);
  p[2] = (uint8_t)(v >> 16);
  p[3] = (uint8_t)(v >> 24);
}

// ---- XXH32
constexpr uint32_t kP1 = 2654435761u, kP2 = 2246822519u, kP3 = 3266489917u, kP4 = 668265263u, kP5 = 374761393u;
LZ4F_HD uint32_t rotl(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }
LZ4F_HD uint32_t xxh_round(uint32_t acc, uint32_t in) { return rotl(acc + in * kP2, 13) * kP1; }

LZ4F_HD uint32_t xxh32(const uint8_t* p, uint64_t n, uint32_t seed = 0) {
  uint64_t i = 0;
  uint32_t h;
  if (n >= 16) {
    uint32_t v1 = seed + kP1 + kP2, v2 = seed + kP2, v3 = seed, v4 = seed - kP1;
    for (; i + 16 <= n; i += 16) {
      v1 = xxh_round(v1, rd32(p + i));
      v2 = xxh_round(v2, rd32(p + i + 4));
      v3 = xxh_round(v3, rd32(p + i + 8));
      v4 = xxh_round(v4, rd32(p + i + 12));
    }
    h = rotl(v1, 1) + rotl(v2, 7) + rotl(v3, 12) + rotl(v4, 18);
  } else {
    h = seed + kP5;
  }
  h += (uint32_t)n;
  for (; i + 4 <= n; i += 4) h = rotl(h + rd32(p + i) * kP3, 17) * kP4;
  for (; i < n; ++i) h = rotl(h + p[i] * kP5, 11) * kP1;
  h ^= h >> 15;
  h *= kP2;
  h ^= h >> 13;
  h *= kP3;
  h ^= h >> 16;
  return h;
}

// ---- descriptor
struct Header {
  uint32_t len;         // bytes up to and including HC
  uint32_t block_max;   // block_bytes(id)
  uint32_t flg;
  uint64_t size;        // content size, kNoSize when the frame states none
};

// kStOk or kStBadHeader: a bad magic number (skippable and legacy ones too),
// version, reserved bit, block size id or HC, a descriptor cut short, DictID.
LZ4F_HD int32_t parse_header(const uint8_t* p, uint64_t n, Header* h) {
  h->size = kNoSize;
  if (n < 7 || rd32(p) != kMagic) return kStBadHeader;
  const uint32_t flg = p[4], bd = p[5];
  if ((flg >> 6) != 1 || (flg & (kFlgReserved | kFlgDict))) return kStBadHeader;
  const uint32_t id = (bd >> 4) & 7;
  if ((bd & 0x8F) || id < kMinBlockId) return kStBadHeader;
  const uint32_t len = 7 + ((flg & kFlgSize) ? 8 : 0);
  if (n < len) return kStBadHeader;
  if (((xxh32(p + 4, len - 5) >> 8) & 0xFF) != p[len - 1]) return kStBadHeader;
  h->len = len;
  h->block_max = block_bytes(id);
  h->flg = flg;
  if (flg & kFlgSize) h->size = (uint64_t)rd32(p + 6) | (uint64_t)rd32(p + 10) << 32;
  return kStOk;
}

// The block size id LZ4F_compressFrame puts in BD: the smallest one, up to
// the id asked for, whose block holds all n bytes (LZ4F_optimalBSID).  The
// blocks are the same either way: such a message is one block.
LZ4F_HD uint32_t frame_block_id(uint64_t n, uint32_t id) {
  uint32_t p = kMinBlockId;
  while (p < id && n > block_bytes(p)) ++p;
  return p;
}

// n bytes forward, 16 at a time then singly; source and destination apart
// (raw blocks, literals)
LZ4F_HD void copy_bytes(uint8_t* d, const uint8_t* s, uint64_t n) {
  uint64_t k = 0;
  for (; k + 16 <= n; k += 16) __builtin_memcpy(d + k, s + k, 16);
  for (; k < n; ++k) d[k] = s[k];
}

// ---- the frame writer: what the compressors, device and host, share
// compress flags (FSG_LZ4F_FLAG_* of include/flare_lz4_gpu.h); the callers reject other bits
constexpr uint32_t kOptContentSum = 1, kOptBlockSums = 2, kOptNoSize = 4;

// The descriptor the compressor writes (independent blocks; block checksums
// and a content checksum as the flags ask; the content size unless kOptNoSize
// is set or n is 0, which LZ4F_compressFrame reads as "unknown"); returns its
// length, 7 or 15.  BD holds the smallest-id rule's id with or without a size.
LZ4F_HD uint32_t write_header(uint8_t* p, uint64_t n, uint32_t id, uint32_t flags) {
  const bool size = n && !(flags & kOptNoSize);
  wr32(p, kMagic);
  p[4] = (uint8_t)(0x40 | kFlgIndep | ((flags & kOptBlockSums) ? kFlgBlockSum : 0) | (size ? kFlgSize : 0) |
                   ((flags & kOptContentSum) ? kFlgSum : 0));
  p[5] = (uint8_t)(frame_block_id(n, id) << 4);
  uint32_t len = 6;
  if (size) {
    wr32(p + 6, (uint32_t)n);
    wr32(p + 10, (uint32_t)(n >> 32));
    len = 14;
  }
  p[len] = (uint8_t)(xxh32(p + 4, len - 4) >> 8);
  return len + 1;
}

// One block at p: the size word, the bytes as stored (the encoded block, or
// the input bytes when `raw`), and with kOptBlockSums the XXH32 of the bytes
// as stored; returns the bytes written.  The serial writer (the host codec);
// the device writes the same fields a wave per message.
LZ4F_HD uint64_t write_block(uint8_t* p, const uint8_t* stored, uint32_t len, bool raw, uint32_t flags) {
  wr32(p, raw ? (len | kRawBit) : len);
  copy_bytes(p + 4, stored, len);
  if (!(flags & kOptBlockSums)) return 4ull + len;
  wr32(p + 4 + len, xxh32(stored, len));
  return 8ull + len;
}

// The end mark, and the content checksum when kOptContentSum asks for it.
LZ4F_HD uint32_t write_end(uint8_t* p, uint32_t flags, uint32_t content_xxh) {
  wr32(p, 0);
  if (!(flags & kOptContentSum)) return 4;
  wr32(p + 4, content_xxh);
  return 8;
}

// Frame bound for the compressor's settings: descriptor 15, a size word per
// block, the bytes themselves (a block that does not shrink is stored raw),
// the end mark and a content checksum.  LZ4F_compressFrameBound gives 19 (its
// largest descriptor, with DictID) in place of 15.
LZ4F_HD uint64_t max_frame_length(uint64_t n, uint32_t id) {
  const uint64_t bs = block_bytes(id);
  return 15 + 4 * ((n + bs - 1) / bs) + n + 4 + 4;
}
// And with the compress flags: a checksum word per block more with
// kOptBlockSums.  (kOptNoSize makes a frame 8 bytes shorter; the bound does
// not follow it.)
LZ4F_HD uint64_t max_frame_length(uint64_t n, uint32_t id, uint32_t flags) {
  const uint64_t bs = block_bytes(id);
  return max_frame_length(n, id) + ((flags & kOptBlockSums) ? 4 * ((n + bs - 1) / bs) : 0);
}

// ---- blocks
// Decoded length of a block from its sequences' lengths alone: the sequence
// whose literals end at the block's last byte is the last one.  false: no such
// sequence, or more than `limit` bytes.
LZ4F_HD bool block_length(const uint8_t* src, uint32_t n, uint64_t limit, uint64_t* len) {
  uint64_t ip = 0, op = 0;
  for (;;) {
    if (ip >= n) return false;
    const uint32_t token = src[ip++];
    uint64_t lit = token >> 4;
    if (lit == 15) {
      uint32_t b;
      do {
        if (ip >= n) return false;
        b = src[ip++];
        lit += b;
      } while (b == 255);
    }
    if (lit > n - ip || op + lit > limit) return false;
    if (ip + lit == n) {
      *len = op + lit;
      return true;
    }
    ip += lit + 2;
    if (ip > n) return false;
    uint64_t ml = (token & 15) + 4;
    if ((token & 15) == 15) {
      uint32_t b;
      do {
        if (ip >= n) return false;
        b = src[ip++];
        ml += b;
      } while (b == 255);
    }
    op += lit + ml;
    if (op > limit) return false;
  }
}

// One block to exactly ulen bytes at dst, by the rules of lz4.hip's
// lz4_decompress_block (the end rules against ulen, offset 0 rejected); a
// match may reach `hist` bytes back before dst (linked blocks: the bytes the
// frame has produced so far; an offset is at most 65,535).
LZ4F_HD bool block_decode(const uint8_t* src, uint32_t n, uint8_t* dst, uint32_t ulen, uint64_t hist) {
  uint32_t ip = 0, op = 0;
  for (;;) {
    if (ip >= n) return false;
    const uint32_t token = src[ip++];
    uint32_t lit = token >> 4;
    if (lit == 15) {
      uint32_t b;
      do {
        if (ip >= n) return false;
        b = src[ip++];
        lit += b;
      } while (b == 255 && lit <= n);
    }
    if (lit > n - ip || lit > ulen - op) return false;
    const bool last = (uint64_t)op + lit + 12 > ulen || (uint64_t)ip + lit + 8 > n;
    if (last && ip + lit != n) return false;
    copy_bytes(dst + op, src + ip, lit);
    if (last) return op + lit == ulen;
    ip += lit;
    op += lit;
    const uint32_t off = (uint32_t)src[ip] | ((uint32_t)src[ip + 1] << 8);
    ip += 2;
    if (off == 0 || off > op + hist) return false;
    uint32_t ml = (token & 15) + 4;
    if ((token & 15) == 15) {
      uint32_t b;
      do {
        if (ip >= n) return false;
        b = src[ip++];
        ml += b;
      } while (b == 255 && ml <= ulen);
    }
    if ((uint64_t)ml + 5 > ulen - op) return false;
    uint8_t* d = dst + op;
    const uint8_t* from = d - off;
    for (uint32_t k = 0; k < ml; ++k) d[k] = from[k];
    op += ml;
  }
}

// The history a linked block can reach: the bytes its frame produced before
// it, as far as an offset goes.
LZ4F_HD uint32_t linked_prefix(uint64_t produced) { return produced < 65535 ? (uint32_t)produced : 65535u; }

// ---- the walk over a frame's size words: the one reader of the block
// structure.  A block's stored bytes lie at in + at; its checksum word, when
// the descriptor flags block checksums, right after them.
struct Block {
  uint64_t at;
  uint32_t size;
  bool raw;
};
struct BlockWalk {
  const uint8_t* in;
  uint64_t n, ip;
  uint32_t block_max, flg;
};
enum WalkStep { kWalkBlock, kWalkEnd, kWalkBad };

LZ4F_HD BlockWalk begin_blocks(const uint8_t* in, uint64_t n, const Header& h) {
  return BlockWalk{in, n, h.len, h.block_max, h.flg};
}
LZ4F_HD uint32_t block_sum_bytes(uint32_t flg) { return (flg & kFlgBlockSum) ? 4 : 0; }

// kWalkBad: no size word left, a size above the block maximum, or the stored
// bytes with their checksum word not inside the input.  kWalkEnd: the end mark.
// kChecked = false: nothing tested, no branch at the load (a second pass over counted blocks).
template <bool kChecked = true>
LZ4F_HD WalkStep next_block(BlockWalk* w, Block* b) {
  if (kChecked && w->n - w->ip < 4) return kWalkBad;
  const uint32_t word = rd32(w->in + w->ip);
  w->ip += 4;
  if (kChecked && word == 0) return kWalkEnd;
  b->at = w->ip;
  b->size = word & ~kRawBit;
  b->raw = word & kRawBit;
  const uint64_t stored = (uint64_t)b->size + block_sum_bytes(w->flg);
  if (kChecked && (b->size > w->block_max || w->n - w->ip < stored)) return kWalkBad;
  w->ip += stored;
  return kWalkBlock;
}

// After kWalkEnd: the content checksum word when the descriptor flags one
// (*stated_xxh, else 0; not verified), and nothing after the frame.
LZ4F_HD bool end_frame(BlockWalk* w, uint32_t* stated_xxh) {
  *stated_xxh = 0;
  if (w->flg & kFlgSum) {
    if (w->n - w->ip < 4) return false;
    *stated_xxh = rd32(w->in + w->ip);
    w->ip += 4;
  }
  return w->ip == w->n;
}

// What a block-parallel reader asks of the structure beyond the walk's own
// rules.  (A block of size 0 is a raw one: the word 0 is the end mark.)
struct BlockRules {
  bool zero_raw;  // an empty raw block is accepted (the lengths call, as the serial decoder does)
  bool sized;     // the sized fast route: ceil(content size / block maximum) blocks, a raw one as long as its place
};

// The whole structure of a frame by `rules`: each(block) for every block in
// order, then *nb blocks and *stated_xxh (end_frame).  false: rejected.
template <typename Each>
LZ4F_HD bool check_blocks(const uint8_t* in, uint64_t n, const Header& h, BlockRules rules, Each each, uint32_t* nb,
                          uint32_t* stated_xxh) {
  const uint64_t bs = h.block_max;
  const uint32_t want = rules.sized ? (uint32_t)((h.size + bs - 1) / bs) : 0xFFFFFFFFu;
  BlockWalk w = begin_blocks(in, n, h);
  Block b;
  uint32_t k = 0;
  WalkStep s;
  for (; (s = next_block(&w, &b)) == kWalkBlock; ++k) {
    if (k == want) return false;
    if (b.size == 0 && !rules.zero_raw) return false;
    if (rules.sized && b.raw && b.size != (h.size - k * bs < bs ? h.size - k * bs : bs)) return false;
    each(b);
  }
  if (s != kWalkEnd || (rules.sized && k != want)) return false;
  *nb = k;
  return end_frame(&w, stated_xxh);
}

// The decoded length of a frame without a content size, from its blocks'
// sequences: the walk's rules, block_length against the block maximum, no
// checksum verified.  false: the frame is corrupt.
LZ4F_HD bool blocks_decoded_length(const uint8_t* in, uint64_t n, const Header& h, uint64_t* total) {
  BlockWalk w = begin_blocks(in, n, h);
  Block b;
  WalkStep s;
  uint32_t xxh;
  for (*total = 0; (s = next_block(&w, &b)) == kWalkBlock;) {
    uint64_t len = b.size;
    if (!b.raw && !block_length(in + b.at, b.size, h.block_max, &len)) return false;
    *total += len;
  }
  return s == kWalkEnd && end_frame(&w, &xxh);
}

// ---- the serial frame decoder: one frame per body, every write below
// out + cap.  *out_len: the decoded length on kStOk, min(content size, 2^32-1)
// on kStSlotTooSmall, else 0.  *checksums (may be null): block and content
// checksums verified.
LZ4F_HD int32_t decode_frame(const uint8_t* in, uint64_t n, uint8_t* out, uint64_t cap, uint32_t* out_len,
                             uint32_t* checksums = nullptr) {
  *out_len = 0;
  Header h;
  if (parse_header(in, n, &h) != kStOk) return kStBadHeader;
  if (h.size != kNoSize && h.size > cap) {
    *out_len = h.size > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)h.size;
    return kStSlotTooSmall;
  }
  const uint64_t limit = h.size != kNoSize ? h.size : cap;
  BlockWalk w = begin_blocks(in, n, h);
  Block b;
  WalkStep s;
  uint64_t op = 0;
  uint32_t sums = 0, stated;
  while ((s = next_block(&w, &b)) == kWalkBlock) {
    const uint8_t* blk = in + b.at;
    if (h.flg & kFlgBlockSum) {
      if (xxh32(blk, b.size) != rd32(blk + b.size)) return kStCorrupt;
      ++sums;
    }
    if (b.raw) {
      if (b.size > limit - op) return kStCorrupt;
      copy_bytes(out + op, blk, b.size);
      op += b.size;
      continue;
    }
    const uint64_t room = limit - op < h.block_max ? limit - op : h.block_max;
    uint64_t len;
    if (!block_length(blk, b.size, room, &len)) return kStCorrupt;
    if (!block_decode(blk, b.size, out + op, (uint32_t)len, (h.flg & kFlgIndep) ? 0 : op)) return kStCorrupt;
    op += len;
  }
  if (s != kWalkEnd || !end_frame(&w, &stated)) return kStCorrupt;
  if (h.flg & kFlgSum) {
    if (xxh32(out, op) != stated) return kStCorrupt;
    ++sums;
  }
  if (h.size != kNoSize && op != h.size) return kStCorrupt;
  *out_len = (uint32_t)op;
  if (checksums) *checksums = sums;
  return kStOk;
}

}  // namespace lz4f
