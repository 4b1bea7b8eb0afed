// lz4_cpu.h -- the host-side LZ4 codec of the drop-in (COMPRESS_TYPE_LZ4,
// /root/reference/flare/rpc/options.proto:74, for which the reference
// registers no handler).  Body = varint32 uncompressed length + one LZ4
// block (include/flare_lz4_gpu.h).  Blocks are those of LZ4 1.9.x
// LZ4_compress_default (acceleration 1; 8,192 16-bit positions hashed from 4
// bytes below 65,547 input bytes, 4,096 32-bit positions hashed from 5 bytes
// above), so they equal the GPU kernels' (csrc/lz4.hip) and liblz4's.
// Product code, independent of oracle/lz4_oracle.c.
#pragma once

#include <cstddef>
#include <cstdint>

namespace flare::lz4::cpu {

constexpr size_t kMaxInput = 0x7E000000;  // LZ4_MAX_INPUT_SIZE

// LZ4_compressBound, and the body bound (5 header bytes more).
inline size_t BlockBound(size_t n) { return n + n / 255 + 16; }
inline size_t MaxCompressedLength(size_t n) { return 5 + BlockBound(n); }

// The most a valid block of n bytes can decode to: every byte of a length
// extension adds at most 255 output bytes, a token with its 2-byte offset at
// most 34.  A body whose header claims more is rejected before anything is
// allocated for it.
inline bool PlausibleLength(uint64_t ulen, size_t block_bytes) {
  return ulen <= 255ull * block_bytes + 64;
}

// One block of n <= kMaxInput bytes into out (BlockBound(n) bytes); returns
// its length.
size_t CompressBlock(const uint8_t* in, size_t n, uint8_t* out);

// One block of n bytes to exactly ulen bytes; false when the block is
// invalid (include/flare_lz4_gpu.h states the rules).
bool DecompressBlock(const uint8_t* in, size_t n, uint8_t* out, size_t ulen);

// Body = header + block.  Compress returns the body length (0 above
// kMaxInput); ReadHeader returns the header length or 0.
size_t Compress(const uint8_t* in, size_t n, uint8_t* out);
size_t ReadHeader(const uint8_t* in, size_t n, uint32_t* ulen);

// ---- LZ4 frames (LZ4 Frame Format 1.6.x; include/flare_lz4_gpu.h, "LZ4
// frames", states the rules).  Same bytes and verdicts as the GPU calls.
uint32_t Xxh32(const uint8_t* in, size_t n, uint32_t seed = 0);
// n + 4 * ceil(n / block size) + 23; 0 for an id outside 4..7
size_t MaxFrameLength(size_t n, int block_size_id);
// The bytes of LZ4F_compressFrame (independent blocks, content size, level 0,
// no block checksums) into out (MaxFrameLength bytes); returns the length.
size_t CompressFrame(const uint8_t* in, size_t n, uint8_t* out, int block_size_id, bool content_checksum);
// The same with a flags word (FSG_LZ4F_FLAG_*; `true` above is bit 0): a
// content checksum, a checksum behind every block over its bytes as stored,
// no content size -- the frame preferences of LZ4F_compressFrame, byte for
// byte.  out: MaxFrameLength(n, id, flags) bytes, 4 per block more with
// kFrameBlockChecksums.  Both return 0 for a flags word with any other bit.
constexpr uint32_t kFrameContentChecksum = 1, kFrameBlockChecksums = 2, kFrameNoContentSize = 4;
size_t MaxFrameLength(size_t n, int block_size_id, uint32_t flags);
size_t CompressFrame(const uint8_t* in, size_t n, uint8_t* out, int block_size_id, uint32_t flags);
// One frame to out (cap bytes): 0 ok, 1 corrupt, 2 bad header, 3 content size
// above cap (the FSG_* status words); *out_len as d_out_len of the GPU call.
int DecompressFrame(const uint8_t* in, size_t n, uint8_t* out, size_t cap, uint32_t* out_len);
// The descriptor's content size (~0 when it states none); *status 0 or 2.
uint64_t FrameContentSize(const uint8_t* in, size_t n, int* status);
// The decoded length of a frame as fsg_lz4f_decoded_lengths_batch gives it:
// the stated content size, or for a frame that states none the sum of its
// blocks' decoded lengths (lz4f::block_length; a raw block's stored size),
// linked blocks or not.  *status 0, 2 (bad header) or 1 (broken block
// structure, a block without a length; the result is 0).  No checksum is
// looked at and nothing is decoded: status 0 does not promise that the frame
// decodes.
uint64_t FrameDecodedLength(const uint8_t* in, size_t n, int* status);

}  // namespace flare::lz4::cpu
