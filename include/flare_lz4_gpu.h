/*
 * flare_lz4_gpu.h -- batched LZ4 block codec on MI355X (gfx950), in
 * libflare_snappy_gpu.so next to the Snappy calls (include/flare_snappy_gpu.h:
 * same batch layout, same status words, same fsg_init / fsg_last_error).
 *
 * Reference interface: none to replace.  The reference names
 * COMPRESS_TYPE_LZ4 = 4 (flare/rpc/options.proto:74) but registers no
 * handler for it (flare/rpc/compress.cc:26-103 holds only what
 * RegisterCompressHandler is given; flare/rpc/global.cc:372-376 registers
 * Snappy/gzip/zlib).  These calls and host/lz4_compress.cc are the handler a
 * maintainer would register at that slot.
 *
 * RPC body (our definition): varint32 of the uncompressed length, then one
 * LZ4 block.  Blocks are byte-equal to LZ4 1.9.x LZ4_compress_default; the
 * decoder accepts exactly the blocks LZ4_decompress_safe(dst capacity =
 * uncompressed length) accepts, except a match of offset 0 (rejected here).
 *
 * What the calls write: the contract of flare_snappy_gpu.h ("What a *_batch
 * call writes") holds here unchanged.  No byte of d_out outside the slots
 * [d_out_off[i], d_out_off[i] + cap_i) is written, with cap_i = d_out_cap[i]
 * for the decode calls (0 allowed) and fsg_lz4_max_compressed_length(
 * d_in_len[i]) for fsg_lz4_compress_batch; slots need no alignment and may
 * touch.  Inside a slot the bytes at and past d_out_len[i] are unspecified
 * (the compressor's headroom, a decode slot larger than the body), as is the
 * whole slot for any status other than FSG_OK.  d_out_len and d_status get
 * exactly n_msgs entries, nothing is written past workspace_bytes, and the
 * input arrays are not written.
 */
#ifndef FLARE_LZ4_GPU_H_
#define FLARE_LZ4_GPU_H_

#include <stddef.h>
#include <stdint.h>

#include "flare_snappy_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Output slot size of one body: 5 (header) + LZ4_compressBound(n). */
size_t fsg_lz4_max_compressed_length(size_t n);

/* Device workspace for fsg_lz4_compress_batch: a 256-byte header, a u32
 * list of n_msgs entries (rounded up to 256 bytes), then 16 KiB of position
 * table per message.  The call zeroes what it uses. */
size_t fsg_lz4_compress_workspace_bytes(uint32_t n_msgs);

/* Batched compress: message i is d_in[d_in_off[i] .. +d_in_len[i]); its body
 * is written to d_out[d_out_off[i] ..] (slot of
 * fsg_lz4_max_compressed_length(d_in_len[i]) bytes, slots disjoint);
 * d_out_len[i] = body length, d_status[i] FSG_OK (FSG_CORRUPT above
 * 0x7E000000 input bytes, LZ4_MAX_INPUT_SIZE).
 *
 * Routing.  Two encoders write the same bytes: one lane per message, and one
 * wave per message with the position table in LDS (64 probes of the match
 * search at a time).  A list kernel names the bodies of at least wave_min
 * bytes; the wave encoder takes those, the lanes the rest, both on `stream`.
 * wave_min is option lz4_encode_wave_min (FSG_L4_ENC_WAVE_MIN): -1 automatic
 * (the measured threshold), 0 every body on the waves,
 * 0xFFFFFFFF or more none.  Option lz4_encode_wave_per_cu
 * (FSG_L4_ENC_WAVE_PER_CU) caps the wave encoder's resident waves per CU (0:
 * as many as LDS holds, 16 KiB a wave).
 *
 * Workspace rule.  With fsg_lz4_compress_workspace_bytes(n_msgs) bytes or
 * more the call routes as above.  A workspace of the earlier size, 16 KiB *
 * n_msgs, is still accepted: the lanes encode every body, with the earlier
 * layout.  Too small a workspace never changes bytes.  A NULL or smaller
 * workspace is FSG_ERR_INVALID_ARG. */
int fsg_lz4_compress_batch(const uint8_t *d_in, const uint64_t *d_in_off,
                           const uint32_t *d_in_len, uint32_t n_msgs,
                           uint8_t *d_out, const uint64_t *d_out_off,
                           uint32_t *d_out_len, int32_t *d_status,
                           void *d_workspace, size_t workspace_bytes,
                           void *stream);

/* Batched decompress: bodies in, d_out[d_out_off[i] ..] with capacity
 * d_out_cap[i]; d_out_len[i] = the header's length; d_status[i]: FSG_OK,
 * FSG_CORRUPT, FSG_BAD_HEADER (varint32, at most 5 bytes), or
 * FSG_SLOT_TOO_SMALL. */
int fsg_lz4_decompress_batch(const uint8_t *d_in, const uint64_t *d_in_off,
                             const uint32_t *d_in_len, uint32_t n_msgs,
                             uint8_t *d_out, const uint64_t *d_out_off,
                             const uint32_t *d_out_cap, uint32_t *d_out_len,
                             int32_t *d_status, void *stream);

/* Device workspace for fsg_lz4_decompress_batch_ws: counters, two u32 per
 * message and the sequence bitmap (one bit per block byte). */
size_t fsg_lz4_decompress_workspace_bytes(uint32_t n_msgs, uint64_t total_in_bytes);

/* fsg_lz4_decompress_batch (same arguments, statuses and bytes) on the
 * two-pass decoder: a lane-per-message index pass (validation + sequence
 * bitmap; blocks over 64 KiB, or over 2 KiB in batches of <= 256 messages,
 * indexed by a wave each), then a wave-per-message execution pass.  Messages whose bitmap
 * does not fit the workspace, or every message when d_workspace is NULL or
 * smaller than fsg_lz4_decompress_workspace_bytes(n_msgs, 0), run the
 * one-pass kernel. */
int fsg_lz4_decompress_batch_ws(const uint8_t *d_in, const uint64_t *d_in_off,
                                const uint32_t *d_in_len, uint32_t n_msgs,
                                uint8_t *d_out, const uint64_t *d_out_off,
                                const uint32_t *d_out_cap, uint32_t *d_out_len,
                                int32_t *d_status, void *d_workspace,
                                size_t workspace_bytes, void *stream);

/* fsg_lz4_decompress_batch_ws in two streams: the index pass (validation +
 * sequence bitmap) on `pass1_stream`, the execution and fallback passes on
 * `stream` behind an event, so that batch k+1's index pass (latency-bound,
 * one lane per message) runs beside batch k's execution (issue-bound) when
 * the two batches have their own workspace, output, d_out_len and d_status
 * buffers.  The inputs must be ready on `pass1_stream`; calls sharing any of
 * those buffers must be ordered by the caller.  Results are valid once
 * `stream` is synchronised.  Same statuses and bytes as
 * fsg_lz4_decompress_batch.  (Snappy's counterpart: fsg_decompress_batch_2s.) */
int fsg_lz4_decompress_batch_2s(const uint8_t *d_in, const uint64_t *d_in_off,
                                const uint32_t *d_in_len, uint32_t n_msgs,
                                uint8_t *d_out, const uint64_t *d_out_off,
                                const uint32_t *d_out_cap, uint32_t *d_out_len,
                                int32_t *d_status, void *d_workspace,
                                size_t workspace_bytes, void *stream,
                                void *pass1_stream);

/* Path report of fsg_lz4_decompress_batch_ws / _2s (see "Path reports" in
 * flare_snappy_gpu.h: a host copy of the workspace's first 256 bytes, the
 * same limits).  path 0: the two-pass decoder, fallback_messages =
 * fallback_bitmap = the messages its one-pass kernel finished; path 1: no
 * usable workspace, every message on the one-pass kernel (by design: it is
 * what fsg_lz4_decompress_batch runs).  The packed-pass causes and
 * huge_messages stay 0. */
int fsg_lz4_decompress_report(const void *header_host_copy, uint32_t n_msgs, size_t workspace_bytes,
                              struct fsg_decode_report *out);

/* Path report of fsg_lz4_compress_batch ("Path reports" in
 * flare_snappy_gpu.h: host code without a HIP call, from a host copy of the
 * workspace's first 256 bytes taken after the call has completed;
 * header_host_copy may be NULL when path is 1 or n_msgs is 0).  It repeats
 * the call's routing expression, so it must be asked with the same n_msgs and
 * workspace_bytes and before the options change.  wave_messages and
 * wave_bytes are counted on the device by the wave encoder. */
struct fsg_lz4_encode_report {
  uint64_t path;           /* 0: list + lanes + waves; 1: old-size workspace, lanes only */
  uint64_t lane_messages;
  uint64_t wave_messages;  /* bodies the wave kernel encoded (counted on the device) */
  uint64_t wave_bytes;     /* their input bytes */
  uint64_t wave_min;       /* threshold the call used (0xFFFFFFFF: no body on the waves) */
};
int fsg_lz4_compress_report(const void *header_host_copy, uint32_t n_msgs,
                            size_t workspace_bytes,
                            struct fsg_lz4_encode_report *out);

/* ------------------------------------------------------------------------
 * LZ4 frames: bodies in the LZ4 Frame Format 1.6.x, which LZ4F_compressFrame
 * and the lz4 command write and read.  The body format above is untouched.
 *
 * Descriptor.  Magic 0x184D2204 (little endian); FLG = version 01 (bits 7-6),
 * B.Indep (5), B.Checksum (4), C.Size (3), C.Checksum (2), reserved 0 (1),
 * DictID (0); BD = block size id 4..7 in bits 6-4 (64 KiB, 256 KiB, 1 MiB,
 * 4 MiB), every other bit 0; the 8-byte content size when C.Size is set;
 * HC = (XXH32(descriptor bytes from FLG through the last optional field,
 * seed 0) >> 8) & 0xFF.  Then blocks: a 4-byte size word (bit 31: stored raw),
 * the bytes, a 4-byte XXH32 of the bytes as stored when B.Checksum is set;
 * a zero size word ends them; then the XXH32 of the content when C.Checksum
 * is set.
 *
 * The compressor writes exactly the bytes of LZ4F_compressFrame (liblz4
 * 1.9.x) with blockMode = independent, blockSizeID as asked for, compression
 * level 0, and the three frame preferences the flags of
 * fsg_lz4f_compress_batch_flags name: every block is
 * LZ4_compress_default of its bytes, stored raw when that is not shorter than
 * they are.
 *   FSG_LZ4F_FLAG_CONTENT_CHECKSUM (contentChecksumFlag): C.Checksum is set
 *     and the XXH32 of the message follows the end mark.
 *   FSG_LZ4F_FLAG_BLOCK_CHECKSUMS (blockChecksumFlag): B.Checksum is set and
 *     every block is followed by the XXH32 of its bytes as stored -- the
 *     encoded block, or the message's own bytes when the block is stored raw.
 *   FSG_LZ4F_FLAG_NO_CONTENT_SIZE (contentSize = 0): no C.Size bit and no
 *     size field, 8 bytes less; without it contentSize = n.
 * Nothing else depends on the flags: the blocks, the size words and BD are
 * the same for all eight combinations.  With bits 0 and 2 this is what the lz4
 * command writes by default.  As in liblz4, BD holds the smallest id, up to
 * the one asked for, whose block holds the whole message (a message of at most
 * 64 KiB says id 4 whatever was asked), with or without a content size.  An
 * empty message has no C.Size field and no blocks (liblz4 reads contentSize 0
 * as "unknown"): 11 bytes, 15 with a content checksum.  A flags word with a
 * bit above the three is FSG_ERR_INVALID_ARG.  fsg_lz4f_compress_batch, the
 * call from before bits 1 and 2 had a meaning, takes bit 0 alone and keeps
 * answering FSG_ERR_INVALID_ARG to every other bit, so nothing changes for a
 * caller of it; with flags 0 or 1 the two calls are the same call.
 *
 * Checksums.  Every XXH32 over message or block bytes -- the content and block
 * checksums the compressor writes, the block checksums of the entries a fast
 * route lists and the content checksum of every frame pending on one in the
 * decompressor, fsg_lz4f_xxh32_batch -- is computed by one kernel, a quad of
 * lanes per byte range (csrc/lz4f_xxh.h).  The serial decoder and the
 * descriptor's HC byte use the serial text (csrc/lz4_frame_format.h).
 *
 * The decompressor accepts one frame per body; bytes after it are
 * FSG_CORRUPT.  FSG_BAD_HEADER: a bad magic number (the skippable and legacy
 * ones included), version, reserved bit, block size id below 4 or HC, a
 * descriptor cut short, DictID set (no dictionaries here).  A content size
 * above d_out_cap[i] is FSG_SLOT_TOO_SMALL with d_out_len[i] = min(content
 * size, 2^32 - 1).  Everything else wrong is FSG_CORRUPT (d_out_len[i] = 0): a
 * size word above the block maximum, input that ends early, a block that does
 * not decode, a checksum mismatch, decoded length != content size, output
 * past the capacity when no content size is given.  A block is judged as the
 * block decoder above judges it, with capacity equal to the block's decoded
 * length (the sequence whose literals end at the block's last byte ends it);
 * offset 0 is rejected; with linked blocks (B.Indep 0) an offset may reach
 * into the earlier blocks' output, as far as the frame has produced.  Every
 * frame this accepts liblz4 accepts with the same bytes; liblz4 also accepts a
 * few this rejects, because it applies the block end rule against a larger
 * capacity.  On FSG_OK d_out_len[i] is the decoded length.
 *
 * Routes.  Frames with independent blocks and a content size within the
 * capacity take the fast route: every block but the last is taken to be full,
 * so block k decodes to min(block size, size - k * block size) bytes at
 * k * block size, all blocks of the batch side by side on the block decoder.
 * Linked blocks, frames without a content size, and every frame the fast route
 * does not accept (a short block in the middle, a block that fails) go to a
 * serial decoder, one lane per message, which alone decides their verdict:
 * correct and slow.  The lz4 command's default output is a frame without a
 * content size, and so is LZ4F_compressFrame's when contentSize is left 0.
 *
 * With option lz4f_nosize_fast (FSG_L4F_NOSIZE_FAST) = 1 (default 0) a frame
 * with independent blocks, no content size and at least one block takes a
 * second fast route.  Its block structure is checked from the size words (no
 * size 0, none above the block maximum, every block with its checksum inside
 * the input, end mark, content checksum when flagged, nothing after the
 * frame); a length pass finds every block's decoded length from its sequences
 * (a raw block's is its stored size), one lane per block, or one wave for a
 * block above option lz4f_length_wave_min (FSG_L4F_LENGTH_WAVE_MIN) bytes:
 * -1 automatic (2 KiB: the wave won at every measured block size and batch,
 * DESIGN.md section 5), 0 every compressed block by wave, >= 0xFFFFFFFF none; a prefix sum over the
 * lengths places the blocks in the slot, and the block decoder runs them side
 * by side.  Short blocks in the middle (LZ4F_compressUpdate with flushes) are
 * no obstacle on this route, and d_out_cap[i] may exceed the decoded length.
 * A frame that fails the structure check, does not fit the workspace, has a
 * block without a length, decodes to more than d_out_cap[i], or has a block or
 * a checksum that fails goes to the serial decoder, so the route never changes
 * a byte or a status.
 *
 * With option lz4f_linked_fast (FSG_L4F_LINKED_FAST) = 1 (default 0) a frame
 * with linked blocks takes a fast route too: one with a content size within
 * the capacity is listed as a sized frame with independent blocks is, one
 * without a content size as the paragraph above lists its frames, and that
 * only when lz4f_nosize_fast is 1 as well (otherwise it stays on the serial
 * decoder).  Each block also gets its prefix, the bytes the frame produced
 * before it, at most 65,535: the index passes of the block decoder, which run
 * on all blocks of the batch side by side, accept offsets that stay inside
 * it, and one wave per frame executes the frame's blocks in order, so every
 * history byte it reads is one it stored before or a raw block put in place
 * by an earlier launch.  The wave stops at the first block that failed or
 * whose bitmap did not fit the workspace; a frame whose wave did not finish
 * all its blocks, and every frame with a block or checksum that fails, goes
 * to the serial decoder (serial_rejected), as does a linked frame whose
 * content size is above the capacity, so this route never changes a byte or a
 * status either.  Frames it answers are counted in fast_linked_messages, not
 * in fast_messages, fast_nosize_messages or serial_linked.
 *
 * "What a *_batch call writes" holds for both calls, every status, route and
 * flag combination, and for fsg_lz4f_xxh32_batch (exactly n_msgs words).
 * Slots for compress: fsg_lz4f_max_frame_length(d_in_len[i], id) for
 * fsg_lz4f_compress_batch, and for fsg_lz4f_compress_batch_flags when flag
 * bit 1 (block checksums) is clear; fsg_lz4f_max_frame_length_flags(
 * d_in_len[i], id, flags) when it is set: a slot of the smaller size is too
 * small for such a call, and the call does not check it. */

/* fsg_lz4f_compress_batch_flags' flags; any other bit is FSG_ERR_INVALID_ARG */
#define FSG_LZ4F_FLAG_CONTENT_CHECKSUM 1u
#define FSG_LZ4F_FLAG_BLOCK_CHECKSUMS 2u
#define FSG_LZ4F_FLAG_NO_CONTENT_SIZE 4u

/* n + 4 * ceil(n / block size) + 23: descriptor (15), a size word per block,
 * the bytes (a block that does not shrink is stored raw), end mark (4),
 * content checksum (4).  LZ4F_compressFrameBound gives 4 more (it counts the
 * largest descriptor, 19 bytes with a DictID).  0 for an id outside 4..7. */
size_t fsg_lz4f_max_frame_length(size_t n, uint32_t block_size_id);

/* The same for a compress call with `flags`: 4 bytes per block more when
 * FSG_LZ4F_FLAG_BLOCK_CHECKSUMS is set, otherwise the value above (a frame
 * without a content size is 8 bytes shorter; the bound does not follow it);
 * 0 for an id outside 4..7 or a flags word with an undefined bit.
 * The slot size for calls with that bit; reached exactly by a message of
 * incompressible bytes with bits 0 and 1 and a content size. */
size_t fsg_lz4f_max_frame_length_flags(size_t n, uint32_t block_size_id, uint32_t flags);

/* Workspace of fsg_lz4f_compress_batch for a batch of n_msgs messages and
 * total_in_bytes input bytes in all: block columns and the block encoder's
 * workspace (16 KiB of position table) for n_msgs + total_in_bytes / block
 * size blocks, and staging for the encoded blocks.  The call takes no input
 * size: it reads from workspace_bytes what the workspace was sized for.
 * Messages whose blocks do not fit a workspace sized for fewer bytes get
 * FSG_CORRUPT with d_out_len 0 (nothing else changes). */
size_t fsg_lz4f_compress_workspace_bytes(uint32_t n_msgs, uint64_t total_in_bytes, uint32_t block_size_id);

/* Batched frame compress, columns as fsg_lz4_compress_batch.  flags:
 * FSG_LZ4F_FLAG_CONTENT_CHECKSUM or 0; every other bit is
 * FSG_ERR_INVALID_ARG (fsg_lz4f_compress_batch_flags below takes all three).
 * Slots of fsg_lz4f_max_frame_length.  No checksum kernel is launched when
 * flags is 0.  The blocks go through the block encoders of
 * fsg_lz4_compress_batch with that call's routing; option lz4f_block_wave_min
 * (FSG_L4F_BLOCK_WAVE_MIN) is their wave threshold, -1 (default) the
 * automatic rule applied to the workspace's block entries.  A NULL workspace
 * or one below fsg_lz4f_compress_workspace_bytes(n_msgs, 0, id) is
 * FSG_ERR_INVALID_ARG; n_msgs == 0 succeeds and launches nothing. */
int fsg_lz4f_compress_batch(const uint8_t *d_in, const uint64_t *d_in_off,
                            const uint32_t *d_in_len, uint32_t n_msgs,
                            uint8_t *d_out, const uint64_t *d_out_off,
                            uint32_t *d_out_len, int32_t *d_status,
                            uint32_t block_size_id, uint32_t flags,
                            void *d_workspace, size_t workspace_bytes,
                            void *stream);

/* The same call with the whole flags word: the FSG_LZ4F_FLAG_* bits above
 * ("The compressor writes ..."); slots as "Slots" there says.  The workspace
 * is that of fsg_lz4f_compress_batch and does not depend on the flags, and no
 * checksum kernel is launched when bits 0 and 1 are clear. */
int fsg_lz4f_compress_batch_flags(const uint8_t *d_in, const uint64_t *d_in_off,
                                  const uint32_t *d_in_len, uint32_t n_msgs,
                                  uint8_t *d_out, const uint64_t *d_out_off,
                                  uint32_t *d_out_len, int32_t *d_status,
                                  uint32_t block_size_id, uint32_t flags,
                                  void *d_workspace, size_t workspace_bytes,
                                  void *stream);

/* Workspace of fsg_lz4f_decompress_batch: block columns for n_msgs +
 * total_in_bytes / 256 blocks (a full 64 KiB block has at least 257 bytes),
 * staging for the blocks, and the block decoder's workspace.  A workspace
 * sized for fewer bytes never changes bytes or statuses: frames whose blocks
 * do not fit go to the serial decoder, blocks whose bitmap does not fit to the
 * block decoder's one-pass kernel. */
size_t fsg_lz4f_decompress_workspace_bytes(uint32_t n_msgs, uint64_t total_in_bytes);

/* Batched frame decompress, columns as fsg_lz4_decompress_batch_ws.  Option
 * lz4f_force_serial (FSG_L4F_FORCE_SERIAL) = 1 sends every frame to the serial
 * decoder; lz4f_nosize_fast, lz4f_length_wave_min and lz4f_linked_fast: "Routes" above.  A NULL workspace or one below
 * fsg_lz4f_decompress_workspace_bytes(n_msgs, 0) is FSG_ERR_INVALID_ARG;
 * n_msgs == 0 succeeds and launches nothing. */
int fsg_lz4f_decompress_batch(const uint8_t *d_in, const uint64_t *d_in_off,
                              const uint32_t *d_in_len, uint32_t n_msgs,
                              uint8_t *d_out, const uint64_t *d_out_off,
                              const uint32_t *d_out_cap, uint32_t *d_out_len,
                              int32_t *d_status, void *d_workspace,
                              size_t workspace_bytes, void *stream);

/* XXH32 (seed `seed`) of each body, d_xxh[i] for [d_in + d_in_off[i],
 * + d_in_len[i]), on the checksum kernel of the frame calls: a quad of lanes
 * per body, 16 bodies per wave.  Bodies may start at any byte address and may
 * be empty; no byte outside a body is read.  No workspace; exactly n_msgs
 * words are written.  For a caller who checksums frames it did not decode
 * here; n_msgs == 0 succeeds and launches nothing. */
int fsg_lz4f_xxh32_batch(const uint8_t *d_in, const uint64_t *d_in_off,
                         const uint32_t *d_in_len, uint32_t n_msgs,
                         uint32_t seed, uint32_t *d_xxh, void *stream);

/* The content size each body's descriptor states, for sizing slots
 * (fsg_uncompressed_lengths_batch's counterpart): d_content_size[i] = the
 * size, or FSG_LZ4F_NO_CONTENT_SIZE when the frame states none or the
 * descriptor is bad; d_status[i] = FSG_OK or FSG_BAD_HEADER. */
#define FSG_LZ4F_NO_CONTENT_SIZE 0xFFFFFFFFFFFFFFFFull
int fsg_lz4f_content_sizes_batch(const uint8_t *d_in, const uint64_t *d_in_off,
                                 const uint32_t *d_in_len, uint32_t n_msgs,
                                 uint64_t *d_content_size, int32_t *d_status,
                                 void *stream);

/* The decoded length of each body's frame, for sizing slots when a frame
 * states no content size: d_length[i] = the stated content size when there is
 * one; otherwise the sum of the blocks' decoded lengths (a raw block's stored
 * size, a compressed block's length from its sequences: the sequence whose
 * literals end at the block's last byte ends it), whether the blocks are
 * linked or not; 0 for a frame without blocks.  d_status[i]: FSG_OK;
 * FSG_BAD_HEADER by the rule of the decompress call; FSG_CORRUPT (d_length[i]
 * = 0) for a frame without a content size whose block structure is broken (a
 * size word above the block maximum, input that ends early, no end mark,
 * bytes after the frame) or that has a block whose sequences give no length
 * or more than the block maximum.  Block and content checksums are not looked
 * at, no block is decoded, and a stated content size is not checked against
 * anything: FSG_OK does NOT promise that the frame decodes, only that a slot
 * of d_length[i] bytes is large enough if it does.  The call takes a
 * decompress workspace (fsg_lz4f_decompress_workspace_bytes; NULL or below
 * that function's value for (n_msgs, 0) is FSG_ERR_INVALID_ARG) and runs the
 * index and length kernels of the decompress call on it; a frame whose blocks
 * do not fit the workspace is walked by one lane, with the same answer. */
int fsg_lz4f_decoded_lengths_batch(const uint8_t *d_in, const uint64_t *d_in_off,
                                   const uint32_t *d_in_len, uint32_t n_msgs,
                                   uint64_t *d_length, int32_t *d_status,
                                   void *d_workspace, size_t workspace_bytes,
                                   void *stream);

/* Path reports ("Path reports" in flare_snappy_gpu.h: host code, from a host
 * copy of the workspace's first 256 bytes taken after the call completed,
 * asked with the call's n_msgs, workspace_bytes and block size id). */
struct fsg_lz4f_encode_report {
  uint64_t blocks;             /* blocks encoded */
  uint64_t raw_blocks;         /* of them stored raw */
  uint64_t overflow_messages;  /* messages that did not fit the workspace (FSG_CORRUPT) */
  uint64_t block_entries;      /* blocks the workspace holds */
  uint64_t block_wave_min;     /* wave threshold of the block encode (0xFFFFFFFF: none) */
};
int fsg_lz4f_compress_report(const void *header_host_copy, uint32_t n_msgs,
                             size_t workspace_bytes, uint32_t block_size_id,
                             struct fsg_lz4f_encode_report *out);

struct fsg_lz4f_decode_report {
  uint64_t fast_messages;      /* answered by the fast route (FSG_OK) */
  uint64_t fast_blocks;        /* their blocks */
  uint64_t empty_messages;     /* frames without blocks, finished by the index pass */
  uint64_t serial_linked;      /* serial route: linked blocks (option lz4f_linked_fast 0, or no content size and lz4f_nosize_fast 0) */
  uint64_t serial_no_size;     /* serial route: no content size (option lz4f_nosize_fast 0) */
  uint64_t serial_rejected;    /* serial route: a fast route, with or without a content size, did not accept the frame */
  uint64_t serial_forced;      /* serial route: option lz4f_force_serial */
  uint64_t checksummed_units;  /* block and content checksums computed */
  uint64_t inner_fallback_blocks; /* blocks the block decoder's one-pass kernel finished */
  uint64_t block_entries;      /* blocks the workspace holds */
  uint64_t fast_nosize_messages; /* answered by the fast route for frames without a content size (FSG_OK) */
  uint64_t fast_nosize_blocks;   /* their blocks */
  uint64_t fast_linked_messages; /* answered by the fast route for linked blocks (FSG_OK) */
  uint64_t fast_linked_blocks;   /* their blocks */
};
int fsg_lz4f_decompress_report(const void *header_host_copy, uint32_t n_msgs,
                               size_t workspace_bytes,
                               struct fsg_lz4f_decode_report *out);

#ifdef __cplusplus
}
#endif
#endif /* FLARE_LZ4_GPU_H_ */
