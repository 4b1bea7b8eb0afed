/*
 * flare_deflate_compress_gpu.h -- batched deflate COMPRESS on MI355X (gfx950):
 * the writing side of include/flare_deflate_gpu.h, which includes this file
 * (the reading side's header keeps its own declarations only).  Raw deflate,
 * zlib and gzip bodies, the formats FSG_INFLATE_RAW / _ZLIB / _GZIP.
 *
 * Reference interface: flare's GzipCompress and ZlibCompress
 * (COMPRESS_TYPE_GZIP = 2 and COMPRESS_TYPE_ZLIB = 3), which write a body
 * through protobuf's GzipOutputStream, that is zlib's deflate.
 *
 * The contract.  The bytes zlib's deflate writes depend on its version and
 * level; no receiver compares them, every receiver inflates.  So the bytes of
 * these bodies are defined by this project: csrc/deflate_format.h states the
 * stream, host/deflate_cpu.cc (fsh_cpu_deflate) is its serial model, and
 * fsg_deflate_batch gives the model's bytes exactly.  What holds for every
 * body, and what the tests ask of zlib: inflate with the format's windowBits
 * returns the input, reaches the stream's end and leaves no byte over.  In
 * Python terms:
 *     d = zlib.decompressobj(wbits); o = d.decompress(body)
 *     o == data and d.eof and not d.unused_data
 * Byte equality with zlib's deflate is not offered at any level.  This call
 * writes one level; flare_deflate_level_gpu.h has the call that takes one.
 *
 * The stream in short (deflate_format.h has all of it): the input is cut into
 * units of 65,472 bytes, compressed independently, one deflate block each --
 * stored, fixed or dynamic, the shortest -- and a coded block that is not the
 * last is followed by an empty stored block (00 00 FF FF behind the padding),
 * as a Z_SYNC_FLUSH writes, so that every unit is a byte string.  zlib
 * wrapper: 78 01, the big-endian Adler-32 behind.  gzip wrapper: 1f 8b 08 00
 * 00 00 00 00 00 03, the CRC-32 and ISIZE behind, little endian.
 *
 * Slots.  Body i is d_in[d_in_off[i] .. + d_in_len[i]); its output goes to
 * d_out[d_out_off[i] ..] in a slot of fsg_deflate_max_length(d_in_len[i],
 * format) bytes.  There is no capacity column, slots need no alignment and may
 * touch, as for fsg_lz4_compress_batch.
 *
 * What the call writes: the contract of flare_snappy_gpu.h ("What a *_batch
 * call writes").  No byte of d_out outside the slots is written; inside a
 * slot only the bytes below d_out_len[i] are written.  d_out_len and d_status
 * get exactly n_msgs entries, the input arrays are not written, nothing is
 * written past workspace_bytes.  No byte outside a body is read, except that
 * the parse reads whole aligned 4-byte words, so up to 3 bytes on either side
 * of a body inside the aligned words that hold its first and last byte (never
 * used).
 *
 * Statuses.  FSG_OK with d_out_len[i] the body's length.  FSG_CORRUPT with
 * d_out_len[i] = 0 and the slot untouched for (1) a body whose slot length
 * does not fit 32 bits (above 4 GiB - 400 KiB: d_out_len is a 32-bit column)
 * and (2) a body whose units the workspace does not hold.  There is no slow
 * fallback route behind this call: a workspace sized by
 * fsg_deflate_workspace_bytes for the batch's total holds every body.
 *
 * Workspace.  A 256-byte header, 24 bytes per body, 40 per unit, a token
 * region of 256 KiB for each of up to 1,024 resident waves, and the units'
 * staging slots.  fsg_deflate_workspace_bytes(n_msgs, total_in_bytes) is
 * enough for any n_msgs bodies of total_in_bytes in all.  The call has the
 * lengths on the device only, so it reads from workspace_bytes how many units
 * the workspace holds; bodies it does not hold get status (2).  The workspace
 * may hold any bytes on entry, must be 16-byte aligned, and must not be
 * shared by two calls in flight.
 *
 * FSG_ERR_INVALID_ARG, decided before any HIP call: a NULL pointer with
 * n_msgs > 0, an unknown format, a workspace that is NULL, misaligned or
 * below fsg_deflate_workspace_bytes(n_msgs, 0).  n_msgs == 0 succeeds and
 * launches nothing.
 */
#ifndef FLARE_DEFLATE_COMPRESS_GPU_H_
#define FLARE_DEFLATE_COMPRESS_GPU_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FSG_DEFLATE_RAW 0u  /* = FSG_INFLATE_RAW */
#define FSG_DEFLATE_ZLIB 1u /* = FSG_INFLATE_ZLIB: what ZlibCompress writes */
#define FSG_DEFLATE_GZIP 2u /* = FSG_INFLATE_GZIP: what GzipCompress writes */

/* n + 5 * max(1, ceil(n / 65472)) + the wrapper's 0, 6 or 18 bytes; 0 for an
 * unknown format.  Exact: a body of stored units has this length. */
size_t fsg_deflate_max_length(size_t n, uint32_t format);

size_t fsg_deflate_workspace_bytes(uint32_t n_msgs, uint64_t total_in_bytes);

int fsg_deflate_batch(const uint8_t *d_in, const uint64_t *d_in_off,
                      const uint32_t *d_in_len, uint32_t n_msgs,
                      uint8_t *d_out, const uint64_t *d_out_off,
                      uint32_t *d_out_len, int32_t *d_status, uint32_t format,
                      void *d_workspace, size_t workspace_bytes, void *stream);

/* What the call did, from a host copy of the workspace's first 256 bytes
 * taken after it completed (host code, no HIP call; asked with the call's
 * n_msgs and workspace_bytes).  FSG_ERR_INVALID_ARG: a NULL pointer or a
 * workspace size the call would have refused. */
struct fsg_deflate_report {
  uint64_t units;          /* units compressed */
  uint64_t stored_units;   /* by the block type chosen */
  uint64_t fixed_units;
  uint64_t dynamic_units;
  uint64_t overflow_messages; /* bodies answered FSG_CORRUPT: not held, or too long */
  uint64_t unit_entries;      /* units the workspace holds */
};
int fsg_deflate_report(const void *header_host_copy, uint32_t n_msgs,
                       size_t workspace_bytes, struct fsg_deflate_report *out);

#ifdef __cplusplus
}
#endif
#endif /* FLARE_DEFLATE_COMPRESS_GPU_H_ */
