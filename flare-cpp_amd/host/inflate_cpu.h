// inflate_cpu.h -- serial inflate over csrc/inflate_format.h: the model the
// device decoder (csrc/inflate.hip) is written from, and the host codec for
// bodies too small to send to the device.  No libz: the product library gains
// no dependency.  include/flare_deflate_gpu.h states the acceptance rule and
// the statuses; these calls give the same verdicts, lengths and bytes as
// fsg_inflate_batch / fsg_inflate_lengths_batch give for one body.
#pragma once

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* format: FSG_INFLATE_RAW / _ZLIB / _GZIP (0, 1, 2).  Returns the body's
 * status word (FSG_OK, FSG_CORRUPT, FSG_BAD_HEADER, FSG_SLOT_TOO_SMALL;
 * FSG_CORRUPT for an unknown format).  *len: the decoded length on FSG_OK,
 * min(true length, 2^32 - 1) on FSG_SLOT_TOO_SMALL, otherwise 0.  Writes
 * out[0 .. min(length, cap)) at most; out may be NULL when cap is 0. */
int fsh_cpu_inflate(uint32_t format, const void *in, size_t n, void *out, size_t cap, uint64_t *len);

/* The same walk with nothing written and the trailing checksum not looked at:
 * *len = the exact decoded length on FSG_OK, otherwise 0. */
int fsh_cpu_inflate_length(uint32_t format, const void *in, size_t n, uint64_t *len);

/* One unit of an indexed gzip body (csrc/gzip_index.h), or a whole deflate
 * stream: the block loop from byte `start` of in[0 .. n).  nonlast = 0: blocks
 * until BFINAL, which must end in byte stop - 1.  nonlast = 1: the unit ends
 * clean after the block that ends exactly at byte `stop`, with exactly chlen
 * bytes decoded and no BFINAL met.  Distances count from out[0].  Returns
 * FSG_OK for a clean unit, FSG_CORRUPT for everything else; *len = the bytes
 * the walk declared so far.  Writes out[0 .. min(*len, cap)) when store. */
int fsh_cpu_inflate_unit(const void *in, size_t n, size_t start, size_t stop, int nonlast, uint32_t chlen, void *out,
                         size_t cap, int store, uint64_t *len);

/* zlib's crc32(0, p, n) and adler32(1, p, n), serial. */
uint32_t fsh_cpu_crc32(const void *p, size_t n);
uint32_t fsh_cpu_adler32(const void *p, size_t n);

#ifdef __cplusplus
}
#endif
