// deflate_cpu.h -- the serial deflate writer over csrc/deflate_format.h: the
// DEFINITION of the bytes fsg_deflate_batch and fsg_deflate_batch_level produce
// (include/flare_deflate_compress_gpu.h, flare_deflate_level_gpu.h), and the host codec behind the gzip
// and zlib compress handlers (gzip_compress.h).  No libz.  The streams are
// legal raw deflate / zlib / gzip bodies that any inflate reads; they are not
// the bytes zlib's deflate would write for the same input.
#pragma once

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* n + 5 * max(1, ceil(n / 65472)) + 0, 6 or 18 wrapper bytes; 0 for an
 * unknown format.  format: FSG_INFLATE_RAW / _ZLIB / _GZIP (0, 1, 2). */
size_t fsh_cpu_deflate_bound(size_t n, uint32_t format);

/* Compresses in[0 .. n) into out[0 .. cap).  Returns 0 (FSG_OK) with *len =
 * the body's length, which never exceeds the bound.  Returns 3
 * (FSG_SLOT_TOO_SMALL) when the body is longer than cap, and 1 (FSG_CORRUPT)
 * for an unknown format; *len is 0 then and out is not written.  Bytes of out
 * at and past *len are never written.  gzip's ISIZE is n mod 2^32. */
int fsh_cpu_deflate(uint32_t format, const void *in, size_t n, void *out, size_t cap, uint64_t *len);

/* The same at a level (csrc/deflate_format.h, "levels"): 0 writes stored
 * units only and the body's length is exactly the bound; 1 is fsh_cpu_deflate,
 * bit for bit; 2 parses with two candidates per hash slot and one lazy step.
 * A level above 2 is 1 (FSG_CORRUPT) with *len = 0, like an unknown format.
 * The bound holds at every level. */
int fsh_cpu_deflate_level(uint32_t format, uint32_t level, const void *in, size_t n, void *out, size_t cap,
                          uint64_t *len);

/* With flags (include/flare_deflate_index_gpu.h): the DEFINITION of the bytes
 * fsg_deflate_batch_flags produces.  flags = 1 (FSG_DEFLATE_FLAG_UNIT_INDEX),
 * gzip only: the 10-byte head is replaced by the 22 + 2 * units bytes of
 * csrc/gzip_index.h (the units' compressed lengths in an `RA` extra
 * subfield); the deflate stream and the trailer are those of flags = 0.  A
 * body of more than 32,762 units is written without the index.  An unknown
 * flag, or the flag with another format, is 1 (FSG_CORRUPT) with *len = 0.
 * fsh_cpu_deflate_bound_flags: the slot bound (0 for what the call refuses). */
size_t fsh_cpu_deflate_bound_flags(size_t n, uint32_t format, uint32_t flags);
int fsh_cpu_deflate_flags(uint32_t format, uint32_t level, uint32_t flags, const void *in, size_t n, void *out,
                          size_t cap, uint64_t *len);

/* The block types of the units the last-named call would choose, for tests
 * and reports: counts[0..3) += stored, fixed, dynamic units of in[0 .. n). */
void fsh_cpu_deflate_unit_types(const void *in, size_t n, uint64_t counts[3]);
/* At a level (level 0: every unit stored); nothing is counted for a level above 2. */
void fsh_cpu_deflate_unit_types_level(uint32_t level, const void *in, size_t n, uint64_t counts[3]);

/* The parse of ONE unit (n <= 65472), for tests: its tokens without the end
 * token into tokens[0 .. cap), the count returned (0 when n is too large or
 * cap too small).  A literal is 0x80000000 | byte, a match length |
 * distance << 9. */
size_t fsh_cpu_deflate_tokens(const void *in, size_t n, uint32_t *tokens, size_t cap);
/* At level 1 or 2; level 0 has no parse and gives 0, as does a level above 2. */
size_t fsh_cpu_deflate_tokens_level(uint32_t level, const void *in, size_t n, uint32_t *tokens, size_t cap);

/* How many of the literal/length and distance code sets built for
 * in[0 .. n) (two per unit) were deeper than 15 bits and went through the
 * length limiter. */
uint64_t fsh_cpu_deflate_limited(const void *in, size_t n);

#ifdef __cplusplus
}
#endif
