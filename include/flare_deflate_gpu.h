/*
 * flare_deflate_gpu.h -- batched inflate and deflate on MI355X (gfx950), in
 * libflare_snappy_gpu.so next to the Snappy and LZ4 calls
 * (include/flare_snappy_gpu.h: same batch layout, same status words, same
 * fsg_init / fsg_last_error).  This file declares and specifies the reading
 * side.  The writing side -- fsg_deflate_batch and its sizing and report
 * calls, whose bodies every inflate reads and whose bytes are this project's
 * own, not zlib's -- is declared and specified in
 * flare_deflate_compress_gpu.h, which this header includes at its end.
 *
 * Reference interface: flare's GzipDecompress and ZlibDecompress
 * (COMPRESS_TYPE_GZIP = 2 and COMPRESS_TYPE_ZLIB = 3, flare/rpc/options.proto,
 * registered in flare/rpc/global.cc), which read a body through protobuf's
 * GzipInputStream, that is zlib's inflate with windowBits 15 | 16 and 15.
 *
 * Acceptance rule.  A body is FSG_OK exactly when zlib 1.2.11's inflate, with
 * the windowBits of the call's format, (1) reaches Z_STREAM_END, (2) has then
 * consumed every input byte and (3) has produced at most d_out_cap[i] bytes;
 * the output bytes are zlib's.  In Python terms:
 *     d = zlib.decompressobj(wbits); o = d.decompress(body)
 *     d.eof and not d.unused_data and len(o) <= cap
 * with wbits -15, 15 and 31 for FSG_INFLATE_RAW, _ZLIB and _GZIP.  One gzip
 * member per body is accepted; bytes after it are FSG_CORRUPT, as bytes after
 * an LZ4 frame are.  There are no preset dictionaries.
 *
 * Statuses.
 *   FSG_BAD_HEADER: a wrapper header that zlib rejects, or one cut short by
 *     the input's end.  zlib format: the mod-31 header check, CM != 8,
 *     CINFO > 7, FDICT set; a header that declares a window below 32 KiB is
 *     accepted, as zlib accepts it.  gzip format: the magic, CM != 8, a
 *     reserved FLG bit, FEXTRA, FNAME or FCOMMENT running past the input, an
 *     FHCRC mismatch.  An empty body in either format.
 *   FSG_SLOT_TOO_SMALL: a stream valid in everything the decoder can judge
 *     that decodes to more than d_out_cap[i] bytes; d_out_len[i] =
 *     min(true length, 2^32 - 1).  Nothing is written past the slot: from the
 *     capacity on the decoder only counts.  The trailing checksum of such a
 *     body is not judged (the bytes past the capacity are not kept).
 *   FSG_CORRUPT, with d_out_len[i] = 0, everything else: BTYPE 3; a stored
 *     block with LEN != ~NLEN; more than 286 literal/length or more than 30
 *     distance symbols; a repeat code with nothing to repeat or one that runs
 *     past the length list; no end-of-block code; an over-subscribed code set;
 *     an incomplete one, except the one zlib's inflate_table allows (a single
 *     code of length 1 in a literal/length or distance set); a symbol with no
 *     code (286, 287, distance 30 or 31, the unused half of a single-code
 *     set); a distance beyond the bytes produced so far (the code itself
 *     reaches 32,768 at most); input that ends before the final block's end,
 *     a wrapper's trailer included; bytes after the stream; an Adler-32,
 *     CRC-32 or ISIZE mismatch.  Also a body above 4 GiB - 64 KiB.
 *
 * What the calls write: the contract of flare_snappy_gpu.h ("What a *_batch
 * call writes") holds for all four calls.  No byte of d_out outside the slots
 * [d_out_off[i], d_out_off[i] + d_out_cap[i]) is written (a capacity of 0 is
 * allowed); slots need no alignment and may touch; inside a slot the bytes at
 * and past d_out_len[i] are unspecified, as is the whole slot for any status
 * other than FSG_OK.  The result columns get exactly n_msgs entries and the
 * input arrays are not written.  Bodies may start at any byte address and no
 * byte outside a body is read, except that the decoder reads whole aligned
 * 4-byte words, so up to 3 bytes on either side of a body inside the aligned
 * words that hold its first and last byte (never used: they are masked off).
 *
 * No workspace: the decode tables live in LDS.  One wave decodes one body, so
 * a batch is as fast as it has bodies ("Deflate").
 * n_msgs == 0 succeeds and launches nothing.  FSG_ERR_INVALID_ARG: a NULL
 * pointer with n_msgs > 0, or an unknown format; both are decided before any
 * HIP call.
 */
#ifndef FLARE_DEFLATE_GPU_H_
#define FLARE_DEFLATE_GPU_H_

#include <stddef.h>
#include <stdint.h>

#include "flare_snappy_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FSG_INFLATE_RAW 0u  /* RFC 1951 alone */
#define FSG_INFLATE_ZLIB 1u /* RFC 1950: what ZlibDecompress reads (windowBits 15) */
#define FSG_INFLATE_GZIP 2u /* RFC 1952: what GzipDecompress reads (windowBits 15 | 16) */

/* Batched inflate, the columns of fsg_lz4_decompress_batch: body i is
 * d_in[d_in_off[i] .. + d_in_len[i]); it decodes into d_out[d_out_off[i] ..]
 * with capacity d_out_cap[i]; d_out_len[i] and d_status[i] as "Statuses"
 * says.  For the zlib and gzip formats a checksum kernel runs behind the
 * decode kernel on `stream` and judges the trailers. */
int fsg_inflate_batch(const uint8_t *d_in, const uint64_t *d_in_off,
                      const uint32_t *d_in_len, uint32_t n_msgs,
                      uint8_t *d_out, const uint64_t *d_out_off,
                      const uint32_t *d_out_cap, uint32_t *d_out_len,
                      int32_t *d_status, uint32_t format, void *stream);

/* The slot-sizing call, for the zlib and raw formats state no length and
 * gzip's ISIZE is one only mod 2^32: the same walk with no output written.
 * d_length[i] = the exact decoded length with d_status[i] FSG_OK; FSG_CORRUPT
 * or FSG_BAD_HEADER (d_length[i] = 0) by the rules above.  The trailing
 * checksum and ISIZE are NOT checked: a decode of a body this call answered
 * FSG_OK can still fail on them (FSG_CORRUPT there).  The trailer's presence
 * is checked: the stream must end exactly 0, 4 or 8 bytes before the body
 * does. */
int fsg_inflate_lengths_batch(const uint8_t *d_in, const uint64_t *d_in_off,
                              const uint32_t *d_in_len, uint32_t n_msgs,
                              uint64_t *d_length, int32_t *d_status,
                              uint32_t format, void *stream);

/* zlib's crc32(0, body, len) / adler32(1, body, len) of each body into
 * d_crc[i] / d_adler[i], on the checksum kernel of the inflate call: a wave
 * per body, coalesced 16-byte loads of whole 16-byte pieces, the tail byte by
 * byte.  Bodies may start at any byte address and may be empty; no byte
 * outside a body is read.  Exactly n_msgs words are written. */
int fsg_crc32_batch(const uint8_t *d_in, const uint64_t *d_in_off,
                    const uint32_t *d_in_len, uint32_t n_msgs,
                    uint32_t *d_crc, void *stream);
int fsg_adler32_batch(const uint8_t *d_in, const uint64_t *d_in_off,
                      const uint32_t *d_in_len, uint32_t n_msgs,
                      uint32_t *d_adler, void *stream);

#ifdef __cplusplus
}
#endif

#include "flare_deflate_compress_gpu.h"

#endif /* FLARE_DEFLATE_GPU_H_ */
