/*
 * flare_deflate_index_gpu.h -- gzip bodies with a UNIT INDEX on MI355X
 * (gfx950): a compress call that writes the index, and inflate calls that use
 * it to give every unit of a body its own wave.  An addition to
 * include/flare_deflate_gpu.h and flare_deflate_compress_gpu.h, whose calls
 * keep their behaviour.
 *
 * Why.  fsg_inflate_batch walks a body with one wave, because deflate says
 * nowhere where a block starts.  The bodies fsg_deflate_batch writes are cut
 * into units of 65,472 input bytes: every unit is a byte string, no match
 * reaches below its unit's first byte, and every unit but the last decodes to
 * exactly 65,472 bytes.  All a parallel reader lacks is where each unit starts
 * in the compressed bytes, and the index says that.
 *
 * The index (csrc/gzip_index.h has all of it) is dictzip's `RA` random-access
 * subfield of the gzip header's extra field: FLG.FEXTRA, and among the XLEN
 * bytes the first subfield with SI1 = 'R', SI2 = 'A':
 *     'R' 'A' LEN(2)   VER(2) = 1   CHLEN(2)   CHCNT(2)   CHCNT x size(2)
 * little endian.  CHLEN is the decoded length of every unit but the last,
 * size k the compressed length of unit k.  Unit k starts at
 * begin + sum(size[< k]), begin being the first byte of the deflate stream,
 * and its output at k * CHLEN.  The last size entry places nothing.  USABLE:
 * the chain up to the subfield is well-formed inside XLEN, VER = 1,
 * CHLEN >= 1, CHCNT >= 1, LEN = 6 + 2 * CHCNT, and
 * begin + sum(size[0 .. CHCNT-2]) <= n - 8.  zlib and every other inflate skip
 * the extra field, fsg_inflate_batch included: these bodies are plain gzip.
 * Any writer may produce them (dictzip does; so does zlib with a
 * Z_FULL_FLUSH per chunk and a hand-written head).
 *
 * ---- Writing: fsg_deflate_batch_flags
 * flare_deflate_level_gpu.h's fsg_deflate_batch_level with a flags word; with
 * flags = 0 it is that call.  FSG_DEFLATE_FLAG_UNIT_INDEX, gzip only: the body
 * starts with 22 + 2 * units bytes,
 *     1f 8b 08 04  00 00 00 00  00 03   XLEN = 10 + 2 * units
 *     'R' 'A'  LEN = 6 + 2 * units   01 00   CHLEN = 65,472   CHCNT = units
 *     the units' compressed lengths, 16 bits each (at most 65,477)
 * followed by the SAME deflate stream and trailer the unflagged call writes,
 * at every level.  A body of more than 32,762 units (XLEN is 16 bits wide) is
 * written without the index.  Slots are fsg_deflate_max_length_flags(len,
 * format, flags) bytes.  host/deflate_cpu.cc (fsh_cpu_deflate_flags) defines
 * the bytes; the device gives them exactly.  Workspace, statuses, what the
 * call writes and fsg_deflate_report are those of fsg_deflate_batch.
 * FSG_ERR_INVALID_ARG before any HIP call, besides what
 * fsg_deflate_batch_level refuses: an unknown flag bit, and
 * FSG_DEFLATE_FLAG_UNIT_INDEX with a format other than FSG_DEFLATE_GZIP.
 *
 * ---- Reading: fsg_inflate_units_batch, fsg_inflate_units_lengths_batch
 * The columns, formats, statuses and write-containment contract of
 * fsg_inflate_batch and fsg_inflate_lengths_batch, plus a workspace.
 *
 * The rule.  For every body, format and capacity, status, length and bytes
 * are what fsg_inflate_batch, or fsg_inflate_lengths_batch, gives.  The index
 * changes the time a body takes, nothing else.  So a body is decoded by units
 * only where that provably coincides with the serial walk: unit 0 starts at
 * `begin`; every unit in front of the last ends on a block boundary exactly
 * at the next unit's start, with no BFINAL met, exactly CHLEN bytes decoded,
 * no distance below the unit's own first byte and nothing corrupt; the last
 * unit runs to BFINAL under the serial walk's end-of-stream rule; and the
 * total fits the slot.  A body that misses any of it -- and so every
 * corrupt, truncated or too-large one -- is walked again as one stream by one
 * wave, and that walk gives its verdict.  Raw and zlib bodies, gzip bodies
 * without a usable index and bodies whose units the workspace does not hold
 * are walked that way from the start.  The gzip trailer is judged by
 * fsg_inflate_batch's checksum kernel.
 *
 * Slots.  Unit k writes only d_out[d_out_off[i] + k * CHLEN ..) up to
 * min(CHLEN, cap - k * CHLEN) bytes (the last unit up to the slot's end), so
 * no byte outside a slot is written whatever the index claims.
 *
 * Workspace.  A 256-byte header, 32 bytes and one redo entry per body, and 32
 * bytes per unit entry.  fsg_inflate_units_workspace_bytes(n_msgs,
 * extra_units) holds n_msgs bodies and extra_units units beyond one per body
 * (for bodies of this project's writer: sum over the bodies of
 * ceil(decoded length / 65,472) - 1; total decoded bytes / 65,472 is enough).
 * The call reads the entries it holds from workspace_bytes.  Indexed bodies
 * keep their units in batch order while the units beyond one per body of all
 * indexed bodies so far fit; the others are decoded serially -- slower, never
 * wrong.  Any bytes on entry, 16-byte aligned, not shared by two calls in
 * flight.
 *
 * FSG_ERR_INVALID_ARG, before any HIP call: what the workspace-less calls
 * refuse; a workspace that is NULL, misaligned or below
 * fsg_inflate_units_workspace_bytes(n_msgs, 0).  n_msgs == 0 with a known
 * format succeeds and launches nothing.
 */
#ifndef FLARE_DEFLATE_INDEX_GPU_H_
#define FLARE_DEFLATE_INDEX_GPU_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FSG_DEFLATE_FLAG_UNIT_INDEX 1u

/* fsg_deflate_max_length plus, where the flagged call writes the index,
 * 12 + 2 * units; 0 for what the call refuses (unknown format or flag, the
 * flag with a format other than gzip). */
size_t fsg_deflate_max_length_flags(size_t n, uint32_t format, uint32_t flags);

int fsg_deflate_batch_flags(const uint8_t *d_in, const uint64_t *d_in_off,
                            const uint32_t *d_in_len, uint32_t n_msgs,
                            uint8_t *d_out, const uint64_t *d_out_off,
                            uint32_t *d_out_len, int32_t *d_status,
                            uint32_t format, uint32_t level, uint32_t flags,
                            void *d_workspace, size_t workspace_bytes,
                            void *stream);

size_t fsg_inflate_units_workspace_bytes(uint32_t n_msgs, uint64_t extra_units);

int fsg_inflate_units_batch(const uint8_t *d_in, const uint64_t *d_in_off,
                            const uint32_t *d_in_len, uint32_t n_msgs,
                            uint8_t *d_out, const uint64_t *d_out_off,
                            const uint32_t *d_out_cap, uint32_t *d_out_len,
                            int32_t *d_status, uint32_t format,
                            void *d_workspace, size_t workspace_bytes,
                            void *stream);

int fsg_inflate_units_lengths_batch(const uint8_t *d_in,
                                    const uint64_t *d_in_off,
                                    const uint32_t *d_in_len, uint32_t n_msgs,
                                    uint64_t *d_length, int32_t *d_status,
                                    uint32_t format, void *d_workspace,
                                    size_t workspace_bytes, void *stream);

/* The routes the bodies of a call took, from a host copy of the workspace's
 * first 256 bytes taken after it completed (host code, no HIP call; asked
 * with the call's n_msgs and workspace_bytes).  The message counts (every
 * field but parallel_units and unit_entries) add up to n_msgs.
 * FSG_ERR_INVALID_ARG: a NULL pointer or a workspace size the call
 * would have refused. */
struct fsg_inflate_units_report {
  uint64_t parallel_messages;     /* decoded unit-parallel */
  uint64_t parallel_units;        /* their units */
  uint64_t serial_no_index;       /* no index: raw and zlib bodies, gzip bodies without one, bodies the wrapper decides */
  uint64_t serial_unusable_index; /* an index that misses a rule */
  uint64_t serial_unit_mismatch;  /* a unit that was not clean, or a total above the capacity */
  uint64_t serial_workspace;      /* the workspace did not hold their units */
  uint64_t unit_entries;          /* unit entries the workspace holds */
};
int fsg_inflate_units_report(const void *header_host_copy, uint32_t n_msgs,
                             size_t workspace_bytes,
                             struct fsg_inflate_units_report *out);

#ifdef __cplusplus
}
#endif
#endif /* FLARE_DEFLATE_INDEX_GPU_H_ */
