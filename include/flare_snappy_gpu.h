/*
 * flare_snappy_gpu.h -- C ABI of the MI355X (gfx950) batched Snappy codec.
 *
 * This is the drop-in boundary underneath flare's CompressType plugin
 * surface.  Each entry point replaces one piece of the reference's CPU path
 * (paths relative to /root/reference):
 *
 *   fsg_max_compressed_length      flare/io/snappy/snappy.cc:55-77
 *                                  (snappy::MaxCompressedLength)
 *   fsg_get_uncompressed_length    snappy.cc:235-244 (strict,
 *                                  GetUncompressedLength(const char*,...))
 *                                  and snappy.cc:692-711 / 870-873 (lenient,
 *                                  GetUncompressedLength(Source*,...))
 *   fsg_compress_batch             snappy.cc:875-954 (snappy::Compress(Source*,
 *                                  Sink*)) as called per message by
 *                                  flare/rpc/policy/snappy_compress.cc:28-38,51-55
 *   fsg_decompress_batch           snappy.cc:1537-1563 (snappy::Uncompress(
 *                                  Source*, Sink*)) as called by
 *                                  snappy_compress.cc:40-49,57-61; with
 *                                  FSG_FLAG_VALIDATE_ONLY it is
 *                                  IsValidCompressed (snappy.cc:1290-1299);
 *                                  with FSG_FLAG_STRICT_HEADER it is the flat
 *                                  Uncompress(const char*, size_t, string*)
 *                                  (snappy.cc:1239-1251).
 *   fsg_decompress_batch_partial   snappy.cc:1530-1535
 *                                  (snappy::UncompressAsMuchAsPossible(
 *                                  Source*, Sink*), SnappyScatteredWriter
 *                                  :1331-1481)
 *   fsg_decompress_batch_iovec     snappy.cc:1122-1132
 *                                  (snappy::RawUncompressToIOVec(const char*,
 *                                  size_t, const iovec*, size_t),
 *                                  SnappyIOVecWriter :963-1120)
 *
 * Conventions: plain C, no exceptions, no torch types.  All buffers passed
 * to *_batch functions are DEVICE pointers (hipMalloc'd or device-mapped
 * pinned host memory); `stream` is a hipStream_t (NULL = default stream).
 * The calls are asynchronous on `stream`: results are valid after the
 * stream is synchronised.  Every function is thread-safe; no global state
 * is mutated after fsg_init.
 *
 * Per-message status words (int32):
 *   FSG_OK              the reference returns true and the output bytes are
 *                       byte-identical to the reference's.
 *   FSG_CORRUPT         the reference returns false (bad offset, overrun,
 *                       premature end, trailing tags, truncated tag).
 *   FSG_BAD_HEADER      the reference returns false while reading the
 *                       varint uncompressed-length header.
 *   FSG_SLOT_TOO_SMALL  caller sizing error: the header's uncompressed length
 *                       exceeds the output slot (not a reference verdict;
 *                       size slots with fsg_get_uncompressed_length).
 *   FSG_IOV_TOO_SMALL   (fsg_decompress_batch_iovec) the stream is valid but
 *                       its iovecs hold fewer bytes than the header's length:
 *                       the reference returns false.
 * On any status other than FSG_OK the content of the output slot is
 * unspecified (the reference's partial output on failure depends on the
 * source fragmentation, snappy.cc:866, and every caller discards it).
 *
 * What a *_batch call writes (tests/test_gpu_containment.py holds every
 * routing to it, byte for byte):
 *   1. Output slots.  No byte of d_out / d_stage outside the union of the
 *      slots [off_i, off_i + cap_i) is written, for every message status and
 *      every routing (kernel variant, option, workspace size, stream form).
 *      cap_i is d_out_cap[i] / d_stage_cap[i] for the decode calls, and
 *      fsg_max_compressed_length(d_in_len[i]) (fsg_lz4_max_compressed_length
 *      for LZ4) for the compress calls.  Slots need no alignment and may
 *      touch: a neighbour's bytes are never clobbered.  A decode slot may have
 *      capacity 0.
 *   2. Slot tails.  Inside a slot, the bytes at and past the reported length
 *      (d_out_len[i]; d_got[i] for the partial call) are unspecified: the
 *      encoders use the slot's headroom as spill room for their wide stores,
 *      a decode slot larger than the body may be written past the body, and
 *      for any status other than FSG_OK the whole slot is unspecified.
 *      Callers must not keep data of their own inside a slot.
 *   3. Validate-only.  With FSG_FLAG_VALIDATE_ONLY nothing in d_out is
 *      written.
 *   4. Result columns.  d_out_len, d_status, d_got, d_produced and d_ulen get
 *      exactly n_msgs entries.
 *   5. Workspace and input.  Nothing is written past workspace_bytes, and
 *      d_in, d_in_off, d_in_len, d_out_off and d_out_cap (d_iov_*, d_stage_off
 *      and d_stage_cap likewise) are not written at all.
 */
#ifndef FLARE_SNAPPY_GPU_H_
#define FLARE_SNAPPY_GPU_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FSG_OK 0
#define FSG_CORRUPT 1
#define FSG_BAD_HEADER 2
#define FSG_SLOT_TOO_SMALL 3
#define FSG_IOV_TOO_SMALL 4

/* Return codes of the host-side calls. */
#define FSG_SUCCESS 0
#define FSG_ERR_INVALID_ARG -1
#define FSG_ERR_HIP -2
#define FSG_ERR_NO_DEVICE -3

/* decompress flags */
#define FSG_FLAG_VALIDATE_ONLY 1u /* IsValidCompressed: no output written   */
#define FSG_FLAG_STRICT_HEADER 2u /* Parse32WithLimit header (flat API)     */

/* Library version string, e.g. "flare-snappy-gpu 0.1 gfx950". */
const char *fsg_version(void);

/* Binds the calling host thread to `device` and caches its properties.
 * Idempotent.  Returns FSG_SUCCESS or a negative error. */
int fsg_init(int device);

/* Last HIP error text seen by this library on the calling thread. */
const char *fsg_last_error(void);

/* Kernel variants for A/B measurement and tests: 0 = automatic choice,
 * 1 = first-generation kernels (decode: one lane per message, tag by tag;
 * encode: one wave per message with the hash table in LDS), 3 = third
 * generation (decode: software-pipelined batched pieces, one lane per
 * message; encode: lane per message with batched speculative probes and the
 * tables in the workspace, the default encoder), 4 = decode only: the
 * two-pass decoder (lane-per-message index pass writing a tag-start bitmap,
 * then one wave per message executing <= 16-byte pieces in dependency rounds
 * through an LDS output window), the default decoder whenever the workspace
 * holds its bitmap, 5 = decode only: the same two passes with one TAG per
 * lane in the execution pass (registers hold a short literal's bytes from the
 * tag prefetch; no piece map), the default since round 3.  (Generation 2 was
 * retired; 2 is rejected.)  Every
 * variant produces identical bytes and statuses.  Process-wide; not for use
 * while other threads launch batches. */
int fsg_select_kernels(int decode_variant, int encode_variant);

/* Test knob: caps the staging region of each fragment of a message longer
 * than 64 KiB (bytes; 0 = the slot split evenly, the default).  A fragment
 * whose output does not fit its region sends its message through the
 * whole-message fallback pass; small caps exercise that path.  Bytes are
 * unaffected.  Process-wide. */
int fsg_set_split_region_cap(uint32_t bytes);

/* Process-wide tuning and test options (no counterpart in the reference,
 * whose codec has no launch choices).  Each starts from its FSG_<NAME>
 * environment variable, read once when the library is loaded; the launch
 * paths read only this table, never the environment.  Names (values are
 * integers; -1 = the library's automatic rule where one exists):
 *   decode_fork (-1 | 0 | 1), split_walk (0..3), split_class, exec_keep
 *   (bytes of history at a window slide, 512..2000, multiple of 16; up to
 *   3024 for the execution pass's 4 KiB-window instance, which a value
 *   above 2000 sets alone),
 *   chunked_huge, small_persist, small_batch, split_huge, walk_order,
 *   lean_walk, exec_big_blocks, exec_prio, exec_big_blocks_fork, exec_pack,
 *   encode_wave_min, encode_wave_share, encode_wave_all_mb,
 *   encode_lanes, encode_wave_per_cu, encode_wave_wg, lz4_big_min,
 *   and the LZ4 side's, described in flare_lz4_gpu.h: lz4_encode_wave_min,
 *   lz4_encode_wave_per_cu, lz4f_force_serial, lz4f_block_wave_min,
 *   lz4f_nosize_fast, lz4f_length_wave_min, lz4f_linked_fast.
 * The launch range-checks what it reads (decode: csrc/decode_v4_plan.h):
 * split_class is taken modulo 16 (size class c = bodies under 2^(16 - c)
 * compressed bytes), exec_pack outside 1..64 means 0, block counts outside
 * 1..2^20 and an exec_keep outside its range mean the default.
 * Every value produces the same bytes and statuses.  Set between batches, not
 * while other threads launch.  FSG_ERR_INVALID_ARG for an unknown name.
 * fsg_default_option returns the built-in default (before the environment). */
int fsg_set_option(const char *name, int64_t value);
int fsg_get_option(const char *name, int64_t *value);
int fsg_default_option(const char *name, int64_t *value);

/* 32 + n + n/6 (snappy.cc:55-77). */
size_t fsg_max_compressed_length(size_t n);

/* Gather: copies n byte ranges (d_src[i], d_len[i]) to d_dst + d_dst_off[i]
 * on the device.  The sources may be pinned HOST memory (hipHostMalloc'd,
 * device-mapped): the kernel reads them over PCIe, which is how the host
 * runtime moves cord_buf blocks from the pinned blockmem_allocate hook
 * (flare/io/cord_buf.cc:159-166) into a packed batch without a staging
 * memcpy (the reference walks backing blocks, cord_buf.cc:1469-1475).
 * d_src / d_len / d_dst_off are device arrays. */
int fsg_gather_blocks(const uint64_t *d_src, const uint32_t *d_len, const uint64_t *d_dst_off,
                      uint32_t n, uint8_t *d_dst, void *stream);

/* Pack (compaction): makes n byte ranges that lie spread over slots -- the
 * outputs of fsg_compress_batch or fsg_lz4_compress_batch in their worst-case
 * slots, or decode outputs -- one dense buffer plus an offsets column, on the
 * device, so that a D2H copy or a sender moves result bytes only (no
 * counterpart in the reference, whose Sink appends each message's bytes where
 * the caller wants them).  With `align` a power of two from 1 to 256:
 *   eff[i]        = (d_status && d_status[i] != FSG_OK) ? 0 : d_len[i]
 *   d_pack_off[i] = sum over j < i of round_up(eff[j], align)      (uint64)
 *   *d_total      = sum over all j of round_up(eff[j], align)
 *   d_dst[d_pack_off[i] .. + eff[i]) = d_src[d_src_off[i] .. + eff[i])
 * A message whose status is not FSG_OK takes no room and none of its bytes
 * are read.  Bytes of d_dst outside those ranges -- alignment padding and
 * everything from *d_total on -- are NOT written.  d_src and d_dst must not
 * overlap (not checked).  d_dst = NULL: only the offsets and the total are
 * computed (d_src / d_src_off may then be NULL too); a caller sizes a
 * destination that way.  A 16-byte-aligned d_dst with align a multiple of 16
 * gets aligned 16-byte stores, and such a packed buffer keeps the 16-byte
 * path of fsg_gather_blocks when it feeds a decode.  Any n_msgs up to
 * 2^32 - 1, totals in uint64; n_msgs = 0 writes *d_total = 0.  The work is
 * balanced by destination bytes, not by message, so batches mixing a million
 * small bodies with bodies of megabytes pack at copy speed.
 * FSG_ERR_INVALID_ARG, before any HIP call, for a null required pointer
 * (d_total always; d_len, d_pack_off, d_workspace and, with d_dst, d_src and
 * d_src_off when n_msgs > 0), an align that is no power of two in 1..256, or
 * workspace_bytes below fsg_pack_workspace_bytes(n_msgs).  The workspace is
 * scratch (block sums of the offset scan). */
size_t fsg_pack_workspace_bytes(uint32_t n_msgs);
int fsg_pack_batch(const uint8_t *d_src, const uint64_t *d_src_off, const uint32_t *d_len,
                   const int32_t *d_status /* may be NULL */, uint32_t n_msgs, uint32_t align,
                   uint8_t *d_dst /* NULL: offsets and total only */, uint64_t *d_pack_off,
                   uint64_t *d_total /* one u64 */, void *d_workspace, size_t workspace_bytes,
                   void *stream);

/* Host-side header parse.  lenient != 0: ReadUncompressedLength rules
 * (5th byte's high bits dropped); lenient == 0: Parse32WithLimit rules.
 * Returns the header byte count (1..5), or 0 if the header is invalid. */
int fsg_get_uncompressed_length(const void *compressed, size_t n,
                                uint32_t *ulen, int lenient);

/* Device header pass: for each message writes its (lenient or strict)
 * uncompressed length into d_ulen (0xFFFFFFFF if the header is invalid).
 * Lets a caller size output slots without a host round trip per message. */
int fsg_uncompressed_lengths_batch(const uint8_t *d_in, const uint64_t *d_in_off,
                                   const uint32_t *d_in_len, uint32_t n_msgs,
                                   uint32_t *d_ulen, int lenient, void *stream);

/* Device workspace for fsg_compress_batch: per-lane hash tables (one
 * htsize-entry table per concurrently encoding lane, htsize per
 * WorkingMemory::GetHashTable, snappy.cc:247-271; 4-byte entries, a position
 * and its fingerprint, so twice the reference's u16 table: up to 16 GiB at
 * the 262,144-lane cap with 64 KiB fragments) plus a work counter.
 * max_in_len bounds every message length of the batch (0 = any).  Passing a
 * smaller or NULL workspace selects the LDS-table wave-per-message encoder. */
size_t fsg_compress_workspace_bytes(uint32_t n_msgs, uint32_t max_in_len);
/* Device workspace for fsg_decompress_batch.  total_in_bytes = the size of
 * the packed input (an upper bound of the sum of d_in_len): the two-pass
 * decoder keeps a tag-start bitmap of 1 bit per input byte there.  With
 * total_in_bytes = 0 (or a NULL / smaller workspace) the single-pass decoder
 * runs; a workspace sized for less input than the batch holds still decodes
 * every message correctly (the overflow falls back to the single-pass
 * kernel).  The workspace is scratch: its content between calls is
 * irrelevant. */
size_t fsg_decompress_workspace_bytes(uint32_t n_msgs, uint64_t total_in_bytes);

/* Batched compress.  Message i is d_in[d_in_off[i] .. +d_in_len[i]); its
 * compressed stream (varint header + 64 KiB fragments, byte-identical to
 * snappy::Compress) is written to d_out[d_out_off[i] ..]; each slot must
 * hold fsg_max_compressed_length(d_in_len[i]) bytes and slots must not
 * overlap.  d_out_len[i] receives the compressed length, d_status[i] FSG_OK.
 * max_in_len: an upper bound of every d_in_len[i] (sizes the LDS hash
 * table; pass 0 for "up to 64 KiB-fragment tables"). */
int fsg_compress_batch(const uint8_t *d_in, const uint64_t *d_in_off,
                       const uint32_t *d_in_len, uint32_t n_msgs,
                       uint32_t max_in_len, uint8_t *d_out,
                       const uint64_t *d_out_off, uint32_t *d_out_len,
                       int32_t *d_status, void *d_workspace,
                       size_t workspace_bytes, void *stream);

/* Batched decompress.  Message i's compressed bytes are
 * d_in[d_in_off[i] .. +d_in_len[i]); output goes to d_out[d_out_off[i] ..]
 * with capacity d_out_cap[i] (slots must not overlap).  d_out_len[i]
 * receives the header's uncompressed length, d_status[i] a FSG_* status.
 * flags: FSG_FLAG_VALIDATE_ONLY (d_out may be NULL), FSG_FLAG_STRICT_HEADER. */
int fsg_decompress_batch(const uint8_t *d_in, const uint64_t *d_in_off,
                         const uint32_t *d_in_len, uint32_t n_msgs,
                         uint8_t *d_out, const uint64_t *d_out_off,
                         const uint32_t *d_out_cap, uint32_t *d_out_len,
                         int32_t *d_status, uint32_t flags, void *d_workspace,
                         size_t workspace_bytes, void *stream);

/* fsg_decompress_batch with its two passes on two streams: pass 1 (header
 * checks, the tag walk, the tag-start bitmap) runs on `pass1_stream`, pass 2
 * (execution) on `stream` after pass 1 (an event).  Same bytes and statuses.
 * A caller decoding a stream of batches alternates two sets of
 * workspace / output / d_out_len / d_status buffers, so batch k+1's pass 1
 * runs beside batch k's pass 2 (the tag walk is latency-bound, the execution
 * issue-bound).  The inputs must be ready on `pass1_stream`; calls that share
 * any of those buffers must be ordered by the caller (pass 1 writes the
 * workspace, d_out_len, d_status and, for messages cut into 64 KiB segments,
 * 4 bytes of d_out).  Results are valid once `stream` is synchronised.
 * Meant for uniform batches: this form never forks the large-message passes
 * onto the side streams (fsg_decompress_batch does for batches of more than
 * 128K messages), so a mixed batch with very large bodies (CM-like) runs its
 * large-message walk before the execution pass and is faster through
 * fsg_decompress_batch.  When the library cannot create its per-device
 * events, `stream` waits on `pass1_stream` and every pass runs on `stream`. */
int fsg_decompress_batch_2s(const uint8_t *d_in, const uint64_t *d_in_off,
                            const uint32_t *d_in_len, uint32_t n_msgs,
                            uint8_t *d_out, const uint64_t *d_out_off,
                            const uint32_t *d_out_cap, uint32_t *d_out_len,
                            int32_t *d_status, uint32_t flags, void *d_workspace,
                            size_t workspace_bytes, void *stream, void *pass1_stream);

/* Batched UncompressAsMuchAsPossible (snappy.cc:1530-1535) over each
 * message's stream cut into `frag`-byte source pieces, as Source::Peek hands
 * them out (0 = one piece, a ByteArraySource; flare's cord_buf blocks carry
 * 8160 bytes).  d_out slots as for fsg_decompress_batch, sized for the
 * header's length.  Per message: d_produced[i] = the reference's return value
 * (SnappyScatteredWriter::Produced(), which counts the 64 KiB block a failing
 * SlowAppend just filled twice); d_got[i] = the bytes its sink receives, which
 * are d_out[d_out_off[i] .. + d_got[i]), byte-identical to the reference's.
 * d_status[i]: FSG_OK (the whole stream decoded), FSG_CORRUPT (it stopped
 * early), FSG_BAD_HEADER (produced 0), or FSG_SLOT_TOO_SMALL (the reference
 * would write past the slot; d_got / d_produced 0).  Workspace as for
 * fsg_decompress_batch.  Streams the batch decoder accepts cost what a
 * decompress costs; the others are walked serially, one lane each: a
 * rejected message of L output bytes costs O(L / 16) serial 16-byte steps
 * (literals, copies reaching 16+ bytes back) up to O(L) byte steps (short-
 * offset copies, block edges) -- a 64 KiB body ~0.2-3 ms on its lane. */
int fsg_decompress_batch_partial(const uint8_t *d_in, const uint64_t *d_in_off,
                                 const uint32_t *d_in_len, uint32_t n_msgs, uint32_t frag,
                                 uint8_t *d_out, const uint64_t *d_out_off,
                                 const uint32_t *d_out_cap, uint32_t *d_got,
                                 uint64_t *d_produced, int32_t *d_status, void *d_workspace,
                                 size_t workspace_bytes, void *stream);

/* Batched RawUncompressToIOVec (snappy.cc:1122-1132).  Message i's iovecs
 * are entries [d_iov_first[i], d_iov_first[i + 1]) of d_iov_base (device
 * addresses) / d_iov_len; d_iov_first has n_msgs + 1 entries.  The stream is
 * decoded into the caller's staging slot (d_stage / d_stage_off / d_stage_cap,
 * sized for the header's length, as fsg_decompress_batch's output) and then
 * copied into the iovecs in order, filling each before the next, as
 * SnappyIOVecWriter does.  d_out_len[i] = the header's length.  d_status[i]:
 * FSG_OK (the reference's true; the iovecs hold its bytes, bytes past the
 * length untouched), FSG_CORRUPT / FSG_BAD_HEADER / FSG_IOV_TOO_SMALL (its
 * false; the iovecs hold what the reference leaves in place: the output's
 * prefix filling every iovec for FSG_IOV_TOO_SMALL, the decoded prefix, a
 * literal cut by the end of input and the last fast append's 16-byte spill
 * for FSG_CORRUPT -- a rejected stream is re-walked serially by one lane,
 * O(output bytes); nothing for FSG_BAD_HEADER), or FSG_SLOT_TOO_SMALL
 * (staging sizing error; the iovecs are untouched). */
int fsg_decompress_batch_iovec(const uint8_t *d_in, const uint64_t *d_in_off,
                               const uint32_t *d_in_len, uint32_t n_msgs,
                               const uint64_t *d_iov_base, const uint64_t *d_iov_len,
                               const uint32_t *d_iov_first, uint8_t *d_stage,
                               const uint64_t *d_stage_off, const uint32_t *d_stage_cap,
                               uint32_t *d_out_len, int32_t *d_status, void *d_workspace,
                               size_t workspace_bytes, void *stream);

/* ---- Path reports: which device path the last batch took.
 *
 * Every route yields the same bytes and statuses, but some are far slower: a
 * serial one-lane-per-message fallback pass finishes the messages the main
 * passes hand over, and a call without a usable workspace runs wholly on the
 * single-pass (decode) or wave-per-message (encode) kernels.  The calls count
 * what they hand over in the first fsg_report_header_bytes (256) bytes of the
 * workspace; these functions turn a HOST copy of those bytes into counts.
 *
 * The library adds no synchronisation: the caller copies the header off the
 * device itself, on the batch call's stream, next to the status column it
 * downloads anyway.  The report functions are pure host code: no HIP call, no
 * device needed.  They repeat the batch call's routing decision from their
 * arguments (pass the batch call's n_msgs, workspace_bytes, flags and
 * max_in_len; workspace_bytes = 0 for a NULL workspace) and from the current
 * fsg_select_kernels / fsg_set_option state, and read the header only when
 * that routing says the workspace was used; header_host_copy may be NULL
 * otherwise.
 *
 * Two limits.  A report describes the LAST call that used that workspace, so
 * the header must be copied before the workspace is reused.  And it must be
 * computed before fsg_select_kernels or the options change, since the routing
 * is repeated from their current values.
 *
 * fsg_decompress_batch_2s takes fsg_decompress_report with its own flags;
 * fsg_decompress_batch_partial and fsg_decompress_batch_iovec decode through
 * the same routing with flags = 0, and fsg_decompress_report covers them with
 * flags = 0.  fsg_lz4_decompress_report (flare_lz4_gpu.h) fills the same
 * decode struct.
 *
 * Return: FSG_SUCCESS, or FSG_ERR_INVALID_ARG when `out` is NULL or when the
 * header is NULL although the routing says it must be read. */
enum {
  FSG_PATH_MAIN = 0,          /* two-pass decoder / table-workspace encoder */
  FSG_PATH_SINGLE_DESIGN = 1, /* single-pass by design: validate-only, or the LZ4 call without a workspace */
  FSG_PATH_NO_WORKSPACE = 2,  /* workspace NULL or too small */
  FSG_PATH_FORCED = 3         /* forced by fsg_select_kernels */
};
struct fsg_decode_report {
  uint64_t path;                   /* FSG_PATH_* */
  uint64_t single_pass_messages;   /* n_msgs when path != 0 */
  uint64_t fallback_messages;      /* decoded serially by pass 3; the three causes sum to it */
  uint64_t fallback_bitmap;        /*   tag bitmap did not fit the workspace */
  uint64_t fallback_wide_offsets;  /*   packed pass: buffer offsets beyond 32 bits */
  uint64_t fallback_pack_guard;    /*   packed pass: iteration guard */
  uint64_t bitmap_words_requested; /* the bitmap allocator's final value */
  uint64_t bitmap_words_capacity;  /* what workspace_bytes leaves for the bitmap */
  uint64_t large_messages;         /* indexed by a wave each */
  uint64_t huge_messages;          /*   the largest of them (listed apart) */
};
struct fsg_encode_report {
  uint64_t path;                  /* 0, 2 or 3 */
  uint64_t no_workspace_messages; /* n_msgs when path != 0 */
  uint64_t units_listed;          /* fragments and long messages on the shared list */
  uint64_t split_messages;        /* messages over 64 KiB */
  uint64_t unit_bytes;            /* bytes of the listed units */
  uint64_t wave_units;            /* of units_listed, the wave encoder's share */
  uint64_t fallback_messages;     /* split messages re-encoded whole by one lane */
};
size_t fsg_report_header_bytes(void);
int fsg_decompress_report(const void *header_host_copy, uint32_t n_msgs, size_t workspace_bytes,
                          uint32_t flags, struct fsg_decode_report *out);
int fsg_compress_report(const void *header_host_copy, uint32_t n_msgs, uint32_t max_in_len,
                        size_t workspace_bytes, struct fsg_encode_report *out);

#ifdef __cplusplus
}
#endif
#endif /* FLARE_SNAPPY_GPU_H_ */
