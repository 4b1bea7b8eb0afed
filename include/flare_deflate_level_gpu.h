/*
 * flare_deflate_level_gpu.h -- compression levels for the batched deflate
 * compress of include/flare_deflate_compress_gpu.h (MI355X, gfx950).
 *
 * Reference interface: flare's GzipCompress(const cord_buf&, cord_buf*, const
 * GzipCompressOptions*), whose options carry a format and a compression
 * level.  The level here is an argument of the call, not a process option.
 *
 * Everything but the level is the contract of the level-less call in
 * flare_deflate_compress_gpu.h, at every level: formats, slots of
 * fsg_deflate_max_length bytes, the workspace of fsg_deflate_workspace_bytes,
 * statuses, what the call writes, and the report.  The level-less call is this
 * call at FSG_DEFLATE_LEVEL_FAST, the same code.
 *
 * The levels.  csrc/deflate_format.h ("levels") states the rule and
 * host/deflate_cpu.cc (fsh_cpu_deflate_level) is its serial model: that text
 * defines the bytes, and the device gives the model's bytes exactly.  Every
 * body at every level is a legal stream that zlib's inflate reads back; byte
 * equality with zlib's deflate is not offered at any level.
 *   STORED  every unit of 65,472 bytes is a stored block, nothing is parsed
 *           and no code is built.  A body's length is exactly
 *           what fsg_deflate_max_length gives (zlib's Z_NO_COMPRESSION).
 *   FAST    one candidate per hash slot, greedy parse.
 *   BEST    the position table holds two candidates per slot (the newer and
 *           the older in one 32-bit word); a position takes the longer match
 *           of the two, the nearer on equal lengths.  One lazy step inside
 *           each window of 64 positions: a position whose successor in the
 *           same window has a longer match becomes a literal.  After a window
 *           each slot it touched takes one new entry, its highest position;
 *           the former older candidate drops out.  Units, blocks, the block
 *           choice, the codes, the wrappers and the bound are those of FAST.
 *           5 to 8 % smaller than FAST on text, source and JSON.
 *
 * FSG_ERR_INVALID_ARG, decided before any HIP call: a level above
 * FSG_DEFLATE_LEVEL_BEST, whatever the other arguments; then what the
 * level-less call refuses.  n_msgs == 0 with a known level and format
 * succeeds and launches nothing.
 */
#ifndef FLARE_DEFLATE_LEVEL_GPU_H_
#define FLARE_DEFLATE_LEVEL_GPU_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FSG_DEFLATE_LEVEL_STORED 0u
#define FSG_DEFLATE_LEVEL_FAST 1u /* what the level-less call writes */
#define FSG_DEFLATE_LEVEL_BEST 2u

int fsg_deflate_batch_level(const uint8_t *d_in, const uint64_t *d_in_off,
                            const uint32_t *d_in_len, uint32_t n_msgs,
                            uint8_t *d_out, const uint64_t *d_out_off,
                            uint32_t *d_out_len, int32_t *d_status,
                            uint32_t format, uint32_t level, void *d_workspace,
                            size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* FLARE_DEFLATE_LEVEL_GPU_H_ */
