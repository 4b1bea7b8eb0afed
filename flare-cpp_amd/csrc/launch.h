// launch.h -- the host entry points of the codec kernels: every launch_*,
// *_workspace_bytes and path-report function, declared once.  Included by
// capi.hip (the callers) and by each .hip that defines one, so a definition
// that drifts from its declaration no longer links as an overload nobody
// calls.
#pragma once

#include "decode_v4_plan.h"  // decode_v4_workspace_bytes, decode_v4_bitmap_capacity_words (inline)
#include "encode_v3_plan.h"
#include "lz4_frame_plan.h"  // and lz4_plan.h: the LZ4 sizes, options and plans (inline)
#include "snappy_device.h"

namespace fsg {

// ---- Snappy decode
hipError_t launch_decode(const u8* in, const u64* in_off, const u32* in_len,
                         u32 n_msgs, u8* out, const u64* out_off,
                         const u32* out_cap, u32* out_len, i32* status,
                         u32 flags, hipStream_t stream);
hipError_t launch_headers(const u8* in, const u64* in_off, const u32* in_len,
                          u32 n_msgs, u32* ulen, int lenient, hipStream_t stream);
hipError_t launch_decode_v3(const u8* in, const u64* in_off, const u32* in_len,
                            u32 n_msgs, u8* out, const u64* out_off,
                            const u32* out_cap, u32* out_len, i32* status,
                            u32 flags, hipStream_t stream);
hipError_t launch_decode_v4(const u8* in, const u64* in_off, const u32* in_len,
                            u32 n_msgs, u8* out, const u64* out_off,
                            const u32* out_cap, u32* out_len, i32* status,
                            u32 flags, void* ws, size_t ws_bytes, hipStream_t stream,
                            int exec_variant, hipStream_t pass1_stream);
hipError_t launch_decode_partial(const u8* in, const u64* in_off, const u32* in_len, u32 n_msgs, u32 frag,
                                 u8* out, const u64* out_off, const u32* out_cap, u32* got, u64* produced,
                                 i32* status, hipStream_t stream);
hipError_t launch_iov_scatter(const u8* in, const u64* in_off, const u32* in_len, const u8* stage,
                              const u64* stage_off, const u32* out_len, u32 n_msgs, const u64* iov_base,
                              const u64* iov_len, const u32* iov_first, i32* status, hipStream_t stream);

// ---- Snappy encode
// (encode_v3_plan.h: encode_tables_workspace_bytes, encode_plan_bytes and encode_v3_plan, inline)
EncodeOpts read_encode_opts();  // this call's encode options, from the option table
hipError_t launch_encode_v3(const u8* in, const u64* in_off, const u32* in_len, u32 n_msgs, u8* out,
                            const u64* out_off, u32* out_len, i32* status, void* ws, hipStream_t stream,
                            const EncodePlan& p);
hipError_t launch_encode(const u8* in, const u64* in_off, const u32* in_len,
                         u32 n_msgs, u32 max_in_len, u8* out, const u64* out_off,
                         u32* out_len, i32* status, hipStream_t stream);

// ---- gather, pack
hipError_t launch_gather_blocks(const u64* src, const u32* len, const u64* dst_off, u32 n, u8* dst,
                                hipStream_t stream);
size_t pack_workspace_bytes(u32 n_msgs);
hipError_t launch_pack(const u8* src, const u64* src_off, const u32* len, const i32* status, u32 n, u32 align,
                       u8* dst, u64* pack_off, u64* total, void* ws, hipStream_t stream);

// ---- LZ4
// (lz4_plan.h: lz4_compress_workspace_bytes, lz4_decode_workspace_bytes, lz4_encode_plan and lz4_decode_plan, inline)
// LZ4 compress (lz4_encode_wave.hip): bodies of at least p.wave_min bytes go to the wave encoder
hipError_t launch_lz4_encode(const u8* in, const u64* in_off, const u32* in_len, u32 n_msgs, u8* out,
                             const u64* out_off, u32* out_len, i32* status, void* ws, hipStream_t stream,
                             const Lz4EncodePlan& p);
hipError_t launch_lz4_encode_lanes(const u8* in, const u64* in_off, const u32* in_len, u32 n_msgs, u8* out,
                                   const u64* out_off, u32* out_len, i32* status, void* tables, u64 wave_min,
                                   hipStream_t stream);
hipError_t launch_lz4_decode(const u8* in, const u64* in_off, const u32* in_len, u32 n_msgs, u8* out,
                             const u64* out_off, const u32* out_cap, u32* out_len, i32* status,
                             hipStream_t stream);
hipError_t launch_lz4_decode_fallback(const u8* in, const u64* in_off, const u32* in_len, u32 n_msgs, u8* out,
                                      const u64* out_off, const u32* out_cap, u32* out_len, i32* status,
                                      u32* fb_count, hipStream_t stream);
// Entries that continue earlier output (the blocks of a linked LZ4 frame).
// word[e] >> shift bytes directly below entry e's slot are its history: the
// index passes accept offsets into them.  An entry with a bit of chained_mask
// is executed by its chain's wave, not by the execution pass: chain c is the
// entries first[c] .. first[c] + count[c], run in order by one wave when
// (state[c] & ~pending_mask) == pending; entries with a bit of skip_mask are
// passed over.  The wave stops at the first entry the index pass did not
// answer FSG_OK, and adds done_add to state[c] only when it ran to the end.
struct Lz4Chains {
  const u32* word;
  u32 shift, chained_mask, skip_mask;
  u32 n_chains;
  const u32* first;
  const u32* count;
  u32* state;
  u32 pending, pending_mask, done_add;
};
// chains = nullptr: no entry has a prefix (the forms of the kernels without one)
hipError_t launch_lz4_decode2(const u8* in, const u64* in_off, const u32* in_len, u32 n_msgs, u8* out,
                              const u64* out_off, const u32* out_cap, u32* out_len, i32* status, void* ws,
                              hipStream_t stream, hipStream_t pass1_stream, const Lz4DecodePlan& p,
                              const Lz4Chains* chains = nullptr);

// ---- LZ4 frames (lz4_frame_encode.hip, lz4_frame_decode.hip;
// include/flare_lz4_gpu.h, "LZ4 frames").  The
// calls get no input size: the workspace says what it was sized for, and the
// plan's w.nb_cap gives the block entries it holds (lz4_frame_plan.h:
// lz4f_*_workspace_bytes, lz4f_encode_plan and lz4f_decode_plan, inline).
hipError_t launch_lz4f_encode(const u8* in, const u64* in_off, const u32* in_len, u32 n_msgs, u8* out,
                              const u64* out_off, u32* out_len, i32* status, u32 block_size_id, u32 flags, void* ws,
                              hipStream_t stream, const Lz4fEncodePlan& p);
// fsg_lz4f_xxh32_batch: XXH32 of each body on the checksum kernel (lz4f_xxh.h), no workspace
hipError_t launch_lz4f_xxh32(const u8* in, const u64* in_off, const u32* in_len, u32 n_msgs, u32 seed, u32* xxh,
                             hipStream_t stream);
hipError_t launch_lz4f_decode(const u8* in, const u64* in_off, const u32* in_len, u32 n_msgs, u8* out,
                              const u64* out_off, const u32* out_cap, u32* out_len, i32* status, void* ws,
                              hipStream_t stream, const Lz4fDecodePlan& p);
// fsg_lz4f_decoded_lengths_batch: on a decompress workspace
hipError_t launch_lz4f_decoded_lengths(const u8* in, const u64* in_off, const u32* in_len, u32 n_msgs, u64* lengths,
                                       i32* status, void* ws, hipStream_t stream, const Lz4fDecodePlan& p);
hipError_t launch_lz4f_content_sizes(const u8* in, const u64* in_off, const u32* in_len, u32 n_msgs, u64* sizes,
                                     i32* status, hipStream_t stream);

// ---- inflate (inflate.hip; include/flare_deflate_gpu.h): a wave per body, no workspace
hipError_t launch_inflate(const u8* in, const u64* in_off, const u32* in_len, u32 n_msgs, u8* out, const u64* out_off,
                          const u32* out_cap, u32* out_len, i32* status, u32 format, hipStream_t stream);
hipError_t launch_inflate_lengths(const u8* in, const u64* in_off, const u32* in_len, u32 n_msgs, u64* lengths,
                                  i32* status, u32 format, hipStream_t stream);
// fsg_crc32_batch / fsg_adler32_batch: the checksum kernel alone
hipError_t launch_inflate_sum(const u8* in, const u64* in_off, const u32* in_len, u32 n_msgs, u32* sum, bool adler,
                              hipStream_t stream);

// the trailer judge behind a decode kernel: zlib or gzip bodies left FSG_OK (n_msgs > 0)
hipError_t launch_inflate_judge(const u8* in, const u64* in_off, const u32* in_len, u32 n_msgs, const u8* out,
                                const u64* out_off, u32* out_len, i32* status, u32 format, hipStream_t stream);

// ---- inflate by units (inflate_units.hip; include/flare_deflate_index_gpu.h): a
// wave per unit of the gzip bodies that carry a unit index.
// inflate_units_entry_capacity: the unit entries a workspace holds (0: below
// inflate_units_workspace_bytes(n_msgs, 0)).
size_t inflate_units_workspace_bytes(u32 n_msgs, u64 extra_units);
u64 inflate_units_entry_capacity(u32 n_msgs, size_t ws_bytes);
hipError_t launch_inflate_units(const u8* in, const u64* in_off, const u32* in_len, u32 n_msgs, u8* out,
                                const u64* out_off, const u32* out_cap, u32* out_len, i32* status, u32 format,
                                void* ws, size_t ws_bytes, hipStream_t stream);
hipError_t launch_inflate_units_lengths(const u8* in, const u64* in_off, const u32* in_len, u32 n_msgs, u64* lengths,
                                        i32* status, u32 format, void* ws, size_t ws_bytes, hipStream_t stream);
struct InflateUnitsHeaderCounts {
  u32 parallel_bodies, parallel_units, no_index, unusable, mismatch, overflow;
};
void inflate_units_header_counts(const void* header, InflateUnitsHeaderCounts* c);

// ---- deflate compress (deflate.hip; include/flare_deflate_compress_gpu.h).  The
// call gets no input size: deflate_unit_capacity gives the units a workspace
// holds (0: below deflate_workspace_bytes(n_msgs, 0)).
size_t deflate_workspace_bytes(u32 n_msgs, u64 total_in_bytes);
u64 deflate_unit_capacity(u32 n_msgs, size_t ws_bytes);
hipError_t launch_deflate(const u8* in, const u64* in_off, const u32* in_len, u32 n_msgs, u8* out, const u64* out_off,
                          u32* out_len, i32* status, u32 format, u32 level, u32 flags, void* ws, size_t ws_bytes,
                          hipStream_t stream);  // level: defl::kLevelStored / Fast / Best (deflate_format.h);
                                                // flags: gzidx::kFlagUnitIndex (gzip_index.h), gzip only
struct DeflateHeaderCounts {
  u32 units, stored, fixed, dynamic, overflow;
};
void deflate_header_counts(const void* header, DeflateHeaderCounts* c);

// ---- path report (capi.hip: fsg_decompress_report and its kin): what each
// codec's 256-byte workspace header holds after a call, read from a host copy
struct DecodeHeaderCounts {
  u32 bitmap_words;  // the bump allocator's final value
  u32 large, huge;   // messages listed for the wave-per-message index pass
  u32 fallback, fallback_bitmap, fallback_wide, fallback_guard;  // pass 3 and its causes
};
struct EncodeHeaderCounts {
  u32 units, split, fallback;
  u64 unit_bytes;
};
struct Lz4EncodeHeaderCounts {
  u32 listed, wave_messages;
  u64 wave_bytes;
};
struct Lz4fEncodeHeaderCounts {
  u32 blocks, raw_blocks, overflow_messages;
};
struct Lz4fDecodeHeaderCounts {
  u32 fast_messages, fast_blocks, empty_messages;
  u32 serial_linked, serial_no_size, serial_rejected, serial_forced;
  u32 checksummed_units, inner_fallback;
  u32 fast_nosize_messages, fast_nosize_blocks;
  u32 fast_linked_messages, fast_linked_blocks;
};
void lz4f_encode_header_counts(const void* header, Lz4fEncodeHeaderCounts* c);
void lz4f_decode_header_counts(const void* header, Lz4fDecodeHeaderCounts* c);
void decode_v4_header_counts(const void* header, DecodeHeaderCounts* c);
void encode_v3_header_counts(const void* header, EncodeHeaderCounts* c);
void lz4_decode_header_counts(const void* header, DecodeHeaderCounts* c);
void lz4_encode_header_counts(const void* header, Lz4EncodeHeaderCounts* c);

}  // namespace fsg
