// gzip_compress.h -- CompressHandlers for COMPRESS_TYPE_GZIP (2) and
// COMPRESS_TYPE_ZLIB (3), shaped like the reference's (flare
// rpc/policy/gzip_compress.h: GzipCompress / GzipDecompress / ZlibCompress /
// ZlibDecompress, same meaning of arguments and return values), written
// against those signatures only.  The reference's third overload,
// GzipCompress(in, out, const GzipCompressOptions*), is taken too: the format
// comes from the options and zlib's compression_level maps onto the levels
// of csrc/deflate_format.h: 0 -> 0 (stored units only), 1 .. 3 (zlib's greedy
// levels) -> 1, 4 .. 9 and -1 (its lazy levels and its default) -> 2, anything
// else returns false.  nullptr equals the two-argument function; the two-
// argument functions write level 1.  unit_index (not the reference's; off by
// default) writes a GZIP body with its units' compressed lengths in the
// header's extra field (include/flare_deflate_index_gpu.h), which
// fsg_inflate_units_batch decodes a wave per unit and every other inflate
// skips; with ZLIB, which has no such field, it returns false.
//
// Compress writes the bodies csrc/deflate_format.h defines (host/deflate_cpu.h:
// legal gzip / zlib streams that any inflate reads, not zlib's bytes);
// Decompress reads whatever zlib's inflate reads
// (include/flare_deflate_gpu.h, "Acceptance rule"), one gzip member per body.
// Per call the host codec runs: one body is one serial walk, which a CPU core
// runs faster than one GPU wave.  Batches go through fsg_deflate_batch and
// fsg_inflate_batch.
#pragma once

#include "compress.h"
#include "cord_buf.h"

namespace flare::rpc::policy {

struct GzipCompressOptions {
  enum Format { GZIP = 1, ZLIB = 2 };
  Format format = GZIP;
  int compression_level = -1;
  bool unit_index = false;
};
bool GzipCompress(const cord_buf& in, cord_buf* out, const GzipCompressOptions* options);

bool GzipCompress(const Message& msg, cord_buf* buf);
bool GzipDecompress(const cord_buf& data, Message* msg);
bool GzipCompress(const cord_buf& in, cord_buf* out);
bool GzipDecompress(const cord_buf& in, cord_buf* out);

bool ZlibCompress(const Message& msg, cord_buf* buf);
bool ZlibDecompress(const cord_buf& data, Message* msg);
bool ZlibCompress(const cord_buf& in, cord_buf* out);
bool ZlibDecompress(const cord_buf& in, cord_buf* out);

}  // namespace flare::rpc::policy

namespace flare::rpc {
// Registers the two handlers at COMPRESS_TYPE_GZIP and COMPRESS_TYPE_ZLIB once
// per process; 0 when both registrations succeeded.
int GlobalInitializeGzipZlib();
}  // namespace flare::rpc
