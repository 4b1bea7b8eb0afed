// gzip_compress.cc -- policy::{Gzip,Zlib}{Compress,Decompress} (see gzip_compress.h).
#include "gzip_compress.h"

#include <cstdio>
#include <mutex>
#include <vector>

#include "deflate_cpu.h"
#include "inflate_cpu.h"

namespace flare::rpc::policy {

namespace {

constexpr uint32_t kZlibFormat = 1, kGzipFormat = 2;  // FSG_INFLATE_ZLIB, FSG_INFLATE_GZIP

bool Deflate(uint32_t format, const cord_buf& in, cord_buf* out, uint32_t level = 1, uint32_t flags = 0) {
  const size_t n = in.size();
  std::vector<uint8_t> src(n);
  in.copy_to(src.data(), n);
  std::vector<uint8_t> body(fsh_cpu_deflate_bound_flags(n, format, flags));
  uint64_t len = 0;
  if (fsh_cpu_deflate_flags(format, level, flags, src.data(), n, body.data(), body.size(), &len) != 0) return false;
  return out->append(body.data(), len) == 0;
}

bool Inflate(uint32_t format, const cord_buf& in, cord_buf* out) {
  const size_t n = in.size();
  std::vector<uint8_t> body(n);
  in.copy_to(body.data(), n);
  // the length comes from walking the peer's stream, which writes nothing;
  // deflate expands by 1,032 at most, so the walk's answer is bounded by the
  // body before anything is allocated for it
  uint64_t len = 0;
  if (fsh_cpu_inflate_length(format, body.data(), n, &len) != 0) return false;
  if (len > 1032ull * n) return false;
  std::vector<uint8_t> raw(len);
  uint64_t got = 0;
  if (fsh_cpu_inflate(format, body.data(), n, raw.data(), len, &got) != 0 || got != len) return false;
  return out->append(raw.data(), len) == 0;
}

bool CompressMessage(bool (*f)(const cord_buf&, cord_buf*), const Message& msg, cord_buf* buf) {
  cord_buf serialized_pb;
  if (msg.SerializeToCordBuf(&serialized_pb)) return f(serialized_pb, buf);
  fprintf(stderr, "[WARNING] Fail to serialize input pb=%p\n", (const void*)&msg);
  return false;
}

bool DecompressMessage(bool (*f)(const cord_buf&, cord_buf*), const char* what, const cord_buf& data, Message* msg) {
  cord_buf binary_pb;
  if (f(data, &binary_pb)) return msg->ParseFromCordBuf(binary_pb);
  fprintf(stderr, "[WARNING] Fail to %s decompress, size=%zu\n", what, data.size());
  return false;
}

}  // namespace

bool GzipCompress(const cord_buf& in, cord_buf* out) { return Deflate(kGzipFormat, in, out); }
bool GzipCompress(const cord_buf& in, cord_buf* out, const GzipCompressOptions* options) {
  if (!options) return GzipCompress(in, out);
  const int z = options->compression_level;
  if (z < -1 || z > 9) return false;
  const uint32_t level = z == 0 ? 0u : z >= 1 && z <= 3 ? 1u : 2u;
  uint32_t format;
  if (options->format == GzipCompressOptions::GZIP)
    format = kGzipFormat;
  else if (options->format == GzipCompressOptions::ZLIB)
    format = kZlibFormat;
  else
    return false;
  if (options->unit_index && format != kGzipFormat) return false;  // zlib has no field to carry it
  return Deflate(format, in, out, level, options->unit_index ? 1u : 0u);  // FSG_DEFLATE_FLAG_UNIT_INDEX
}
bool GzipDecompress(const cord_buf& in, cord_buf* out) { return Inflate(kGzipFormat, in, out); }
bool ZlibCompress(const cord_buf& in, cord_buf* out) { return Deflate(kZlibFormat, in, out); }
bool ZlibDecompress(const cord_buf& in, cord_buf* out) { return Inflate(kZlibFormat, in, out); }

bool GzipCompress(const Message& msg, cord_buf* buf) {
  return CompressMessage(static_cast<bool (*)(const cord_buf&, cord_buf*)>(GzipCompress), msg, buf);
}
bool GzipDecompress(const cord_buf& data, Message* msg) {
  return DecompressMessage(static_cast<bool (*)(const cord_buf&, cord_buf*)>(GzipDecompress), "gzip", data, msg);
}
bool ZlibCompress(const Message& msg, cord_buf* buf) {
  return CompressMessage(static_cast<bool (*)(const cord_buf&, cord_buf*)>(ZlibCompress), msg, buf);
}
bool ZlibDecompress(const cord_buf& data, Message* msg) {
  return DecompressMessage(static_cast<bool (*)(const cord_buf&, cord_buf*)>(ZlibDecompress), "zlib", data, msg);
}

}  // namespace flare::rpc::policy

namespace flare::rpc {

int GlobalInitializeGzipZlib() {
  static std::once_flag once;
  static int rc = -1;
  std::call_once(once, [] {
    const int g = RegisterCompressHandler(
        COMPRESS_TYPE_GZIP, CompressHandler{policy::GzipCompress, policy::GzipDecompress, "gzip"});
    const int z = RegisterCompressHandler(
        COMPRESS_TYPE_ZLIB, CompressHandler{policy::ZlibCompress, policy::ZlibDecompress, "zlib"});
    rc = g == 0 && z == 0 ? 0 : -1;
  });
  return rc;
}

}  // namespace flare::rpc
