// test_gzip_options.cc -- policy::GzipCompress(in, out, const
// GzipCompressOptions*) (host/gzip_compress.h) on the host alone; run by
// tests/test_deflate_level.py, which reads the bodies with Python's zlib and
// compares them with the host model's bytes for the mapped level.
//   test_gzip_options RAW_IN OUT_DIR
// writes OUT_DIR/<gzip|zlib>_<level>.bin for compression_level 0, 1, 6 and -1
// (named m1), checks that nullptr equals the two-argument function, that the
// default options are gzip at level -1, that every body decompresses with
// the format's handler, and that levels 10 and -2 and an unknown format
// return false and append nothing.
#include <cstdio>
#include <fstream>
#include <iterator>
#include <string>

#include "cord_buf.h"
#include "gzip_compress.h"

using flare::cord_buf;
using flare::rpc::policy::GzipCompressOptions;
namespace policy = flare::rpc::policy;

static int g_failures = 0;
#define CHECK(c)                                                            \
  do {                                                                      \
    if (!(c)) {                                                             \
      fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); \
      ++g_failures;                                                         \
    }                                                                       \
  } while (0)

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  std::ifstream fin(argv[1], std::ios::binary);
  const std::string raw((std::istreambuf_iterator<char>(fin)), std::istreambuf_iterator<char>());
  const std::string dir = argv[2];
  cord_buf in;
  in.append(raw);

  cord_buf two, null3, dflt;
  CHECK(policy::GzipCompress(in, &two));
  CHECK(policy::GzipCompress(in, &null3, nullptr));
  CHECK(two.to_string() == null3.to_string());
  GzipCompressOptions o;
  CHECK(o.format == GzipCompressOptions::GZIP && o.compression_level == -1);
  CHECK(policy::GzipCompress(in, &dflt, &o));
  std::string sizes;
  for (int f = 0; f < 2; ++f) {
    o.format = f == 0 ? GzipCompressOptions::GZIP : GzipCompressOptions::ZLIB;
    for (int level : {0, 1, 6, -1}) {
      o.compression_level = level;
      cord_buf out, back;
      CHECK(policy::GzipCompress(in, &out, &o));
      CHECK(f == 0 ? policy::GzipDecompress(out, &back) : policy::ZlibDecompress(out, &back));
      CHECK(back.to_string() == raw);
      if (f == 0 && level == -1) CHECK(out.to_string() == dflt.to_string());
      if (f == 0 && level == 1) CHECK(out.to_string() == two.to_string());
      const std::string name =
          dir + "/" + (f == 0 ? "gzip_" : "zlib_") + (level < 0 ? std::string("m1") : std::to_string(level)) + ".bin";
      std::ofstream(name, std::ios::binary) << out.to_string();
      sizes += " " + std::to_string(out.size());
    }
    for (int level : {10, -2, 100, -100}) {
      o.compression_level = level;
      cord_buf out;
      CHECK(!policy::GzipCompress(in, &out, &o));
      CHECK(out.size() == 0);
    }
  }
  o.format = static_cast<GzipCompressOptions::Format>(3);
  o.compression_level = 6;
  cord_buf none;
  CHECK(!policy::GzipCompress(in, &none, &o) && none.size() == 0);
  printf("sizes%s\n%d failures\n", sizes.c_str(), g_failures);
  return g_failures ? 1 : 0;
}
