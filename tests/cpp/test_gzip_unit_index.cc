// test_gzip_unit_index.cc -- GzipCompressOptions::unit_index
// (host/gzip_compress.h) on the host alone; run by tests/test_gzip_index.py,
// which reads the bodies with Python's zlib and compares them with the host
// model's flagged bytes.
//   test_gzip_unit_index RAW_IN OUT_DIR
// writes OUT_DIR/index_<level>.bin for compression_level 0, 1 and -1 (named
// m1) with unit_index set, checks that the option is off by default and that
// off equals the three-argument call without it, that every body decompresses
// with GzipDecompress, that the bytes behind the longer head equal the
// unflagged body's behind its 10, and that unit_index with ZLIB returns false
// and appends nothing.
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
  const size_t units = raw.empty() ? 1 : (raw.size() + 65471) / 65472;

  GzipCompressOptions o;
  CHECK(!o.unit_index);
  for (int level : {0, 1, -1}) {
    o.format = GzipCompressOptions::GZIP;
    o.compression_level = level;
    o.unit_index = false;
    cord_buf plain, indexed, back;
    CHECK(policy::GzipCompress(in, &plain, &o));
    o.unit_index = true;
    CHECK(policy::GzipCompress(in, &indexed, &o));
    const std::string p = plain.to_string(), x = indexed.to_string();
    CHECK(x.size() == p.size() + 12 + 2 * units);
    CHECK(x.size() > 22 && x[3] == 4 && x[12] == 'R' && x[13] == 'A');
    CHECK(x.substr(22 + 2 * units) == p.substr(10));
    CHECK(policy::GzipDecompress(indexed, &back));
    CHECK(back.to_string() == raw);
    const std::string name = dir + "/index_" + (level < 0 ? std::string("m1") : std::to_string(level)) + ".bin";
    std::ofstream(name, std::ios::binary) << x;
    o.format = GzipCompressOptions::ZLIB;
    cord_buf none;
    CHECK(!policy::GzipCompress(in, &none, &o) && none.size() == 0);
  }
  printf("%d failures\n", g_failures);
  return g_failures ? 1 : 0;
}
