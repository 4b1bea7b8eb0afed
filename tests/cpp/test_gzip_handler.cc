// test_gzip_handler.cc -- the gzip and zlib CompressHandlers
// (host/gzip_compress.h: policy::GzipCompress / GzipDecompress / ZlibCompress /
// ZlibDecompress, GlobalInitializeGzipZlib) on the host alone; run by
// tests/test_deflate.py, which reads what the handler wrote with Python's zlib.
//   test_gzip_handler GZIP_IN RAW_OUT ZLIB_OUT
// registers the handlers at types 2 and 3, round-trips bodies and a message,
// reads a gzip body spelled out here, rejects broken bodies, decompresses the
// gzip body in GZIP_IN (any body zlib writes) into RAW_OUT, and writes the
// handler's zlib body of the same bytes to ZLIB_OUT.
#include <cstdio>
#include <fstream>
#include <iterator>
#include <string>

#include "compress.h"
#include "cord_buf.h"
#include "gzip_compress.h"
#include "snappy_message.h"

using flare::cord_buf;
using namespace flare::rpc;

static int g_failures = 0;
#define CHECK(c)                                                            \
  do {                                                                      \
    if (!(c)) {                                                             \
      fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); \
      ++g_failures;                                                         \
    }                                                                       \
  } while (0)

static std::string pattern(int len) {  // the reference tests' text loop
  std::string t;
  while ((int)t.size() < len) {
    for (int i = 0; i < 26 && (int)t.size() < len; i++) t.push_back('a' + i);
    for (int i = 0; i < 10 && (int)t.size() < len; i++) t.push_back('0' + i);
  }
  return t;
}

typedef bool (*Codec)(const cord_buf&, cord_buf*);

int main(int argc, char** argv) {
  if (argc != 4) return 2;
  CHECK(FindCompressHandler(COMPRESS_TYPE_GZIP) == nullptr && FindCompressHandler(COMPRESS_TYPE_ZLIB) == nullptr);
  CHECK(GlobalInitializeGzipZlib() == 0);
  CHECK(std::string(CompressTypeToCStr(COMPRESS_TYPE_GZIP)) == "gzip");
  CHECK(std::string(CompressTypeToCStr(COMPRESS_TYPE_ZLIB)) == "zlib");
  CHECK(GlobalInitializeGzipZlib() == 0);  // once per process: the same answer
  // a second registration of either type fails
  CHECK(RegisterCompressHandler(COMPRESS_TYPE_GZIP,
                                CompressHandler{policy::GzipCompress, policy::GzipDecompress, "again"}) != 0);
  CHECK(RegisterCompressHandler(COMPRESS_TYPE_ZLIB,
                                CompressHandler{policy::ZlibCompress, policy::ZlibDecompress, "again"}) != 0);
  const Codec comp[2] = {policy::GzipCompress, policy::ZlibCompress};
  const Codec decomp[2] = {policy::GzipDecompress, policy::ZlibDecompress};
  for (int t = 0; t < 2; ++t) {
    for (int n : {0, 1, 8160, 8161, 300000}) {  // 8,160: one cord_buf block, and one byte more
      cord_buf in, out, back;
      in.append(pattern(n));
      CHECK(comp[t](in, &out));
      CHECK(decomp[t](out, &back));
      CHECK(back.to_string() == pattern(n));
      CHECK(n < 1000 || out.size() < (size_t)n / 4);
      CHECK(!decomp[1 - t](out, &back));  // the other wrapper
      std::string f = out.to_string();
      cord_buf cut, more, flip;
      cut.append(f.substr(0, f.size() - 1));
      CHECK(!decomp[t](cut, &back));
      more.append(f + "x");
      CHECK(!decomp[t](more, &back));
      f[f.size() - 2] ^= 1;  // the trailer: checksum or ISIZE
      flip.append(f);
      CHECK(!decomp[t](flip, &back));
    }
  }
  for (CompressType type : {COMPRESS_TYPE_GZIP, COMPRESS_TYPE_ZLIB}) {
    snappy_message::SnappyMessageProto m, m2;
    m.set_text(pattern(12435));
    for (int i = 0; i < 3; ++i) m.add_numbers(i * 7);
    cord_buf b;
    CHECK(SerializeAsCompressedData(m, &b, type));
    CHECK(ParseFromCompressedData(b, &m2, type));
    CHECK(m2.text() == m.text() && m2.numbers_size() == 3);
  }
  {
    // "abc" as a stored block in a gzip member, byte by byte: header, 01 03 00
    // fc ff, the bytes, CRC-32 0x352441c2, ISIZE 3
    const unsigned char known[] = {0x1f, 0x8b, 0x08, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0x03, 0x01, 0x03,
                                   0x00, 0xfc, 0xff, 'a',  'b',  'c',  0xc2, 0x41, 0x24, 0x35, 0x03, 0x00,
                                   0x00, 0x00};
    cord_buf in, back, bad, back2;
    in.append(std::string(reinterpret_cast<const char*>(known), sizeof known));
    CHECK(policy::GzipDecompress(in, &back));
    CHECK(back.to_string() == "abc");
    std::string k(reinterpret_cast<const char*>(known), sizeof known);
    k[16] = 'x';  // the CRC no longer holds
    bad.append(k);
    CHECK(!policy::GzipDecompress(bad, &back2));
    cord_buf empty, back3;
    CHECK(!policy::GzipDecompress(empty, &back3) && !policy::ZlibDecompress(empty, &back3));
  }
  {
    std::ifstream fin(argv[1], std::ios::binary);
    const std::string body((std::istreambuf_iterator<char>(fin)), std::istreambuf_iterator<char>());
    cord_buf in, back, z;
    in.append(body);
    CHECK(policy::GzipDecompress(in, &back));
    std::ofstream(argv[2], std::ios::binary) << back.to_string();
    CHECK(policy::ZlibCompress(back, &z));
    std::ofstream(argv[3], std::ios::binary) << z.to_string();
  }
  printf("%d failures\n", g_failures);
  return g_failures ? 1 : 0;
}
