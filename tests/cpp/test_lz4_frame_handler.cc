// test_lz4_frame_handler.cc -- the LZ4 frame CompressHandler
// (host/lz4_compress.h: policy::Lz4FrameCompress / Lz4FrameDecompress,
// GlobalInitializeLz4Frame) on the host alone; run by tests/test_lz4f.py,
// which compares what it prints and writes with the frame oracle.
//   test_lz4_frame_handler FRAME_IN RAW_OUT
// registers the handler at COMPRESS_TYPE_LZ4, prints "frame <hex>" for the
// reference tests' 200-byte text loop, round-trips bodies and a message
// through the registry, rejects broken frames, and decompresses the frame in
// FRAME_IN (any frame liblz4 writes) into RAW_OUT.
#include <cstdio>
#include <fstream>
#include <iterator>
#include <string>

#include "compress.h"
#include "cord_buf.h"
#include "lz4_compress.h"
#include "lz4_cpu.h"
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

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  CHECK(GlobalInitializeLz4Frame() == 0);
  CHECK(std::string(CompressTypeToCStr(COMPRESS_TYPE_LZ4)) == "lz4f");
  CHECK(GlobalInitializeLz4() != 0);  // the type is taken: one of the two handlers
  {
    cord_buf in, out, back;
    in.append(pattern(200));
    CHECK(policy::Lz4FrameCompress(in, &out));
    printf("frame ");
    for (unsigned char c : out.to_string()) printf("%02x", c);
    printf("\n");
    CHECK(policy::Lz4FrameDecompress(out, &back));
    CHECK(back.to_string() == pattern(200));
  }
  for (int n : {0, 1, 65536, 65537, 300000}) {
    cord_buf in, out, back;
    in.append(pattern(n));
    CHECK(policy::Lz4FrameCompress(in, &out));
    CHECK(policy::Lz4FrameDecompress(out, &back));
    CHECK(back.to_string() == pattern(n));
    std::string f = out.to_string();
    cord_buf cut, more, flip;
    cut.append(f.substr(0, f.size() - 1));
    CHECK(!policy::Lz4FrameDecompress(cut, &back));
    more.append(f + "x");
    CHECK(!policy::Lz4FrameDecompress(more, &back));
    f[0] ^= 1;
    flip.append(f);
    CHECK(!policy::Lz4FrameDecompress(flip, &back));
  }
  {
    snappy_message::SnappyMessageProto m, m2;
    m.set_text(pattern(12435));
    for (int i = 0; i < 3; ++i) m.add_numbers(i * 7);
    cord_buf b;
    CHECK(SerializeAsCompressedData(m, &b, COMPRESS_TYPE_LZ4));
    CHECK(ParseFromCompressedData(b, &m2, COMPRESS_TYPE_LZ4));
    CHECK(m2.text() == m.text() && m2.numbers_size() == 3);
  }
  {
    // a 15-byte descriptor that claims 2^40 bytes: refused by the length
    // bound before anything is allocated for it
    cord_buf in, out, back;
    in.append(pattern(200));
    CHECK(policy::Lz4FrameCompress(in, &out));
    std::string f = out.to_string();
    f[11] = 1;  // content size + 2^40, HC made right again
    f[14] = (char)(flare::lz4::cpu::Xxh32(reinterpret_cast<const uint8_t*>(f.data()) + 4, 10) >> 8);
    cord_buf huge;
    huge.append(f);
    CHECK(!policy::Lz4FrameDecompress(huge, &back));
  }
  {
    std::ifstream fin(argv[1], std::ios::binary);
    const std::string frame((std::istreambuf_iterator<char>(fin)), std::istreambuf_iterator<char>());
    cord_buf in, back;
    in.append(frame);
    CHECK(policy::Lz4FrameDecompress(in, &back));
    std::ofstream(argv[2], std::ios::binary) << back.to_string();
  }
  printf("%d failures\n", g_failures);
  return g_failures ? 1 : 0;
}
