// lz4f_length_check.cc -- flare::lz4::cpu::FrameDecodedLength (host/lz4_cpu.cc)
// as a stand-alone program, built with -fsanitize=address,undefined by
// tests/test_lz4f_nosize.py: every frame sits in a heap buffer of exactly its
// length, so a read past the input is a report.
//
//   lz4f_length_check <in> <out>
//   in:  records of u32 length, the frame's bytes
//   out: records of i32 status, u64 length
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "lz4_cpu.h"

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* fi = fopen(argv[1], "rb");
  FILE* fo = fopen(argv[2], "wb");
  if (!fi || !fo) return 2;
  uint32_t n;
  while (fread(&n, 4, 1, fi) == 1) {
    uint8_t* frame = new uint8_t[n];
    if (n && fread(frame, 1, n, fi) != n) return 2;
    int32_t st = -9;
    const uint64_t len = flare::lz4::cpu::FrameDecodedLength(frame, n, &st);
    fwrite(&st, 4, 1, fo);
    fwrite(&len, 8, 1, fo);
    delete[] frame;
  }
  fclose(fi);
  return fclose(fo) == 0 ? 0 : 2;
}
