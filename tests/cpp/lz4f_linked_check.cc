// lz4f_linked_check.cc -- lz4f::linked_prefix (csrc/lz4_frame_format.h), the
// history a linked block can reach, as a stand-alone program built with
// -fsanitize=address,undefined by tests/test_lz4f_linked.py.
//
//   lz4f_linked_check <in> <out>
//   in:  u64 values: the bytes a frame produced before a block
//   out: u32 values: the block's prefix
#include <cstdint>
#include <cstdio>

#include "lz4_frame_format.h"

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* fi = fopen(argv[1], "rb");
  FILE* fo = fopen(argv[2], "wb");
  if (!fi || !fo) return 2;
  uint64_t produced;
  while (fread(&produced, 8, 1, fi) == 1) {
    const uint32_t p = lz4f::linked_prefix(produced);
    fwrite(&p, 4, 1, fo);
  }
  fclose(fi);
  return fclose(fo) == 0 ? 0 : 2;
}
