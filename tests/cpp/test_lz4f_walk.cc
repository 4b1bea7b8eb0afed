// test_lz4f_walk.cc -- the walk over an LZ4 frame's size words
// (csrc/lz4_frame_format.h: next_block, end_frame, check_blocks,
// blocks_decoded_length) as a stand-alone program, built with
// -fsanitize=address,undefined by tests/test_lz4f_walk.py.  It includes that
// header alone; every frame sits in a heap buffer of exactly its length, so a
// read past the input is a report.  (The staging sum is the device caller's
// own: no shared code computes it, so it is not reported.)
//
//   test_lz4f_walk <in> <out>
//   in:  records of u32 length, the frame's bytes
//   out: a line per frame, "bad_header" or five fields separated by " | ":
//        serial   -- the cursor alone, as decode_frame walks it
//        lengths  -- check_blocks, an empty raw block accepted
//        unsized  -- check_blocks, no block of size 0
//        sized    -- check_blocks by the sized fast route's rules ("-": no content size)
//        length   -- blocks_decoded_length ("-": the frame states its size)
//        a rule set's field: "reject", "miscounted" (the count or the unchecked
//        second walk differs), or "accept <blocks> <stated xxh> <at>:<size>:<raw> ..."
//        the length field:   "reject", or "accept <decoded length>"
#include <cstdint>
#include <cstdio>
#include <vector>

#include "lz4_frame_format.h"

namespace {

void print_blocks(FILE* fo, bool ok, uint32_t nb, uint32_t xxh, const std::vector<lz4f::Block>& blocks) {
  if (!ok || nb != blocks.size()) {
    fputs(ok ? "miscounted" : "reject", fo);
    return;
  }
  fprintf(fo, "accept %u %u", nb, xxh);
  for (const lz4f::Block& b : blocks) fprintf(fo, " %llu:%u:%d", (unsigned long long)b.at, b.size, b.raw ? 1 : 0);
}

void by_rules(FILE* fo, const uint8_t* f, uint64_t n, const lz4f::Header& h, lz4f::BlockRules rules) {
  std::vector<lz4f::Block> blocks;
  uint32_t nb = 0, xxh = 0;
  const bool ok = lz4f::check_blocks(f, n, h, rules, [&](const lz4f::Block& b) { blocks.push_back(b); }, &nb, &xxh);
  // the listing pass of the device: the accepted frame again with nothing tested,
  // one word beyond the last block (the end mark) decoded and dropped
  lz4f::BlockWalk w = lz4f::begin_blocks(f, n, h);
  lz4f::Block u;
  bool same = true;
  for (uint32_t k = 0; ok && k <= nb; ++k) {
    lz4f::next_block<false>(&w, &u);
    if (k < nb && (u.at != blocks[k].at || u.size != blocks[k].size || u.raw != blocks[k].raw)) same = false;
  }
  print_blocks(fo, ok, same ? nb : ~0u, xxh, blocks);
}

void serial(FILE* fo, const uint8_t* f, uint64_t n, const lz4f::Header& h) {
  std::vector<lz4f::Block> blocks;
  lz4f::BlockWalk w = lz4f::begin_blocks(f, n, h);
  lz4f::Block b;
  lz4f::WalkStep s;
  uint32_t xxh = 0;
  while ((s = lz4f::next_block(&w, &b)) == lz4f::kWalkBlock) blocks.push_back(b);
  const bool ok = s == lz4f::kWalkEnd && lz4f::end_frame(&w, &xxh);
  print_blocks(fo, ok, (uint32_t)blocks.size(), xxh, blocks);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* fi = fopen(argv[1], "rb");
  FILE* fo = fopen(argv[2], "w");
  if (!fi || !fo) return 2;
  uint32_t n;
  while (fread(&n, 4, 1, fi) == 1) {
    uint8_t* f = new uint8_t[n];
    if (n && fread(f, 1, n, fi) != n) return 2;
    lz4f::Header h;
    if (lz4f::parse_header(f, n, &h) != lz4f::kStOk) {
      fprintf(fo, "bad_header\n");
      delete[] f;
      continue;
    }
    const bool sized = h.size != lz4f::kNoSize;
    serial(fo, f, n, h);
    fprintf(fo, " | ");
    by_rules(fo, f, n, h, lz4f::BlockRules{true, false});
    fprintf(fo, " | ");
    by_rules(fo, f, n, h, lz4f::BlockRules{false, false});
    fprintf(fo, " | ");
    if (sized) by_rules(fo, f, n, h, lz4f::BlockRules{false, true});
    else fprintf(fo, "-");
    uint64_t total = 0;
    if (sized) fprintf(fo, " | -\n");
    else if (lz4f::blocks_decoded_length(f, n, h, &total)) fprintf(fo, " | accept %llu\n", (unsigned long long)total);
    else fprintf(fo, " | reject\n");
    delete[] f;
  }
  fclose(fi);
  return fclose(fo) == 0 ? 0 : 2;
}
