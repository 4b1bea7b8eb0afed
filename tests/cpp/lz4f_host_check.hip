// lz4f_host_check.hip -- TEST HELPER: runs the serial LZ4 frame decoder of the
// GPU kernels (flare-cpp_amd/csrc/lz4_frame_format.h, __host__ __device__) on
// the CPU, built with AddressSanitizer and UBSan by tests/test_lz4f.py, so an
// out-of-bounds access shows up without a GPU.  The output buffer has exactly
// `cap` bytes.  No HIP calls.
//   lz4f_host_check IN OUT : IN = records [u32 cap][u32 n][frame]
//                            OUT = [i32 status][u32 out_len][out_len bytes if status 0]
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../flare-cpp_amd/csrc/lz4_frame_format.h"

static bool rd(FILE* f, void* p, size_t n) { return fread(p, 1, n, f) == n; }

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) return 2;
  for (;;) {
    uint32_t cap, n;
    if (!rd(in, &cap, 4)) break;
    if (!rd(in, &n, 4)) return 3;
    // exact-size heap blocks: one byte past either is a sanitizer report
    uint8_t* src = static_cast<uint8_t*>(malloc(n ? n : 1));
    uint8_t* dst = static_cast<uint8_t*>(malloc(cap ? cap : 1));
    if (n && !rd(in, src, n)) return 3;
    uint32_t len = 0;
    const int32_t st = lz4f::decode_frame(n ? src : nullptr, n, cap ? dst : nullptr, cap, &len);
    fwrite(&st, 4, 1, out);
    fwrite(&len, 4, 1, out);
    if (st == 0) fwrite(dst, 1, len, out);
    free(src);
    free(dst);
  }
  fclose(out);
  return 0;
}
