// test_path_report.cc -- the host runtime's device-path counters
// (fsh_device_path_stats): after every batch call the runtime downloads the
// workspace's 256-byte counter header and sums the path reports
// (include/flare_snappy_gpu.h).
//   ./test_path_report --cpu   the counters' C ABI before anything ran
//   ./test_path_report --gpu   a batch on the fast path leaves them alone, a
//                              batch forced into the encoder's whole-message
//                              fallback raises them (MI355X)
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/flare_snappy_gpu.h"
#include "../../include/flare_snappy_host.h"
#include "cord_buf.h"
#include "gpu_codec.h"
#include "snappy_compress.h"

extern "C" void dg_text_body(uint64_t index, uint8_t* out, size_t n);
extern "C" void dg_random_body(uint64_t index, uint8_t* out, size_t n);

using flare::cord_buf;
using namespace flare::rpc;

namespace {
int g_failures = 0;
#define CHECK(c)                                                          \
  do {                                                                    \
    if (!(c)) {                                                           \
      fprintf(stderr, "  %s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); \
      ++g_failures;                                                       \
    }                                                                     \
  } while (0)

constexpr uint64_t kUnset = 0xABABABABABABABABull;

std::string body(bool random, uint64_t index, size_t n) {
  std::string s(n, '\0');
  (random ? dg_random_body : dg_text_body)(index, reinterpret_cast<uint8_t*>(&s[0]), n);
  return s;
}

std::string host_compress(const std::string& s) {
  std::string o(fsh_max_compressed_length(s.size()), '\0');
  o.resize(fsh_cpu_compress(reinterpret_cast<const uint8_t*>(s.data()), s.size(), reinterpret_cast<uint8_t*>(&o[0])));
  return o;
}

void cpu_cases() {
  // min(n, 3) values, all 0 before anything ran
  for (size_t n = 0; n <= 5; ++n) {
    uint64_t v[5];
    for (auto& x : v) x = kUnset;
    fsh_device_path_stats(v, n);
    for (size_t i = 0; i < 5; ++i) CHECK(v[i] == (i < n && i < 3 ? 0 : kUnset));
  }
  // fsh_stats keeps its 8 values
  uint64_t v[10];
  for (auto& x : v) x = kUnset;
  fsh_stats(v, 10);
  for (int i = 0; i < 8; ++i) CHECK(v[i] != kUnset);
  CHECK(v[8] == kUnset && v[9] == kUnset);
  CHECK(fsg_report_header_bytes() == 256);
}

// One explicit compress batch of `bodies`; checks the bytes against the host codec's.
void compress_batch(const std::vector<std::string>& bodies, std::vector<cord_buf>* outs) {
  const size_t n = bodies.size();
  std::vector<cord_buf> ins(n);
  outs->assign(n, cord_buf());
  std::vector<const cord_buf*> pi;
  std::vector<cord_buf*> po;
  for (size_t i = 0; i < n; ++i) {
    ins[i].append(bodies[i]);
    pi.push_back(&ins[i]);
    po.push_back(&(*outs)[i]);
  }
  std::vector<bool> ok;
  CHECK(flare::gpu::SnappyGpuCodec::Instance().CompressBatch(pi, po, &ok));
  for (size_t i = 0; i < n; ++i) CHECK((*outs)[i].to_string() == host_compress(bodies[i]));
}

void gpu_cases() {
  fsh_set_gpu_min_bytes(0);
  if (fsh_init_devices(0) < 1) {
    fprintf(stderr, "GPU codec unavailable\n");
    ++g_failures;
    return;
  }
  uint64_t p0[3], p1[3], s0[8], s1[8];
  // ---- the fast path: 64 text bodies of 64 KiB, compressed and decompressed
  std::vector<std::string> text;
  for (int i = 0; i < 64; ++i) text.push_back(body(false, 2000 + i, 65536));
  fsh_device_path_stats(p0, 3);
  fsh_stats(s0, 8);
  std::vector<cord_buf> comp;
  compress_batch(text, &comp);
  {
    std::vector<cord_buf> back(text.size());
    std::vector<const cord_buf*> pi;
    std::vector<cord_buf*> po;
    for (size_t i = 0; i < text.size(); ++i) {
      pi.push_back(&comp[i]);
      po.push_back(&back[i]);
    }
    std::vector<bool> ok;
    CHECK(flare::gpu::SnappyGpuCodec::Instance().UncompressBatch(pi, po, &ok));
    for (size_t i = 0; i < text.size(); ++i) CHECK(ok[i] && back[i].equals(text[i]));
  }
  fsh_device_path_stats(p1, 3);
  fsh_stats(s1, 8);
  CHECK(s1[1] - s0[1] == 2 * text.size());  // all of it on the device
  for (int i = 0; i < 3; ++i) CHECK(p1[i] == p0[i]);
  // ---- the encoder's whole-message fallback: staging regions capped below
  // what a fragment of a random body needs
  std::vector<std::string> rnd;
  for (int i = 0; i < 3; ++i) rnd.push_back(body(true, 3000 + i, 200000));
  CHECK(fsg_set_split_region_cap(4096) == FSG_SUCCESS);
  std::vector<cord_buf> out;
  compress_batch(rnd, &out);
  CHECK(fsg_set_split_region_cap(0) == FSG_SUCCESS);
  fsh_device_path_stats(p0, 3);
  printf("  fallback messages +%llu, single-pass +%llu, fallback batches +%llu\n",
         (unsigned long long)(p0[0] - p1[0]), (unsigned long long)(p0[1] - p1[1]),
         (unsigned long long)(p0[2] - p1[2]));
  CHECK(p0[0] - p1[0] == 3);
  CHECK(p0[1] == p1[1]);
  CHECK(p0[2] - p1[2] >= 1);
  fsh_shutdown();
}
}  // namespace

int main(int argc, char** argv) {
  bool gpu = false;
  for (int i = 1; i < argc; ++i) gpu = gpu || !strcmp(argv[i], "--gpu");
  if (gpu) {
    GlobalInitializeSnappyGpu();
    gpu_cases();
  } else {
    cpu_cases();
  }
  printf("%d failures\n", g_failures);
  return g_failures ? 1 : 0;
}
