// test_pack_output.cc -- the handler's packed compress path: compressed
// outputs are packed on the device (fsg_pack_batch) before the D2H copy, so
// the copy and the pinned slab carry compressed bytes, not worst-case slots.
//   ./test_pack_output --cpu   the 8-value fsh_stats and the threshold's environment parsing
//   ./test_pack_output --gpu   the packed path against the host codec (MI355X);
//                              run with FLARE_SNAPPY_GPU_PACK_MIN_BYTES=0 (every
//                              chunk packs) or a huge value (none does)
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../../include/flare_snappy_host.h"
#include "cord_buf.h"
#include "gpu_codec.h"
#include "snappy_compress.h"

extern "C" void dg_text_body(uint64_t index, uint8_t* out, size_t n);

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

std::string text_body(uint64_t index, size_t n) {
  std::string s(n, '\0');
  dg_text_body(index, reinterpret_cast<uint8_t*>(&s[0]), n);
  return s;
}

std::string host_compress(const std::string& s) {
  std::string o(fsh_max_compressed_length(s.size()), '\0');
  o.resize(fsh_cpu_compress(reinterpret_cast<const uint8_t*>(s.data()), s.size(), reinterpret_cast<uint8_t*>(&o[0])));
  return o;
}

size_t round16(size_t x) { return (x + 15) & ~size_t(15); }

void cpu_cases() {
  // fsh_stats: 8 values, and only as many as the caller asks for
  uint64_t v[10];
  for (auto& x : v) x = 0xABABABABABABABABull;
  fsh_stats(v, 10);
  for (int i = 0; i < 8; ++i) CHECK(v[i] != 0xABABABABABABABABull);
  CHECK(v[8] == 0xABABABABABABABABull && v[9] == 0xABABABABABABABABull);
  CHECK(v[6] == 0 && v[7] == 0);  // nothing has run
  for (auto& x : v) x = 0xABABABABABABABABull;
  fsh_stats(v, 6);
  CHECK(v[5] != 0xABABABABABABABABull && v[6] == 0xABABABABABABABABull && v[7] == 0xABABABABABABABABull);
  // FLARE_SNAPPY_GPU_PACK_MIN_BYTES
  unsetenv("FLARE_SNAPPY_GPU_PACK_MIN_BYTES");
  CHECK(flare::gpu::PackMinBytesFromEnv() == flare::gpu::kPackMinBytesDefault);
  CHECK((flare::gpu::kPackMinBytesDefault & (flare::gpu::kPackMinBytesDefault - 1)) == 0);  // a power of two
  setenv("FLARE_SNAPPY_GPU_PACK_MIN_BYTES", "0", 1);
  CHECK(flare::gpu::PackMinBytesFromEnv() == 0);
  setenv("FLARE_SNAPPY_GPU_PACK_MIN_BYTES", "123456", 1);
  CHECK(flare::gpu::PackMinBytesFromEnv() == 123456);
  setenv("FLARE_SNAPPY_GPU_PACK_MIN_BYTES", "18446744073709551615", 1);
  CHECK(flare::gpu::PackMinBytesFromEnv() == ~size_t(0));
  setenv("FLARE_SNAPPY_GPU_PACK_MIN_BYTES", "", 1);
  CHECK(flare::gpu::PackMinBytesFromEnv() == flare::gpu::kPackMinBytesDefault);
  setenv("FLARE_SNAPPY_GPU_PACK_MIN_BYTES", "lots", 1);
  CHECK(flare::gpu::PackMinBytesFromEnv() == flare::gpu::kPackMinBytesDefault);
  unsetenv("FLARE_SNAPPY_GPU_PACK_MIN_BYTES");
}

// 64 text bodies of 64 KiB and 200 of 1..5,000 bytes, compressed by
// concurrent callers of the handler so that they coalesce into device batches.
void gpu_cases() {
  const bool expect_packed = flare::gpu::PackMinBytesFromEnv() == 0;
  fsh_set_gpu_min_bytes(0);
  if (fsh_init_devices(0) < 1) {
    fprintf(stderr, "GPU codec unavailable\n");
    ++g_failures;
    return;
  }
  std::vector<std::string> bodies;
  for (int i = 0; i < 64; ++i) bodies.push_back(text_body(1000 + i, 65536));
  for (int i = 0; i < 200; ++i) bodies.push_back(text_body(5000 + i, 1 + (size_t)(i * 4999 / 199)));
  const size_t n = bodies.size();
  std::vector<std::string> expect(n);
  size_t packed_bound = 0, slot_sum = 0;
  for (size_t i = 0; i < n; ++i) {
    expect[i] = host_compress(bodies[i]);
    packed_bound += round16(expect[i].size());
    slot_sum += round16(fsh_max_compressed_length(bodies[i].size()));
  }
  uint64_t s0[8], s1[8];
  fsh_stats(s0, 8);
  std::vector<cord_buf> outs(n);
  std::atomic<int> bad{0};
  {
    std::vector<std::thread> th;
    const int kThreads = 12;
    for (int t = 0; t < kThreads; ++t)
      th.emplace_back([&, t] {
        for (size_t i = t; i < n; i += kThreads) {
          cord_buf in;
          in.append(bodies[i]);
          if (!policy::SnappyCompress(in, &outs[i])) bad++;
        }
      });
    for (auto& x : th) x.join();
  }
  fsh_stats(s1, 8);
  CHECK(bad.load() == 0);
  for (size_t i = 0; i < n; ++i) CHECK(outs[i].to_string() == expect[i]);  // the host codec's bytes
  CHECK(s1[1] - s0[1] == n);                                              // all on the device
  const uint64_t batches = s1[0] - s0[0], chunks = s1[7] - s0[7], moved = s1[6] - s0[6];
  printf("  %zu bodies in %llu batches, %llu packed chunks, D2H %llu bytes (packed bound %zu, slots %zu)\n", n,
         (unsigned long long)batches, (unsigned long long)chunks, (unsigned long long)moved, packed_bound, slot_sum);
  CHECK(s1[5] > s0[5]);  // outputs of 2 KiB or more are still adopted
  if (expect_packed) {
    CHECK(chunks >= 1 && chunks >= batches);  // every chunk packed
    CHECK(moved <= packed_bound + 16 * chunks);
    CHECK(moved < slot_sum);
  } else {
    CHECK(chunks == 0);
    CHECK(moved == slot_sum);
  }
  // an adopted output (the 64 KiB bodies compress to well over 2 KiB) decodes back
  for (size_t i : {size_t(0), size_t(63), n - 1}) {
    cord_buf back;
    CHECK(policy::SnappyDecompress(outs[i], &back));
    CHECK(back.equals(bodies[i]));
  }
  // a device error still sends the batch to the host codec, same bytes
  uint64_t e0[8], e1[8];
  fsh_stats(e0, 8);
  flare::gpu::InjectDeviceErrorsForTesting(1);
  cord_buf in, out;
  in.append(bodies[0]);
  CHECK(policy::SnappyCompress(in, &out));
  fsh_stats(e1, 8);
  CHECK(e1[3] - e0[3] == 1);
  CHECK(e1[7] == e0[7] && e1[6] == e0[6]);
  CHECK(out.to_string() == expect[0]);
  // one explicit batch (one device batch): same bytes, one more run of the path
  std::vector<cord_buf> ins(n), outs2(n);
  std::vector<const cord_buf*> pi;
  std::vector<cord_buf*> po;
  for (size_t i = 0; i < n; ++i) {
    ins[i].append(bodies[i]);
    pi.push_back(&ins[i]);
    po.push_back(&outs2[i]);
  }
  std::vector<bool> ok;
  fsh_stats(e0, 8);
  CHECK(flare::gpu::SnappyGpuCodec::Instance().CompressBatch(pi, po, &ok));
  fsh_stats(e1, 8);
  for (size_t i = 0; i < n; ++i) CHECK(outs2[i].to_string() == expect[i]);
  if (expect_packed) {
    CHECK(e1[7] > e0[7]);
    CHECK(e1[6] - e0[6] <= packed_bound + 16 * (e1[7] - e0[7]));
  } else {
    CHECK(e1[7] == e0[7]);
    CHECK(e1[6] - e0[6] == slot_sum);
  }
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
