// pack_latency.cc -- where packing the compress outputs on the device starts
// to pay: p50 latency of SnappyGpuCodec::CompressBatch for small batches of
// text bodies with the packed path forced on (FLARE_SNAPPY_GPU_PACK_MIN_BYTES
// = 0), forced off (a huge value) and at the built-in default.  The packed
// path trades a second stream synchronisation and two more launches for a
// D2H of compressed bytes instead of worst-case slots; the default threshold
// (kPackMinBytesDefault, host/gpu_codec.h) is read off this table.
//   ./build/pack_latency [calls] [size]      (defaults 200 65536)
// The device runtime is restarted for every row, so each reads its own
// threshold.  Prints one JSON line per (batch, mode).
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "cord_buf.h"
#include "gpu_codec.h"

extern "C" void dg_text_body(uint64_t index, uint8_t* out, size_t n);

using flare::cord_buf;

int main(int argc, char** argv) {
  const int calls = argc > 1 ? atoi(argv[1]) : 200;
  const size_t size = argc > 2 ? strtoull(argv[2], nullptr, 10) : 65536;
  auto& codec = flare::gpu::SnappyGpuCodec::Instance();
  codec.SetMinGpuBytes(0);
  struct Mode {
    const char* name;
    const char* env;  // nullptr: unset (the default)
  };
  const Mode modes[] = {{"off", "18446744073709551615"}, {"on", "0"}, {"default", nullptr}};
  using clk = std::chrono::steady_clock;
  for (size_t batch : {size_t(1), size_t(4), size_t(16), size_t(64), size_t(256)}) {
    std::vector<cord_buf> raw(batch);
    std::string body(size, '\0');
    for (size_t i = 0; i < batch; ++i) {
      dg_text_body(0x7E47ull * 1000003ull + i, reinterpret_cast<uint8_t*>(&body[0]), size);
      raw[i].append(body);
    }
    std::vector<const cord_buf*> in(batch);
    for (size_t i = 0; i < batch; ++i) in[i] = &raw[i];
    for (const Mode& m : modes) {
      if (m.env) setenv("FLARE_SNAPPY_GPU_PACK_MIN_BYTES", m.env, 1);
      else unsetenv("FLARE_SNAPPY_GPU_PACK_MIN_BYTES");
      if (codec.InitDevices(0) < 1) {
        fprintf(stderr, "GPU codec unavailable: %s\n", codec.error().c_str());
        return 1;
      }
      const auto s0 = codec.stats();
      std::vector<double> us;
      size_t out_bytes = 0;
      for (int c = -20; c < calls; ++c) {  // 20 warm-up calls
        std::vector<cord_buf> comp(batch);
        std::vector<cord_buf*> co(batch);
        for (size_t i = 0; i < batch; ++i) co[i] = &comp[i];
        std::vector<bool> ok;
        const auto t0 = clk::now();
        codec.CompressBatch(in, co, &ok);
        const auto t1 = clk::now();
        if (c >= 0) us.push_back(std::chrono::duration<double, std::micro>(t1 - t0).count());
        out_bytes = 0;
        for (auto& x : comp) out_bytes += x.size();
      }
      const auto s1 = codec.stats();
      std::sort(us.begin(), us.end());
      size_t slot_bytes = 0;
      for (size_t i = 0; i < batch; ++i) slot_bytes += (32 + size + size / 6 + 15) & ~size_t(15);
      printf("{\"batch\": %zu, \"size\": %zu, \"mode\": \"%s\", \"slot_bytes\": %zu, \"out_bytes\": %zu, "
             "\"p50_us\": %.1f, \"p10_us\": %.1f, \"p90_us\": %.1f, \"d2h_bytes_per_call\": %llu, "
             "\"packed_chunks\": %llu}\n",
             batch, size, m.name, slot_bytes, out_bytes, us[us.size() / 2], us[us.size() / 10],
             us[us.size() * 9 / 10], (unsigned long long)((s1.d2h_bytes - s0.d2h_bytes) / (calls + 20)),
             (unsigned long long)(s1.packed_chunks - s0.packed_chunks));
      fflush(stdout);
    }
  }
  codec.Shutdown();
  return 0;
}
