// capi.hip -- extern "C" boundary of libflare_snappy_gpu.so.
// Declarations and the reference interface each call replaces:
// include/flare_snappy_gpu.h.
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/flare_deflate_gpu.h"
#include "../../include/flare_deflate_index_gpu.h"
#include "../../include/flare_deflate_level_gpu.h"
#include "../../include/flare_lz4_gpu.h"
#include "../../include/flare_snappy_gpu.h"
#include "deflate_format.h"
#include "gzip_index.h"
#include "launch.h"
#include "launch_util.h"
#include "options.h"
#include "snappy_device.h"

namespace {
thread_local char g_err[256] = "";

int env_int(const char* name) {
  const char* e = getenv(name);
  return e ? atoi(e) : 0;
}

// ---- the option table (csrc/options.h): name, environment variable, default
struct OptDesc {
  const char* name;
  const char* env;
  int64_t dflt;
};
constexpr OptDesc kOptDesc[fsg::kOptCount] = {
    {"decode_fork", "FSG_DECODE_FORK", -1},
    {"split_walk", "FSG_SPLIT_WALK", 3},
    {"split_class", "FSG_SPLIT_CLASS", 4},
    {"exec_keep", "FSG_EXEC_KEEP", -1},
    {"chunked_huge", "FSG_CHUNKED_HUGE", 1},
    {"small_persist", "FSG_SMALL_PERSIST", 3584},
    {"small_batch", "FSG_SMALL_BATCH", 64},
    {"split_huge", "FSG_SPLIT_HUGE", 1},
    {"walk_order", "FSG_WALK_ORDER", 1},
    {"lean_walk", "FSG_LEAN_WALK", 1},
    {"exec_big_blocks", "FSG_EXEC_BIG_BLOCKS", 512},
    {"exec_prio", "FSG_EXEC_PRIO", 1},
    {"exec_big_blocks_fork", "FSG_EXEC_BIG_BLOCKS_FORK", 1024},
    {"exec_pack", "FSG_EXEC_PACK", 32},
    {"encode_wave_min", "FSG_ENCODE_WAVE_MIN", 16384},
    {"encode_wave_share", "FSG_ENCODE_WAVE_SHARE", 475},
    {"encode_wave_all_mb", "FSG_ENCODE_WAVE_ALL_MB", 640},
    {"encode_lanes", "FSG_ENCODE_LANES", 0},
    {"encode_wave_per_cu", "FSG_ENCODE_WAVE_PER_CU", 0},
    {"encode_wave_wg", "FSG_ENCODE_WAVE_WG", 1},
    {"lz4_big_min", "FSG_L4_BIG_MIN", -1},
    {"lz4_encode_wave_min", "FSG_L4_ENC_WAVE_MIN", -1},
    {"lz4_encode_wave_per_cu", "FSG_L4_ENC_WAVE_PER_CU", 0},
    {"lz4f_force_serial", "FSG_L4F_FORCE_SERIAL", 0},
    {"lz4f_block_wave_min", "FSG_L4F_BLOCK_WAVE_MIN", -1},
    {"lz4f_nosize_fast", "FSG_L4F_NOSIZE_FAST", 0},
    {"lz4f_length_wave_min", "FSG_L4F_LENGTH_WAVE_MIN", -1},
    {"lz4f_linked_fast", "FSG_L4F_LINKED_FAST", 0},
};
// DecodeOpts' initialisers (decode_v4_plan.h, which the CPU test of the launch
// plan uses as "the defaults") are this table's
constexpr bool decode_opts_defaults_ok() {
  constexpr fsg::DecodeOpts o;
  const int64_t v[] = {o.decode_fork, o.split_walk, o.split_class, o.exec_keep, o.chunked_huge,
                       o.small_persist, o.small_batch, o.split_huge, o.walk_order, o.lean_walk,
                       o.exec_big_blocks, o.exec_prio, o.exec_big_blocks_fork, o.exec_pack};
  for (int i = 0; i <= fsg::kOptExecPack; ++i)
    if (v[i] != kOptDesc[i].dflt) return false;
  return true;
}
static_assert(fsg::kOptExecPack == 13 && decode_opts_defaults_ok(), "DecodeOpts defaults differ from the option table");
// and EncodeOpts' (encode_v3_plan.h)
constexpr bool encode_opts_defaults_ok() {
  constexpr fsg::EncodeOpts o;
  const int64_t v[] = {o.encode_wave_min, o.encode_wave_share, o.encode_wave_all_mb,
                       o.encode_lanes, o.encode_wave_per_cu, o.encode_wave_wg};
  for (int i = fsg::kOptEncodeWaveMin; i <= fsg::kOptEncodeWaveWg; ++i)
    if (v[i - fsg::kOptEncodeWaveMin] != kOptDesc[i].dflt) return false;
  return true;
}
static_assert(fsg::kOptEncodeWaveMin == 14 && fsg::kOptEncodeWaveWg == 19 && encode_opts_defaults_ok(),
              "EncodeOpts defaults differ from the option table");
// and Lz4Opts' (lz4_plan.h)
constexpr bool lz4_opts_defaults_ok() {
  constexpr fsg::Lz4Opts o;
  const int64_t v[] = {o.lz4_big_min, o.lz4_encode_wave_min, o.lz4_encode_wave_per_cu, o.lz4f_force_serial,
                       o.lz4f_block_wave_min, o.lz4f_nosize_fast, o.lz4f_length_wave_min, o.lz4f_linked_fast};
  for (int i = fsg::kOptLz4BigMin; i <= fsg::kOptLz4fLinkedFast; ++i)
    if (v[i - fsg::kOptLz4BigMin] != kOptDesc[i].dflt) return false;
  return true;
}
static_assert(fsg::kOptLz4BigMin == 20 && fsg::kOptLz4fLinkedFast == 27 && lz4_opts_defaults_ok(),
              "Lz4Opts defaults differ from the option table");
static_assert(fsg::kEncRouteMain == FSG_PATH_MAIN && fsg::kEncRouteNoWorkspace == FSG_PATH_NO_WORKSPACE &&
                  fsg::kEncRouteForced == FSG_PATH_FORCED,
              "EncodeRoute differs from FSG_PATH_*");
std::atomic<int64_t> g_opt[fsg::kOptCount];
// the environment, once, when the library is loaded
[[maybe_unused]] const bool g_opt_init = [] {
  for (int i = 0; i < fsg::kOptCount; ++i) {
    const char* e = getenv(kOptDesc[i].env);
    g_opt[i].store(e && *e ? strtoll(e, nullptr, 10) : kOptDesc[i].dflt);
  }
  return true;
}();
// this call's LZ4 options
fsg::Lz4Opts read_lz4_opts() {
  fsg::Lz4Opts o;
  o.lz4_big_min = fsg::opt(fsg::kOptLz4BigMin);
  o.lz4_encode_wave_min = fsg::opt(fsg::kOptLz4EncodeWaveMin);
  o.lz4_encode_wave_per_cu = fsg::opt(fsg::kOptLz4EncodeWavePerCu);
  o.lz4f_force_serial = fsg::opt(fsg::kOptLz4fForceSerial);
  o.lz4f_block_wave_min = fsg::opt(fsg::kOptLz4fBlockWaveMin);
  o.lz4f_nosize_fast = fsg::opt(fsg::kOptLz4fNosizeFast);
  o.lz4f_length_wave_min = fsg::opt(fsg::kOptLz4fLengthWaveMin);
  o.lz4f_linked_fast = fsg::opt(fsg::kOptLz4fLinkedFast);
  return o;
}
int find_opt(const char* name) {
  if (!name) return -1;
  for (int i = 0; i < fsg::kOptCount; ++i)
    if (strcmp(name, kOptDesc[i].name) == 0) return i;
  return -1;
}
// Kernel variants (0 = automatic).  Initialised from FSG_DECODE_KERNEL /
// FSG_ENCODE_KERNEL, changeable with fsg_select_kernels for A/B runs.
std::atomic<int> g_decode_variant{env_int("FSG_DECODE_KERNEL")};
std::atomic<int> g_encode_variant{env_int("FSG_ENCODE_KERNEL")};
// Test knob: cap the staging region of a split message's fragments (bytes;
// 0 = slot / fragments).  Small caps force the whole-message fallback pass.
std::atomic<unsigned> g_region_cap{(unsigned)env_int("FSG_TEST_REGION_CAP")};

int record(hipError_t e, const char* where) {
  if (e == hipSuccess) return FSG_SUCCESS;
  snprintf(g_err, sizeof(g_err), "%s: %s", where, hipGetErrorString(e));
  return FSG_ERR_HIP;
}
}  // namespace

int64_t fsg::opt(fsg::Opt o) { return g_opt[o].load(std::memory_order_relaxed); }

extern "C" {

int fsg_set_option(const char* name, int64_t value) {
  const int i = find_opt(name);
  if (i < 0) return FSG_ERR_INVALID_ARG;
  g_opt[i].store(value, std::memory_order_relaxed);
  return FSG_SUCCESS;
}

int fsg_get_option(const char* name, int64_t* value) {
  const int i = find_opt(name);
  if (i < 0 || !value) return FSG_ERR_INVALID_ARG;
  *value = g_opt[i].load(std::memory_order_relaxed);
  return FSG_SUCCESS;
}

int fsg_default_option(const char* name, int64_t* value) {
  const int i = find_opt(name);
  if (i < 0 || !value) return FSG_ERR_INVALID_ARG;
  *value = kOptDesc[i].dflt;
  return FSG_SUCCESS;
}

const char* fsg_version(void) { return "flare-snappy-gpu 0.1 gfx950"; }

const char* fsg_last_error(void) { return g_err; }

int fsg_set_split_region_cap(uint32_t bytes) {
  g_region_cap.store(bytes);
  return FSG_SUCCESS;
}

int fsg_select_kernels(int decode_variant, int encode_variant) {
  // generation 2 (persistent-lane decode, literal lane encode) was retired:
  // superseded by 3/4 on every workload
  if (decode_variant < 0 || decode_variant > 5 || decode_variant == 2 || encode_variant < 0 ||
      encode_variant > 3 || encode_variant == 2)
    return FSG_ERR_INVALID_ARG;
  g_decode_variant.store(decode_variant);
  g_encode_variant.store(encode_variant);
  return FSG_SUCCESS;
}

int fsg_init(int device) {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n == 0) {
    snprintf(g_err, sizeof(g_err), "fsg_init: no HIP device (%s)",
             hipGetErrorString(e));
    return FSG_ERR_NO_DEVICE;
  }
  if (device < 0 || device >= n) return FSG_ERR_INVALID_ARG;
  return record(hipSetDevice(device), "hipSetDevice");
}

size_t fsg_max_compressed_length(size_t n) { return 32 + n + n / 6; }

int fsg_gather_blocks(const uint64_t* d_src, const uint32_t* d_len, const uint64_t* d_dst_off,
                      uint32_t n, uint8_t* d_dst, void* stream) {
  if (n && (!d_src || !d_len || !d_dst_off || !d_dst)) return FSG_ERR_INVALID_ARG;
  return record(fsg::launch_gather_blocks(d_src, d_len, d_dst_off, n, d_dst, (hipStream_t)stream),
                "fsg_gather_blocks");
}

size_t fsg_pack_workspace_bytes(uint32_t n_msgs) { return fsg::pack_workspace_bytes(n_msgs); }

int fsg_pack_batch(const uint8_t* d_src, const uint64_t* d_src_off, const uint32_t* d_len,
                   const int32_t* d_status, uint32_t n_msgs, uint32_t align, uint8_t* d_dst,
                   uint64_t* d_pack_off, uint64_t* d_total, void* d_workspace, size_t workspace_bytes,
                   void* stream) {
  if (align == 0 || align > 256 || (align & (align - 1)) || !d_total) return FSG_ERR_INVALID_ARG;
  // offsets and total only (d_dst NULL): the sources are not read
  if (n_msgs && (!d_len || !d_pack_off || !d_workspace || (d_dst && (!d_src || !d_src_off)) ||
                 workspace_bytes < fsg::pack_workspace_bytes(n_msgs)))
    return FSG_ERR_INVALID_ARG;
  return record(fsg::launch_pack(d_src, d_src_off, d_len, d_status, n_msgs, align, d_dst, d_pack_off, d_total,
                                 d_workspace, (hipStream_t)stream),
                "fsg_pack_batch");
}

int fsg_get_uncompressed_length(const void* compressed, size_t n,
                                uint32_t* ulen, int lenient) {
  const uint8_t* p = static_cast<const uint8_t*>(compressed);
  uint32_t r = 0;
  for (int i = 0; i < 5; ++i) {
    if ((size_t)i >= n) return 0;
    uint32_t c = p[i];
    r |= (c & 0x7fu) << (7 * i);
    if (c < 128) {
      if (!lenient && i == 4 && c >= 16) return 0;  // Parse32WithLimit
      *ulen = r;
      return i + 1;
    }
  }
  return 0;
}

int fsg_uncompressed_lengths_batch(const uint8_t* d_in, const uint64_t* d_in_off,
                                   const uint32_t* d_in_len, uint32_t n_msgs,
                                   uint32_t* d_ulen, int lenient, void* stream) {
  if (n_msgs && (!d_in || !d_in_off || !d_in_len || !d_ulen))
    return FSG_ERR_INVALID_ARG;
  return record(fsg::launch_headers(d_in, d_in_off, d_in_len, n_msgs, d_ulen,
                                    lenient, (hipStream_t)stream),
                "fsg_uncompressed_lengths_batch");
}

size_t fsg_compress_workspace_bytes(uint32_t n_msgs, uint32_t max_in_len) {
  // per-lane hash tables, then the fragment plan for messages > 64 KiB
  return fsg::encode_tables_workspace_bytes(n_msgs, max_in_len, nullptr) +
         fsg::encode_plan_bytes(n_msgs, max_in_len);
}
size_t fsg_decompress_workspace_bytes(uint32_t n_msgs, uint64_t total_in_bytes) {
  // total_in_bytes = 0: no size known, only the single-pass decoders run.
  return total_in_bytes ? fsg::decode_v4_workspace_bytes(n_msgs, total_in_bytes) : 256;
}

// ---- routing, shared by the batch calls and their path reports
namespace {
// fsg_compress_batch and fsg_compress_report: the call's plan (route, sizes,
// launches; encode_v3_plan.h) from the current options and kernel selection
fsg::EncodePlan encode_plan(uint32_t n_msgs, uint32_t max_in_len, size_t workspace_bytes, bool have_ws) {
  return fsg::encode_v3_plan(n_msgs, max_in_len, workspace_bytes, have_ws,
                             g_encode_variant.load(std::memory_order_relaxed),
                             g_region_cap.load(std::memory_order_relaxed), fsg::read_encode_opts());
}
// decompress_impl: FSG_PATH_MAIN = the two-pass decoder (v4)
int decode_path(bool have_ws, size_t workspace_bytes, uint32_t n_msgs, uint32_t flags) {
  const int forced = g_decode_variant.load(std::memory_order_relaxed);
  if (flags & FSG_FLAG_VALIDATE_ONLY) return FSG_PATH_SINGLE_DESIGN;
  if (forced == 1 || forced == 3) return FSG_PATH_FORCED;
  return have_ws && workspace_bytes >= fsg::decode_v4_workspace_bytes(n_msgs, 0) ? FSG_PATH_MAIN
                                                                                 : FSG_PATH_NO_WORKSPACE;
}
// The LZ4 calls and their reports: the call's plan (routes, sizes, launches;
// lz4_plan.h, lz4_frame_plan.h) from the current options.
// fsg_lz4_decompress_batch_ws: the two-pass decoder when p.two_pass and there
// is a workspace; fsg_lz4_compress_batch: p.route, p.wave_min
fsg::Lz4DecodePlan lz4_decode_plan(uint32_t n_msgs, size_t workspace_bytes) {
  return fsg::lz4_decode_plan(n_msgs, workspace_bytes, 0, read_lz4_opts());
}
fsg::Lz4EncodePlan lz4_encode_plan(uint32_t n_msgs, size_t workspace_bytes) {
  return fsg::lz4_encode_plan(n_msgs, workspace_bytes, read_lz4_opts());
}
// the reports state "none" as 0xFFFFFFFF
uint64_t report_wave_min(fsg::u64 wave_min) { return wave_min < 0xFFFFFFFFull ? wave_min : 0xFFFFFFFFull; }
}  // namespace

size_t fsg_report_header_bytes(void) { return 256; }

int fsg_decompress_report(const void* header_host_copy, uint32_t n_msgs, size_t workspace_bytes, uint32_t flags,
                          struct fsg_decode_report* out) {
  if (!out) return FSG_ERR_INVALID_ARG;
  *out = fsg_decode_report{};
  out->path = (uint64_t)decode_path(workspace_bytes != 0, workspace_bytes, n_msgs, flags);
  if (out->path != FSG_PATH_MAIN) {
    out->single_pass_messages = n_msgs;
    return FSG_SUCCESS;
  }
  out->bitmap_words_capacity = fsg::decode_v4_bitmap_capacity_words(n_msgs, workspace_bytes);
  if (n_msgs == 0) return FSG_SUCCESS;  // nothing was launched, the header not written
  if (!header_host_copy) return FSG_ERR_INVALID_ARG;
  fsg::DecodeHeaderCounts c;
  fsg::decode_v4_header_counts(header_host_copy, &c);
  out->fallback_messages = c.fallback;
  out->fallback_bitmap = c.fallback_bitmap;
  out->fallback_wide_offsets = c.fallback_wide;
  out->fallback_pack_guard = c.fallback_guard;
  out->bitmap_words_requested = c.bitmap_words;
  out->large_messages = c.large;
  out->huge_messages = c.huge;
  return FSG_SUCCESS;
}

int fsg_compress_report(const void* header_host_copy, uint32_t n_msgs, uint32_t max_in_len, size_t workspace_bytes,
                        struct fsg_encode_report* out) {
  if (!out) return FSG_ERR_INVALID_ARG;
  *out = fsg_encode_report{};
  const fsg::EncodePlan p = encode_plan(n_msgs, max_in_len, workspace_bytes, workspace_bytes != 0);
  out->path = (uint64_t)p.route;
  if (out->path != FSG_PATH_MAIN) {
    out->no_workspace_messages = n_msgs;
    return FSG_SUCCESS;
  }
  if (n_msgs == 0) return FSG_SUCCESS;
  if (!header_host_copy) return FSG_ERR_INVALID_ARG;
  fsg::EncodeHeaderCounts c;
  fsg::encode_v3_header_counts(header_host_copy, &c);
  out->units_listed = c.units;
  out->split_messages = c.split;
  out->unit_bytes = c.unit_bytes;
  out->fallback_messages = c.fallback;
  // the wave encoder's share: wave_quota, when the wave encoder ran
  if (p.wave_min) out->wave_units = fsg::wave_quota_of(c.units, c.unit_bytes, p.share_permille, p.all_bytes);
  return FSG_SUCCESS;
}

int fsg_lz4_decompress_report(const void* header_host_copy, uint32_t n_msgs, size_t workspace_bytes,
                              struct fsg_decode_report* out) {
  if (!out) return FSG_ERR_INVALID_ARG;
  *out = fsg_decode_report{};
  const fsg::Lz4DecodePlan p = lz4_decode_plan(n_msgs, workspace_bytes);
  if (workspace_bytes == 0 || !p.two_pass) {
    out->path = FSG_PATH_SINGLE_DESIGN;
    out->single_pass_messages = n_msgs;
    return FSG_SUCCESS;
  }
  out->bitmap_words_capacity = p.cap_words;
  if (n_msgs == 0) return FSG_SUCCESS;
  if (!header_host_copy) return FSG_ERR_INVALID_ARG;
  fsg::DecodeHeaderCounts c;
  fsg::lz4_decode_header_counts(header_host_copy, &c);
  out->fallback_messages = c.fallback;
  out->fallback_bitmap = c.fallback_bitmap;
  out->bitmap_words_requested = c.bitmap_words;
  out->large_messages = c.large;
  return FSG_SUCCESS;
}

int fsg_lz4_compress_report(const void* header_host_copy, uint32_t n_msgs, size_t workspace_bytes,
                            struct fsg_lz4_encode_report* out) {
  if (!out) return FSG_ERR_INVALID_ARG;
  *out = fsg_lz4_encode_report{};
  const fsg::Lz4EncodePlan p = lz4_encode_plan(n_msgs, workspace_bytes);
  out->path = (uint64_t)p.route;
  out->wave_min = report_wave_min(p.wave_min);
  out->lane_messages = n_msgs;
  if (out->path != 0 || n_msgs == 0) return FSG_SUCCESS;
  if (!header_host_copy) return FSG_ERR_INVALID_ARG;
  fsg::Lz4EncodeHeaderCounts c;
  fsg::lz4_encode_header_counts(header_host_copy, &c);
  out->wave_messages = c.wave_messages;
  out->wave_bytes = c.wave_bytes;
  out->lane_messages = n_msgs - c.wave_messages;
  return FSG_SUCCESS;
}

int fsg_compress_batch(const uint8_t* d_in, const uint64_t* d_in_off,
                       const uint32_t* d_in_len, uint32_t n_msgs,
                       uint32_t max_in_len, uint8_t* d_out,
                       const uint64_t* d_out_off, uint32_t* d_out_len,
                       int32_t* d_status, void* d_workspace,
                       size_t workspace_bytes, void* stream) {
  if (n_msgs && (!d_in || !d_in_off || !d_in_len || !d_out || !d_out_off ||
                 !d_out_len || !d_status))
    return FSG_ERR_INVALID_ARG;
  // The lane-per-message encoder with global-memory tables when the
  // workspace allows it (v3: batched speculative probes, the default);
  // otherwise the wave-per-message LDS-table encoder (v1).
  const fsg::EncodePlan p = encode_plan(n_msgs, max_in_len, workspace_bytes, d_workspace != nullptr);
  if (p.route == fsg::kEncRouteMain)
    return record(fsg::launch_encode_v3(d_in, d_in_off, d_in_len, n_msgs, d_out, d_out_off, d_out_len, d_status,
                                        d_workspace, (hipStream_t)stream, p),
                  "fsg_compress_batch");
  return record(fsg::launch_encode(d_in, d_in_off, d_in_len, n_msgs, max_in_len,
                                   d_out, d_out_off, d_out_len, d_status,
                                   (hipStream_t)stream),
                "fsg_compress_batch");
}

namespace {
int decompress_impl(const uint8_t* d_in, const uint64_t* d_in_off, const uint32_t* d_in_len,
                    uint32_t n_msgs, uint8_t* d_out, const uint64_t* d_out_off,
                    const uint32_t* d_out_cap, uint32_t* d_out_len, int32_t* d_status,
                    uint32_t flags, void* d_workspace, size_t workspace_bytes, void* stream,
                    void* pass1_stream);
}  // namespace

int fsg_decompress_batch(const uint8_t* d_in, const uint64_t* d_in_off,
                         const uint32_t* d_in_len, uint32_t n_msgs,
                         uint8_t* d_out, const uint64_t* d_out_off,
                         const uint32_t* d_out_cap, uint32_t* d_out_len,
                         int32_t* d_status, uint32_t flags, void* d_workspace,
                         size_t workspace_bytes, void* stream) {
  return decompress_impl(d_in, d_in_off, d_in_len, n_msgs, d_out, d_out_off, d_out_cap, d_out_len,
                         d_status, flags, d_workspace, workspace_bytes, stream, nullptr);
}

int fsg_decompress_batch_2s(const uint8_t* d_in, const uint64_t* d_in_off,
                            const uint32_t* d_in_len, uint32_t n_msgs,
                            uint8_t* d_out, const uint64_t* d_out_off,
                            const uint32_t* d_out_cap, uint32_t* d_out_len,
                            int32_t* d_status, uint32_t flags, void* d_workspace,
                            size_t workspace_bytes, void* stream, void* pass1_stream) {
  return decompress_impl(d_in, d_in_off, d_in_len, n_msgs, d_out, d_out_off, d_out_cap, d_out_len,
                         d_status, flags, d_workspace, workspace_bytes, stream, pass1_stream);
}

}  // extern "C"

namespace {
int decompress_impl(const uint8_t* d_in, const uint64_t* d_in_off, const uint32_t* d_in_len,
                    uint32_t n_msgs, uint8_t* d_out, const uint64_t* d_out_off,
                    const uint32_t* d_out_cap, uint32_t* d_out_len, int32_t* d_status,
                    uint32_t flags, void* d_workspace, size_t workspace_bytes, void* stream,
                    void* pass1_stream) {
  const bool validate = flags & FSG_FLAG_VALIDATE_ONLY;
  if (n_msgs && (!d_in || !d_in_off || !d_in_len || !d_out_len || !d_status ||
                 (!validate && (!d_out || !d_out_off || !d_out_cap))))
    return FSG_ERR_INVALID_ARG;
  // Kernel choice: the two-pass decoder (v4: lane-per-message index pass +
  // wave-per-message execution) when the workspace holds its tag bitmap;
  // otherwise the software-pipelined lane-per-message decoder (v3); v1 walks
  // tags without touching output for validate-only.  FSG_DECODE_KERNEL or
  // fsg_select_kernels force a variant (A/B runs).
  const int forced = g_decode_variant.load(std::memory_order_relaxed);
  // (decode_path: the same decision, which fsg_decompress_report repeats)
  const bool two_pass = decode_path(d_workspace != nullptr, workspace_bytes, n_msgs, flags) == FSG_PATH_MAIN;
  if (!two_pass && pass1_stream && pass1_stream != stream) {
    // single-pass kernels run on `stream` alone: order it after pass1_stream,
    // where the caller made the inputs ready
    const hipError_t e = fsg::order_after((hipStream_t)stream, (hipStream_t)pass1_stream);
    if (e != hipSuccess) return record(e, "fsg_decompress_batch_2s");
  }
  if (validate || forced == 1)
    return record(fsg::launch_decode(d_in, d_in_off, d_in_len, n_msgs, d_out, d_out_off,
                                     d_out_cap, d_out_len, d_status, flags,
                                     (hipStream_t)stream),
                  "fsg_decompress_batch");
  if (two_pass) {
    // (messages whose bitmap does not fit the workspace are finished by the
    // two-pass launches' serial fallback pass).  Execution pass: one tag per
    // lane (5, the default) or <= 16-byte pieces per lane (4).
    return record(fsg::launch_decode_v4(d_in, d_in_off, d_in_len, n_msgs, d_out, d_out_off,
                                        d_out_cap, d_out_len, d_status, flags, d_workspace,
                                        workspace_bytes, (hipStream_t)stream, forced == 4 ? 4 : 5,
                                        (hipStream_t)pass1_stream),
                  "fsg_decompress_batch");
  }
  return record(fsg::launch_decode_v3(d_in, d_in_off, d_in_len, n_msgs, d_out, d_out_off,
                                      d_out_cap, d_out_len, d_status, flags, (hipStream_t)stream),
                "fsg_decompress_batch");
}
}  // namespace

extern "C" {

int fsg_decompress_batch_partial(const uint8_t* d_in, const uint64_t* d_in_off, const uint32_t* d_in_len,
                                 uint32_t n_msgs, uint32_t frag, uint8_t* d_out, const uint64_t* d_out_off,
                                 const uint32_t* d_out_cap, uint32_t* d_got, uint64_t* d_produced,
                                 int32_t* d_status, void* d_workspace, size_t workspace_bytes, void* stream) {
  if (n_msgs && (!d_in || !d_in_off || !d_in_len || !d_out || !d_out_off || !d_out_cap || !d_got ||
                 !d_produced || !d_status))
    return FSG_ERR_INVALID_ARG;
  // the batch decoder (lenient header, as the Source path reads it), then the
  // streams it rejected through the scattered-writer model
  const int r = decompress_impl(d_in, d_in_off, d_in_len, n_msgs, d_out, d_out_off, d_out_cap, d_got, d_status,
                                0u, d_workspace, workspace_bytes, stream, nullptr);
  if (r != FSG_SUCCESS) return r;
  return record(fsg::launch_decode_partial(d_in, d_in_off, d_in_len, n_msgs, frag, d_out, d_out_off, d_out_cap,
                                           d_got, d_produced, d_status, (hipStream_t)stream),
                "fsg_decompress_batch_partial");
}

int fsg_decompress_batch_iovec(const uint8_t* d_in, const uint64_t* d_in_off, const uint32_t* d_in_len,
                               uint32_t n_msgs, const uint64_t* d_iov_base, const uint64_t* d_iov_len,
                               const uint32_t* d_iov_first, uint8_t* d_stage, const uint64_t* d_stage_off,
                               const uint32_t* d_stage_cap, uint32_t* d_out_len, int32_t* d_status,
                               void* d_workspace, size_t workspace_bytes, void* stream) {
  if (n_msgs && (!d_in || !d_in_off || !d_in_len || !d_iov_base || !d_iov_len || !d_iov_first || !d_stage ||
                 !d_stage_off || !d_stage_cap || !d_out_len || !d_status))
    return FSG_ERR_INVALID_ARG;
  const int r = decompress_impl(d_in, d_in_off, d_in_len, n_msgs, d_stage, d_stage_off, d_stage_cap, d_out_len,
                                d_status, 0u, d_workspace, workspace_bytes, stream, nullptr);
  if (r != FSG_SUCCESS) return r;
  return record(fsg::launch_iov_scatter(d_in, d_in_off, d_in_len, d_stage, d_stage_off, d_out_len, n_msgs,
                                        d_iov_base, d_iov_len, d_iov_first, d_status, (hipStream_t)stream),
                "fsg_decompress_batch_iovec");
}

// ---- LZ4 (include/flare_lz4_gpu.h)
size_t fsg_lz4_max_compressed_length(size_t n) { return 5 + n + n / 255 + 16; }

size_t fsg_lz4_compress_workspace_bytes(uint32_t n_msgs) { return fsg::lz4_compress_workspace_bytes(n_msgs); }

int fsg_lz4_compress_batch(const uint8_t* d_in, const uint64_t* d_in_off, const uint32_t* d_in_len,
                           uint32_t n_msgs, uint8_t* d_out, const uint64_t* d_out_off, uint32_t* d_out_len,
                           int32_t* d_status, void* d_workspace, size_t workspace_bytes, void* stream) {
  if (n_msgs && (!d_in || !d_in_off || !d_in_len || !d_out || !d_out_off || !d_out_len || !d_status ||
                 !d_workspace))
    return FSG_ERR_INVALID_ARG;
  const fsg::Lz4EncodePlan p = lz4_encode_plan(n_msgs, workspace_bytes);  // (the routing of fsg_lz4_compress_report)
  if (n_msgs && !p.valid) return FSG_ERR_INVALID_ARG;
  return record(fsg::launch_lz4_encode(d_in, d_in_off, d_in_len, n_msgs, d_out, d_out_off, d_out_len, d_status,
                                       d_workspace, (hipStream_t)stream, p),
                "fsg_lz4_compress_batch");
}

int fsg_lz4_decompress_batch(const uint8_t* d_in, const uint64_t* d_in_off, const uint32_t* d_in_len,
                             uint32_t n_msgs, uint8_t* d_out, const uint64_t* d_out_off,
                             const uint32_t* d_out_cap, uint32_t* d_out_len, int32_t* d_status, void* stream) {
  if (n_msgs && (!d_in || !d_in_off || !d_in_len || !d_out || !d_out_off || !d_out_cap || !d_out_len || !d_status))
    return FSG_ERR_INVALID_ARG;
  return record(fsg::launch_lz4_decode(d_in, d_in_off, d_in_len, n_msgs, d_out, d_out_off, d_out_cap, d_out_len,
                                       d_status, (hipStream_t)stream),
                "fsg_lz4_decompress_batch");
}

size_t fsg_lz4_decompress_workspace_bytes(uint32_t n_msgs, uint64_t total_in_bytes) {
  return fsg::lz4_decode_workspace_bytes(n_msgs, total_in_bytes);
}

int fsg_lz4_decompress_batch_ws(const uint8_t* d_in, const uint64_t* d_in_off, const uint32_t* d_in_len,
                                uint32_t n_msgs, uint8_t* d_out, const uint64_t* d_out_off,
                                const uint32_t* d_out_cap, uint32_t* d_out_len, int32_t* d_status,
                                void* d_workspace, size_t workspace_bytes, void* stream) {
  if (n_msgs && (!d_in || !d_in_off || !d_in_len || !d_out || !d_out_off || !d_out_cap || !d_out_len || !d_status))
    return FSG_ERR_INVALID_ARG;
  // no usable workspace: the one-pass lane kernel (same results)
  const fsg::Lz4DecodePlan p = lz4_decode_plan(n_msgs, workspace_bytes);
  if (!d_workspace || !p.two_pass)
    return fsg_lz4_decompress_batch(d_in, d_in_off, d_in_len, n_msgs, d_out, d_out_off, d_out_cap, d_out_len,
                                    d_status, stream);
  return record(fsg::launch_lz4_decode2(d_in, d_in_off, d_in_len, n_msgs, d_out, d_out_off, d_out_cap, d_out_len,
                                        d_status, d_workspace, (hipStream_t)stream, nullptr, p),
                "fsg_lz4_decompress_batch_ws");
}

int fsg_lz4_decompress_batch_2s(const uint8_t* d_in, const uint64_t* d_in_off, const uint32_t* d_in_len,
                                uint32_t n_msgs, uint8_t* d_out, const uint64_t* d_out_off,
                                const uint32_t* d_out_cap, uint32_t* d_out_len, int32_t* d_status,
                                void* d_workspace, size_t workspace_bytes, void* stream, void* pass1_stream) {
  if (n_msgs && (!d_in || !d_in_off || !d_in_len || !d_out || !d_out_off || !d_out_cap || !d_out_len || !d_status))
    return FSG_ERR_INVALID_ARG;
  const fsg::Lz4DecodePlan p = lz4_decode_plan(n_msgs, workspace_bytes);
  if (!d_workspace || !p.two_pass) {
    // the one-pass kernel on `stream`, ordered behind pass1_stream's work
    if (pass1_stream && pass1_stream != stream) {
      const hipError_t e = fsg::order_after((hipStream_t)stream, (hipStream_t)pass1_stream);
      if (e != hipSuccess) return record(e, "fsg_lz4_decompress_batch_2s");
    }
    return fsg_lz4_decompress_batch(d_in, d_in_off, d_in_len, n_msgs, d_out, d_out_off, d_out_cap, d_out_len,
                                    d_status, stream);
  }
  return record(fsg::launch_lz4_decode2(d_in, d_in_off, d_in_len, n_msgs, d_out, d_out_off, d_out_cap, d_out_len,
                                        d_status, d_workspace, (hipStream_t)stream, (hipStream_t)pass1_stream, p),
                "fsg_lz4_decompress_batch_2s");
}

// ---- LZ4 frames (include/flare_lz4_gpu.h, "LZ4 frames")
size_t fsg_lz4f_max_frame_length(size_t n, uint32_t block_size_id) {
  if (block_size_id < 4 || block_size_id > 7) return 0;
  const size_t bs = (size_t)1 << (8 + 2 * block_size_id);
  return 15 + 4 * ((n + bs - 1) / bs) + n + 4 + 4;
}

size_t fsg_lz4f_max_frame_length_flags(size_t n, uint32_t block_size_id, uint32_t flags) {
  if (block_size_id < 4 || block_size_id > 7 || flags > 7) return 0;
  const size_t bs = (size_t)1 << (8 + 2 * block_size_id);
  return fsg_lz4f_max_frame_length(n, block_size_id) + ((flags & FSG_LZ4F_FLAG_BLOCK_CHECKSUMS) ? 4 * ((n + bs - 1) / bs) : 0);
}

int fsg_lz4f_xxh32_batch(const uint8_t* d_in, const uint64_t* d_in_off, const uint32_t* d_in_len, uint32_t n_msgs,
                         uint32_t seed, uint32_t* d_xxh, void* stream) {
  if (n_msgs == 0) return FSG_SUCCESS;
  if (!d_in || !d_in_off || !d_in_len || !d_xxh) return FSG_ERR_INVALID_ARG;
  return record(fsg::launch_lz4f_xxh32(d_in, d_in_off, d_in_len, n_msgs, seed, d_xxh, (hipStream_t)stream),
                "fsg_lz4f_xxh32_batch");
}

size_t fsg_lz4f_compress_workspace_bytes(uint32_t n_msgs, uint64_t total_in_bytes, uint32_t block_size_id) {
  if (block_size_id < 4 || block_size_id > 7) return 0;
  return fsg::lz4f_compress_workspace_bytes(n_msgs, total_in_bytes, block_size_id);
}

int fsg_lz4f_compress_batch_flags(const uint8_t* d_in, const uint64_t* d_in_off, const uint32_t* d_in_len,
                                  uint32_t n_msgs, uint8_t* d_out, const uint64_t* d_out_off, uint32_t* d_out_len,
                                  int32_t* d_status, uint32_t block_size_id, uint32_t flags, void* d_workspace,
                                  size_t workspace_bytes, void* stream) {
  const uint32_t known = FSG_LZ4F_FLAG_CONTENT_CHECKSUM | FSG_LZ4F_FLAG_BLOCK_CHECKSUMS | FSG_LZ4F_FLAG_NO_CONTENT_SIZE;
  if (block_size_id < 4 || block_size_id > 7 || (flags & ~known)) return FSG_ERR_INVALID_ARG;
  if (n_msgs == 0) return FSG_SUCCESS;
  if (!d_in || !d_in_off || !d_in_len || !d_out || !d_out_off || !d_out_len || !d_status || !d_workspace)
    return FSG_ERR_INVALID_ARG;
  const fsg::Lz4fEncodePlan p = fsg::lz4f_encode_plan(n_msgs, workspace_bytes, block_size_id, read_lz4_opts());
  if (!p.valid) return FSG_ERR_INVALID_ARG;
  return record(fsg::launch_lz4f_encode(d_in, d_in_off, d_in_len, n_msgs, d_out, d_out_off, d_out_len, d_status,
                                        block_size_id, flags, d_workspace, (hipStream_t)stream, p),
                "fsg_lz4f_compress_batch");
}

// the call from before the flags word had bits 1 and 2: it keeps rejecting them
int fsg_lz4f_compress_batch(const uint8_t* d_in, const uint64_t* d_in_off, const uint32_t* d_in_len,
                            uint32_t n_msgs, uint8_t* d_out, const uint64_t* d_out_off, uint32_t* d_out_len,
                            int32_t* d_status, uint32_t block_size_id, uint32_t flags, void* d_workspace,
                            size_t workspace_bytes, void* stream) {
  if (flags & ~FSG_LZ4F_FLAG_CONTENT_CHECKSUM) return FSG_ERR_INVALID_ARG;
  return fsg_lz4f_compress_batch_flags(d_in, d_in_off, d_in_len, n_msgs, d_out, d_out_off, d_out_len, d_status,
                                       block_size_id, flags, d_workspace, workspace_bytes, stream);
}

size_t fsg_lz4f_decompress_workspace_bytes(uint32_t n_msgs, uint64_t total_in_bytes) {
  return fsg::lz4f_decompress_workspace_bytes(n_msgs, total_in_bytes);
}

int fsg_lz4f_decompress_batch(const uint8_t* d_in, const uint64_t* d_in_off, const uint32_t* d_in_len,
                              uint32_t n_msgs, uint8_t* d_out, const uint64_t* d_out_off,
                              const uint32_t* d_out_cap, uint32_t* d_out_len, int32_t* d_status,
                              void* d_workspace, size_t workspace_bytes, void* stream) {
  if (n_msgs == 0) return FSG_SUCCESS;
  if (!d_in || !d_in_off || !d_in_len || !d_out || !d_out_off || !d_out_cap || !d_out_len || !d_status ||
      !d_workspace)
    return FSG_ERR_INVALID_ARG;
  const fsg::Lz4fDecodePlan p = fsg::lz4f_decode_plan(n_msgs, workspace_bytes, read_lz4_opts());
  if (!p.valid) return FSG_ERR_INVALID_ARG;
  return record(fsg::launch_lz4f_decode(d_in, d_in_off, d_in_len, n_msgs, d_out, d_out_off, d_out_cap, d_out_len,
                                        d_status, d_workspace, (hipStream_t)stream, p),
                "fsg_lz4f_decompress_batch");
}

int fsg_lz4f_decoded_lengths_batch(const uint8_t* d_in, const uint64_t* d_in_off, const uint32_t* d_in_len,
                                   uint32_t n_msgs, uint64_t* d_length, int32_t* d_status, void* d_workspace,
                                   size_t workspace_bytes, void* stream) {
  if (n_msgs == 0) return FSG_SUCCESS;
  if (!d_in || !d_in_off || !d_in_len || !d_length || !d_status || !d_workspace) return FSG_ERR_INVALID_ARG;
  const fsg::Lz4fDecodePlan p = fsg::lz4f_decode_plan(n_msgs, workspace_bytes, read_lz4_opts());
  if (!p.valid) return FSG_ERR_INVALID_ARG;
  return record(fsg::launch_lz4f_decoded_lengths(d_in, d_in_off, d_in_len, n_msgs, d_length, d_status, d_workspace,
                                                 (hipStream_t)stream, p),
                "fsg_lz4f_decoded_lengths_batch");
}

int fsg_lz4f_content_sizes_batch(const uint8_t* d_in, const uint64_t* d_in_off, const uint32_t* d_in_len,
                                 uint32_t n_msgs, uint64_t* d_content_size, int32_t* d_status, void* stream) {
  if (n_msgs && (!d_in || !d_in_off || !d_in_len || !d_content_size || !d_status)) return FSG_ERR_INVALID_ARG;
  return record(fsg::launch_lz4f_content_sizes(d_in, d_in_off, d_in_len, n_msgs, d_content_size, d_status,
                                               (hipStream_t)stream),
                "fsg_lz4f_content_sizes_batch");
}

// ---- inflate (include/flare_deflate_gpu.h)
int fsg_inflate_batch(const uint8_t* d_in, const uint64_t* d_in_off, const uint32_t* d_in_len, uint32_t n_msgs,
                      uint8_t* d_out, const uint64_t* d_out_off, const uint32_t* d_out_cap, uint32_t* d_out_len,
                      int32_t* d_status, uint32_t format, void* stream) {
  if (format > FSG_INFLATE_GZIP) return FSG_ERR_INVALID_ARG;
  if (n_msgs == 0) return FSG_SUCCESS;
  if (!d_in || !d_in_off || !d_in_len || !d_out || !d_out_off || !d_out_cap || !d_out_len || !d_status)
    return FSG_ERR_INVALID_ARG;
  return record(fsg::launch_inflate(d_in, d_in_off, d_in_len, n_msgs, d_out, d_out_off, d_out_cap, d_out_len,
                                    d_status, format, (hipStream_t)stream),
                "fsg_inflate_batch");
}

int fsg_inflate_lengths_batch(const uint8_t* d_in, const uint64_t* d_in_off, const uint32_t* d_in_len,
                              uint32_t n_msgs, uint64_t* d_length, int32_t* d_status, uint32_t format,
                              void* stream) {
  if (format > FSG_INFLATE_GZIP) return FSG_ERR_INVALID_ARG;
  if (n_msgs == 0) return FSG_SUCCESS;
  if (!d_in || !d_in_off || !d_in_len || !d_length || !d_status) return FSG_ERR_INVALID_ARG;
  return record(fsg::launch_inflate_lengths(d_in, d_in_off, d_in_len, n_msgs, d_length, d_status, format,
                                            (hipStream_t)stream),
                "fsg_inflate_lengths_batch");
}

int fsg_crc32_batch(const uint8_t* d_in, const uint64_t* d_in_off, const uint32_t* d_in_len, uint32_t n_msgs,
                    uint32_t* d_crc, void* stream) {
  if (n_msgs == 0) return FSG_SUCCESS;
  if (!d_in || !d_in_off || !d_in_len || !d_crc) return FSG_ERR_INVALID_ARG;
  return record(fsg::launch_inflate_sum(d_in, d_in_off, d_in_len, n_msgs, d_crc, false, (hipStream_t)stream),
                "fsg_crc32_batch");
}

int fsg_adler32_batch(const uint8_t* d_in, const uint64_t* d_in_off, const uint32_t* d_in_len, uint32_t n_msgs,
                      uint32_t* d_adler, void* stream) {
  if (n_msgs == 0) return FSG_SUCCESS;
  if (!d_in || !d_in_off || !d_in_len || !d_adler) return FSG_ERR_INVALID_ARG;
  return record(fsg::launch_inflate_sum(d_in, d_in_off, d_in_len, n_msgs, d_adler, true, (hipStream_t)stream),
                "fsg_adler32_batch");
}

// ---- deflate compress (include/flare_deflate_compress_gpu.h)
size_t fsg_deflate_max_length(size_t n, uint32_t format) { return (size_t)defl::max_length(n, format); }

size_t fsg_deflate_workspace_bytes(uint32_t n_msgs, uint64_t total_in_bytes) {
  return fsg::deflate_workspace_bytes(n_msgs, total_in_bytes);
}

int fsg_deflate_batch(const uint8_t* d_in, const uint64_t* d_in_off, const uint32_t* d_in_len, uint32_t n_msgs,
                      uint8_t* d_out, const uint64_t* d_out_off, uint32_t* d_out_len, int32_t* d_status,
                      uint32_t format, void* d_workspace, size_t workspace_bytes, void* stream) {
  return fsg_deflate_batch_level(d_in, d_in_off, d_in_len, n_msgs, d_out, d_out_off, d_out_len, d_status, format,
                                 FSG_DEFLATE_LEVEL_FAST, d_workspace, workspace_bytes, stream);
}

// (include/flare_deflate_level_gpu.h)
int fsg_deflate_batch_level(const uint8_t* d_in, const uint64_t* d_in_off, const uint32_t* d_in_len, uint32_t n_msgs,
                            uint8_t* d_out, const uint64_t* d_out_off, uint32_t* d_out_len, int32_t* d_status,
                            uint32_t format, uint32_t level, void* d_workspace, size_t workspace_bytes,
                            void* stream) {
  return fsg_deflate_batch_flags(d_in, d_in_off, d_in_len, n_msgs, d_out, d_out_off, d_out_len, d_status, format,
                                 level, 0, d_workspace, workspace_bytes, stream);
}

// ---- the unit index (include/flare_deflate_index_gpu.h)
static bool deflate_flags_ok(uint32_t format, uint32_t flags) {
  return !(flags & ~FSG_DEFLATE_FLAG_UNIT_INDEX) && (flags == 0 || format == FSG_DEFLATE_GZIP);
}

size_t fsg_deflate_max_length_flags(size_t n, uint32_t format, uint32_t flags) {
  if (format > FSG_DEFLATE_GZIP || !deflate_flags_ok(format, flags)) return 0;
  const uint64_t units = defl::unit_count(n);
  return (size_t)(defl::max_length(n, format) +
                  (gzidx::writes_index(format, flags, units) ? gzidx::head_bytes((uint32_t)units) - 10 : 0));
}

int fsg_deflate_batch_flags(const uint8_t* d_in, const uint64_t* d_in_off, const uint32_t* d_in_len, uint32_t n_msgs,
                            uint8_t* d_out, const uint64_t* d_out_off, uint32_t* d_out_len, int32_t* d_status,
                            uint32_t format, uint32_t level, uint32_t flags, void* d_workspace,
                            size_t workspace_bytes, void* stream) {
  if (level > FSG_DEFLATE_LEVEL_BEST) return FSG_ERR_INVALID_ARG;
  if (format > FSG_DEFLATE_GZIP) return FSG_ERR_INVALID_ARG;
  if (!deflate_flags_ok(format, flags)) return FSG_ERR_INVALID_ARG;
  if (n_msgs == 0) return FSG_SUCCESS;
  if (!d_in || !d_in_off || !d_in_len || !d_out || !d_out_off || !d_out_len || !d_status || !d_workspace)
    return FSG_ERR_INVALID_ARG;
  if (reinterpret_cast<uintptr_t>(d_workspace) & 15u) return FSG_ERR_INVALID_ARG;
  if (fsg::deflate_unit_capacity(n_msgs, workspace_bytes) == 0) return FSG_ERR_INVALID_ARG;
  return record(fsg::launch_deflate(d_in, d_in_off, d_in_len, n_msgs, d_out, d_out_off, d_out_len, d_status, format,
                                    level, flags, d_workspace, workspace_bytes, (hipStream_t)stream),
                "fsg_deflate_batch");
}

size_t fsg_inflate_units_workspace_bytes(uint32_t n_msgs, uint64_t extra_units) {
  return fsg::inflate_units_workspace_bytes(n_msgs, extra_units);
}

static bool inflate_units_ws_ok(uint32_t n_msgs, const void* d_workspace, size_t workspace_bytes) {
  return d_workspace && !(reinterpret_cast<uintptr_t>(d_workspace) & 15u) &&
         fsg::inflate_units_entry_capacity(n_msgs, workspace_bytes) != 0;
}

int fsg_inflate_units_batch(const uint8_t* d_in, const uint64_t* d_in_off, const uint32_t* d_in_len, uint32_t n_msgs,
                            uint8_t* d_out, const uint64_t* d_out_off, const uint32_t* d_out_cap,
                            uint32_t* d_out_len, int32_t* d_status, uint32_t format, void* d_workspace,
                            size_t workspace_bytes, void* stream) {
  if (format > FSG_INFLATE_GZIP) return FSG_ERR_INVALID_ARG;
  if (n_msgs == 0) return FSG_SUCCESS;
  if (!d_in || !d_in_off || !d_in_len || !d_out || !d_out_off || !d_out_cap || !d_out_len || !d_status)
    return FSG_ERR_INVALID_ARG;
  if (!inflate_units_ws_ok(n_msgs, d_workspace, workspace_bytes)) return FSG_ERR_INVALID_ARG;
  return record(fsg::launch_inflate_units(d_in, d_in_off, d_in_len, n_msgs, d_out, d_out_off, d_out_cap, d_out_len,
                                          d_status, format, d_workspace, workspace_bytes, (hipStream_t)stream),
                "fsg_inflate_units_batch");
}

int fsg_inflate_units_lengths_batch(const uint8_t* d_in, const uint64_t* d_in_off, const uint32_t* d_in_len,
                                    uint32_t n_msgs, uint64_t* d_length, int32_t* d_status, uint32_t format,
                                    void* d_workspace, size_t workspace_bytes, void* stream) {
  if (format > FSG_INFLATE_GZIP) return FSG_ERR_INVALID_ARG;
  if (n_msgs == 0) return FSG_SUCCESS;
  if (!d_in || !d_in_off || !d_in_len || !d_length || !d_status) return FSG_ERR_INVALID_ARG;
  if (!inflate_units_ws_ok(n_msgs, d_workspace, workspace_bytes)) return FSG_ERR_INVALID_ARG;
  return record(fsg::launch_inflate_units_lengths(d_in, d_in_off, d_in_len, n_msgs, d_length, d_status, format,
                                                  d_workspace, workspace_bytes, (hipStream_t)stream),
                "fsg_inflate_units_lengths_batch");
}

int fsg_inflate_units_report(const void* header_host_copy, uint32_t n_msgs, size_t workspace_bytes,
                             struct fsg_inflate_units_report* out) {
  if (!header_host_copy || !out) return FSG_ERR_INVALID_ARG;
  const uint64_t cap = fsg::inflate_units_entry_capacity(n_msgs, workspace_bytes);
  if (n_msgs && cap == 0) return FSG_ERR_INVALID_ARG;
  fsg::InflateUnitsHeaderCounts c;
  fsg::inflate_units_header_counts(header_host_copy, &c);
  out->parallel_messages = c.parallel_bodies;
  out->parallel_units = c.parallel_units;
  out->serial_no_index = c.no_index;
  out->serial_unusable_index = c.unusable;
  out->serial_unit_mismatch = c.mismatch;
  out->serial_workspace = c.overflow;
  out->unit_entries = cap;
  return FSG_SUCCESS;
}

int fsg_deflate_report(const void* header_host_copy, uint32_t n_msgs, size_t workspace_bytes,
                       struct fsg_deflate_report* out) {
  if (!header_host_copy || !out) return FSG_ERR_INVALID_ARG;
  const uint64_t cap = fsg::deflate_unit_capacity(n_msgs, workspace_bytes);
  if (n_msgs && cap == 0) return FSG_ERR_INVALID_ARG;
  fsg::DeflateHeaderCounts c;
  fsg::deflate_header_counts(header_host_copy, &c);
  out->units = c.units;
  out->stored_units = c.stored;
  out->fixed_units = c.fixed;
  out->dynamic_units = c.dynamic;
  out->overflow_messages = c.overflow;
  out->unit_entries = cap;
  return FSG_SUCCESS;
}

int fsg_lz4f_compress_report(const void* header_host_copy, uint32_t n_msgs, size_t workspace_bytes,
                             uint32_t block_size_id, struct fsg_lz4f_encode_report* out) {
  if (!out || block_size_id < 4 || block_size_id > 7) return FSG_ERR_INVALID_ARG;
  *out = fsg_lz4f_encode_report{};
  if (n_msgs == 0) return FSG_SUCCESS;
  const fsg::Lz4fEncodePlan p = fsg::lz4f_encode_plan(n_msgs, workspace_bytes, block_size_id, read_lz4_opts());
  out->block_entries = p.valid ? p.w.nb_cap : 0;
  if (!p.valid || !header_host_copy) return FSG_ERR_INVALID_ARG;
  out->block_wave_min = report_wave_min(p.inner.wave_min);
  fsg::Lz4fEncodeHeaderCounts c;
  fsg::lz4f_encode_header_counts(header_host_copy, &c);
  out->blocks = c.blocks;
  out->raw_blocks = c.raw_blocks;
  out->overflow_messages = c.overflow_messages;
  return FSG_SUCCESS;
}

int fsg_lz4f_decompress_report(const void* header_host_copy, uint32_t n_msgs, size_t workspace_bytes,
                               struct fsg_lz4f_decode_report* out) {
  if (!out) return FSG_ERR_INVALID_ARG;
  *out = fsg_lz4f_decode_report{};
  if (n_msgs == 0) return FSG_SUCCESS;
  const fsg::Lz4fDecodePlan p = fsg::lz4f_decode_plan(n_msgs, workspace_bytes, read_lz4_opts());
  out->block_entries = p.valid ? p.w.nb_cap : 0;
  if (!p.valid || !header_host_copy) return FSG_ERR_INVALID_ARG;
  fsg::Lz4fDecodeHeaderCounts c;
  fsg::lz4f_decode_header_counts(header_host_copy, &c);
  out->fast_messages = c.fast_messages;
  out->fast_blocks = c.fast_blocks;
  out->empty_messages = c.empty_messages;
  out->serial_linked = c.serial_linked;
  out->serial_no_size = c.serial_no_size;
  out->serial_rejected = c.serial_rejected;
  out->serial_forced = c.serial_forced;
  out->checksummed_units = c.checksummed_units;
  out->inner_fallback_blocks = c.inner_fallback;
  out->fast_nosize_messages = c.fast_nosize_messages;
  out->fast_nosize_blocks = c.fast_nosize_blocks;
  out->fast_linked_messages = c.fast_linked_messages;
  out->fast_linked_blocks = c.fast_linked_blocks;
  return FSG_SUCCESS;
}

}  // extern "C"
