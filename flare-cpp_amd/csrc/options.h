// options.h -- process-wide tuning and test options of libflare_snappy_gpu.so.
//
// Each option starts from its FSG_<NAME> environment variable, read ONCE when
// the library is loaded (A/B tooling sets them per process), and is changed
// afterwards only through fsg_set_option (include/flare_snappy_gpu.h).  The
// launch paths read the table's atomics, never the environment: getenv is not
// safe against a concurrent setenv in a multi-threaded server, and a variable
// must not silently change what a running process launches.
#pragma once
#include <cstdint>

namespace fsg {

enum Opt : int {
  // Snappy two-pass decode (snappy_decode_v4.hip, read_decode_opts; read once per call into DecodeOpts and range-checked in decode_v4_plan.h)
  kOptDecodeFork,         // -1 automatic (> 128K messages), 0 one stream, 1 forked path
  kOptSplitWalk,          // forked small-message execution order 0..3 (3 default)
  kOptSplitClass,         // walk class split point of mode 3
  kOptExecKeep,           // history kept at a window slide (bytes, 512..kMaxKeep, multiple of 16)
  kOptChunkedHuge,        // chunked pass 1b for the huge bodies of the forked path
  kOptSmallPersist,       // forked small-message grid (blocks; 0 = a wave per message)
  kOptSmallBatch,         // batches of at most this many messages index on pass 1b
  kOptSplitHuge,          // huge bodies on a second side stream
  kOptWalkOrder,          // planned lane walk in size-class order
  kOptLeanWalk,           // two-stream form: the lean lane walk
  kOptExecBigBlocks,      // one-stream exec launch: large-message blocks
  kOptExecPrio,           // exec pass priority raise around round-A loads
  kOptExecBigBlocksFork,  // forked path: large-message exec blocks
  kOptExecPack,           // forked path: short bodies per packed execution batch (0 = a wave per body)
  // Snappy encode (snappy_encode_v3.hip, read_encode_opts; read once per call into EncodeOpts and range-checked in encode_v3_plan.h)
  kOptEncodeWaveMin,      // long-unit threshold of the wave encoder (bytes; 0 = lanes only)
  kOptEncodeWaveShare,    // wave encoder's share of long units (permille)
  kOptEncodeWaveAllMb,    // all long units to the wave encoder below this many MiB
  kOptEncodeLanes,        // lanes in flight of the lane encoder (0 = all)
  kOptEncodeWavePerCu,    // wave encoder waves per CU (0 = as many as LDS holds)
  kOptEncodeWaveWg,       // wave encoder waves per workgroup (1..5; their tables share the workgroup's LDS)
  // LZ4 two-pass decode (lz4_decode2.hip)
  kOptLz4BigMin,          // -1 automatic; blocks above this many bytes take the wave walk
  // LZ4 compress (lz4_encode_wave.hip)
  kOptLz4EncodeWaveMin,   // -1 automatic; bodies of at least this many bytes take the wave encoder (>= 0xFFFFFFFF: none)
  kOptLz4EncodeWavePerCu, // wave encoder waves per CU (0 = as many as LDS holds)
  // LZ4 frames (lz4_frame_encode.hip, lz4_frame_decode.hip)
  kOptLz4fForceSerial,    // 1: every frame on the serial decoder
  kOptLz4fBlockWaveMin,   // the block encode's wave threshold (as lz4_encode_wave_min; -1: its automatic rule)
  kOptLz4fNosizeFast,     // 1: frames with independent blocks and no content size on the block decoders
  kOptLz4fLengthWaveMin,  // -1 automatic; blocks above this many bytes get their length by a wave (>= 0xFFFFFFFF: none)
  kOptLz4fLinkedFast,     // 1: frames with linked blocks on the block decoders, a wave per frame executing in order
  kOptCount
};

// Current value (relaxed load).
int64_t opt(Opt o);

}  // namespace fsg
