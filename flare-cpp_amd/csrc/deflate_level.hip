// deflate_level.hip -- the unit kernel of the batched deflate compress at
// levels 0 (stored units only) and 2 (two candidates per hash slot, one lazy
// step inside the window): fsg_deflate_batch_level
// (include/flare_deflate_level_gpu.h).  The kernel is deflate_unit.h's, which
// says why these two instantiations have a file of their own; plan, checksum
// and assemble launches are deflate.hip's, shared by all levels.
#include "deflate_unit.h"

namespace fsg {

hipError_t launch_deflate_units_level(u32 level, u32 waves, const u8* in, const u64* in_off, u32* hdr, u32* units,
                                      u32* tokens, u8* stage, hipStream_t stream) {
  if (level == defl::kLevelStored)
    deflate_unit_kernel<defl::kLevelStored><<<waves, 64, 0, stream>>>(in, in_off, hdr, units, tokens, stage);
  else if (level == defl::kLevelBest)
    deflate_unit_kernel<defl::kLevelBest><<<waves, 64, 0, stream>>>(in, in_off, hdr, units, tokens, stage);
  else
    return hipErrorInvalidValue;
  return hipGetLastError();
}

}  // namespace fsg
