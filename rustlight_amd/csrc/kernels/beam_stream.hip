// beam_stream.hip — the photon beams' gather (k_beam_gather) for scenes whose BVH is streamed from L2 / HBM; see beam.hip.h
#include "common.hip.h"
#include "beam.hip.h"

namespace rl {
void launch_beam_stream(dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const RenderConst& rc, const DeviceScene& ds, const StackConf& stc, const BeamConst& bc) {
    hipLaunchKernelGGL((k_beam_gather<false>), grid, block, lds_bytes, st, rc, ds, stc, bc);
}
}  // namespace rl
