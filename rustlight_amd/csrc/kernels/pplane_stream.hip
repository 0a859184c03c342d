// pplane_stream.hip — the photon planes' gather (k_pplane_gather) for scenes that stream their BVH; see pplane.hip.h
#include "common.hip.h"
#include "pplane.hip.h"

namespace rl {
void launch_pplane_stream(dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const RenderConst& rc, const DeviceScene& ds, const StackConf& stc, const PPlaneConst& pc) {
    hipLaunchKernelGGL((k_pplane_gather<false>), grid, block, lds_bytes, st, rc, ds, stc, pc);
}
}  // namespace rl
