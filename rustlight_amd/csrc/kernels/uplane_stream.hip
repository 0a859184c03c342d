// uplane_stream.hip — the uncorrelated photon planes with the BVH streamed from L2 / HBM; see uplane.hip.h
#include "common.hip.h"
#include "uplane.hip.h"

namespace rl {
void launch_uplane_stream(int mode, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const RenderConst& rc, const DeviceScene& ds, const StackConf& stc, const UPlaneConst& uc) {
    launch_uplane_impl<false>(mode, grid, block, lds_bytes, st, rc, ds, stc, uc);
}
}  // namespace rl
