// uplane_lds.hip — the uncorrelated photon planes for scenes staged in LDS; see uplane.hip.h
#include "common.hip.h"
#include "uplane.hip.h"

namespace rl {
void launch_uplane_lds(int mode, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const RenderConst& rc, const DeviceScene& ds, const StackConf& stc, const UPlaneConst& uc) {
    launch_uplane_impl<true>(mode, grid, block, lds_bytes, st, rc, ds, stc, uc);
}
}  // namespace rl
