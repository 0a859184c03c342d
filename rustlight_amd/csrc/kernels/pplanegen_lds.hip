// pplanegen_lds.hip — the photon planes' generation kernels (k_pplane_generate, k_pplane_shoot) for scenes staged in LDS; see pplanegen.hip.h
#include "common.hip.h"
#include "pplanegen.hip.h"

namespace rl {
void launch_pplanegen_lds(int which, int mat, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const RenderConst& rc, const DeviceScene& ds, const StackConf& stc,
                         const VplConst& vc, const VplPathsConst& pc, const PPlaneGenConst& xc) {
    launch_pplanegen_impl<true>(which, mat, grid, block, lds_bytes, st, rc, ds, stc, vc, pc, xc);
}
}  // namespace rl
