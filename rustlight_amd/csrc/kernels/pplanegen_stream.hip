// pplanegen_stream.hip — the photon planes' generation kernels (k_pplane_generate, k_pplane_shoot) for scenes that stream their BVH; see pplanegen.hip.h
#include "common.hip.h"
#include "pplanegen.hip.h"

namespace rl {
void launch_pplanegen_stream(int which, int mat, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const RenderConst& rc, const DeviceScene& ds, const StackConf& stc,
                         const VplConst& vc, const VplPathsConst& pc, const PPlaneGenConst& xc) {
    launch_pplanegen_impl<false>(which, mat, grid, block, lds_bytes, st, rc, ds, stc, vc, pc, xc);
}
}  // namespace rl
