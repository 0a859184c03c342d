// light_stream.hip — k_light_fused for scenes that stream their BVH from L2 / HBM; see light.hip.h
#include "common.hip.h"
#include "light.hip.h"

namespace rl {
void launch_light_stream(int mat, bool medium, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const RenderConst& rc, const DeviceScene& ds, const StackConf& stc, const LightConst& lc) {
    launch_light_impl<false>(mat, medium, grid, block, lds_bytes, st, rc, ds, stc, lc);
}
}  // namespace rl
