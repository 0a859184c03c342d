// vpl_stream.hip — the VPL kernels for scenes that stream their BVH from L2 / HBM; see vpl.hip.h
#include "common.hip.h"
#include "vpl.hip.h"

namespace rl {
void launch_vpl_stream(int which, int mat, bool medium, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const RenderConst& rc, const DeviceScene& ds, const StackConf& stc, const VplConst& vc) {
    launch_vpl_impl<false>(which, mat, medium, grid, block, lds_bytes, st, rc, ds, stc, vc);
}
}  // namespace rl
