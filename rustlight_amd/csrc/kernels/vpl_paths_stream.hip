// vpl_paths_stream.hip — k_vpl_shoot for scenes that stream their BVH; see vpl_paths.hip.h
#include "common.hip.h"
#include "vpl_paths.hip.h"

namespace rl {
void launch_vpl_paths_stream(bool write, int mat, bool medium, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const RenderConst& rc, const DeviceScene& ds, const StackConf& stc, const VplPathsConst& pc) {
    launch_vpl_paths_impl<false>(write, mat, medium, grid, block, lds_bytes, st, rc, ds, stc, pc);
}
}  // namespace rl
