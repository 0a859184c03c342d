// bre_stream.hip — the beam radiance estimate's gather for scenes that stream their BVH from L2 / HBM; see bre.hip.h
#include "common.hip.h"
#include "bre.hip.h"

namespace rl {
void launch_bre_stream(bool hg, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const RenderConst& rc, const DeviceScene& ds, const StackConf& stc, const BreConst& bc) {
    launch_bre_impl<false>(hg, grid, block, lds_bytes, st, rc, ds, stc, bc);
}
}  // namespace rl
