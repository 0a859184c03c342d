// pntaylor_stream.hip — the point-normal integrator's Taylor strategies for a BVH streamed from L2 / HBM; see pntaylor.hip.h
#include "common.hip.h"
#include "pntaylor.hip.h"

namespace rl {
void launch_pntaylor_stream(bool chain, int strategy, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const RenderConst& rc, const DeviceScene& ds, const StackConf& stc, const PnConst& pc) {
    launch_pntaylor_impl<false>(chain, strategy, grid, block, lds_bytes, st, rc, ds, stc, pc);
}
}  // namespace rl
