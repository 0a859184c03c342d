// fused_strat_stream.hip — k_path_fused_strat for scenes that stream their BVH from L2 / HBM; see fused_strat.hip.h
#include "common.hip.h"
#include "fused_strat.hip.h"

namespace rl {
void launch_fused_strat_stream(bool medium, bool area_only, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const RenderConst& rc, const DeviceScene& ds, const StackConf& stc) {
    launch_fused_strat_impl<false>(medium, area_only, grid, block, lds_bytes, st, rc, ds, stc);
}
}  // namespace rl
