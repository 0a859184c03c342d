// pn_stream.hip — the point-normal single-scattering integrator for scenes whose BVH is streamed from L2 / HBM; see pn.hip.h
#include "common.hip.h"
#include "pn.hip.h"

namespace rl {
void launch_pn_stream(bool chain, int strategy, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const RenderConst& rc, const DeviceScene& ds, const StackConf& stc, const PnConst& pc) {
    launch_pn_impl<false>(chain, strategy, grid, block, lds_bytes, st, rc, ds, stc, pc);
}
}  // namespace rl
