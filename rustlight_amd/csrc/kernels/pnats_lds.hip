// pnats_lds.hip — the point-normal integrator over the light tree for scenes staged in LDS; see pnats.hip.h
#include "common.hip.h"
#include "pnats.hip.h"

namespace rl {
void launch_pnats_lds(bool chain, int selector, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const RenderConst& rc, const DeviceScene& ds, const StackConf& stc, const PnConst& pc) {
    launch_pnats_impl<true>(chain, selector, grid, block, lds_bytes, st, rc, ds, stc, pc);
}
}  // namespace rl
