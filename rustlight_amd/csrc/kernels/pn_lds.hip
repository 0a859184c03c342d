// pn_lds.hip — the point-normal single-scattering integrator for scenes staged in LDS; see pn.hip.h
#include "common.hip.h"
#include "pn.hip.h"

namespace rl {
void launch_pn_lds(bool chain, int strategy, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const RenderConst& rc, const DeviceScene& ds, const StackConf& stc, const PnConst& pc) {
    launch_pn_impl<true>(chain, strategy, grid, block, lds_bytes, st, rc, ds, stc, pc);
}
}  // namespace rl
