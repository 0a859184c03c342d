// pnmis_lds.hip — the point-normal integrator's MIS estimators for scenes staged in LDS; see pnmis.hip.h
#include "common.hip.h"
#include "pnmis.hip.h"

namespace rl {
void launch_pnmis_lds(bool chain, int family, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const RenderConst& rc, const DeviceScene& ds, const StackConf& stc, const PnConst& pc) {
    launch_pnmis_impl<true>(chain, family, grid, block, lds_bytes, st, rc, ds, stc, pc);
}
}  // namespace rl
