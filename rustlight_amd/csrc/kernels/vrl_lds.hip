// vrl_lds.hip — the virtual ray lights' chain pass (k_vrl_chain, which reads no scene) and their gather (k_vrl_gather) for scenes staged in LDS; see vrl.hip.h
#include "common.hip.h"
#include "vrl.hip.h"

namespace rl {
__global__ void __launch_bounds__(64) k_vrl_chain(RenderConst rc, VrlConst vc) { vrl_chain(rc, vc); }
void launch_vrl_chain(hipStream_t st, const RenderConst& rc, const VrlConst& vc) {
    hipLaunchKernelGGL(k_vrl_chain, dim3((rc.n_owned + 63u) / 64u), dim3(64), 0, st, rc, vc);
}
void launch_vrl_lds(dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const RenderConst& rc, const DeviceScene& ds, const StackConf& stc, const VrlConst& vc) {
    hipLaunchKernelGGL((k_vrl_gather<true>), grid, block, lds_bytes, st, rc, ds, stc, vc);
}
}  // namespace rl
