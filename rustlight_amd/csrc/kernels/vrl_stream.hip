// vrl_stream.hip — the virtual ray lights' gather (k_vrl_gather) with the BVH streamed from L2 / HBM; see vrl.hip.h
#include "common.hip.h"
#include "vrl.hip.h"

namespace rl {
void launch_vrl_stream(dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const RenderConst& rc, const DeviceScene& ds, const StackConf& stc, const VrlConst& vc) {
    hipLaunchKernelGGL((k_vrl_gather<false>), grid, block, lds_bytes, st, rc, ds, stc, vc);
}
}  // namespace rl
