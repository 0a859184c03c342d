// fused_strat.hip.h — k_path_fused_strat: the persistent kernel (fused.hip.h: fused_body.inc.h) with the stratified sampler (RL_STREAM_STRATIFIED,
// sampler.hip.h), per-pixel work items.  Instantiated for the run-time material switch only (MAT = -1: a specialised MAT never changes an image),
// both MEDIUM forms and both light forms; fused_strat_lds.hip / fused_strat_stream.hip compile the LDS-staged and the streaming family side by side.
#pragma once
#include "fused.hip.h"

namespace rl {

template <bool MEDIUM, bool LDS_SCENE, int LIGHTS>
__global__ void __launch_bounds__(256, LDS_SCENE ? RL_FUSED_WAVES : RL_FUSED_WAVES_STREAMING) k_path_fused_strat(RenderConst rc_arg, DeviceScene sc_arg, StackConf stc) {
    constexpr int MAT = -1;
    constexpr bool QUEUE = false;
    using SMP = StratSampler;
#include "fused_body.inc.h"
}

template <bool LDS_SCENE>
static void launch_fused_strat_impl(bool medium, bool area_only, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const RenderConst& rc, const DeviceScene& ds, const StackConf& stc) {
    with_flag(medium, [&](auto MED) { with_flag(area_only, [&](auto AREA) {
        constexpr int LIGHTS = decltype(AREA)::value ? LIGHTS_AREA_ONLY : LIGHTS_ANY;
        hipLaunchKernelGGL((k_path_fused_strat<decltype(MED)::value, LDS_SCENE, LIGHTS>), grid, block, lds_bytes, st, rc, ds, stc);
    }); });
}

}  // namespace rl
