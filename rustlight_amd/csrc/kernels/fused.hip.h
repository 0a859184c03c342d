// fused.hip.h — k_path_fused, the persistent form of the pipeline, and its launcher; instantiated by fused_lds.hip (scene staged in LDS)
// and fused_stream.hip (BVH streamed from L2 / HBM) so that the two families compile in parallel, and once more each by fused_*_fast.hip with
// RL_FAST_MATH (NUM = 1: the opt-in tolerance build; the template parameter only keeps the kernel symbols of the two builds apart).
#pragma once
#ifdef RL_STAGE_TIMERS
#include <algorithm>
#include <cstdlib>
#include <vector>
#endif

#ifndef RL_FUSED_QUEUE
#define RL_FUSED_QUEUE 0    // 1 (fusedq_lds.hip / fusedq_stream.hip): this translation unit instantiates the queue-fed form of the kernel
#endif

namespace rl {

// ------------------------------------------------------------------------------------------
// k_path_fused<MAT, MEDIUM, LDS> — the persistent form of the pipeline for scenes with one BSDF type: one
// launch, one lane per pixel item, the four stage functions above run back-to-back per iteration
// (raygen -> extend -> shade -> shadow) with the path state in registers and LDS (FusedState) and the scene +
// traversal stacks in LDS.  Same functions, same order of operations, same results as the wavefront kernels;
// what disappears is ~1.4 KB/sample of state traffic through HBM and ~2000 kernel boundaries per render.
#ifdef RL_STAGE_TIMERS
__device__ unsigned long long g_stage_timers[32];      // [0..3] cycles per stage, [4..7] live lanes per stage, [8] lane slots, [16..] shadow-stage occupancy (dump_stage_timers_impl)
#endif
// QUEUE: the form that takes its work from the chain pass's completion queue (the evaluation pass of reference-order streams, launched beside the chain pass): an
// instantiation of its own (fusedq_lds.hip / fusedq_stream.hip), so that the per-sample kernel's code is exactly what it is without it.
// The body is fused_body.inc.h: k_path_fused includes it with the independent sampler (SMP = Rng), k_path_fused_strat (fused_strat.hip.h) with StratSampler.
template <int MAT, bool MEDIUM, bool LDS_SCENE, int LIGHTS, int NUM, bool QUEUE = false>
__global__ void __launch_bounds__(256, LDS_SCENE ? RL_FUSED_WAVES : RL_FUSED_WAVES_STREAMING) k_path_fused(RenderConst rc_arg, DeviceScene sc_arg, StackConf stc) {
    using SMP = Rng;
#include "fused_body.inc.h"
}


template <bool LDS_SCENE>
static void launch_fused_impl(int mat, bool medium, bool area_only, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const RenderConst& rc, const DeviceScene& ds, const StackConf& stc) {
    with_bsdf(mat, [&](auto M) { with_flag(medium, [&](auto MED) { with_flag(area_only, [&](auto AREA) {
        constexpr int MAT = decltype(M)::value, LIGHTS = decltype(AREA)::value ? LIGHTS_AREA_ONLY : LIGHTS_ANY;
        hipLaunchKernelGGL((k_path_fused<MAT, decltype(MED)::value, LDS_SCENE, LIGHTS, RL_NUMERICS_ID, RL_FUSED_QUEUE != 0>), grid, block, lds_bytes, st, rc, ds, stc);
    }); }); });
}
template <bool LDS_SCENE>
static void dump_stage_timers_impl() {
#ifdef RL_STAGE_TIMERS
    // dev-only build: per-stage cycle shares and active-lane fractions of the fused loop
    unsigned long long h[32];
    hipMemcpyFromSymbol(h, HIP_SYMBOL(g_stage_timers), sizeof(h));
    const double tot = (double)(h[0] + h[1] + h[2] + h[3]);
    const char* names[4] = {"raygen", "extend", "shade", "shadow"};
    for (int k = 0; k < 4; k++) std::fprintf(stderr, "[stage] %-7s cycles %5.1f %%  lanes %5.1f %%\n", names[k], 100.0 * h[k] / tot, 100.0 * h[4 + k] / (double)h[8]);
    {
        const double it = (double)(h[16] + h[17] + h[18] + h[19] + h[20]), ex = it - (double)h[16], pr = (double)(h[21] + h[22] + h[23] + h[24]);
        if (it > 0) std::fprintf(stderr, "[stage] shadow stage: runs in %.1f %% of the wave-iterations; where it runs the wave holds 1-16 / 17-32 / 33-48 / 49-64 shadow rays in %.1f / %.1f / %.1f / %.1f %% (%.1f lanes on average)\n",
                                 100.0 * ex / it, 100.0 * h[17] / std::max(1.0, ex), 100.0 * h[18] / std::max(1.0, ex), 100.0 * h[19] / std::max(1.0, ex), 100.0 * h[20] / std::max(1.0, ex), (double)h[7] / std::max(1.0, ex));
        if (pr > 0) std::fprintf(stderr, "[stage] pairs of consecutive iterations: neither holds shadow rays %.1f %%, one does %.1f %%, both and <= 64 together %.1f %% (one traversal could serve both), both and > 64 %.1f %%\n",
                                 100.0 * h[21] / pr, 100.0 * h[22] / pr, 100.0 * h[23] / pr, 100.0 * h[24] / pr);
    }
    std::memset(h, 0, sizeof(h)); hipMemcpyToSymbol(HIP_SYMBOL(g_stage_timers), h, sizeof(h));
#endif
}

}  // namespace rl
