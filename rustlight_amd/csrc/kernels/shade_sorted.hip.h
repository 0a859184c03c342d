// shade_sorted.hip.h — the material-sorting shade stage of the wavefront pipeline, generic over the sampler (sampler.hip.h): its body is
// shade_sorted_body.inc.h, which k_shade_sorted (shade.hip) includes with SMP = Rng and k_shade_sorted_strat (shade_strat.hip) with SMP = StratSampler.
#pragma once

namespace rl {

// k_shade_sorted<MEDIUM>: mixed-material scenes.  Stream compaction + material sort with wave64 ballot and
// prefix popcounts, local to the workgroup's 256 slots (no global atomics, no queue in HBM): live slots are
// binned by the BSDF type of the surface they hit, then each BSDF's code runs once over its packed bin, so
// a wave never mixes two BSDFs.
static constexpr int kNumBins = 5;
// CHUNKS: 256-slot chunks of the pool per workgroup.  With sample-parallel pixels on a scene most camera rays miss, only one
// slot in eight carries a vertex; one chunk would leave a single part-filled wave per workgroup (and this kernel's register
// footprint allows 3 workgroups per CU), so sparse pools are gathered four chunks at a time into full waves
// (508 k-triangle scene, 128 spp: 781 -> 645 ms; the traversal kernels gain nothing from the same trick).
// 3 waves/SIMD (168 VGPRs, 11 spilled) beat the unconstrained 182-VGPR build at 2 waves and a 128-VGPR build at 4 (647 / 621 / 653 ms)
#ifndef RL_SORT_WAVES
#define RL_SORT_WAVES 3
#endif

}  // namespace rl
